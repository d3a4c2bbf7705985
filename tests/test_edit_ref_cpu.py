"""The restatement of the edit-distance ranking (tests/edit_ref.py) pinned by literals, its vectorised form held
against its loops, and both against a memoised recursive definition over a dense edit space.  No GPU, no libsuggest_hip."""
import numpy as np
import pytest

import edit_ref as ref


def test_literals():
    assert ref.distance("kitten", "sitting", "levenshtein") == 3 and ref.distance("kitten", "sitting", "osa") == 3
    assert ref.distance("ab", "ba", "levenshtein") == 2 and ref.distance("ab", "ba", "osa") == 1
    # ca -> abc: 3 under both.  Unrestricted Damerau's 2 (ca -> ac -> abc) edits the transposed pair again, which optimal string
    # alignment forbids.  (2 is Damerau's figure alone: Levenshtein has no transposition at all, and osa <= levenshtein always.)
    assert ref.distance("ca", "abc", "levenshtein") == 3 and ref.distance("ca", "abc", "osa") == 3
    assert ref.distance_recursive("ca", "abc", "levenshtein") == 3 and ref.distance_recursive("ca", "abc", "osa") == 3
    for mode in ref.MODES:
        assert ref.distance("", "", mode) == 0 and ref.distance("", "abc", mode) == 3 and ref.distance("abcd", "", mode) == 4
        assert ref.distance(b"\xff\xfe", "\ufffd\ufffd", mode) == 0
        assert ref.distance("\u212a", "k", mode, fold=True) == 0 and ref.distance("\u212a", "k", mode, fold=False) == 1
        assert ref.distance("\u0130x", "ix", mode, fold=True) == 0              # (a folding pair that changes width)
        assert ref.distance("TOYOTA", "toyota", mode, fold=True) == 0 and ref.distance("TOYOTA", "toyota", mode, fold=False) == 6


def test_decoding_is_go_range():
    assert ref.decode(b"a\xd0\x9d\xe2\x84\xaa\xf0\x9f\x98\x80") == [0x61, 0x41D, 0x212A, 0x1F600]
    assert ref.decode(b"\xf0\x9f\x98") == [0xFFFD] * 3                          # a truncated 4-byte rune: a U+FFFD per byte
    assert ref.decode(b"\xc0\x80") == [0xFFFD, 0xFFFD] and ref.decode(b"\xed\xa0\x80") == [0xFFFD] * 3     # overlong, surrogate
    assert ref.decode(b"\x80a\xffb\xc3") == [0xFFFD, 0x61, 0xFFFD, 0x62, 0xFFFD]
    assert ref.decode("\ufffd".encode()) == [0xFFFD]


def test_symmetry_and_the_vectorised_form_against_the_loops():
    rng = np.random.default_rng(11)
    for _ in range(300):
        la, lb = int(rng.integers(0, 90)), int(rng.integers(0, 90))
        alpha = int(rng.choice([2, 3, 26]))
        a, b = rng.integers(0, alpha, la).tolist(), rng.integers(0, alpha, lb).tolist()
        for mode, loop in (("levenshtein", ref.levenshtein), ("osa", ref.osa)):
            want = loop(a, b)
            assert ref.distance_vec(a, b, mode) == want == loop(b, a) == ref.distance_vec(b, a, mode), (mode, a, b)


def test_the_recursive_definition_on_a_dense_edit_space():
    rng = np.random.default_rng(12)
    pairs, differ = 0, 0
    for _ in range(3000):
        a = tuple(rng.integers(0, 3, int(rng.integers(0, 10))).tolist())
        b = tuple(rng.integers(0, 3, int(rng.integers(0, 10))).tolist())
        lev, osa = ref.distance_recursive(a, b, "levenshtein"), ref.distance_recursive(a, b, "osa")
        assert ref.levenshtein(a, b) == lev and ref.osa(a, b) == osa and ref.distance_vec(a, b, "levenshtein") == lev and ref.distance_vec(a, b, "osa") == osa
        assert abs(len(a) - len(b)) <= osa <= lev <= max(len(a), len(b))
        pairs += 1
        differ += osa < lev
    assert pairs == 3000 and differ > 0            # (some pairs are cheaper with a transposition)


def test_rerank_by_hand():
    ids = [[5, 6, 7, 8], [1, 2, 3, 4], [9, 9, 9, 9]]
    sc = [[.9, .8, .7, .6], [.5, .4, .3, .2], [1, 1, 1, 1]]
    d = [[2, 1, 2, 0], [3, 3, 1, 7], [4, 4, 4, 4]]
    i2, s2, d2, c2 = ref.rerank(ids, sc, d, [4, 3, 0xFFFFFFFD], row=4)
    assert i2.tolist() == [8, 6, 5, 7, 3, 1, 2, 0, 9, 9, 9, 9] and d2.tolist() == [0, 1, 2, 2, 1, 3, 3, 0, 4, 4, 4, 4]
    assert s2.tolist() == [.6, .8, .9, .7, .3, .5, .4, 0, 1, 1, 1, 1] and c2.tolist() == [4, 3, 0xFFFFFFFD]
    i2, s2, d2, c2 = ref.rerank(ids, None, d, [4, 3, 0], row=4, max_distance=1, k_out=1)
    assert s2 is None and i2.tolist() == [8, 0, 0, 0, 3, 0, 0, 0, 0, 0, 0, 0] and c2.tolist() == [1, 1, 0]
    i2, _, d2, c2 = ref.rerank(np.arange(7), None, [5, 9, 1, 1, 0, 0, 0], [2, 9], row_offs=[0, 2, 4], max_distance=4)       # ragged, a spare tail
    assert i2.tolist() == [0, 0, 2, 3, 4, 5, 6] and d2.tolist() == [0, 0, 1, 1, 0, 0, 0] and c2.tolist() == [0, 2]


def test_edit_rows_by_hand():
    lines = [b"nissan", b"toyota", b"", b"TOYOTA corolla"]
    dist, outside = ref.edit_rows(["nisan", "toyoat"], [[0, 1, 2, 3], [1, 7, 3, 0]], [3, 3], lines, row=4, mode="osa")
    assert dist.tolist() == [1, 6, 5, ref.NONE, 1, ref.NONE, 9, ref.NONE] and outside == 1
    dist, outside = ref.edit_rows(["nisan", "toyoat"], [[0, 1, 2, 3], [1, 7, 3, 0]], [0xFFFFFFFF, 1], lines, row=4)
    assert dist.tolist() == [ref.NONE] * 4 + [2] + [ref.NONE] * 3 and outside == 0


@pytest.mark.parametrize("r", [0x41, 0x41D, 0x1F600])
def test_peq_hash_is_seven_bits(r):
    assert 0 <= ref.peq_hash(r) < 128
