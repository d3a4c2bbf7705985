"""The shapes of the edit-search tests contain the situations their tests are about (tests/edit_search_shapes.py) — asserted here, on
the CPU, from the restatement alone, so that no test passes for want of a hard case.  Also holds the vectorised brute force of
tests/edit_search_ref.py against edit_ref's loops."""
import numpy as np
import pytest

import edit_ref as ref
import edit_search_ref as sref
import edit_search_shapes as shp
import oracle
from conftest import CARS_DESC


def test_the_vectorised_distances_equal_the_loops():
    lines = shp.array_lines(257) + shp.dense_lines()[:200] + shp.tie_lines()[:20]
    queries = [b"", b"c", "xК".encode(), b"abcD", shp.LONG70[:64].encode(), b"\xff\xfeab", b"toyoat", "été €".encode()]
    for mode in ref.MODES:
        for fold in (True, False):
            dm = sref.distance_matrix(queries, lines, mode, fold)
            for i, q in enumerate(queries):
                for d in range(0, len(lines), 3):
                    assert dm[i, d] == ref.distance(q, lines[d], mode, fold), (mode, fold, q, lines[d])


def test_the_array_dictionary():
    lines = shp.array_lines(257)
    assert [len(shp.array_lines(n)) for n in shp.ARRAY_SIZES] == list(shp.ARRAY_SIZES) and shp.array_lines(65) == lines[:65]
    rs = [ref.runes(l, False) for l in lines]
    assert sum(len(r) == 0 for r in rs[:64]) >= 2 and any(len(r) == 70 for r in rs[:64])
    assert any(ref.RUNE_ERROR in r for r in rs[:64])                                         # invalid bytes, a truncated rune
    widths = {len(chr(c).encode()) for r in rs[:64] for c in r if c != ref.RUNE_ERROR}
    assert widths == {1, 2, 3, 4}
    for up, low in shp.CASE_PAIRS:
        i, j = lines.index(("x" + up).encode()), lines.index(("x" + low).encode())
        assert i < 64 and j < 64 and ref.runes(lines[i], True) == ref.runes(lines[j], True) and rs[i] != rs[j]
    runes_f, sig_f = sref.arrays(lines, True)
    runes_u, sig_u = sref.arrays(lines, False)
    assert np.array_equal(runes_f, runes_u) and not np.array_equal(sig_f, sig_u)            # folding changes signatures, not lengths
    assert sref.sig_bit(0x41) != sref.sig_bit(0x61) and 0 <= min(map(sref.sig_bit, range(0x500))) and max(map(sref.sig_bit, range(0x500))) == 63


@pytest.fixture(scope="module")
def dense():
    lines = shp.dense_lines()
    return lines, shp.dense_queries(lines)


def test_the_dense_dictionary_and_its_queries(dense):
    lines, queries = dense
    assert len(lines) == 2048 and len(queries) == 64
    lens = [len(ref.decode(l)) for l in lines]
    assert min(lens) == 1 and max(lens) == 12 and {c for l in lines for c in l.decode()} == set(shp.DENSE_ALPHABET)
    assert [len(ref.decode(q)) for q in queries[:4]] == [0, 1, 64, 65]
    assert ref.decode(queries[4]) == [ref.RUNE_ERROR] * 3
    assert ref.runes(queries[5], True) == ref.runes(lines[5], True) and ref.runes(queries[5], False) != ref.runes(lines[5], False)


@pytest.mark.parametrize("max_distance", [2, 5])
def test_the_cut_falls_inside_a_group_that_spans_slices(dense, max_distance):
    """at k = 7, for a quarter of the queries at least: more matches than k, more strings at the cut-off distance than are still
    wanted there, and those strings in more than one slice — for 2 and for 7 slices"""
    lines, queries = dense
    dm = shp.matrix("dense", lines, queries, "levenshtein", True)
    k = 7
    for n_slices in (2, 7):
        hard = 0
        for i in range(len(queries)):
            row = dm[i]
            if row[0] < 0:
                continue
            hist = np.bincount(row[row <= max_distance], minlength=max_distance + 1)
            if hist.sum() <= k:
                continue
            cut = int(np.nonzero(np.cumsum(hist) >= k)[0][0])
            want = k - int(hist[:cut].sum())
            at = np.nonzero(row == cut)[0]
            hard += at.size > want and len({sref.slice_of(int(d), len(lines), n_slices) for d in at}) > 1
        assert hard * 4 >= len(queries), (n_slices, hard)


def test_some_row_has_fewer_matches_than_the_widest_k(dense):
    lines, queries = dense
    for mode in ref.MODES:
        for fold in (True, False):
            dm = shp.matrix("dense", lines, queries, mode, fold)
            for md in shp.MAX_DISTANCES[:3]:
                counts = sref.search(dm, 1024, md)[2]
                assert np.any((counts < 1024) & (counts > 0)), (mode, fold, md)
            assert np.any(sref.search(dm, 1024, 32)[2] == 1024)
            assert sref.search(dm, 7, 2)[2][3] == sref.TOO_LONG and np.all(dm[2] > 32)      # 65 runes: flagged; 64 runes: answered, no match


def test_the_repeated_string_lies_in_every_slice():
    lines = shp.tie_lines()
    copies = [i for i, l in enumerate(lines) if l == shp.TIE]
    assert len(copies) == 500 and {sref.slice_of(i, len(lines), 7) for i in copies} == set(range(7))
    dm = sref.distance_matrix(shp.TIE_QUERIES, lines, "levenshtein", True)
    ids, dist, counts, hist = sref.search(dm, 499, 2)
    assert hist[0][0] >= 500 and counts[0] == 499 and np.all(dist[0] == 0)
    assert ids[0].tolist() == [i for i, l in enumerate(lines) if ref.runes(l, True) == ref.runes(shp.TIE, True)][:499]      # ties by docID


def test_the_transposition_queries_tell_the_modes_apart():
    lines, queries = shp.transposition_cases()
    lev = sref.search(sref.distance_matrix(queries, lines, "levenshtein", True), 4, 1)
    osa = sref.search(sref.distance_matrix(queries, lines, "osa", True), 4, 1)
    assert np.all(osa[2] == 1) and np.all(lev[2] == 0) and np.array_equal(osa[0][:, 0], np.arange(len(lines)))
    assert not np.array_equal(lev[0], osa[0])


def test_the_chunk_queries():
    assert len(shp.chunk_queries(shp.dense_lines())) == 300


def test_cars_queries_have_a_match_the_candidate_route_misses(cars_lines):
    """from brute force and the CPU oracle alone: some string within two edits of a query is not among the 16 candidates the
    q-gram search proposes"""
    lines = [bytes(l) for l in cars_lines]
    queries = shp.cars_queries(lines)
    assert len(queries) == 200
    dm = shp.matrix("cars", lines, queries, "levenshtein", True)
    ids, dist, counts, hist = sref.search(dm, 1024, 2)
    assert np.all(counts < 1024)                                 # a row of 1 024 holds every match
    ora = oracle.OracleIndex(lines, **CARS_DESC)
    qb, qo = oracle.pack_strings(queries)
    o_ids, _, o_cnt, _ = ora.suggest_batch(qb, qo, "jaccard", 0.5, 16)
    missed = 0
    for i in range(len(queries)):
        cand = set(o_ids[i, :min(int(o_cnt[i]), 16)].tolist()) if o_cnt[i] < ref.COUNT_FLAG_MIN else set()
        missed += len(set(ids[i, :counts[i]].tolist()) - cand)
    assert missed >= 1
    assert int(hist[:, 1:].sum()) > 100 and int((counts > 0).sum()) > 150
