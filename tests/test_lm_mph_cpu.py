"""LanguageModel.save(..., mph=True) (sg_lm_store_binary_ex with SG_LM_STORE_MPH): the .lm file with the minimal perfect hash
Go's RetrieveLMFromBinary reads after the model (pkg/lm/binary.go:59-98, pkg/mph/mph.go).  The golden vector is the reference's
own tests/golden/lm/test.lm, all 658 bytes: its 104-byte tail is the MPH of 12 words, which pins hash, bucket order (Go 1.14
sort.Slice under a non-strict less), the seed search and the free-slot order.  Larger vocabularies are held against
tests/mph_ref.py, whose Get is first pinned on the reference's file.  CPU only: host code."""
import os

import pytest

import mph_ref
from lm_store_shapes import LM_DIR, SG_E_UNSUPPORTED, gen_vocab, model_part, write_vocab_model

SIZES = (0, 1, 2, 12, 13, 40, 41, 1000, 50000)


def _golden():
    data = open(os.path.join(LM_DIR, "test.lm"), "rb").read()
    assert len(data) == 658
    return data


def test_fixture_model_with_mph_equals_the_reference_file(tmp_path):
    from suggest_amd.spell import LanguageModel
    src = LanguageModel(LM_DIR, id_order="count")
    lm_path, cdb_path = str(tmp_path / "out.lm"), str(tmp_path / "out.cdb")
    src.save(lm_path, cdb_path, mph=True)
    assert open(lm_path, "rb").read() == _golden()
    assert open(cdb_path, "rb").read() == open(os.path.join(LM_DIR, "test.cdb"), "rb").read()
    back = LanguageModel(binary=lm_path, dictionary=cdb_path)                  # the loader ignores the tail
    assert back.words() == src.words()


def test_the_checker_reads_the_reference_section():
    """Covers none of the library: mph_ref's Load and Get map every word of the file Go wrote to its id, and its Build gives
    that section back."""
    from suggest_amd.spell import LanguageModel
    data = _golden()
    tail = data[len(model_part(data)):]
    assert len(tail) == 104
    values, auxiliary, used = mph_ref.load(tail)
    assert used == 104 and len(values) == 12 and len(auxiliary) == 12
    words = LanguageModel(LM_DIR, id_order="count").words()
    assert len(words) == 12
    assert [mph_ref.get(values, auxiliary, w) for w in words] == list(range(12))
    assert mph_ref.store(*mph_ref.build(words)) == tail


def test_save_without_mph_is_unchanged(tmp_path):
    from suggest_amd import _lib
    from suggest_amd.spell import LanguageModel
    src = LanguageModel(LM_DIR, id_order="count")
    a, b, c = (str(tmp_path / n) for n in ("a.lm", "b.lm", "c.lm"))
    src.save(a, str(tmp_path / "a.cdb"))
    src.save(b, str(tmp_path / "b.cdb"), mph=False)
    assert _lib.lib().sg_lm_store_binary(src._h, c.encode(), str(tmp_path / "c.cdb").encode()) == 0
    want = model_part(_golden())
    assert open(a, "rb").read() == want and open(b, "rb").read() == want and open(c, "rb").read() == want
    assert _lib.lib().sg_lm_store_binary_ex(src._h, a.encode(), str(tmp_path / "a.cdb").encode(), 2) == -1   # an unknown flag


@pytest.mark.parametrize("n", SIZES)
def test_generated_vocabulary(n, tmp_path):
    from suggest_amd.spell import LanguageModel
    words = gen_vocab(n)
    assert len(words) == n == len(set(words))
    if n >= 2:
        assert min(len(w) for w in words) == 1 and max(len(w) for w in words) == 300
        assert any(w[0] >= 0x80 for w in words) or n < 12
    write_vocab_model(str(tmp_path), words)
    lm = LanguageModel(str(tmp_path), order=1, id_order="lines")
    assert lm.words() == words
    paths = [(str(tmp_path / ("%s.lm" % t)), str(tmp_path / ("%s.cdb" % t))) for t in "ab"]
    for p in paths:
        lm.save(*p, mph=True)
    data = open(paths[0][0], "rb").read()
    assert data == open(paths[1][0], "rb").read()                              # two saves are identical
    lm.save(str(tmp_path / "plain.lm"), str(tmp_path / "plain.cdb"))
    plain = open(str(tmp_path / "plain.lm"), "rb").read()
    assert data[:len(plain)] == plain and model_part(data) == plain
    tail = data[len(plain):]
    values, auxiliary, used = mph_ref.load(tail)
    assert used == len(tail) == 8 + 8 * n
    if n == 0:
        assert tail == bytes(8)
        return
    assert sorted(values) == list(range(n))                                    # a permutation of the ids
    assert [mph_ref.get(values, auxiliary, w) for w in words] == list(range(n))
    assert tail == mph_ref.store(*mph_ref.build(words))                        # word for word


def test_a_word_listed_twice_is_refused_before_a_file_is_written(tmp_path):
    from suggest_amd import _lib
    from suggest_amd.spell import LanguageModel
    write_vocab_model(str(tmp_path), [b"a", b"b", b"a"])
    lm = LanguageModel(str(tmp_path), order=1, id_order="lines")
    with pytest.raises(_lib.SuggestHipError) as e:
        lm.save(str(tmp_path / "x.lm"), str(tmp_path / "x.cdb"), mph=True)
    assert e.value.code == SG_E_UNSUPPORTED and "twice" in str(e.value)
    assert not (tmp_path / "x.lm").exists() and not (tmp_path / "x.cdb").exists()
