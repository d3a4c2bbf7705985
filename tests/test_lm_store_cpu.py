"""LanguageModel.save (sg_lm_store_binary): any model written in the production format — <name>.lm as nGramModel.Store writes it
(ngram_model.go:100-121, packed_array.go:96-116) and <name>.cdb as BuildCDBDictionary does (pkg/dictionary/helpers.go:52-100).
The golden vector is the reference's own fixture pair tests/golden/lm/test.{lm,cdb}: the model of the 1/2/3-gm files next to it.
The minimal perfect hash behind the model part of test.lm is not written.  CPU only: host code."""
import os

import numpy as np
import pytest

LM_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "lm")


def _model_part(data):
    """the prefix of a .lm file that holds the model: version, order, the levels (where test_lm_binary._levels_of_file stops)"""
    assert data[:5] == b"0.0.2"
    order, pos = data[5], 6
    for _ in range(order):
        nl = data.index(b"\n", pos)
        cs, vs, _total = (int(x) for x in data[pos:nl].split())
        pos = nl + 1 + cs + vs
    return data[:pos]


def _same_model(a, b):
    assert a.order == b.order
    assert a.words() == b.words()
    for i in range(a.order):
        (ac, av, at), (bc, bv, bt) = a.level(i), b.level(i)
        assert np.array_equal(ac, bc) and np.array_equal(av, bv) and at == bt, i


def test_saved_fixture_model_equals_the_reference_files(tmp_path, reference_tests):
    from suggest_amd.spell import LanguageModel
    src = LanguageModel(LM_DIR, id_order="count")
    lm_path, cdb_path = str(tmp_path / "out.lm"), str(tmp_path / "out.cdb")
    src.save(lm_path, cdb_path)
    golden_cdb = open(os.path.join(LM_DIR, "test.cdb"), "rb").read()
    assert len(golden_cdb) == 2421
    assert open(cdb_path, "rb").read() == golden_cdb
    golden_lm = open(os.path.join(LM_DIR, "test.lm"), "rb").read()
    assert golden_lm.startswith(b"0.0.2\x03" + b"8 96 20\n")
    assert open(lm_path, "rb").read() == _model_part(golden_lm)
    back = LanguageModel(binary=lm_path, dictionary=cdb_path)
    _same_model(back, src)
    g = reference_tests["lm"]
    for sent, expected in g["score_sentence"]:
        assert abs(back.ScoreSentence(sent) - expected) < g["tolerance"], sent


def test_line_order_model_round_trips(tmp_path):
    from suggest_amd.spell import LanguageModel
    src = LanguageModel(LM_DIR, id_order="lines")
    lm_path, cdb_path = str(tmp_path / "lines.lm"), str(tmp_path / "lines.cdb")
    src.save(lm_path, cdb_path)
    _same_model(LanguageModel(binary=lm_path, dictionary=cdb_path), src)
    assert src.words() != LanguageModel(LM_DIR, id_order="count").words()


def test_unwritable_path_is_an_error(tmp_path):
    from suggest_amd import _lib
    from suggest_amd.spell import LanguageModel
    src = LanguageModel(LM_DIR, id_order="count")
    missing = tmp_path / "no_such_directory"
    with pytest.raises(_lib.SuggestHipError) as e:
        src.save(str(missing / "a.lm"), str(tmp_path / "a.cdb"))
    assert e.value.code == -1 and "a.lm" in str(e.value)
    assert not (tmp_path / "a.cdb").exists()
    with pytest.raises(_lib.SuggestHipError) as e:
        src.save(str(tmp_path / "b.lm"), str(missing / "b.cdb"))
    assert e.value.code == -1 and "b.cdb" in str(e.value)
