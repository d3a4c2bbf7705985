"""LanguageModel.save_ngrams on the GPU (sg_lm_store_google, device = 0): the lines of <dir>/<k>-gm formatted by the kernels of
suggest_amd/csrc/lm_store.inc.  The referee is the host writer (device = -1), which tests/test_lm_ngrams_cpu.py holds against
the reference's fixture files and the host count builder: the device writer's files must equal its files byte for byte, and
load back as the model."""
import os

import numpy as np
import pytest

from lm_store_shapes import (ALPHA_WIDE, COUNT_EDGES, LM_DIR, ORDERS, corpus_20k, gm_files, gm_lines, long_word_corpus, same_model, store_times,
                             tile_corpus, write_counts_model)

pytestmark = pytest.mark.gpu


def _both(lm, tmp_path, tag=""):
    """-> (host files, device files) of the model, each a list of bytes per k"""
    host, dev = tmp_path / ("host" + tag), tmp_path / ("dev" + tag)
    host.mkdir(); dev.mkdir()
    lm.save_ngrams(host, device=-1)
    lm.save_ngrams(dev, device=0)
    t = store_times()
    assert all(x >= 0 for x in t) and t[1] > 0                                 # kernels ran
    return gm_files(host, lm.order), gm_files(dev, lm.order)


def _reloads(lm, directory, alphabet):
    from suggest_amd.spell import LanguageModel
    same_model(LanguageModel(str(directory), lm.order, "<S>", "</S>", alphabet, id_order="lines"), lm, "reload")


def test_fixture_model(tmp_path):
    from suggest_amd.spell import LanguageModel
    for id_order in ("count", "lines"):
        lm = LanguageModel(LM_DIR, id_order=id_order)
        host, dev = _both(lm, tmp_path, id_order)
        assert dev == host
        assert sorted(dev[2].split(b"\n")) == sorted(open(os.path.join(LM_DIR, "3-gm"), "rb").read().split(b"\n"))


@pytest.mark.parametrize("order", ORDERS)
def test_model_from_corpus(order, tmp_path):
    from suggest_amd.spell import LanguageModel
    lm = LanguageModel.from_corpus(corpus_20k(), order, "<S>", "</S>", ALPHA_WIDE, ("\n",), id_order="count")
    assert len(lm.level(order - 1)[1]) > 100 and any(w[0] >= 0x80 for w in lm.words())
    host, dev = _both(lm, tmp_path)
    assert dev == host
    _reloads(lm, tmp_path / "dev", ALPHA_WIDE)


@pytest.mark.parametrize("m", (63, 64, 65))
def test_wavefront_edges(m, tmp_path):
    from suggest_amd.spell import LanguageModel
    lm = LanguageModel.from_corpus(tile_corpus(m), 3, "<S>", "</S>", ("english", "numbers"), ("\n",), id_order="lines")
    assert [len(lm.level(i)[1]) for i in range(3)] == [m + 2, m + 1, m]       # 63, 64 and 65 entries are among them
    host, dev = _both(lm, tmp_path)
    assert dev == host
    assert [f.count(b"\n") for f in dev] == [m + 2, m + 1, m]
    _reloads(lm, tmp_path / "dev", ("english", "numbers"))


def test_lines_of_2400_bytes(tmp_path):
    """words of 300 bytes at order 8: 64 lines are 150 KB, far beyond anything a workgroup could stage in LDS"""
    from suggest_amd.spell import LanguageModel
    lm = LanguageModel.from_corpus(long_word_corpus(), 8, "<S>", "</S>", ("english",), ("\n",), id_order="count")
    host, dev = _both(lm, tmp_path)
    top = gm_lines(tmp_path / "host", 8)
    assert len(top) >= 20 and min(len(ln) for ln in top) > 1800 and max(len(ln) for ln in top) > 2400
    assert dev == host
    _reloads(lm, tmp_path / "dev", ("english",))


def test_digit_boundaries(tmp_path):
    from suggest_amd.spell import LanguageModel
    src = tmp_path / "src"
    src.mkdir()
    write_counts_model(str(src))
    lm = LanguageModel(str(src), 2, "<S>", "</S>", ("english", "numbers"), id_order="lines")
    host, dev = _both(lm, tmp_path)
    assert dev == host
    assert sorted(int(ln.split(b"\t")[1]) for ln in gm_lines(tmp_path / "dev", 2)) == sorted(COUNT_EDGES)


def test_slices_with_boundaries_inside_wavefronts(tmp_path):
    from suggest_amd import _lib
    from suggest_amd.spell import LanguageModel
    lm = LanguageModel.from_corpus(corpus_20k(), 3, "<S>", "</S>", ALPHA_WIDE, ("\n",), id_order="count")
    whole = tmp_path / "whole"
    whole.mkdir()
    lm.save_ngrams(whole, device=0)
    want = gm_files(whole, 3)
    assert len(want[2]) > 20 * 4096                                            # the top level spans many slices
    L = _lib.lib()
    sliced, host = tmp_path / "sliced", tmp_path / "host"
    sliced.mkdir(); host.mkdir()
    try:
        _lib.check(L.sg_debug_lm_store_slice_bytes(4096))
        lm.save_ngrams(sliced, device=0)
        lm.save_ngrams(host, device=-1)                                        # (the host writer has no slices)
    finally:
        _lib.check(L.sg_debug_lm_store_slice_bytes(0))
    assert gm_files(sliced, 3) == want and gm_files(host, 3) == want
    # a slice ends at a line that fits 4096 bytes: with lines of 10 .. 40 bytes that is no multiple of 64 lines
    lens = [len(ln) + 1 for ln in gm_lines(whole, 3)]
    first = int(np.searchsorted(np.cumsum(lens), 4096, side="right"))
    assert first % 64 != 0


def test_scoring_and_predict_are_unchanged_by_a_save(tmp_path):
    from suggest_amd.spell import LanguageModel, SpellChecker
    text = corpus_20k()
    lm = LanguageModel.from_corpus(text, 3, "<S>", "</S>", ALPHA_WIDE, ("\n",), id_order="count")
    sc = SpellChecker(lm)
    lines = [ln for ln in text.split(b"\n")[:200]]
    queries = [ln[:-1] for ln in lines if len(ln) > 3][:100]
    scores = lm.score_text_batch(lines)
    ids, cnt = sc.predict_batch(queries, 5, 0.4)
    assert int(cnt.sum()) > 0
    lm.save_ngrams(tmp_path, device=0)
    again = lm.score_text_batch(lines)
    for a, b in zip(scores, again):
        assert np.array_equal(a, b)
    ids2, cnt2 = sc.predict_batch(queries, 5, 0.4)
    assert np.array_equal(cnt, cnt2) and np.array_equal(ids, ids2)
