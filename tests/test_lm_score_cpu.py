"""Sentence scoring on the GPU (sg_lm_score_text_batch, sg_lm_score_text_batch_device, sg_lm_score_word_ids_batch): what can be
checked without one — the exports, the argument checks that come before any HIP call, and the Go shim's calls against the
header's prototypes."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from conftest import GOLDEN, ROOT

SCORE_SYMBOLS = ("sg_lm_score_text_batch", "sg_lm_score_text_batch_device", "sg_lm_score_word_ids_batch")
SG_OK, SG_E_INVALID = 0, -1


@pytest.fixture(scope="module")
def lm():
    from suggest_amd import LanguageModel
    return LanguageModel(os.path.join(GOLDEN, "lm"), 3)


def test_scoring_entry_points_are_exported():
    from suggest_amd import _lib
    L = _lib.lib()
    header = open(os.path.join(ROOT, "include", "suggest_hip.h")).read()
    for name in SCORE_SYMBOLS:
        assert name in _lib.EXPORTS, name
        assert re.search(r"\bint\s+%s\s*\(" % name, header), name
        assert hasattr(L, name), name


def test_null_arguments_are_invalid_without_a_gpu(lm):
    from suggest_amd import _lib
    L = _lib.lib()
    blob = np.frombuffer(b"i am sam", dtype=np.uint8).copy()
    offs = np.array([0, len(blob)], dtype=np.uint64)
    ids = np.array([0, 1, 2], dtype=np.uint32)
    id_offs = np.array([0, 3], dtype=np.uint64)
    sc = np.zeros(1, dtype=np.float64)
    cnt = np.zeros(1, dtype=np.uint32)
    b, o, s, w, u = blob.ctypes.data, offs.ctypes.data, sc.ctypes.data, cnt.ctypes.data, cnt.ctypes.data
    # sg_lm_score_text_batch: null lm, offsets, scores
    assert L.sg_lm_score_text_batch(None, 0, b, o, 1, s, w, u) == SG_E_INVALID
    assert L.sg_lm_score_text_batch(lm._h, 0, b, None, 1, s, w, u) == SG_E_INVALID
    assert L.sg_lm_score_text_batch(lm._h, 0, b, o, 1, None, w, u) == SG_E_INVALID
    assert L.sg_lm_score_text_batch(lm._h, 0, None, o, 1, s, w, u) == SG_E_INVALID       # bytes to read, no text
    assert L.sg_lm_score_text_batch(lm._h, -1, b, o, 1, s, w, u) == SG_E_INVALID
    desc = np.array([0, 5, 3], dtype=np.uint64)                                              # offsets that go back
    assert L.sg_lm_score_text_batch(lm._h, 0, b, desc.ctypes.data, 2, s, w, u) == SG_E_INVALID
    # the device variant
    assert L.sg_lm_score_text_batch_device(None, 0, b, o, 1, len(blob), s, w, u, None) == SG_E_INVALID
    assert L.sg_lm_score_text_batch_device(lm._h, 0, b, None, 1, len(blob), s, w, u, None) == SG_E_INVALID
    assert L.sg_lm_score_text_batch_device(lm._h, 0, b, o, 1, len(blob), None, w, u, None) == SG_E_INVALID
    assert L.sg_lm_score_text_batch_device(lm._h, 0, None, o, 1, len(blob), s, w, u, None) == SG_E_INVALID
    assert L.sg_lm_score_text_batch_device(lm._h, 0, b, o, 1, (1 << 30) + 1, s, w, u, None) == SG_E_INVALID
    # sg_lm_score_word_ids_batch
    assert L.sg_lm_score_word_ids_batch(None, 0, ids.ctypes.data, id_offs.ctypes.data, 1, s) == SG_E_INVALID
    assert L.sg_lm_score_word_ids_batch(lm._h, 0, ids.ctypes.data, None, 1, s) == SG_E_INVALID
    assert L.sg_lm_score_word_ids_batch(lm._h, 0, ids.ctypes.data, id_offs.ctypes.data, 1, None) == SG_E_INVALID
    assert L.sg_lm_score_word_ids_batch(lm._h, 0, None, id_offs.ctypes.data, 1, s) == SG_E_INVALID
    assert b"null" in L.sg_last_error()


def test_an_empty_batch_is_ok_without_a_gpu(lm):
    from suggest_amd import _lib
    L = _lib.lib()
    offs = np.zeros(1, dtype=np.uint64)
    sc = np.zeros(1, dtype=np.float64)
    assert L.sg_lm_score_text_batch(lm._h, 0, None, offs.ctypes.data, 0, sc.ctypes.data, None, None) == SG_OK
    assert L.sg_lm_score_text_batch_device(lm._h, 0, None, offs.ctypes.data, 0, 0, sc.ctypes.data, None, None, None) == SG_OK
    assert L.sg_lm_score_word_ids_batch(lm._h, 0, None, offs.ctypes.data, 0, sc.ctypes.data) == SG_OK
    assert lm.score_word_ids_batch(np.zeros(0, np.uint32), offs).shape == (0,)
    s, w, u = lm.score_text_batch([])
    assert s.shape == w.shape == u.shape == (0,)
    assert lm.ScoreSentenceBatch([]).shape == (0,)


def _prototypes(header):
    """name -> number of parameters of every sg_* prototype of the header"""
    out = {}
    for m in re.finditer(r"\b(sg_[a-z_]+)\s*\(([^;{]*?)\)\s*;", header, re.S):
        params = m.group(2).strip()
        out[m.group(1)] = 0 if params in ("", "void") else params.count(",") + 1
    return out


def _go_calls(src, prefix):
    """(name, number of arguments) of every C.<prefix>*(...) call of the Go source (nested parentheses balanced)"""
    calls = []
    for m in re.finditer(r"\bC\.(%s[a-z_]*)\s*\(" % re.escape(prefix), src):
        depth, i, args, cur = 1, m.end(), 0, ""
        while depth:
            c = src[i]
            if c in "([{":
                depth += 1
            elif c in ")]}":
                depth -= 1
            if depth == 1 and c == ",":
                args += 1
            cur += c
            i += 1
        calls.append((m.group(1), 0 if not cur[:-1].strip() else args + 1))
    return calls


def test_go_shim_score_calls_match_the_header():
    header = open(os.path.join(ROOT, "include", "suggest_hip.h")).read()
    go = open(os.path.join(ROOT, "go", "suggesthip", "suggesthip.go")).read()
    protos = _prototypes(header)
    calls = _go_calls(go, "sg_lm_score")
    assert ("sg_lm_score_text_batch", 8) in calls, calls           # the shim reaches the batch scorer
    for name, n_args in calls:
        assert name in protos, name
        assert protos[name] == n_args, (name, n_args, protos[name])
