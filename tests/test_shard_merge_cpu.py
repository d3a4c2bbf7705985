"""A dictionary sharded by docID range behind one handle (sg_sharded): what can be checked without a GPU — the numpy
statement of the merge against distributed.merge_topk, the ABI's declarations and argument checks, the bindings' shape."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import shard_ref
from conftest import ROOT

NEW = ("sg_sharded_build", "sg_sharded_adopt", "sg_sharded_retain", "sg_sharded_release", "sg_sharded_shards", "sg_sharded_suggest_batch",
       "sg_sharded_suggest_batch_device", "sg_sharded_autocomplete_batch", "sg_debug_shard_slice_bytes", "sg_debug_shard_merge", "sg_debug_shard_merge_time")

# (W, n, k, flags, dup_run): the generator of tests/test_gpu_shard_merge.py at sizes a Python loop walks in a moment
CASES = [(1, 1, 1, "none", False), (2, 5, 10, "none", False), (3, 63, 10, "one", False), (3, 7, 65, "all", False),
         (64, 3, 4, "one", False), (2, 9, 64, "none", False), (4, 257, 3, "one", False)]


@pytest.mark.parametrize("W,n,k,flags,dup_run", CASES)
def test_shard_ref_equals_merge_topk(W, n, k, flags, dup_run):
    import torch
    from suggest_amd.distributed import merge_topk
    ids, sc, cnt, doc_lo = shard_ref.make_case(W, n, k, seed=W * 1000 + n * 10 + k, flags=flags, dup_run=dup_run)
    assert not shard_ref.has_equal_keys(ids, sc, cnt, doc_lo)     # such cases are left out here: strict by construction
    r_ids, r_sc, r_cnt = shard_ref.merge(ids, sc, cnt, doc_lo)
    g = torch.from_numpy(ids.astype(np.int64) + doc_lo.astype(np.int64)[:, None, None])
    m_ids, m_sc, m_cnt = merge_topk(g, torch.from_numpy(sc), torch.from_numpy(cnt.astype(np.int64)), k)
    assert np.array_equal(m_cnt.numpy().astype(np.uint32), r_cnt)
    flagged = r_cnt >= shard_ref.FLAG_MIN
    keep = ~flagged
    assert np.array_equal(m_ids.numpy()[keep].astype(np.uint32), r_ids[keep])
    assert np.array_equal(m_sc.numpy()[keep].view(np.uint64), r_sc[keep].view(np.uint64))
    assert not r_ids[flagged].any() and not r_sc[flagged].view(np.uint64).any()      # a flagged row is zeroed
    tail = np.arange(k)[None, :] >= np.minimum(r_cnt, k)[:, None]
    assert not r_ids[tail & keep[:, None]].any() and not r_sc.view(np.uint64)[tail & keep[:, None]].any()


def test_shard_ref_keeps_the_source_order_of_equal_keys():
    """worked by hand: shard 0 holds document 7 three times at 0.5 (it repeats a term), shard 1 starts at docID 10"""
    ids = np.array([[[3, 7, 7, 7]], [[0, 1, 2, 9]]], dtype=np.uint32)
    sc = np.array([[[1.0, 0.5, 0.5, 0.5]], [[0.75, 0.5, 0.5, 0.25]]])
    cnt = np.array([[4], [3]], dtype=np.uint32)
    assert shard_ref.has_equal_keys(ids, sc, cnt, [0, 10])
    r_ids, r_sc, r_cnt = shard_ref.merge(ids, sc, cnt, [0, 10])
    assert r_cnt.tolist() == [4] and r_ids.tolist() == [[3, 10, 7, 7]] and r_sc.tolist() == [[1.0, 0.75, 0.5, 0.5]]
    ids6 = np.concatenate([ids, np.zeros((2, 1, 2), dtype=np.uint32)], axis=2)
    sc6 = np.concatenate([sc, np.zeros((2, 1, 2))], axis=2)
    r_ids, r_sc, r_cnt = shard_ref.merge(ids6, sc6, cnt, [0, 10])
    assert r_cnt.tolist() == [6] and r_ids.tolist() == [[3, 10, 7, 7, 7, 11]] and r_sc.tolist() == [[1.0, 0.75, 0.5, 0.5, 0.5, 0.5]]


def test_shard_ref_autocomplete_is_the_rows_one_after_the_other():
    ids, _, cnt, doc_lo = shard_ref.make_case(3, 20, 6, seed=5, flags="one")
    r_ids, r_sc, r_cnt = shard_ref.merge(ids, None, cnt, doc_lo, autocomplete=True)
    assert r_sc is None
    for q in range(20):
        if (cnt[:, q] >= shard_ref.FLAG_MIN).any():
            assert r_cnt[q] == cnt[:, q].max() and not r_ids[q].any()
            continue
        want = np.concatenate([ids[s, q, :cnt[s, q]].astype(np.uint64) + doc_lo[s] for s in range(3)])[:6]
        assert r_cnt[q] == len(want) and np.array_equal(r_ids[q, :len(want)], want) and not r_ids[q, len(want):].any()


def test_exports_and_header_declarations():
    from suggest_amd import _lib, ShardedIndex
    L = _lib.lib()
    header = open(os.path.join(ROOT, "include", "suggest_hip.h"), encoding="utf-8").read()
    for name in NEW:
        assert name in _lib.EXPORTS and hasattr(L, name), name
        assert re.search(r"\b%s\s*\(" % name, header), name
    assert "#define SG_MAX_SHARDS 64u" in header and _lib.SG_MAX_SHARDS == 64
    assert "typedef struct sg_sharded sg_sharded;" in header
    for method in ("adopt", "suggest_batch", "suggest_batch_device", "autocomplete_batch", "shards", "close"):
        assert callable(getattr(ShardedIndex, method))


def _host_index(docs):
    from suggest_amd import IndexDescription, NGramIndex, synth
    return NGramIndex(docs, IndexDescription(**synth.DESCRIPTION), upload=False)


def test_bad_arguments_are_invalid_without_a_gpu():
    from suggest_amd import _lib
    from suggest_amd.index import IndexDescription, _c_desc
    from suggest_amd import synth
    L = _lib.lib()
    INVALID = -1
    err = lambda: L.sg_last_error().decode()                                   # noqa: E731
    out = C.c_void_p()
    desc = _c_desc(IndexDescription(**synth.DESCRIPTION))
    offs = np.array([0, 3, 6], dtype=np.uint64)
    blob = np.frombuffer(b"abcdef", dtype=np.uint8).copy()
    dev = (C.c_int * 1)(0)
    ids = np.zeros(8, dtype=np.uint32); sc = np.zeros(8, dtype=np.float64); cnt = np.zeros(8, dtype=np.uint32)
    # null handle, null offsets, k == 0
    assert L.sg_sharded_suggest_batch(None, blob.ctypes.data, offs.ctypes.data, 2, 0, 0.5, 4, ids.ctypes.data, sc.ctypes.data, cnt.ctypes.data) == INVALID
    assert L.sg_sharded_suggest_batch_device(None, None, None, 2, 0, 0.5, 4, None, None, None, None) == INVALID
    assert L.sg_sharded_autocomplete_batch(None, blob.ctypes.data, offs.ctypes.data, 2, 4, ids.ctypes.data, cnt.ctypes.data) == INVALID
    assert L.sg_sharded_shards(None, None, None, 0) == 0
    L.sg_sharded_retain(None); L.sg_sharded_release(None)
    assert L.sg_sharded_build(blob.ctypes.data, None, 2, C.byref(desc), 2, dev, 1, -1, C.byref(out)) == INVALID
    assert L.sg_sharded_build(blob.ctypes.data, offs.ctypes.data, 2, C.byref(desc), 2, None, 1, -1, C.byref(out)) == INVALID
    assert L.sg_sharded_build(blob.ctypes.data, offs.ctypes.data, 2, C.byref(desc), 2, dev, 0, -1, C.byref(out)) == INVALID
    assert L.sg_sharded_build(blob.ctypes.data, offs.ctypes.data, 2, C.byref(desc), 2, dev, 1, -1, None) == INVALID
    # n_shards of 0 or 65
    for n_shards in (0, 65):
        assert L.sg_sharded_build(blob.ctypes.data, offs.ctypes.data, 2, C.byref(desc), n_shards, dev, 1, -1, C.byref(out)) == INVALID
        assert "n_shards" in err()
    a, b = _host_index([b"alpha", b"beta"]), _host_index([b"gamma", b"delta", b"epsilon"])
    hs = (C.c_void_p * 65)(*([a._h.value, b._h.value] + [a._h.value] * 63))
    lo = np.zeros(65, dtype=np.uint64)
    for n_shards in (0, 65):
        assert L.sg_sharded_adopt(hs, lo.ctypes.data, n_shards, C.byref(out)) == INVALID and "n_shards" in err()
    assert L.sg_sharded_adopt(None, lo.ctypes.data, 2, C.byref(out)) == INVALID
    assert L.sg_sharded_adopt(hs, None, 2, C.byref(out)) == INVALID
    assert L.sg_sharded_adopt(hs, lo.ctypes.data, 2, None) == INVALID

    def adopt(doc_lo):
        x = np.asarray(doc_lo, dtype=np.uint64)
        rc = L.sg_sharded_adopt(hs, x.ctypes.data, 2, C.byref(out))
        return rc, err()
    rc, msg = adopt([5, 3]);                       assert rc == INVALID and "ascend" in msg            # doc_lo that descends
    rc, msg = adopt([0, 1]);                       assert rc == INVALID and "overlap" in msg           # a has two documents
    rc, msg = adopt([0, 2 ** 32 - 2]);             assert rc == INVALID and "2^32" in msg              # b has three
    rc, msg = adopt([2 ** 32 + 1, 2 ** 32 + 9]);   assert rc == INVALID and "2^32" in msg
    rc, msg = adopt([0, 2 ** 32 - 3]);             assert rc == INVALID and "not uploaded" in msg      # the ranges pass: the next check speaks
    assert not out.value
    # the kernel's direct hook: k == 0, too many shards, null arrays
    one = np.zeros((1, 1, 1), dtype=np.uint32)
    args = lambda W, k: (0, one.ctypes.data, sc.ctypes.data, cnt.ctypes.data, lo.ctypes.data, W, 1, k, 0, ids.ctypes.data, sc.ctypes.data, cnt.ctypes.data)   # noqa: E731
    assert L.sg_debug_shard_merge(*args(1, 0)) == INVALID
    assert L.sg_debug_shard_merge(*args(65, 1)) == INVALID
    assert L.sg_debug_shard_merge(*args(0, 1)) == INVALID
    assert L.sg_debug_shard_merge(0, None, sc.ctypes.data, cnt.ctypes.data, lo.ctypes.data, 1, 1, 1, 0, ids.ctypes.data, sc.ctypes.data, cnt.ctypes.data) == INVALID
    assert L.sg_debug_shard_merge(0, one.ctypes.data, None, cnt.ctypes.data, lo.ctypes.data, 1, 1, 1, 0, ids.ctypes.data, sc.ctypes.data, cnt.ctypes.data) == INVALID
    assert L.sg_debug_shard_slice_bytes(4096) == 0 and L.sg_debug_shard_slice_bytes(0) == 0


def test_go_shim_arities_match_the_header():
    """go/suggesthip/suggesthip.go has never met a Go compiler: the new calls pass as many arguments as the header declares"""
    go = open(os.path.join(ROOT, "go", "suggesthip", "suggesthip.go"), encoding="utf-8").read()
    header = open(os.path.join(ROOT, "include", "suggest_hip.h"), encoding="utf-8").read()
    for fn in ("sg_sharded_build", "sg_sharded_adopt", "sg_sharded_suggest_batch", "sg_sharded_autocomplete_batch", "sg_sharded_release", "sg_sharded_retain"):
        decl = re.search(r"(?:int|void) %s\(([^;]*)\);" % fn, header).group(1)
        call = re.search(r"C\.%s\(([^\n]*)\)\n" % fn, go)
        assert call, fn
        depth, n = 0, 1
        for ch in call.group(1):
            depth += ch in "([{"
            depth -= ch in ")]}"
            n += ch == "," and depth == 0
        assert n == decl.count(",") + 1, fn
    for sig in ("func BuildSharded(", "func AdoptSharded(", "func (s *Sharded) SuggestBatch(", "func (s *Sharded) AutocompleteBatch(", "func (s *Sharded) Close() error"):
        assert sig in go, sig


def test_cpp_sharded_index_compiles(tmp_path):
    src = tmp_path / "sharded.cpp"
    src.write_text('#include "suggest_hip.hpp"\n'
                   'size_t f(const std::shared_ptr<suggest::dictionary::Dictionary>& d, const suggest::IndexDescription& desc,\n'
                   '         const std::vector<std::shared_ptr<suggest::NGramIndex>>& parts) {\n'
                   '  suggest::ShardedIndex a(d, desc, 4, {0, 1}, true);\n'
                   '  auto b = suggest::ShardedIndex::Adopt(parts, {0, 4000000000ull});\n'
                   '  auto r = a.Suggest("query", 0.5, suggest::metric::CosineMetric(), 10);\n'
                   '  auto c = b->Autocomplete("que", 5);\n'
                   '  auto rb = a.SuggestBatch({"x", "y"}, 0.5, suggest::metric::JaccardMetric(), 3);\n'
                   '  auto cb = b->AutocompleteBatch({"x"}, 3);\n'
                   '  return r.size() + c.size() + rb.size() + cb.size() + a.Shards().size() + (a.Handle() != nullptr);\n'
                   '}\n')
    r = subprocess.run(["g++", "-std=c++17", "-Wall", "-fsyntax-only", "-I" + os.path.join(ROOT, "include"), str(src)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
