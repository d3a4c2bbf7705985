"""The complete search by edit distance on the device (suggest_amd/csrc/edit_search.inc).  Every test compares ids,
distances, counts and histograms with the brute force of tests/edit_search_ref.py for equality, on the shapes of
tests/edit_search_shapes.py (asserted to be hard by tests/test_edit_search_shapes_cpu.py)."""
import contextlib
import threading

import numpy as np
import pytest

import edit_ref as ref
import edit_search_ref as sref
import edit_search_shapes as shp
from conftest import CARS_DESC

pytestmark = pytest.mark.gpu

CONFIGS = [(m, f) for m in ref.MODES for f in (True, False)]
GUARD = 16


@pytest.fixture(scope="module")
def torch():
    import torch  # (before the library: both must resolve the same libamdhip64, suggest_amd/_lib.py)
    return torch


@pytest.fixture(scope="module")
def dense(torch):
    from suggest_amd.dictionary import DeviceDictionary
    lines = shp.dense_lines()
    dd = DeviceDictionary(lines, device=0)
    return dict(lines=lines, queries=shp.dense_queries(lines), dd=dd, ix={f: dd.edit_index(fold_case=f) for f in (True, False)})


@contextlib.contextmanager
def forced(slices=0, row_bytes=0):
    from suggest_amd import _lib
    L = _lib.lib()
    assert L.sg_debug_edit_search_slices(slices) == 0 and L.sg_debug_edit_search_bytes(row_bytes) == 0
    try:
        yield
    finally:
        L.sg_debug_edit_search_slices(0)
        L.sg_debug_edit_search_bytes(0)


def _assert_equal(got, want, what):
    for g, w, name in zip(got, want, ("ids", "dist", "counts", "hist")):
        g, w = np.asarray(g).reshape(w.shape), np.asarray(w)
        bad = np.argwhere(g != w)
        assert bad.size == 0, (what, name, bad[:4].tolist(), g[tuple(bad[0])], w[tuple(bad[0])])


def _to_dev(torch, a):
    a = np.ascontiguousarray(a)
    view = {np.dtype(np.uint32): np.int32, np.dtype(np.uint64): np.int64, np.dtype(np.uint8): np.uint8}[a.dtype]
    return torch.from_numpy(a.view(view).copy()).to("cuda:0")


def _device(torch, ix, queries, k, max_distance, transpositions=False, stream=None, hist=True):
    """sg_edit_search_device on tensors, guard words behind every output -> (ids, dist, counts, hist or None)"""
    from suggest_amd.index import pack_strings
    qb, qo = pack_strings(queries)
    n_q, bins = len(queries), max_distance + 1
    d_q, d_qo = _to_dev(torch, qb if qb.size else np.zeros(1, dtype=np.uint8)), _to_dev(torch, qo)
    outs = [torch.full((n + GUARD,), 0x6E6E6E6E, dtype=torch.int32, device="cuda:0") for n in (n_q * k, n_q * k, n_q, n_q * bins)]
    torch.cuda.synchronize()
    ix.search_device(ix.config(max_distance, transpositions), d_q.data_ptr(), d_qo.data_ptr(), n_q, k, outs[0].data_ptr(), outs[1].data_ptr(),
                     outs[2].data_ptr(), outs[3].data_ptr() if hist else None, stream=0 if stream is None else stream.cuda_stream)
    torch.cuda.synchronize()
    res = []
    for t, n in zip(outs, (n_q * k, n_q * k, n_q, n_q * bins)):
        a = t.cpu().numpy().view(np.uint32)
        assert np.all(a[n:] == 0x6E6E6E6E), "words behind an output were written"
        res.append(a[:n])
    if not hist:
        assert np.all(res[3] == 0x6E6E6E6E)
    return res[0].reshape(n_q, k), res[1].reshape(n_q, k), res[2], res[3].reshape(n_q, bins) if hist else None


# ---- 1: the two arrays, word for word ----
@pytest.mark.parametrize("fold", [True, False])
@pytest.mark.parametrize("n_docs", shp.ARRAY_SIZES)
def test_the_arrays_equal_the_restatement(torch, n_docs, fold):
    from suggest_amd.dictionary import DeviceDictionary
    lines = shp.array_lines(n_docs)
    ix = DeviceDictionary(lines, device=0).edit_index(fold_case=fold)
    runes, sig = sref.arrays(lines, fold)
    assert np.array_equal(ix.array("runes"), runes) and np.array_equal(ix.array("sig"), sig)
    queries = [b"", b"x" + "ä".encode(), lines[n_docs // 2], shp.LONG70[:64].encode()]       # ... and a search over them
    dm = sref.distance_matrix(queries, lines, "osa", fold)
    _assert_equal(ix.search(queries, 7, 5, transpositions=True), sref.search(dm, 7, 5), (n_docs, fold))


# ---- 2: the dense dictionary ----
@pytest.mark.parametrize("slices", shp.SLICES)
@pytest.mark.parametrize("mode,fold", CONFIGS)
def test_dense_dictionary(torch, dense, mode, fold, slices):
    """64 queries — empty, one rune, 64 runes, 65 runes (flagged), invalid bytes, another case — x max_distance 0, 1, 2, 5, 32 x
    k 1, 7, 64, 1 024: the cut inside a group of equal distances that spans slices, rows with fewer than k matches; under the poison"""
    from suggest_amd import _lib
    dm = shp.matrix("dense", dense["lines"], dense["queries"], mode, fold)
    ix = dense["ix"][fold]
    with forced(slices=slices), _lib.poisoned(1):
        for md in shp.MAX_DISTANCES:
            for k in shp.KS:
                want = sref.search(dm, k, md)
                _assert_equal(ix.search(dense["queries"], k, md, transpositions=mode == "osa"), want, (md, k, "host buffers"))
                if k in (7, 1024):
                    _assert_equal(_device(torch, ix, dense["queries"], k, md, mode == "osa"), want, (md, k, "device"))
    assert want[2][3] == sref.TOO_LONG


def test_automatic_slices_and_no_histogram(torch, dense):
    dm = shp.matrix("dense", dense["lines"], dense["queries"], "levenshtein", True)
    want = sref.search(dm, 10, 2)
    _assert_equal(dense["ix"][True].search(dense["queries"], 10, 2), want, "automatic")
    ids, dist, counts, _ = _device(torch, dense["ix"][True], dense["queries"], 10, 2, hist=False)
    _assert_equal((ids, dist, counts), want[:3], "no histogram")
    with pytest.raises(Exception):
        dense["ix"][False].search_device(dense["ix"][True].config(2), 0, 0, 1, 1, 0, 0, 0)      # fold_case differs: refused before a pointer is followed


# ---- 3: ties by docID ----
@pytest.mark.parametrize("k", shp.TIE_KS)
def test_ties_by_doc_id(torch, k):
    from suggest_amd.dictionary import DeviceDictionary
    lines = shp.tie_lines()
    ix = DeviceDictionary(lines, device=0).edit_index()
    with forced(slices=7):
        for mode in ref.MODES:
            dm = shp.matrix("ties", lines, shp.TIE_QUERIES, mode, True)
            got = ix.search(shp.TIE_QUERIES, k, 2, transpositions=mode == "osa")
            _assert_equal(got, sref.search(dm, k, 2), (k, mode))
    assert got[2][0] == k and np.all(got[1][0] == 0) and np.all(np.diff(got[0][0].astype(np.int64)) > 0)      # k copies, docID ascending


# ---- 4: the two modes ----
def test_osa_and_levenshtein_differ_on_transpositions(torch):
    from suggest_amd.dictionary import DeviceDictionary
    lines, queries = shp.transposition_cases()
    ix = DeviceDictionary(lines, device=0).edit_index()
    rows = {}
    for mode in ref.MODES:
        rows[mode] = ix.search(queries, 4, 1, transpositions=mode == "osa")
        _assert_equal(rows[mode], sref.search(sref.distance_matrix(queries, lines, mode, True), 4, 1), mode)
    assert not np.array_equal(rows["osa"][2], rows["levenshtein"][2]) and not np.array_equal(rows["osa"][0], rows["levenshtein"][0])


# ---- 5: chunks ----
def test_chunked_call_equals_the_unchunked(torch, dense):
    """the row budget lowered to 96 queries' rows: 300 queries take four chunks"""
    queries = shp.chunk_queries(dense["lines"])
    k, slices = 7, 2
    dm = shp.matrix("chunks", dense["lines"], queries, "levenshtein", True)
    want = sref.search(dm, k, 2)
    with forced(slices=slices):
        whole = dense["ix"][True].search(queries, k, 2)
    per_query = (1 + slices) * (k * 8 + 4)
    assert len(queries) == 300 and -(-len(queries) // 100) >= 3           # a budget of 100 queries' rows: three chunks at least
    with forced(slices=slices, row_bytes=100 * per_query):
        chunked = dense["ix"][True].search(queries, k, 2)
        chunked_dev = _device(torch, dense["ix"][True], queries, k, 2)
    _assert_equal(whole, want, "whole")
    _assert_equal(chunked, whole, "chunked")
    _assert_equal(chunked_dev, whole, "chunked, device")
    with forced(slices=7, row_bytes=1):                          # a query per chunk
        _assert_equal(dense["ix"][True].search(queries[:20], k, 2), [w[:20] for w in want], "a query per chunk")


# ---- 6: cars.dict: what the candidate route misses ----
def test_cars_holds_every_match_the_candidate_route_missed(torch, cars_lines):
    from suggest_amd import IndexDescription, NGramIndex
    from suggest_amd.dictionary import DeviceDictionary
    lines = [bytes(l) for l in cars_lines]
    queries = shp.cars_queries(lines)
    dm = shp.matrix("cars", lines, queries, "levenshtein", True)
    dd = DeviceDictionary(lines, device=0)
    ix = dd.edit_index()
    for k in (10, 1024):
        got = ix.search(queries, k, 2)
        _assert_equal(got, sref.search(dm, k, 2), k)
    ids, dist, counts, hist = got
    nx = NGramIndex(cars_lines, IndexDescription(**CARS_DESC))
    c_ids, _, _, c_cnt = nx.suggest_batch_edit(dd, queries, "jaccard", 0.5, 16, 16, mode="levenshtein", max_distance=2)
    nx.close()
    missed = 0
    for i in range(len(queries)):
        truth = set(np.nonzero(dm[i] <= 2)[0].tolist())
        cand = set(c_ids[i, :int(c_cnt[i])].tolist()) if c_cnt[i] < ref.COUNT_FLAG_MIN else set()
        assert cand <= truth
        assert truth - cand <= set(ids[i, :int(counts[i])].tolist()), i
        missed += len(truth - cand)
    assert missed >= 1


# ---- 7: threads ----
def test_two_threads_on_their_own_streams(torch, dense):
    """sg_edit_search_device writes nothing of the handle: two threads, a stream each, one index, the same batch"""
    want = sref.search(shp.matrix("dense", dense["lines"], dense["queries"], "osa", True), 64, 5)
    out, errors = [None, None], []

    def work(t):
        try:
            torch.cuda.set_device(0)
            st = torch.cuda.Stream()
            for _ in range(3):
                out[t] = _device(torch, dense["ix"][True], dense["queries"], 64, 5, True, stream=st)
        except Exception as e:  # noqa: BLE001
            errors.append(e)
    threads = [threading.Thread(target=work, args=(t,)) for t in range(2)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert not errors, errors
    for a, b in zip(out[0], out[1]):
        assert np.array_equal(a, b)
    _assert_equal(out[0], want, "threads")


# ---- 8: the rows as strings ----
def test_search_strings(torch, dense):
    dm = shp.matrix("dense", dense["lines"], dense["queries"], "levenshtein", True)
    ids, dist, counts, hist = sref.search(dm, 7, 2)
    rows, g_dist, g_counts, g_hist = dense["ix"][True].search_strings(dense["queries"], 7, 2)
    assert np.array_equal(g_dist, dist) and np.array_equal(g_counts, counts) and np.array_equal(g_hist, hist)
    for i, row in enumerate(rows):
        n = 0 if counts[i] == sref.TOO_LONG else int(counts[i])
        assert row == [dense["lines"][int(d)] for d in ids[i, :n]], i
    assert sum(len(r) for r in rows) > 100


def test_cpp_mirror_on_the_device():
    import os
    import subprocess
    from conftest import GOLDEN, ROOT
    binary = os.path.join(ROOT, "tests", "cpp", "_build", "edit_search_test")
    if not os.path.exists(binary):
        subprocess.check_call(["make", "-C", os.path.join(ROOT, "tests", "cpp"), "-f", "edit_search.mk"], stdout=subprocess.DEVNULL)
    r = subprocess.run([binary, GOLDEN], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "0 failed" in r.stdout, (r.returncode, r.stdout, r.stderr)
