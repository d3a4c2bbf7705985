"""CPU-only checks of the complete search by edit distance (sg_edit_index / sg_edit_search, include/suggest_hip.h):
the host-resident index through the C ABI and the Python binding on the shared shapes, equal to the brute force of
tests/edit_search_ref.py word for word; the index's two arrays against their restatement; the soundness of the two bounds as a
property over random pairs; every refusal that needs no GPU."""
import ctypes as C

import numpy as np
import pytest

import edit_ref as ref
import edit_search_ref as sref
import edit_search_shapes as shp

NEW = ("sg_edit_index_create", "sg_edit_index_retain", "sg_edit_index_release", "sg_edit_search_device", "sg_edit_search", "sg_debug_edit_index_array",
       "sg_debug_edit_search_slices", "sg_debug_edit_search_bytes")
CONFIGS = [(m, f) for m in ref.MODES for f in (True, False)]
GUARD = 8


def _host_index(lines, fold):
    from suggest_amd.dictionary import DeviceDictionary
    return DeviceDictionary(lines, device=-1).edit_index(fold_case=fold)


def _call(ix, queries, k, max_distance, mode="levenshtein", fold=None, null=None, hist=True):
    """sg_edit_search itself, guard words behind every output -> (rc, message, ids, dist, counts, hist)"""
    from suggest_amd import _lib
    from suggest_amd.index import pack_strings
    L = _lib.lib()
    qb, qo = pack_strings(queries)
    n_q = len(queries)
    bins = min(max_distance, 32) + 1
    ids = np.full(n_q * k + GUARD, 0xEEEEEEEE, dtype=np.uint32)
    dist = np.full(n_q * k + GUARD, 0xEEEEEEEE, dtype=np.uint32)
    counts = np.full(n_q + GUARD, 0xEEEEEEEE, dtype=np.uint32)
    h = np.full(n_q * bins + GUARD, 0xEEEEEEEE, dtype=np.uint32)
    cfg = _lib.SgEditConfig(_lib.SG_EDIT_OSA if mode == "osa" else (0 if mode == "levenshtein" else mode), int(ix.fold_case if fold is None else fold),
                            max_distance, 0)
    a = dict(cfg=C.byref(cfg), q_offs=qo.ctypes.data, ids=ids.ctypes.data, dist=dist.ctypes.data, counts=counts.ctypes.data)
    if null:
        a[null] = None
    with ix._use() as handle:
        rc = L.sg_edit_search(None if null == "index" else handle, a["cfg"], qb.ctypes.data if qb.size else None, a["q_offs"], n_q, k, a["ids"], a["dist"],
                              a["counts"], h.ctypes.data if hist else None)
    for arr, n in ((ids, n_q * k), (dist, n_q * k), (counts, n_q), (h, n_q * bins)):
        assert np.all(arr[n:] == 0xEEEEEEEE), "words behind an output were written"
    return rc, L.sg_last_error().decode(), ids[:n_q * k].reshape(n_q, k), dist[:n_q * k].reshape(n_q, k), counts[:n_q], h[:n_q * bins].reshape(n_q, bins)


def _assert_equal(got, want, what):
    for g, w, name in zip(got, want, ("ids", "dist", "counts", "hist")):
        bad = np.argwhere(g != w)
        assert bad.size == 0, (what, name, bad[:4].tolist(), g[tuple(bad[0])], w[tuple(bad[0])])


@pytest.mark.parametrize("mode,fold", CONFIGS)
def test_host_index_equals_brute_force_on_the_dense_dictionary(mode, fold):
    lines = shp.dense_lines()
    queries = shp.dense_queries(lines)
    dm = shp.matrix("dense", lines, queries, mode, fold)
    ix = _host_index(lines, fold)
    for md in shp.MAX_DISTANCES:
        for k in shp.KS:
            rc, msg, *got = _call(ix, queries, k, md, mode)
            assert rc == 0, msg
            _assert_equal(got, sref.search(dm, k, md), (md, k))
    ids, dist, counts, hist = ix.search(queries, 7, 2, transpositions=mode == "osa")            # the binding
    _assert_equal((ids, dist, counts, hist), sref.search(dm, 7, 2), "binding")
    assert counts[3] == sref.TOO_LONG and not ids[3].any() and not hist[3].any() and counts[2] == 0           # 65 runes flagged, 64 answered


@pytest.mark.parametrize("mode", ref.MODES)
def test_host_index_ties_and_transpositions(mode):
    lines = shp.tie_lines()
    dm = sref.distance_matrix(shp.TIE_QUERIES, lines, mode, True)
    ix = _host_index(lines, True)
    for k in shp.TIE_KS:
        rc, msg, *got = _call(ix, shp.TIE_QUERIES, k, 2, mode)
        assert rc == 0, msg
        _assert_equal(got, sref.search(dm, k, 2), k)
    lines, queries = shp.transposition_cases()
    rc, msg, *got = _call(_host_index(lines, True), queries, 4, 1, mode)
    _assert_equal(got, sref.search(sref.distance_matrix(queries, lines, mode, True), 4, 1), "transpositions")
    assert got[2].tolist() == [1 if mode == "osa" else 0] * len(lines)


def test_host_index_on_cars(cars_lines):
    lines = [bytes(l) for l in cars_lines]
    queries = shp.cars_queries(lines)
    dm = shp.matrix("cars", lines, queries, "levenshtein", True)
    rc, msg, *got = _call(_host_index(lines, True), queries, 10, 2, hist=True)
    assert rc == 0, msg
    _assert_equal(got, sref.search(dm, 10, 2), "cars")
    rc, msg, ids, dist, counts, _ = _call(_host_index(lines, True), queries[:20], 10, 2, hist=False)       # without histograms
    assert rc == 0 and np.array_equal(ids, got[0][:20]) and np.array_equal(counts, got[2][:20])


@pytest.mark.parametrize("fold", [True, False])
@pytest.mark.parametrize("n_docs", shp.ARRAY_SIZES)
def test_the_arrays_equal_the_restatement(n_docs, fold):
    lines = shp.array_lines(n_docs)
    ix = _host_index(lines, fold)
    runes, sig = sref.arrays(lines, fold)
    assert np.array_equal(ix.array("runes"), runes) and np.array_equal(ix.array("sig"), sig)


@pytest.mark.parametrize("mode", ref.MODES)
def test_neither_bound_exceeds_the_distance(mode):
    """the soundness of the filter: over random pairs — copies with a few edits, transpositions among them, and unrelated strings,
    alphabets of 3 to 5 000 runes — max(length bound, signature bound) <= distance"""
    tight = 0
    for a, b in shp.rune_pairs(4000):
        d = ref.distance_runes(a, b, mode)
        by_len, by_sig = sref.bounds(a, b)
        assert by_len <= d and by_sig <= d, (a, b, d, by_len, by_sig)
        tight += max(by_len, by_sig) == d and d > 0
    assert tight > 100                                             # (and the bounds are not vacuous)


def test_the_65_rune_flag_and_the_limits_of_a_query():
    lines = [b"a" * 64, b"a" * 65, b"", "é".encode() * 64]
    ix = _host_index(lines, True)
    queries = [b"a" * 64, b"a" * 65, "é".encode() * 64, "é".encode() * 65, b"\xff" * 64, b"\xff" * 65, b"", b"a" * 300]
    rc, msg, ids, dist, counts, hist = _call(ix, queries, 3, 32)
    assert rc == 0, msg
    _assert_equal((ids, dist, counts, hist), sref.search(sref.distance_matrix(queries, lines, "levenshtein", True), 3, 32), "limits")
    assert counts.tolist() == [2, sref.TOO_LONG, 1, sref.TOO_LONG, 0, sref.TOO_LONG, 1, sref.TOO_LONG]
    assert ids[0].tolist() == [0, 1, 0] and dist[0].tolist() == [0, 1, 0] and hist[0].tolist() == [1, 1] + [0] * 31
    assert ids[2].tolist() == [3, 0, 0] and ids[6].tolist() == [2, 0, 0] and dist[6].tolist() == [0, 0, 0]      # the empty query: the document's rune count
    for i in (1, 3, 5, 7):
        assert not ids[i].any() and not dist[i].any() and not hist[i].any()


def test_refusals_that_need_no_gpu():
    from suggest_amd import _lib
    L = _lib.lib()
    ix = _host_index([b"nissan", b"toyota"], True)
    qs = ["nisan", "toyta"]
    assert _call(ix, qs, 3, 2, fold=False)[:2] == (-1, "edit search: fold_case differs from the index's")
    assert _call(_host_index([b"nissan"], False), qs, 3, 2, fold=True)[0] == -1
    for md in (33, 0xFFFFFFFF):
        assert _call(ix, qs, 3, md)[:2] == (-1, "edit search: max_distance above 32")
    for k in (0, 1025):
        assert _call(ix, qs, k, 2)[:2] == (-1, "edit search: k should be in 1 .. 1024")
    assert _call(ix, qs, 1024, 32)[0] == 0
    assert _call(ix, qs, 3, 2, mode=2)[:2] == (-1, "unknown edit mode")
    for name in ("cfg", "q_offs", "ids", "dist", "counts"):
        assert _call(ix, qs, 3, 2, null=name)[:2] == (-1, "null argument"), name
    assert _call(ix, qs, 3, 2, null="index")[:2] == (-1, "null edit index")
    h = C.c_void_p()
    assert L.sg_edit_index_create(None, 1, C.byref(h)) == -1 and L.sg_last_error() == b"null dictionary"
    with ix.dictionary._use() as dh:
        assert L.sg_edit_index_create(dh, 1, None) == -1
    n = C.c_uint64()
    with ix._use() as handle:
        cfg = ix.config(2)
        x = np.zeros(64, dtype=np.uint64).ctypes.data   # (a host address stands in for device ones: refused before a pointer is followed)
        assert L.sg_edit_search_device(handle, C.byref(cfg), x, x, 2, 3, x, x, x, None, None) == -2 and b"host-resident" in L.sg_last_error()
        assert L.sg_edit_search_device(handle, C.byref(cfg), x, x, 2, 0, x, x, x, None, None) == -1
        assert L.sg_edit_search(handle, C.byref(cfg), None, None, 0, 3, None, None, None, None) == 0             # nothing to do
        assert L.sg_debug_edit_index_array(handle, 2, None, 0, C.byref(n)) == -1
        assert L.sg_debug_edit_index_array(handle, 1, None, 0, C.byref(n)) == 0 and n.value == 16
        assert L.sg_debug_edit_index_array(handle, 1, x, 8, C.byref(n)) == -1 and b"too small" in L.sg_last_error()
    assert L.sg_debug_edit_index_array(None, 0, None, 0, C.byref(n)) == -1
    assert L.sg_debug_edit_search_slices(3) == 0 and L.sg_debug_edit_search_slices(0) == 0
    assert L.sg_debug_edit_search_bytes(1 << 20) == 0 and L.sg_debug_edit_search_bytes(0) == 0
    offs = np.array([0, 3, 2], dtype=np.uint64)
    out = np.zeros(16, dtype=np.uint32)
    with ix._use() as handle:
        assert L.sg_edit_search(handle, C.byref(cfg), out.ctypes.data, offs.ctypes.data, 2, 3, out.ctypes.data, out.ctypes.data, out.ctypes.data, None) == -1
        assert L.sg_last_error() == b"query offsets must not decrease"


def test_the_index_retains_its_dictionary():
    from suggest_amd.dictionary import DeviceDictionary
    d = DeviceDictionary([b"nissan", b"toyota", b"nisan"], device=-1)
    ix = d.edit_index()
    d.close()                                                      # the index holds its own reference
    ids, dist, counts, hist = ix.search(["Nissan"], 5, 1)
    assert ids.tolist() == [[0, 2, 0, 0, 0]] and dist.tolist() == [[0, 1, 0, 0, 0]] and counts.tolist() == [2] and hist.tolist() == [[1, 1]]
    ix.close()
    with pytest.raises(ValueError):
        ix.search(["x"], 1, 1)


def test_python_bindings():
    from suggest_amd import EditIndex, _lib
    assert set(NEW) <= set(_lib.EXPORTS) and all(hasattr(_lib.lib(), n) for n in NEW)
    ix = _host_index([b"nissan", b"toyota", b"Toyota"], False)
    assert isinstance(ix, EditIndex) and (ix.n_docs, ix.device, ix.fold_case) == (3, -1, False)
    ids, dist, counts, hist = ix.search(["toyoat"], 2, 2, transpositions=True)
    assert (ids.tolist(), dist.tolist(), counts.tolist(), hist.tolist()) == ([[1, 2]], [[1, 2]], [2], [[0, 1, 1]])
    assert ix.search(["toyoat"], 2, 1)[2].tolist() == [0]


def test_cpp_mirror_runs_in_cpu_mode():
    import os
    import subprocess
    from conftest import GOLDEN, ROOT
    binary = os.path.join(ROOT, "tests", "cpp", "_build", "edit_search_test")
    if not os.path.exists(binary):
        subprocess.check_call(["make", "-C", os.path.join(ROOT, "tests", "cpp"), "-f", "edit_search.mk"], stdout=subprocess.DEVNULL)
    r = subprocess.run([binary, "--cpu", GOLDEN], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "0 failed" in r.stdout, (r.returncode, r.stdout, r.stderr)


def test_go_shim_arity_matches_the_header():
    import os
    import re
    from conftest import ROOT
    go = open(os.path.join(ROOT, "go", "suggesthip", "suggesthip.go"), encoding="utf-8").read()
    header = open(os.path.join(ROOT, "include", "suggest_hip.h"), encoding="utf-8").read()
    for name, want in (("sg_edit_search", 10), ("sg_edit_index_create", 3)):
        decl = re.search(r"int %s\(([^;]*)\);" % name, header).group(1)
        call = re.search(r"C\.%s\(([^\n]*)\)\n" % name, go)
        assert call, name
        depth, n = 0, 1
        for ch in call.group(1):
            depth += ch in "([{"
            depth -= ch in ")]}"
            n += ch == "," and depth == 0
        assert n == decl.count(",") + 1 == want, name
    assert "func (d *DeviceDictionary) EditSearch(" in go
