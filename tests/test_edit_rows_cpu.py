"""CPU-only checks of the edit-distance ranking (sg_edit_rows / sg_edit_rerank, include/suggest_hip.h): the
host-resident handle through the C ABI and the Python binding on the shared shapes, equal to tests/edit_ref.py word for word; the
kernels' own statement of the bit-vector recurrence run on the host (sg_debug_edit_bitvector); every refusal that needs no GPU."""
import ctypes as C

import numpy as np
import pytest

import edit_ref as ref
import edit_shapes as shp
from conftest import CARS_DESC

NEW = ("sg_edit_rows_device", "sg_edit_rows", "sg_edit_rerank_device", "sg_edit_rerank", "sg_suggest_batch_edit", "sg_debug_edit_slice_bytes",
       "sg_debug_edit_bitvector")
CONFIGS = [(m, f) for m in ref.MODES for f in (True, False)]


@pytest.fixture(scope="module")
def shapes():
    return shp.build()


@pytest.fixture(scope="module")
def host_dict(shapes):
    from suggest_amd.dictionary import DeviceDictionary
    return DeviceDictionary(shapes["lines"], device=-1)


def _call(d, queries, ids, counts, mode="levenshtein", fold=True, row=None, row_offs=None, slots=None, scores=None, rerank=False, k_out=1, max_distance=None,
          null=None):
    """sg_edit_rows / sg_edit_rerank themselves -> (rc, message, dist, ids, scores, counts)"""
    from suggest_amd import _lib
    from suggest_amd.dictionary import edit_config
    from suggest_amd.index import pack_strings
    L = _lib.lib()
    qb, qo = pack_strings(queries)
    ids = np.array(ids, dtype=np.uint32)
    if row is None:
        row = 0 if row_offs is not None else (ids.shape[1] if ids.ndim == 2 else 0)
    ids = ids.reshape(-1)
    counts = np.array(counts, dtype=np.uint32)
    slots = ids.size if slots is None else slots
    ro = None if row_offs is None else np.ascontiguousarray(row_offs, dtype=np.uint64)
    sc = None if scores is None else np.array(scores, dtype=np.float64).reshape(-1)
    dist = np.full(slots + 8, 0xEEEEEEEE, dtype=np.uint32)
    cfg = edit_config(mode, fold, max_distance) if isinstance(mode, str) else _lib.SgEditConfig(mode, int(fold), ref.NONE, 0)
    a = dict(cfg=C.byref(cfg), q_offs=qo.ctypes.data, ids=ids.ctypes.data, counts=counts.ctypes.data, dist=dist.ctypes.data)
    if null:
        a[null] = None
    q = qb.ctypes.data if qb.size else None
    rop = None if ro is None else ro.ctypes.data
    with d._use() as h:
        if rerank:
            rc = L.sg_edit_rerank(h, a["cfg"], q, a["q_offs"], a["ids"], None if sc is None else sc.ctypes.data, a["counts"], rop, len(counts), row, slots, k_out,
                                  a["dist"])
        else:
            rc = L.sg_edit_rows(h, a["cfg"], q, a["q_offs"], a["ids"], a["counts"], rop, len(counts), row, slots, a["dist"])
    assert np.all(dist[slots:] == 0xEEEEEEEE), "words behind the distances were written"
    return rc, L.sg_last_error().decode(), dist[:slots], ids, sc, counts


def test_the_shapes_are_as_described(shapes):
    lines, nm = shapes["lines"], shapes["named"]
    assert [len(ref.decode(lines[nm[k]])) for k in ("empty", "one", "c64", "c300", "long4096")] == [0, 1, 64, 300, 4096]
    assert lines[-1].endswith(b"\xf0\x9f\x98") and ref.decode(lines[-1])[-3:] == [0xFFFD] * 3
    full = ref.runes(lines[nm["full64"]], True)
    assert len(set(full)) == 64 == len(full) and ref.runes(lines[nm["full64"]], False) == full          # a full table under either fold
    col = shapes["collide"]
    assert len({ref.peq_hash(r) for r in col + [ord("a")]}) == 1 and len(set(col)) == 8
    assert [len(ref.decode(shp.query_of(n))) for n in shp.QUERY_RUNES] == list(shp.QUERY_RUNES)
    assert ref.runes("\u212a", True) == (ord("k"),) and len("\u212a".encode()) == 3 and ref.runes("\u0130", True) == (ord("i"),)
    assert len(shapes["dense"]) * 60 >= 3000


@pytest.mark.parametrize("mode,fold", CONFIGS)
@pytest.mark.parametrize("case", ["lengths", "dense", "special"])
def test_host_handle_distances_equal_the_restatement(host_dict, shapes, case, mode, fold):
    queries, ids, counts = {"lengths": shp.length_cases, "dense": shp.dense_cases, "special": shp.special_cases}[case](shapes)
    want, outside = ref.edit_rows(queries, ids, counts, shapes["lines"], row=ids.shape[1], mode=mode, fold=fold)
    rc, msg, dist = _call(host_dict, queries, ids, counts, mode, fold)[:3]
    assert (rc, outside) == (0, 0), msg
    assert np.array_equal(dist, want)
    got = host_dict.edit_distances(queries, ids, counts, mode=mode, fold_case=fold)                 # the binding
    assert got.shape == ids.shape and np.array_equal(got.reshape(-1), want)


def test_the_long_pair_on_the_host(host_dict, shapes):
    q = shapes["lines"][shapes["named"]["long4096"]][::-1] + b"ab"
    ids = [[shapes["named"]["long4096"]]]
    for mode in ref.MODES:
        want = ref.edit_rows([q], ids, [1], shapes["lines"], row=1, mode=mode)[0]
        assert 0 < want[0] < 4096
        assert np.array_equal(_call(host_dict, [q], ids, [1], mode)[2], want)


@pytest.mark.parametrize("mode", ref.MODES)
def test_the_kernels_recurrence_on_the_host(mode):
    """edit_block_step / edit_long_column as the kernels run them, against the loops: the dense space, every query length of the
    shapes (one word, the last bit of the word, block carries), alphabets of 2, 3 and 200 runes"""
    from suggest_amd import _lib
    L = _lib.lib()
    rng = np.random.default_rng(31)
    out = C.c_uint32()

    def check(a, b):
        a32, b32 = np.array(a, dtype=np.uint32), np.array(b, dtype=np.uint32)
        assert L.sg_debug_edit_bitvector(_lib.SG_EDIT_OSA if mode == "osa" else 0, a32.ctypes.data if a32.size else None, a32.size,
                                         b32.ctypes.data if b32.size else None, b32.size, C.byref(out)) == 0
        assert out.value == ref.distance_runes(a, b, mode), (a, b)
    for _ in range(2000):
        check(rng.integers(0, 3, int(rng.integers(0, 10))).tolist(), rng.integers(0, 3, int(rng.integers(0, 10))).tolist())
    for m in (1, 2, 63, 64, 65, 66, 127, 128, 129, 191, 192, 193, 300):
        for alpha in (2, 3, 200):
            for n in (0, 1, 63, 64, 65, 130, 257):
                check(rng.integers(0, alpha, m).tolist(), rng.integers(0, alpha, n).tolist())
    col = shp.colliding_runes(8)
    check(col[:5] + [ord("a")], [ord("a")] + col[3:8] + col[:2])                 # colliding and absent runes
    check(list(range(0x4E00, 0x4E40)), list(range(0x4E07, 0x4E40)) + list(range(0x4E00, 0x4E07)))      # a full table
    a = rng.integers(0, 3, 1000).tolist()
    check(a, a[3:500] + a[520:] + [1, 2])


def _rerank_want(shapes, queries, ids, scores, counts, mode, fold, row=0, row_offs=None, max_distance=ref.NONE, k_out=None):
    dist, outside = ref.edit_rows(queries, ids, counts, shapes["lines"], row=row, row_offs=row_offs, mode=mode, fold=fold)
    return ref.rerank(ids, scores, dist, counts, row=row, row_offs=row_offs, max_distance=max_distance, k_out=k_out), outside


@pytest.mark.parametrize("row", [1, 64, 65, 300])
@pytest.mark.parametrize("max_distance,k_out", [(None, None), (1, None), (0, 3), (None, 7), (40, 1)])
def test_host_handle_rerank_rows(host_dict, shapes, row, max_distance, k_out):
    queries, ids, scores, counts = shp.row_cases(shapes, row)
    md = ref.NONE if max_distance is None else max_distance
    for mode, fold, sc in (("osa", True, scores), ("levenshtein", False, None)):                  # fuzzy rows; autocomplete rows (no scores)
        (w_ids, w_sc, w_d, w_c), outside = _rerank_want(shapes, queries, ids, sc, counts, mode, fold, row=row, max_distance=md, k_out=k_out)
        rc, msg, dist, g_ids, g_sc, g_c = _call(host_dict, queries, ids, counts, mode, fold, scores=sc, rerank=True, k_out=row if k_out is None else k_out,
                                                max_distance=max_distance)
        assert (rc, outside) == (0, 0), msg
        assert np.array_equal(g_ids, w_ids) and np.array_equal(dist, w_d) and np.array_equal(g_c, w_c)
        assert sc is None or np.array_equal(g_sc.view(np.uint64), w_sc.view(np.uint64))
        flagged = int(np.nonzero(counts >= ref.COUNT_FLAG_MIN)[0][0])
        assert np.array_equal(g_ids.reshape(-1, row)[flagged], ids[flagged]) and g_c[flagged] == counts[flagged]      # untouched
        assert np.all(dist.reshape(-1, row)[flagged] == ref.NONE)
    b_ids, b_sc, b_d, b_c = host_dict.edit_rerank(queries, ids, counts, scores=scores, k_out=k_out, mode="osa", max_distance=max_distance)
    (w_ids, w_sc, w_d, w_c), _ = _rerank_want(shapes, queries, ids, scores, counts, "osa", True, row=row, max_distance=md, k_out=k_out)
    assert b_ids.shape == ids.shape and np.array_equal(b_ids.reshape(-1), w_ids) and np.array_equal(b_d.reshape(-1), w_d) and np.array_equal(b_c, w_c)
    assert np.array_equal(b_sc.reshape(-1), w_sc)


def test_host_handle_ragged_rows(host_dict, shapes):
    queries, ids, scores, counts, ro, slots = shp.ragged_cases(shapes)
    want, outside = ref.edit_rows(queries, ids, counts, shapes["lines"], row_offs=ro)
    rc, msg, dist = _call(host_dict, queries, ids, counts, row_offs=ro, slots=slots)[:3]
    assert (rc, outside) == (0, 0) and np.array_equal(dist, want) and np.all(dist[int(ro[-1]):] == ref.NONE)
    (w_ids, w_sc, w_d, w_c), _ = _rerank_want(shapes, queries, ids, scores, counts, "levenshtein", True, row_offs=ro, max_distance=6, k_out=100)
    rc, msg, dist, g_ids, g_sc, g_c = _call(host_dict, queries, ids, counts, row_offs=ro, slots=slots, scores=scores, rerank=True, k_out=100, max_distance=6)
    assert rc == 0, msg
    assert np.array_equal(g_ids, w_ids) and np.array_equal(dist, w_d) and np.array_equal(g_c, w_c) and np.array_equal(g_sc, w_sc)
    assert np.array_equal(g_ids[int(ro[-1]):], ids[int(ro[-1]):])                       # the spare tail is no row's


def test_tie_order_and_the_distance_cut(host_dict, shapes):
    nm = shapes["named"]
    # equal distances keep (score descending, docID ascending) as the search left them; a row of equal distances is unchanged
    ids = [[nm["toyota"], nm["ATOYOT"], nm["toyota corolla"], nm["TOYOTA COROLLA"]], [nm["nissan"], nm["nsisan"], nm["niva"], nm["one"]]]
    sc = [[.9, .9, .5, .5], [.8, .7, .7, .1]]
    rc, msg, dist, g_ids, g_sc, g_c = _call(host_dict, ["toyota corola", "xxxxxx"], ids, [4, 4], "osa", True, scores=sc, rerank=True, k_out=4)
    assert rc == 0 and dist.tolist() == [1, 1, 7, 9, 6, 6, 6, 6] and g_c.tolist() == [4, 4]
    assert g_ids.tolist() == [ids[0][2], ids[0][3], ids[0][0], ids[0][1]] + ids[1] and g_sc.tolist() == [.5, .5, .9, .9, .8, .7, .7, .1]
    # strictly descending distances: the order is fully reversed
    rev = [[nm["c300"], nm["c64"], nm["nissan"], nm["one"]]]
    rc, msg, dist, g_ids, _, g_c = _call(host_dict, ["q"], rev, [4], rerank=True, k_out=4)
    assert rc == 0 and g_ids.tolist() == rev[0][::-1] and dist.tolist() == sorted(dist.tolist()) and len(set(dist.tolist())) == 4
    # a cut that removes every entry of a row
    rc, msg, dist, g_ids, g_sc, g_c = _call(host_dict, ["toyota corola", "xxxxxx"], ids, [4, 4], "osa", True, scores=sc, rerank=True, k_out=4, max_distance=1)
    assert rc == 0 and g_c.tolist() == [2, 0] and g_ids.tolist() == [ids[0][2], ids[0][3], 0, 0, 0, 0, 0, 0] and dist.tolist() == [1, 1, 0, 0, 0, 0, 0, 0]
    assert g_sc.tolist() == [.5, .5, 0, 0, 0, 0, 0, 0]


def test_an_id_outside_the_dictionary_is_counted_and_reported(host_dict, shapes):
    n = len(shapes["lines"])
    ids = [[shapes["named"]["nissan"], n, 0xFFFFFFFF, shapes["named"]["niva"]]]
    rc, msg, dist, *_ = _call(host_dict, ["nisan"], ids, [4])
    assert (rc, msg) == (-1, "docID outside the dictionary") and dist.tolist() == [1, ref.NONE, ref.NONE, 2]       # the rest is delivered
    rc, msg, dist, g_ids, _, g_c = _call(host_dict, ["nisan"], ids, [4], rerank=True, k_out=4)
    assert rc == -1 and g_ids.tolist() == [ids[0][0], ids[0][3], n, 0xFFFFFFFF] and dist.tolist() == [1, 2, ref.NONE, ref.NONE] and g_c.tolist() == [4]
    rc, msg, dist, g_ids, _, g_c = _call(host_dict, ["nisan"], ids, [4], rerank=True, k_out=4, max_distance=5)
    assert rc == -1 and g_ids.tolist() == [ids[0][0], ids[0][3], 0, 0] and g_c.tolist() == [2]
    assert _call(host_dict, ["nisan"], ids, [1])[0] == 0                                   # ids past the count are not looked at
    with pytest.raises(Exception):
        host_dict.edit_distances(["nisan"], np.array(ids, dtype=np.uint32), [4])


def test_refusals_that_need_no_gpu(host_dict, shapes):
    from suggest_amd import IndexDescription, NGramIndex, _lib
    from suggest_amd.dictionary import edit_config
    L = _lib.lib()
    ids = np.zeros((2, 3), dtype=np.uint32)
    qs = ["a", "b"]
    for rerank in (False, True):
        for name in ("cfg", "q_offs", "ids", "counts", "dist"):
            rc, msg = _call(host_dict, qs, ids, [1, 1], null=name, rerank=rerank)[:2]
            assert (rc, msg) == (-1, "null argument"), name
        assert _call(host_dict, qs, ids, [1, 1], mode=2, rerank=rerank)[:2] == (-1, "unknown edit mode")
        assert _call(host_dict, qs, ids, [1, 1], row=4, rerank=rerank)[:2] == (-1, "dictionary rows: slots is below n_rows * row")
        assert _call(host_dict, qs, ids.reshape(-1), [1, 1], row_offs=[0, 4, 3], rerank=rerank)[:2] == (-1, "row offsets must not decrease")
        assert _call(host_dict, qs, ids.reshape(-1), [1, 1], row_offs=[0, 4, 9], rerank=rerank)[:2] == (-1, "edit rows: slots is below the last row offset")
    assert _call(host_dict, qs, ids, [1, 1], rerank=True, k_out=0)[:2] == (-1, "k_out should be greater or equal to 1")
    assert _call(host_dict, [b"x" * 65537, "b"], ids, [1, 1])[:2] == (-1, "a query of more than 65536 bytes")
    assert _call(host_dict, [b"x" * 65536, "b"], ids, [0, 1])[0] == 0
    cfg = edit_config()
    assert L.sg_edit_rows(None, C.byref(cfg), None, None, None, None, None, 0, 0, 0, None) == -1 and L.sg_last_error() == b"null dictionary"
    with host_dict._use() as h:
        assert L.sg_edit_rows(h, C.byref(cfg), None, None, None, None, None, 0, 0, 0, None) == 0         # nothing to do
        x = ids.ctypes.data            # (host addresses stand in for device ones: everything here is refused before a pointer is followed)
        assert L.sg_edit_rows_device(h, C.byref(cfg), x, x, x, x, None, 2, 3, 6, x, x, None) == -2 and b"host-resident" in L.sg_last_error()
        assert L.sg_edit_rerank_device(h, C.byref(cfg), x, x, x, x, x, None, 2, 3, 6, 3, x, x, None) == -2
        assert L.sg_edit_rows_device(h, C.byref(cfg), x, x, x, x, None, 2, 3, 6, x, None, None) == -1
        assert L.sg_edit_rerank_device(h, C.byref(cfg), x, x, x, x, x, None, 2, 3, 6, 0, x, x, None) == -1
        assert L.sg_edit_rows_device(h, None, x, x, x, x, None, 2, 3, 6, x, x, None) == -1
    # search-and-rank checks what the plain search checks, in its order — the upload first — then its own arguments
    d = IndexDescription(ngram_size=CARS_DESC["ngram_size"], wrap=CARS_DESC["wrap"], pad=CARS_DESC["pad"], alphabet=CARS_DESC["alphabet"])
    ix = NGramIndex([b"nissan", b"toyota"], d, upload=False)
    with pytest.raises(_lib.SuggestHipError) as e:
        ix.suggest_batch_edit(host_dict, ["nisan"], "cosine", 0.5, 8, 3)
    assert e.value.code == -3
    assert L.sg_suggest_batch_edit(None, None, None, 0, 0, 0.5, 8, None, None, 3, None, None, None, None) == -1 and L.sg_last_error() == b"null index"
    with pytest.raises(ValueError):
        edit_config("damerau")
    assert L.sg_debug_edit_bitvector(7, None, 0, None, 0, C.byref(C.c_uint32())) == -1
    assert L.sg_debug_edit_slice_bytes(1 << 20) == 0 and L.sg_debug_edit_slice_bytes(0) == 0


def test_python_bindings():
    from suggest_amd import _lib
    from suggest_amd.dictionary import DeviceDictionary
    assert set(NEW) <= set(_lib.EXPORTS) and all(hasattr(_lib.lib(), n) for n in NEW)
    assert C.sizeof(_lib.SgEditConfig) == 16
    d = DeviceDictionary([b"nissan", b"toyota"], device=-1)
    assert d.edit_distances(["Nisan"], [[0, 1]], [2]).tolist() == [[1, 6]]
    assert d.edit_distances(["Nisan"], [[0, 1]], [2], fold_case=False).tolist() == [[2, 6]]
    ids, sc, dist, cnt = d.edit_rerank(["toyoat"], [[0, 1]], [2], scores=[[.9, .8]], mode="osa", max_distance=2)
    assert (ids.tolist(), sc.tolist(), dist.tolist(), cnt.tolist()) == ([[1, 0]], [[.8, 0]], [[1, 0]], [1])
    with pytest.raises(ValueError):
        d.edit_distances(["a", "b"], [[0, 1]], [2])


def test_cpp_mirror_runs_in_cpu_mode():
    import os
    import subprocess
    from conftest import GOLDEN, ROOT
    binary = os.path.join(ROOT, "tests", "cpp", "_build", "edit_rank_test")
    if not os.path.exists(binary):
        subprocess.check_call(["make", "-C", os.path.join(ROOT, "tests", "cpp"), "-f", "edit_rank.mk"], stdout=subprocess.DEVNULL)
    r = subprocess.run([binary, "--cpu", GOLDEN], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "0 failed" in r.stdout, (r.returncode, r.stdout, r.stderr)


def test_go_shim_arity_matches_the_header():
    """go/suggesthip/suggesthip.go has never met a Go compiler: its call passes as many arguments as the header declares"""
    import os
    import re
    from conftest import ROOT
    go = open(os.path.join(ROOT, "go", "suggesthip", "suggesthip.go"), encoding="utf-8").read()
    header = open(os.path.join(ROOT, "include", "suggest_hip.h"), encoding="utf-8").read()
    decl = re.search(r"int sg_suggest_batch_edit\(([^;]*)\);", header).group(1)
    call = re.search(r"C\.sg_suggest_batch_edit\(([^\n]*)\)\n", go)
    assert call
    depth, n = 0, 1
    for ch in call.group(1):
        depth += ch in "([{"
        depth -= ch in ")]}"
        n += ch == "," and depth == 0
    assert n == decl.count(",") + 1 == 14
    assert "func (i *Index) SuggestEdit(dict *DeviceDictionary, queries []string, similarity float64, m metric.Metric, k int, rerank EditDistance)" in go
    for field in ("mode", "fold_case", "max_distance"):
        assert "cfg.%s" % field in go and re.search(r"\b%s;" % field, header)


def test_search_config_rerank_and_result_item():
    from suggest_amd import EditDistance, ResultItem, SearchConfig, Service
    plain = ResultItem(0.5, "nissan")
    assert plain.distance is None and repr(plain) == "ResultItem(score=0.5, value='nissan')" and plain == ResultItem(0.5, "nissan")
    ranked = ResultItem(0.5, "nissan", 1)
    assert ranked.distance == 1 and repr(ranked) == "ResultItem(score=0.5, value='nissan', distance=1)" and ranked != plain and ranked == ResultItem(0.5, "nissan", 1)
    e = EditDistance()
    assert (e.candidates, e.transpositions, e.fold_case, e.max_distance, e.mode) == (64, False, True, None, "levenshtein")
    assert EditDistance(transpositions=True).mode == "osa"
    assert SearchConfig("q", 10, "jaccard", 0.5).rerank is None and SearchConfig("q", 10, "jaccard", 0.5, rerank=e).rerank is e
    for bad in (lambda: EditDistance(candidates=0), lambda: EditDistance(max_distance=-1), lambda: SearchConfig("q", 65, "jaccard", 0.5, rerank=e)):
        with pytest.raises(ValueError):
            bad()
    s = Service(device=0)                                      # no device dictionary: a re-rank has nothing to read the strings from
    with pytest.raises(KeyError):
        s.suggest("cars", SearchConfig("q", 3, "jaccard", 0.5, rerank=e))
    with pytest.raises(KeyError):
        s.suggest_batch("cars", ["q"], 3, "jaccard", 0.5, rerank=e)
