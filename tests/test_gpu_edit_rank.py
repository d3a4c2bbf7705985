"""Result rows ranked by edit distance on the device (suggest_amd/csrc/edit_rank.inc).  Every distance and every
re-ranked row the device gives is compared word for word with tests/edit_ref.py, in both modes, folded and unfolded, through the
host-buffer calls and the _device calls, on the smallest shapes at which the kernels can go wrong (tests/edit_shapes.py).  All
comparisons are exact integer and bit equality."""
import threading

import numpy as np
import pytest

import edit_ref as ref
import edit_shapes as shp
from conftest import CARS_DESC

pytestmark = pytest.mark.gpu

CONFIGS = [(m, f) for m in ref.MODES for f in (True, False)]
GUARD = 16


@pytest.fixture(scope="module")
def torch():
    import torch  # (before the library: both must resolve the same libamdhip64, suggest_amd/_lib.py)
    return torch


@pytest.fixture(scope="module")
def shapes(torch):
    from suggest_amd.dictionary import DeviceDictionary
    s = shp.build()
    s["dd"] = DeviceDictionary(s["lines"], device=0)
    return s


@pytest.fixture(scope="module")
def cars(torch, cars_lines):
    from suggest_amd import IndexDescription, NGramIndex
    from suggest_amd.dictionary import DeviceDictionary
    lines = [l.encode("utf-8") if isinstance(l, str) else bytes(l) for l in cars_lines]
    ix = NGramIndex(cars_lines, IndexDescription(**CARS_DESC))
    yield dict(lines=lines, ix=ix, dd=DeviceDictionary(lines, device=0))
    ix.close()


def _to_dev(torch, a):
    a = np.ascontiguousarray(a)
    view = {np.dtype(np.uint32): np.int32, np.dtype(np.uint64): np.int64, np.dtype(np.uint8): np.uint8, np.dtype(np.float64): np.float64}[a.dtype]
    return torch.from_numpy(a.view(view).copy()).to("cuda:0")


def _device(torch, dd, queries, ids, counts, mode, fold, row=0, row_offs=None, slots=None, scores=None, rerank=False, k_out=1, max_distance=None, stream=None):
    """sg_edit_rows_device / sg_edit_rerank_device on tensors -> (dist, the GUARD words behind it, info [2], ids, scores, counts)"""
    from suggest_amd.dictionary import edit_config
    from suggest_amd.index import pack_strings
    qb, qo = pack_strings(queries)
    ids = np.ascontiguousarray(ids, dtype=np.uint32).reshape(-1)
    counts = np.ascontiguousarray(counts, dtype=np.uint32)
    slots = ids.size if slots is None else slots
    d_q = _to_dev(torch, qb if qb.size else np.zeros(1, dtype=np.uint8))
    d_qo, d_ids, d_cnt = _to_dev(torch, qo), _to_dev(torch, ids), _to_dev(torch, counts)
    d_ro = None if row_offs is None else _to_dev(torch, np.asarray(row_offs, dtype=np.uint64))
    d_sc = None if scores is None else _to_dev(torch, np.asarray(scores, dtype=np.float64).reshape(-1))
    d_dist = torch.full((slots + GUARD,), 0x6E6E6E6E, dtype=torch.int32, device="cuda:0")
    d_info = torch.full((2,), -1, dtype=torch.int64, device="cuda:0")
    torch.cuda.synchronize()
    cfg = edit_config(mode, fold, max_distance)
    sp = 0 if stream is None else stream.cuda_stream
    ro = None if d_ro is None else d_ro.data_ptr()
    if rerank:
        dd.edit_rerank_device(cfg, d_q.data_ptr(), d_qo.data_ptr(), d_ids.data_ptr(), None if d_sc is None else d_sc.data_ptr(), d_cnt.data_ptr(), ro,
                              len(counts), row, slots, k_out, d_dist.data_ptr(), d_info.data_ptr(), stream=sp)
    else:
        dd.edit_rows_device(cfg, d_q.data_ptr(), d_qo.data_ptr(), d_ids.data_ptr(), d_cnt.data_ptr(), ro, len(counts), row, slots, d_dist.data_ptr(),
                            d_info.data_ptr(), stream=sp)
    torch.cuda.synchronize()
    dist = d_dist.cpu().numpy().view(np.uint32)
    return (dist[:slots], dist[slots:], d_info.cpu().numpy().view(np.uint64), d_ids.cpu().numpy().view(np.uint32),
            None if d_sc is None else d_sc.cpu().numpy(), d_cnt.cpu().numpy().view(np.uint32))


def _both_routes_distances(torch, shapes, queries, ids, counts, mode, fold, row=0, row_offs=None, slots=None):
    from suggest_amd import _lib
    want, outside = ref.edit_rows(queries, ids, counts, shapes["lines"], row=row, row_offs=row_offs, mode=mode, fold=fold)
    if slots is not None and slots > want.size:
        want = np.concatenate([want, np.full(slots - want.size, ref.NONE, dtype=np.uint32)])
    with _lib.poisoned(1):
        dist, guard, info = _device(torch, shapes["dd"], queries, ids, counts, mode, fold, row=row, row_offs=row_offs, slots=slots)[:3]
        host = None
        if outside == 0 and (slots is None or slots == np.asarray(ids).size):
            host = shapes["dd"].edit_distances(queries, np.asarray(ids, dtype=np.uint32), counts, row_offs=row_offs, mode=mode, fold_case=fold)
    assert info.tolist() == [0, outside]
    bad = np.nonzero(dist != want)[0]
    assert bad.size == 0, (bad[:8], dist[bad[:8]], want[bad[:8]])
    assert np.all(guard == 0x6E6E6E6E)
    assert host is None or np.array_equal(host.reshape(-1), want)
    return want


# ---- 1: distances on the shapes ----
@pytest.mark.parametrize("mode,fold", CONFIGS)
@pytest.mark.parametrize("case", ["lengths", "dense", "special"])
def test_distances_equal_the_restatement(torch, shapes, case, mode, fold):
    """query lengths 0, 1, 63, 64, 65, 127, 128, 129, 1 000 x candidate lengths 0, 1, 64, 300; a dense set of pairs over three
    letters; multi-byte runes, invalid bytes, the truncated rune at the blob's end, width-changing folds, the full Peq table,
    colliding and absent runes"""
    queries, ids, counts = {"lengths": shp.length_cases, "dense": shp.dense_cases, "special": shp.special_cases}[case](shapes)
    _both_routes_distances(torch, shapes, queries, ids, counts, mode, fold, row=ids.shape[1])


@pytest.mark.parametrize("mode", ref.MODES)
def test_the_long_pair_in_slices(torch, shapes, mode):
    """4 096 x 4 096 runes on the long kernel, among five more long rows, with a budget below two regions (a region of either
    route is above 256 KiB): one workgroup, six slices; the budget still holds every row's masks"""
    from suggest_amd import _lib
    nm = shapes["named"]
    big = shapes["lines"][nm["long4096"]]
    queries = [big[::-1] + b"ab", shp.query_of(65), shp.query_of(300, 1), b"nisan", shp.query_of(129, 2), shp.query_of(1000, 3), big[100:]]
    ids = np.array([[nm["long4096"], nm["c300"], nm["empty"]]] * len(queries), dtype=np.uint32)
    assert _lib.lib().sg_debug_edit_slice_bytes(64 << 10) == 0
    try:
        want = _both_routes_distances(torch, shapes, queries, ids, [3] * len(queries), mode, True, row=3)
    finally:
        _lib.lib().sg_debug_edit_slice_bytes(0)
    assert 0 < want[0] < 4096 and want[18] == 100


@pytest.mark.parametrize("mode,fold", CONFIGS)
def test_long_rows_without_room_for_masks(torch, shapes, mode, fold):
    """a budget of one byte leaves no room for a row of Peq masks: the long kernel walks the sorted pairs instead"""
    from suggest_amd import _lib
    nm = shapes["named"]
    queries = [shp.query_of(n, 4) for n in (65, 127, 128, 129, 300, 1000)] + [shapes["lines"][nm["full64"]] + b"x", shapes["lines"][nm["c300"]][::-1]]
    ids = np.array([[nm["c300"], nm["c64"], nm["full64_rot"], nm["empty"], nm["three_byte"]]] * len(queries), dtype=np.uint32)
    assert _lib.lib().sg_debug_edit_slice_bytes(1) == 0
    try:
        _both_routes_distances(torch, shapes, queries, ids, [5] * len(queries), mode, fold, row=5)
    finally:
        _lib.lib().sg_debug_edit_slice_bytes(0)


# ---- 2: rows of every width: the lane stride, the re-rank's switch of routes ----
@pytest.mark.parametrize("row", shp.ROW_SLOTS)
def test_rows_distances_and_rerank(torch, shapes, row):
    """counts 0, 1, row and above; a flagged row between ordinary ones, its slots as they were; slots past a count are not read (one
    holds an id >= n_docs); re-rank with k_out < row, max_distance 0, 1 and none; fuzzy rows and autocomplete rows (no scores)"""
    from suggest_amd import _lib
    queries, ids, scores, counts = shp.row_cases(shapes, row)
    flagged = int(np.nonzero(counts >= ref.COUNT_FLAG_MIN)[0][0])
    _both_routes_distances(torch, shapes, queries, ids, counts, "osa", True, row=row)
    d_lev = _both_routes_distances(torch, shapes, queries, ids, counts, "levenshtein", False, row=row, slots=ids.size + 3)      # spare slots
    assert np.all(d_lev[ids.size:] == ref.NONE)
    for max_distance, k_out, sc in ((None, row, scores), (1, row, scores), (0, max(1, row // 3), None), (None, max(1, row - 1), None), (60, 7, scores)):
        md = ref.NONE if max_distance is None else max_distance
        d0, _ = ref.edit_rows(queries, ids, counts, shapes["lines"], row=row, mode="osa", fold=True)
        w_ids, w_sc, w_d, w_c = ref.rerank(ids, sc, d0, counts, row=row, max_distance=md, k_out=k_out)
        with _lib.poisoned(2):
            dist, guard, info, g_ids, g_sc, g_c = _device(torch, shapes["dd"], queries, ids, counts, "osa", True, row=row, scores=sc, rerank=True, k_out=k_out,
                                                          max_distance=max_distance)
            h_ids, h_sc, h_d, h_c = shapes["dd"].edit_rerank(queries, ids, counts, scores=sc, k_out=k_out, mode="osa", max_distance=max_distance)
        assert info.tolist() == [0, 0] and np.all(guard == 0x6E6E6E6E)
        for got in ((g_ids, g_sc, dist, g_c), (h_ids.reshape(-1), None if h_sc is None else h_sc.reshape(-1), h_d.reshape(-1), h_c)):
            assert np.array_equal(got[0], w_ids) and np.array_equal(got[2], w_d) and np.array_equal(got[3], w_c), (max_distance, k_out)
            assert sc is None or np.array_equal(got[1].view(np.uint64), w_sc.view(np.uint64))
        assert np.array_equal(g_ids.reshape(-1, row)[flagged], ids[flagged]) and np.all(dist.reshape(-1, row)[flagged] == ref.NONE)


def test_ragged_rows(torch, shapes):
    from suggest_amd import _lib
    queries, ids, scores, counts, ro, slots = shp.ragged_cases(shapes)
    for mode, fold in CONFIGS[:2]:
        _both_routes_distances(torch, shapes, queries, ids, counts, mode, fold, row_offs=ro, slots=slots)
    d0, _ = ref.edit_rows(queries, ids, counts, shapes["lines"], row_offs=ro)
    for max_distance, k_out, sc in ((None, slots, scores), (6, 100, scores), (2, 1, None)):
        md = ref.NONE if max_distance is None else max_distance
        w_ids, w_sc, w_d, w_c = ref.rerank(ids, sc, d0, counts, row_offs=ro, max_distance=md, k_out=k_out)
        with _lib.poisoned(1):
            dist, guard, info, g_ids, g_sc, g_c = _device(torch, shapes["dd"], queries, ids, counts, "levenshtein", True, row_offs=ro, slots=slots, scores=sc,
                                                          rerank=True, k_out=k_out, max_distance=max_distance)
        assert info.tolist() == [0, 0] and np.all(guard == 0x6E6E6E6E)
        assert np.array_equal(g_ids, w_ids) and np.array_equal(dist, w_d) and np.array_equal(g_c, w_c)
        assert sc is None or np.array_equal(g_sc.view(np.uint64), w_sc.view(np.uint64))
        assert np.array_equal(g_ids[int(ro[-1]):], ids[int(ro[-1]):])                       # the spare tail is no row's


# ---- 2b: the host-buffer calls on the shared host-call path: slices, the poison, a block above the staging limit ----
def _slice_batch(shapes, ragged):
    """six rows of three slots (ragged: 3, 0, 2, 3, 1, 3), counts within the rows -> (queries, blob, offs, ids, scores, counts, row_offs)"""
    from suggest_amd.index import pack_strings
    rng = np.random.default_rng(515)
    pool = shp.short_ids(shapes)
    queries = [shp.query_of(n, seed=9) for n in (4, 0, 7, 12, 3, 9)]
    lens = [3, 0, 2, 3, 1, 3] if ragged else [3] * 6
    ro = np.concatenate([[0], np.cumsum(lens)]).astype(np.uint64)
    ids = pool[rng.integers(0, len(pool), int(ro[-1]))].astype(np.uint32)
    scores = np.round(rng.random(int(ro[-1])), 1)
    counts = np.array([min(c, n) for c, n in zip((3, 1, 2, 3, 0, 2), lens)], dtype=np.uint32)
    blob, offs = pack_strings(queries)
    return queries, blob, offs, ids, scores, counts, ro


@pytest.mark.parametrize("family", [0, 1, 2])
@pytest.mark.parametrize("ragged", [False, True])
def test_host_calls_on_a_slice_of_a_batch(torch, shapes, ragged, family):
    """edit_distances and edit_rerank on rows 2..4 of a six-row batch, handed over as a slice — the whole query blob and offsets whose
    first is not zero — equal the restatement on those rows, with the poison off and under both pattern families."""
    from suggest_amd import _lib
    queries, blob, offs, ids, scores, counts, ro = _slice_batch(shapes, ragged)
    lo, hi = 2, 5
    s0, s1 = int(ro[lo]), int(ro[hi])
    assert offs[lo] != 0
    q, i, s, c = queries[lo:hi], ids[s0:s1], scores[s0:s1], counts[lo:hi]
    geo = dict(row_offs=(ro[lo:hi + 1] - ro[lo])) if ragged else dict(row=3)
    d0, outside = ref.edit_rows(q, i, c, shapes["lines"], mode="osa", fold=True, **geo)
    w_ids, w_sc, w_d, w_c = ref.rerank(i, s, d0, c, max_distance=ref.NONE, k_out=2, **geo)
    assert outside == 0
    host_geo = dict(row_offs=geo["row_offs"]) if ragged else {}
    ids_in = i if ragged else i.reshape(-1, 3)
    sc_in = s if ragged else s.reshape(-1, 3)
    with _lib.poisoned(family):
        _lib.poison_stats()
        dist = shapes["dd"].edit_distances(None, ids_in, c, mode="osa", fold_case=True, blob=blob, offs=offs[lo:hi + 1], **host_geo)
        st = _lib.poison_stats()
        g_ids, g_sc, g_d, g_c = shapes["dd"].edit_rerank(None, ids_in, c, scores=sc_in, k_out=2, mode="osa", blob=blob, offs=offs[lo:hi + 1], **host_geo)
    assert np.array_equal(dist.reshape(-1), d0)
    assert np.array_equal(g_ids.reshape(-1), w_ids) and np.array_equal(g_d.reshape(-1), w_d) and np.array_equal(g_c, w_c)
    assert np.array_equal(g_sc.reshape(-1).view(np.uint64), w_sc.view(np.uint64))
    assert (st["out_ids"] >= i.size * 4) == (family != 0), st           # the distances are a result region of the shared path


def test_rerank_above_the_staging_limit(torch, shapes):
    """65 536 rows x 64 candidates — 64 distinct rows tiled 1 024 times, strings of 16 runes at most: with 8 + 4 + 4 + 4 bytes per slot
    the call's block is 84 MB, above the 64 MiB a synchronous call stages, so ids, scores and counts go in and come back straight
    from / to the caller's arrays.  The batch is handed over as a slice (a query in front of the blob, offsets whose first is not
    zero): above the limit such offsets are rebased through the staging buffer alone.  Expected: the restatement's answer for the
    64 rows, tiled."""
    from suggest_amd.index import pack_strings
    rng = np.random.default_rng(616)
    pool = np.array([i for i in shp.short_ids(shapes) if len(ref.runes(shapes["lines"][i], True)) <= 16], dtype=np.uint32)
    assert len(pool) >= 16
    n, row, tiles = 64, 64, 1024
    queries = [shp.query_of(int(rng.integers(0, 17)), seed=i) for i in range(n)]
    ids = pool[rng.integers(0, len(pool), (n, row))].astype(np.uint32)
    scores = -np.sort(-np.round(rng.random((n, row)), 1), axis=1)
    counts = rng.integers(0, row + 1, n).astype(np.uint32)
    d0, outside = ref.edit_rows(queries, ids, counts, shapes["lines"], row=row, mode="osa", fold=True)
    w_ids, w_sc, w_d, w_c = ref.rerank(ids, scores, d0, counts, row=row, max_distance=3, k_out=10)
    assert outside == 0 and n * tiles * row * 20 > 64 << 20
    blob, offs = pack_strings([b"in front"] + queries * tiles)
    assert offs[1] != 0
    g_ids, g_sc, g_d, g_c = shapes["dd"].edit_rerank(None, np.tile(ids, (tiles, 1)), np.tile(counts, tiles), scores=np.tile(scores, (tiles, 1)),
                                                     k_out=10, mode="osa", max_distance=3, blob=blob, offs=offs[1:])
    assert np.array_equal(g_ids.reshape(tiles, -1), np.tile(w_ids, (tiles, 1)))
    assert np.array_equal(g_d.reshape(tiles, -1), np.tile(w_d, (tiles, 1)))
    assert np.array_equal(g_sc.reshape(tiles, -1).view(np.uint64), np.tile(w_sc.view(np.uint64), (tiles, 1)))
    assert np.array_equal(g_c.reshape(tiles, -1), np.tile(w_c, (tiles, 1)))


def test_an_id_outside_the_dictionary(torch, shapes):
    from suggest_amd import _lib
    n = len(shapes["lines"])
    nm = shapes["named"]
    ids = np.array([[nm["nissan"], n, 0xFFFFFFFF, nm["niva"]], [n + 5, nm["one"], nm["one"], nm["one"]]], dtype=np.uint32)
    queries = ["nisan", shp.query_of(70)]                                   # one row on each kernel
    dist, guard, info = _device(torch, shapes["dd"], queries, ids, [4, 2], "levenshtein", True, row=4)[:3]
    want, outside = ref.edit_rows(queries, ids, [4, 2], shapes["lines"], row=4)
    assert outside == 3 and info.tolist() == [0, 3] and np.array_equal(dist, want) and dist[:4].tolist() == [1, ref.NONE, ref.NONE, 2]
    with pytest.raises(_lib.SuggestHipError) as e:
        shapes["dd"].edit_distances(queries, ids, [4, 2])
    assert e.value.code == -1 and "docID outside the dictionary" in str(e.value)
    dist, guard, info, g_ids, _, g_c = _device(torch, shapes["dd"], queries, ids, [4, 2], "levenshtein", True, row=4, rerank=True, k_out=4)
    w = ref.rerank(ids, None, want, [4, 2], row=4)
    assert np.array_equal(g_ids, w[0]) and np.array_equal(dist, w[2]) and g_c.tolist() == [4, 2] and info.tolist() == [0, 3]


def test_equal_and_descending_distances(torch, shapes):
    nm = shapes["named"]
    ids = [[nm["toyota"], nm["ATOYOT"], nm["toyota corolla"], nm["TOYOTA COROLLA"]], [nm["nissan"], nm["nsisan"], nm["niva"], nm["one"]],
           [nm["c300"], nm["c64"], nm["nissan"], nm["one"]]]
    sc = [[.9, .9, .5, .5], [.8, .7, .7, .1], [.4, .3, .2, .1]]
    g_ids, g_sc, dist, g_c = shapes["dd"].edit_rerank(["toyota corola", "xxxxxx", "q"], ids, [4, 4, 4], scores=sc, mode="osa")
    assert dist.tolist() == [[1, 1, 7, 9], [6, 6, 6, 6], [0, 6, 64, 300]] and g_c.tolist() == [4, 4, 4]
    assert g_ids.tolist() == [[ids[0][2], ids[0][3], ids[0][0], ids[0][1]], ids[1], ids[2][::-1]]          # ties keep their order; unchanged; reversed
    assert g_sc.tolist() == [[.5, .5, .9, .9], sc[1], sc[2][::-1]]


# ---- 3: search and rank in one call ----
def _typos(lines, n, seed):
    rng = np.random.RandomState(seed)
    out = []
    for i in rng.randint(0, len(lines), n):
        s = list(lines[int(i)].decode("utf-8", "ignore"))
        for _ in range(int(rng.randint(0, 3))):
            if len(s) < 2:
                break
            p = int(rng.randint(0, len(s) - 1))
            op = int(rng.randint(0, 4))
            if op == 0:
                s[p], s[p + 1] = s[p + 1], s[p]
            elif op == 1:
                del s[p]
            elif op == 2:
                s.insert(p, "x")
            else:
                s[p] = s[p].swapcase()
        out.append("".join(s).encode("utf-8"))
    return out


@pytest.mark.parametrize("kc,k,mode,max_distance", [(64, 10, "osa", None), (64, 10, "levenshtein", 2), (1100, 64, "osa", None), (5, 5, "osa", 0)])
def test_search_and_rank_is_the_independent_composition(torch, cars, kc, k, mode, max_distance):
    """sg_suggest_batch_edit's rows = the restated re-rank applied to the rows of the existing suggest_batch(k = k_candidates); the
    plain call's rows before and after are bit-identical"""
    from suggest_amd import _lib
    queries = _typos(cars["lines"], 300, 5) + [b"", b"zzzzqqqq"]
    before = cars["ix"].suggest_batch(queries, "jaccard", 0.3, kc)
    with _lib.poisoned(1):
        ids, sc, dist, cnt = cars["ix"].suggest_batch_edit(cars["dd"], queries, "jaccard", 0.3, kc, k, mode=mode, max_distance=max_distance)
    after = cars["ix"].suggest_batch(queries, "jaccard", 0.3, kc)
    for a, b in zip(before, after):
        assert np.array_equal(np.asarray(a).view(np.uint8), np.asarray(b).view(np.uint8))
    b_ids, b_sc, b_cnt = before
    assert int((b_cnt > k).sum()) > 0 or kc == k
    d0, outside = ref.edit_rows(queries, b_ids, b_cnt, cars["lines"], row=kc, mode=mode, fold=True)
    w_ids, w_sc, w_d, w_c = ref.rerank(b_ids, b_sc, d0, b_cnt, row=kc, max_distance=ref.NONE if max_distance is None else max_distance, k_out=k)
    assert outside == 0
    assert np.array_equal(cnt, w_c)
    assert np.array_equal(ids, w_ids.reshape(-1, kc)[:, :k]) and np.array_equal(dist, w_d.reshape(-1, kc)[:, :k])
    assert np.array_equal(sc.view(np.uint64), w_sc.reshape(-1, kc)[:, :k].view(np.uint64))


def test_search_and_rank_refusals(torch, cars, shapes):
    from suggest_amd import _lib
    from suggest_amd.dictionary import DeviceDictionary
    for kc, k in ((8, 0), (8, 9), (0, 0), (65537, 3)):
        with pytest.raises(_lib.SuggestHipError) as e:
            cars["ix"].suggest_batch_edit(cars["dd"], ["nisan"], "jaccard", 0.5, kc, k)
        assert e.value.code == -1, (kc, k)
    host = DeviceDictionary(cars["lines"][:10], device=-1)
    with pytest.raises(_lib.SuggestHipError) as e:
        cars["ix"].suggest_batch_edit(host, ["nisan"], "jaccard", 0.5, 8, 3)
    assert e.value.code == -2
    with pytest.raises(_lib.SuggestHipError) as e:                          # a dictionary shorter than the index: ids outside it, reported
        assert len(cars["lines"]) - 1 >= len(shapes["lines"])
        cars["ix"].suggest_batch_edit(shapes["dd"], [cars["lines"][-1]], "jaccard", 0.5, 8, 3)
    assert e.value.code == -1 and "docID outside the dictionary" in str(e.value)
    assert cars["ix"].suggest_batch_edit(cars["dd"], [], "jaccard", 0.5, 8, 3)[3].size == 0


# ---- 4: threads ----
def test_three_threads_on_their_own_streams(torch, shapes):
    """sg_edit_rerank_device writes nothing of the handle: three threads, a stream each, one dictionary"""
    cases = [shp.row_cases(shapes, row, seed=9) for row in (64, 65, 1025)]
    want = []
    for (queries, ids, scores, counts), row in zip(cases, (64, 65, 1025)):
        d0, _ = ref.edit_rows(queries, ids, counts, shapes["lines"], row=row, mode="osa", fold=True)
        want.append(ref.rerank(ids, scores, d0, counts, row=row, max_distance=50, k_out=row))
    out, errors = [None] * 3, []

    def work(t):
        try:
            torch.cuda.set_device(0)
            st = torch.cuda.Stream()
            queries, ids, scores, counts = cases[t]
            for _ in range(3):
                out[t] = _device(torch, shapes["dd"], queries, ids, counts, "osa", True, row=ids.shape[1], scores=scores, rerank=True, k_out=ids.shape[1],
                                 max_distance=50, stream=st)
        except Exception as e:  # noqa: BLE001
            errors.append(e)
    threads = [threading.Thread(target=work, args=(t,)) for t in range(3)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert not errors, errors
    for t in range(3):
        dist, guard, info, g_ids, g_sc, g_c = out[t]
        w_ids, w_sc, w_d, w_c = want[t]
        assert np.array_equal(g_ids, w_ids) and np.array_equal(dist, w_d) and np.array_equal(g_c, w_c) and np.array_equal(g_sc.view(np.uint64), w_sc.view(np.uint64))


# ---- 5: the callers above the C ABI ----
def test_service_suggest_with_rerank(torch, cars):
    """Service.suggest / suggest_batch with SearchConfig(rerank=EditDistance(...)) = the restated re-rank of the plain rows, with the
    dictionary's strings and a distance per item; without rerank= nothing changes"""
    from suggest_amd import EditDistance, IndexDescription, ResultItem, SearchConfig, Service
    svc = Service(device=0, device_dictionary=True)
    svc.add_index("cars", cars["lines"], IndexDescription(**CARS_DESC))
    plain = Service(device=0)
    plain.add_index("cars", cars["lines"], IndexDescription(**CARS_DESC))
    queries = _typos(cars["lines"], 40, 8)
    for rr in (EditDistance(candidates=64, transpositions=True), EditDistance(candidates=16, max_distance=2, fold_case=False)):
        k = 5
        b_ids, b_sc, b_cnt = cars["ix"].suggest_batch(queries, "jaccard", 0.3, rr.candidates)
        d0, _ = ref.edit_rows(queries, b_ids, b_cnt, cars["lines"], row=rr.candidates, mode=rr.mode, fold=rr.fold_case)
        w_ids, w_sc, w_d, w_c = ref.rerank(b_ids, b_sc, d0, b_cnt, row=rr.candidates, max_distance=ref.NONE if rr.max_distance is None else rr.max_distance,
                                           k_out=k)
        want = [[ResultItem(float(w_sc[i * rr.candidates + j]), cars["lines"][int(w_ids[i * rr.candidates + j])].decode("utf-8", "replace"),
                            int(w_d[i * rr.candidates + j])) for j in range(int(w_c[i]))] for i in range(len(queries))]
        assert svc.suggest_batch("cars", queries, k, "jaccard", 0.3, rerank=rr) == want
        for i in (0, 7, 23):
            assert svc.suggest("cars", SearchConfig(queries[i], k, "jaccard", 0.3, rerank=rr)) == want[i]
        assert sum(len(r) for r in want) > 20
    got = svc.suggest("cars", SearchConfig(queries[0], 5, "jaccard", 0.3))
    assert got == plain.suggest("cars", SearchConfig(queries[0], 5, "jaccard", 0.3)) and all(r.distance is None for r in got)
    with pytest.raises(ValueError):                           # the strings are not on the device
        plain.suggest("cars", SearchConfig(queries[0], 5, "jaccard", 0.3, rerank=EditDistance()))
    with pytest.raises(ValueError):
        svc.suggest_many("cars", [SearchConfig(queries[0], 5, "jaccard", 0.3, rerank=EditDistance())])


def test_cpp_mirror_on_the_device():
    import os
    import subprocess
    from conftest import GOLDEN, ROOT
    binary = os.path.join(ROOT, "tests", "cpp", "_build", "edit_rank_test")
    if not os.path.exists(binary):
        subprocess.check_call(["make", "-C", os.path.join(ROOT, "tests", "cpp"), "-f", "edit_rank.mk"], stdout=subprocess.DEVNULL)
    r = subprocess.run([binary, GOLDEN], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "0 failed" in r.stdout, (r.returncode, r.stdout, r.stderr)
