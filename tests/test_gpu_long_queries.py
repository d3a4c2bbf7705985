"""sg_long_kernel (long_tokenize, long_query, the slot lock) against the CPU oracle through the C ABI, bit for bit, on the
inputs of tests/long_query_shapes.py: a dense dictionary (segments of hundreds of documents, lists above 256 raw entries,
documents that repeat a term, 8-bit-gap lists), queries on both sides of the slot's limits (65 536 windows, 65 536 bytes), long
queries through paging, long prefixes and a tabulated metric, the reference's panic / dead-lock flags, and the four scratch
slots shared by the launches of several threads.  test_long_query_shapes_cpu.py shows on the oracle alone that the inputs reach
those edges; the control test here shows that it is sg_long_kernel that answers them."""
import ctypes as C
import threading

import numpy as np
import pytest

import long_query_shapes as lq
import oracle
from test_gpu_parity import assert_same

pytestmark = pytest.mark.gpu

ALL_CALLS = lq.DENSE_CALLS + (lq.FLAG_CALL,)


def _index(docs, desc, **kw):
    from suggest_amd import NGramIndex, IndexDescription
    return NGramIndex(docs, IndexDescription(**desc), **kw)


@pytest.fixture(scope="module")
def dense():
    """the dictionary, the oracle and the oracle's rows of every call, computed once"""
    d = lq.dense()
    ora = oracle.OracleIndex(d["docs"], **lq.DENSE_DESC)
    qb, qo = oracle.pack_strings(d["queries"])
    d["packed"] = (qb, qo)
    d["long"] = lq.long_set(ora, lq.DENSE_DESC, d["queries"])
    d["want"] = {call: ora.suggest_batch(qb, qo, *call) for call in ALL_CALLS}
    d["flag_packed"] = oracle.pack_strings(d["flag_queries"])
    d["flag_want"] = ora.suggest_batch(*d["flag_packed"], *lq.FLAG_CALL)
    d["gpu"] = {}
    return d, ora


def _dense_gpu(d, monkeypatch, g8):
    """one index per SG_G8 value, shared by the tests of the module"""
    if g8 not in d["gpu"]:
        monkeypatch.setenv("SG_G8", str(g8))
        monkeypatch.delenv("SG_NO_LONG_QUERIES", raising=False)
        d["gpu"][g8] = _index(d["docs"], lq.DENSE_DESC)
    return d["gpu"][g8]


# every call under SG_G8=2 (every list in 8-bit gaps); the widest call and the flagged one under the other two formats (a case
# takes 2 to 10 s on the MI355X, dice 0.4 with k = 100 in HBM rows the longest: sg_long_kernel runs eight workgroups of one
# wavefront over 110 long queries)
ROWS = [(2, call) for call in ALL_CALLS] + [(g8, call) for g8 in (0, 1) for call in (lq.DENSE_CALLS[4], lq.FLAG_CALL)]


@pytest.mark.parametrize("g8,call", ROWS, ids=["g8=%d-%s-%g-k%d" % ((g8,) + call) for g8, call in ROWS])
def test_dense_rows(dense, monkeypatch, g8, call):
    """Every row of the mixed batch, long and short, under each posting format (SG_G8: 8-bit gaps never / where they save
    chunks / everywhere): the j0 loop over segments of up to 442 documents, several candidates per ballot, the filter of a
    full top-k, counters reused between segments, lists above 256 raw entries in the secondary-entry search, k in a slot and
    in HBM rows, and jaccard 0.95, whose windows are empty (the reference panics or dead-locks: the flags are compared)."""
    d, ora = dense
    gpu = _dense_gpu(d, monkeypatch, g8)
    qb, qo = d["packed"]
    metric, alpha, k = call
    assert_same(gpu.suggest_batch(blob=qb, offs=qo, metric=metric, similarity=alpha, k=k), d["want"][call], d["queries"])
    if call == lq.FLAG_CALL:
        fb, fo = d["flag_packed"]
        got = gpu.suggest_batch(blob=fb, offs=fo, metric=metric, similarity=alpha, k=k)
        assert_same(got, d["flag_want"], d["flag_queries"])
        assert (got[2] == lq.COUNT_PANIC).any() and (got[2] == lq.COUNT_DEADLOCK).any()


def test_control_the_long_kernel_answered(dense, monkeypatch):
    """Without the long-query scratch (SG_NO_LONG_QUERIES=1) exactly the queries that the oracle's tokens and the rune count
    call long come back SG_COUNT_TOO_LONG, and every other row is still the oracle's: the rows that test_dense_rows compared
    for that set were sg_long_kernel's."""
    d, ora = dense
    monkeypatch.setenv("SG_NO_LONG_QUERIES", "1")
    monkeypatch.setenv("SG_G8", "2")
    gpu = _index(d["docs"], lq.DENSE_DESC)
    qb, qo = d["packed"]
    for call in (lq.DENSE_CALLS[0], lq.DENSE_CALLS[4]):
        metric, alpha, k = call
        ids, sc, cnt = gpu.suggest_batch(blob=qb, offs=qo, metric=metric, similarity=alpha, k=k)
        assert set(np.nonzero(cnt == lq.COUNT_TOO_LONG)[0].tolist()) == d["long"]
        short = np.array(sorted(set(range(len(d["queries"]))) - d["long"]))
        want = d["want"][call]
        assert_same((ids[short], sc[short], cnt[short]), (want[0][short], want[1][short], want[2][short]), [d["queries"][i] for i in short])
    gpu.close()
    # ... and with the scratch the same rows are real ones
    got = _dense_gpu(d, monkeypatch, 2).suggest_batch(blob=qb, offs=qo, metric="jaccard", similarity=0.5, k=10)
    assert not (got[2] == lq.COUNT_TOO_LONG).any() and all(got[2][i] >= 1 for i in d["long"] if d["want"][lq.DENSE_CALLS[0]][2][i] >= 1)


def test_long_queries_page_through_every_candidate(dense, monkeypatch):
    """sg_suggest_batch_from on long queries (autocomplete == 2: by_doc_key, out_aux, ac_first): every candidate, ascending
    docID, three and 64 to a page, against the oracle's Suggest with k = twice the dictionary, as multisets of (docID, score
    bits) — documents with several entries included — and each row's (overlap, segment) reproduces its score."""
    d, ora = dense
    gpu = _dense_gpu(d, monkeypatch, 2)
    metric, alpha = lq.PAGING
    n_multi = n_page3 = 0
    for q in d["paging"]:
        oi, os_, oc = ora.suggest_batch(*oracle.pack_strings([q]), metric, alpha, 2 * len(d["docs"]))[:3]
        assert oc[0] < 0xFFFFFFF0
        want = sorted((int(oi[0, j]), int(os_.view(np.uint64)[0, j])) for j in range(int(oc[0])))
        n_multi += len(want) != len({x for x, _ in want})
        n_a = len(ora.tokenize(q))
        for page in (3, 64):
            if len(want) / page > 300:
                continue
            n_page3 += page == 3
            rows = gpu.suggest_all(q, metric, alpha, page=page)
            ids = [r[0] for r in rows]
            assert ids == sorted(ids)
            got = sorted((r[0], int(np.float64(r[1]).view(np.uint64))) for r in rows)
            assert got == want, (q, page, got[:5], want[:5])
            for doc, s, ov, seg in rows:
                assert np.float64(oracle.metric_score(metric, ov, n_a, seg)).view(np.uint64) == np.float64(s).view(np.uint64)
    assert n_multi >= 2 and n_page3 >= 4


def test_long_prefixes_page_through_every_match(dense, monkeypatch):
    """autocomplete_all with prefixes of more than 144 runes (sg_autocomplete_one_from: ac_first in long_query), 7 to a page"""
    d, ora = dense
    gpu = _dense_gpu(d, monkeypatch, 2)
    n_paged = 0
    for p in d["prefixes"]:
        o_ids, o_cnt = ora.autocomplete_batch(*oracle.pack_strings([p]), len(d["docs"]))[:2]
        want = o_ids[0, :int(o_cnt[0])].tolist()
        n_paged += len(want) > 7
        assert gpu.autocomplete_all(p, page=7) == want
    assert n_paged >= 2


def test_long_queries_with_a_tabulated_metric():
    """SG_TABLE in long_query: tables of a_max = 40 filled from the oracle's metric functions; over "abc" a long query has at
    most 29 n-grams and gets the native metric's rows; the one with more than 40 comes back SG_COUNT_TOO_LONG between
    neighbours that are answered."""
    from suggest_amd import _lib
    from suggest_amd.index import MetricTables
    t = lq.table_dictionary()
    gpu = _index(t["docs"], lq.DENSE_DESC)
    ora = oracle.OracleIndex(t["docs"], **lq.DENSE_DESC)
    qs, over = t["queries"], t["over"]
    qb, qo = oracle.pack_strings(qs)
    S, n_a = gpu.stats()["n_segments"], lq.TABLE_A_MAX + 1
    keep = np.array([i for i in range(len(qs)) if i != over])
    for metric, alpha in (("jaccard", 0.5), ("cosine", 0.3)):
        score = np.zeros((n_a, S, n_a))
        thr = np.zeros((n_a, S), np.int32)
        mn = np.array([oracle.metric_min_y(metric, alpha, a) for a in range(n_a)], np.int32)
        mx = np.array([min(oracle.metric_max_y(metric, alpha, a), 2**31 - 1) for a in range(n_a)], np.int32)
        for a in range(1, n_a):
            for b in range(max(0, int(mn[a])), min(S - 1, int(mx[a])) + 1):
                thr[a, b] = oracle.metric_threshold(metric, alpha, a, b)
                for o in range(max(0, int(thr[a, b])), a + 1):
                    score[a, b, o] = oracle.metric_score(metric, o, a, b)
        h = C.c_void_p()
        _lib.check(_lib.lib().sg_metric_tables_create(gpu._h, lq.TABLE_A_MAX, mn.ctypes.data, mx.ctypes.data, thr.ctypes.data, score.ctypes.data, C.byref(h)))
        ids, sc, cnt = gpu.suggest_batch(blob=qb, offs=qo, k=10, tables=MetricTables(h, lq.TABLE_A_MAX))
        assert cnt[over] == lq.COUNT_TOO_LONG
        want = ora.suggest_batch(qb, qo, metric, alpha, 10)
        assert_same((ids[keep], sc[keep], cnt[keep]), (want[0][keep], want[1][keep], want[2][keep]), [qs[i] for i in keep])
        assert_same(gpu.suggest_batch(blob=qb, offs=qo, metric=metric, similarity=alpha, k=10), want, qs)      # the native metric


def test_slots_are_shared_by_the_launches_of_several_threads(dense, monkeypatch):
    """Four scratch slots, up to eight workgroups a launch, three host threads (a stream each) on one handle: every batch of 12
    long and 200 short queries comes back as the rows of a single-threaded call, which are the oracle's."""
    d, ora = dense
    gpu = _dense_gpu(d, monkeypatch, 2)
    qs = lq.thread_batch(d)
    qb, qo = oracle.pack_strings(qs)
    want = gpu.suggest_batch(blob=qb, offs=qo, metric="cosine", similarity=0.3, k=10)
    assert_same(want, ora.suggest_batch(qb, qo, "cosine", 0.3, 10), qs)
    errors = []

    def worker():
        try:
            for _ in range(3):
                assert_same(gpu.suggest_batch(blob=qb, offs=qo, metric="cosine", similarity=0.3, k=10), want, qs)
        except BaseException as exc:  # noqa: BLE001
            errors.append(repr(exc))

    threads = [threading.Thread(target=worker, daemon=True) for _ in range(3)]
    [t.start() for t in threads]
    [t.join(60) for t in threads]
    assert not any(t.is_alive() for t in threads), "a launch did not come back within 60 s"
    assert not errors, errors


@pytest.mark.parametrize("case", sorted(lq.LIMIT_CASES))
def test_limits(case):
    """Queries on both sides of every limit of a slot (SG_LONG_MAX_TERMS windows, 65 536 bytes, the hash table from 64 words to
    SG_LONG_HASH), at q = 1, 2, 3, 5 and 8, two-byte letters (the sequential decode over 32 768 runes and more), texts that are
    all or nearly all spaces: the flagged ones are SG_COUNT_TOO_LONG between answered ones, every other row is the oracle's."""
    c = lq.LIMIT_CASES[case]
    L = lq.limits(case)
    qs = L["queries"]
    gpu = _index(L["docs"], L["desc"])
    ora = oracle.OracleIndex(L["docs"], **L["desc"])
    qb, qo = oracle.pack_strings(qs)
    keep = np.array([i for i in range(len(qs)) if i != L["flagged"]])
    for metric, alpha, k in (("cosine", 0.5, 10),) + ((("overlap", 0.3, 70),) if case == "q2_36" else ()):
        ids, sc, cnt = gpu.suggest_batch(blob=qb, offs=qo, metric=metric, similarity=alpha, k=k)
        want = ora.suggest_batch(qb, qo, metric, alpha, k)
        if L["flagged"] is not None:
            assert cnt[L["flagged"]] == lq.COUNT_TOO_LONG
        assert_same((ids[keep], sc[keep], cnt[keep]), (want[0][keep], want[1][keep], want[2][keep]), [qs[i][:60] for i in keep])
        assert all(cnt[i] >= 1 for i in L["on_document"])
    if c.get("doc_65536"):
        # build_tokenize_long at the slot's limit: a document of exactly 65 536 bytes through the device builder
        from suggest_amd import NGramIndex, IndexDescription
        assert NGramIndex(L["docs"], IndexDescription(**L["desc"]), upload=False, build="device").digest() == gpu.digest()
