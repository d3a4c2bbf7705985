"""Tabulated metrics that behave differently from the five of pkg/metric (foreign_metric_shapes.py) through every launch a
tabulated metric can take, against the brute-force statement of the reference's Suggest (foreign_metric_ref.py): ids, the bits of
the scores, counts and both flags, every call with the scratch and the result rows poisoned (sg_debug_poison).

The ladder (2 080 documents, every (|A|, |B|, overlap) cell with 1 .. 64) passes 4 x 2^9 counters, so under SG_LOG2_CNT=9 the fused
kernel leaves its counter-per-document path; `pipeline` is sg_plan_kernel -> stream -> verify (plan2 refuses tables), where
k = 2 080 keeps the top-k rows in HBM.  The long ladder (about 200 symbols) sends queries of 129 .. 200 n-grams to sg_long_kernel.
NaN scores are out of scope."""
import ctypes as C

import numpy as np
import pytest

import foreign_metric_ref as ref
import foreign_metric_shapes as fm
import oracle

pytestmark = pytest.mark.gpu

N_Q = len(fm.QUERIES)


class World:
    def __init__(self, g8=None):
        from suggest_amd import IndexDescription, NGramIndex
        with pytest.MonkeyPatch.context() as mp:
            if g8 is not None:
                mp.setenv("SG_G8", str(g8))                    # (read at the first upload: inside the constructor)
            self.gpu = NGramIndex(fm.DOCS, IndexDescription(**fm.DESC))
        assert self.gpu.stats()["n_segments"] == fm.S_LADDER
        self.packed = oracle.pack_strings(fm.QUERIES)
        self._tables = {}

    def tables(self, family, name, s):
        if (name, s) not in self._tables:
            self._tables[name, s] = self.gpu.metric_tables(family[name], s, 64)
        return self._tables[name, s]

    def rows(self, k, pipeline=False, **how):
        """one poisoned call of the ladder's 64 queries; asserts whether it took the three launches"""
        from suggest_amd._lib import poisoned
        qb, qo = self.packed
        before = self.gpu.pipe_stats()
        with poisoned(1):
            got = self.gpu.suggest_batch(blob=qb, offs=qo, k=k, **how)
        after = self.gpu.pipe_stats()
        assert after["queries"] - before["queries"] == (N_Q if pipeline else 0), (pipeline, how)
        self.left = {x: after[x] - before[x] for x in ("unplanned", "overflow", "repeats")}     # queries the fused kernel took back
        return got


@pytest.fixture(scope="module")
def brute():
    docs, queries = fm.ladder_tokens()
    return ref.BruteForce(docs, queries, fm.S_LADDER), fm.family()


@pytest.fixture(scope="module")
def world():
    w = World()
    yield w
    w.gpu.close()


@pytest.fixture(scope="module")
def world_g8():
    w = World(g8=2)
    yield w
    w.gpu.close()


def _check(w, brute, name, k, launch, extra=None):
    """the three similarities of one (metric, k) under one launch -> nothing differs from the brute force"""
    bf, family = brute
    knobs, pipeline = fm.LAUNCHES[launch]
    differ = []
    try:
        w.gpu.tune(**dict(knobs, **(extra or {})))
        for s in fm.SIMILARITIES:
            want = bf.suggest(family[name], s, k)
            got = w.rows(k, pipeline, tables=w.tables(family, name, s))
            if pipeline:
                print("%s >= %s k = %d %s: of %d queries the fused kernel took back %s" % (name, s, k, extra or "", N_Q, w.left))
                if extra and "SG_PIPE_CAND_CAP" in extra:
                    assert sum(w.left.values()) < N_Q, (name, s, k, w.left)       # the plan, stream and verify launches answered some
            d = ref.differences(got, want)
            if d:
                differ.append((s, d))
            if pipeline:                                       # plan2 refuses tables: with it on or off, sg_plan_kernel plans them
                w.gpu.tune(SG_PLAN2=0)
                other = w.rows(k, pipeline, tables=w.tables(family, name, s))
                w.gpu.tune(SG_PLAN2=1)
                d = ref.differences(other, want)
                if d:
                    differ.append((s, "SG_PLAN2=0", d))
    finally:
        w.gpu.tune(SG_PLAN2=1, SG_ROOMY=2, SG_SPLIT_CHUNKS=65536, SG_PIPE_CAND_CAP=64, **fm.DEFAULTS)
    assert not differ, (name, k, launch, extra, differ[:4])


@pytest.mark.parametrize("k", fm.KS)
@pytest.mark.parametrize("launch", list(fm.LAUNCHES))
@pytest.mark.parametrize("name", sorted(fm.REQUIRED))
def test_rows_under_every_launch(world, brute, name, launch, k):
    _check(world, brute, name, k, launch)


@pytest.mark.parametrize("k", fm.KS)
@pytest.mark.parametrize("name", sorted(fm.REQUIRED))
def test_rows_of_queries_that_stay_in_the_pipeline(world, brute, name, k):
    """The ladder's `pipeline` launch has 64 candidate slots per query, and result sets of hundreds send all but 2 .. 17 of the 64
    queries back to the fused kernel (the figures are printed).  With 4 096 slots, 11 .. 64 stay with the plan, stream and verify
    launches (measured on an MI355X; fewest at the low similarity): Wobbly's falling thresholds in the plan's groups among them."""
    _check(world, brute, name, k, "pipeline", dict(SG_PIPE_CAND_CAP=4096))


VARIANTS = {
    "tighten-always": dict(SG_TIGHTEN=1),
    "tighten-never": dict(SG_TIGHTEN=0),
    "parts": dict(SG_SPLIT_CHUNKS=8),
    "queue-small": dict(SG_ROOMY=0),
    "queue-large": dict(SG_ROOMY=1),
}


@pytest.mark.parametrize("k", fm.KS)
@pytest.mark.parametrize("variant", list(VARIANTS))
@pytest.mark.parametrize("name", sorted(fm.REQUIRED))
def test_rows_past_the_counter_per_document_path(world, brute, name, variant, k):
    _check(world, brute, name, k, "counters-512", VARIANTS[variant])


@pytest.mark.parametrize("k", fm.KS)
@pytest.mark.parametrize("name", sorted(fm.REQUIRED))
def test_rows_from_8_bit_gaps(world_g8, brute, name, k):
    _check(world_g8, brute, name, k, "counters-512")


@pytest.mark.parametrize("name", sorted(fm.REQUIRED))
def test_both_routes_to_tables(world, brute, name):
    """suggest_batch(queries, metric object) tabulates by itself; an explicit metric_tables handle serves two calls"""
    bf, family = brute
    s, k = 0.5, 10
    want = bf.suggest(family[name], s, k)
    from suggest_amd._lib import poisoned
    with poisoned(2):
        auto = world.gpu.suggest_batch(fm.QUERIES, family[name], s, k)
    assert not ref.differences(auto, want), (name, ref.differences(auto, want))
    tb = world.gpu.metric_tables(family[name], s, 64)
    first = world.rows(k, tables=tb)
    second = world.rows(65, tables=tb)
    assert not ref.differences(first, want) and not ref.differences(second, bf.suggest(family[name], s, 65))
    tb.close()


@pytest.mark.parametrize("name", ["wobbly", "above", "below"])
def test_every_candidate_by_document(world, brute, name):
    """sg_suggest_batch_from with tables: pages of 7 and of 5 000; the multiset of (docID, score bits) is the brute force's at
    k = everything, and aux carries the segment and the overlap the score came from"""
    bf, family = brute
    m, s = family[name], 0.5
    tb = world.tables(family, name, s)
    cands = bf.candidates(m, s)
    from suggest_amd._lib import poisoned
    paged = 0
    with poisoned(1):
        for qi, q in enumerate(fm.QUERIES):
            c = cands[qi]
            if not isinstance(c, tuple):                        # flagged: the batch call says which flag
                cnt = world.gpu.suggest_batch_from([q], m, s, 0, 16, tables=tb)[3]
                assert int(cnt[0]) == c, (name, qi)
                continue
            want = sorted(zip(c[0].tolist(), c[1].view(np.uint64).tolist(), c[2].tolist(), c[3].tolist()))
            for page in (7, 5000):
                if page == 7 and (qi % 8 != 3 or len(want) > 800):       # (a hundred pages at the most)
                    continue
                rows = world.gpu.suggest_all(q, m, s, page=page, tables=tb)
                assert [r[0] for r in rows] == sorted(r[0] for r in rows)
                got = sorted((d, int(np.float64(x).view(np.uint64)), seg, ov) for d, x, ov, seg in rows)
                assert got == want, (name, qi, page, got[:3], want[:3])
                paged += page == 7 and len(want) > 7
    assert paged >= 3


# ---- the long ladder: sg_long_kernel with tables ------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def long_world():
    from suggest_amd import IndexDescription, NGramIndex
    gpu = NGramIndex(fm.LONG_DOCS, IndexDescription(**fm.LONG_DESC))
    assert gpu.stats()["n_segments"] == fm.LONG_S
    docs, queries = fm.long_tokens()
    yield gpu, ref.BruteForce(docs, queries, fm.LONG_S), fm.family(fm.LONG_S)
    gpu.close()


@pytest.mark.parametrize("name", ["tversky", "wobbly", "above"])
def test_long_queries(long_world, name):
    """queries of 129 .. 200 n-grams under tables of a_max = 200 built with numpy; the one of 201 comes back SG_COUNT_TOO_LONG
    between answered neighbours; Above flags 199 (dead-lock) and 200 (panic)"""
    from suggest_amd import _lib
    from suggest_amd._lib import poisoned
    from suggest_amd.index import MetricTables
    gpu, bf, family = long_world
    m, s = family[name], 0.5
    over = 40
    qs = fm.LONG_QUERIES[:over] + [fm.LONG_OVER] + fm.LONG_QUERIES[over:]
    keep = np.array([i for i in range(len(qs)) if i != over])
    qb, qo = oracle.pack_strings(qs)
    mn, mx, thr, score = fm.numpy_tables(m, s, fm.LONG_A_MAX, fm.LONG_S)
    h = C.c_void_p()
    _lib.check(_lib.lib().sg_metric_tables_create(gpu._h, fm.LONG_A_MAX, mn.ctypes.data, mx.ctypes.data, thr.ctypes.data, score.ctypes.data, C.byref(h)))
    tb = MetricTables(h, fm.LONG_A_MAX)
    for k in (10, len(fm.LONG_DOCS)):
        want = bf.suggest(m, s, k)
        with poisoned(1):
            ids, sc, cnt = gpu.suggest_batch(blob=qb, offs=qo, k=k, tables=tb)
        assert cnt[over] == ref.TOO_LONG
        d = ref.differences((ids[keep], sc[keep], cnt[keep]), want)
        assert not d, (name, k, d)
        if name == "above":
            assert want[2][-1] == ref.PANIC and want[2][-2] == ref.DEADLOCK and (want[2][:-2] >= 1).all()
        else:
            assert (want[2] >= 1).all() and (want[2] < ref.TOO_LONG).all()
    tb.close()


# ---- control: tables filled from the native formulas still give the native rows -----------------------------------------------
@pytest.mark.parametrize("metric,s", [("jaccard", 0.4), ("cosine", 0.55), ("dice", 0.3), ("overlap", 0.7), ("exact", 1.0)])
def test_native_backed_tables_equal_the_native_call(world, metric, s):
    from suggest_amd.metric import resolve

    class Opaque:                                              # a duck: no code, the built-in's four methods
        def __init__(self, inner):
            self.MinY, self.MaxY, self.Threshold, self.Distance = inner.MinY, inner.MaxY, inner.Threshold, inner.Distance
    qb, qo = world.packed
    tb = world.gpu.metric_tables(Opaque(resolve(metric)), s, 64)
    for k in (10, len(fm.DOCS)):
        native = world.gpu.suggest_batch(blob=qb, offs=qo, metric=metric, similarity=s, k=k)
        assert not ref.differences(world.rows(k, tables=tb), native), (metric, k)
    tb.close()
