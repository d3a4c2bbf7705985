"""The stream kernel's group entry and sub-row cut (suggest_amd/csrc/pipeline.inc: `enter()`, the window's cut) over every path
they have: rows of the three launches (SG_PIPE=1) against the fused kernel's (SG_PIPE=0) and the CPU oracle's — ids, score bit
patterns, counts — with the scratch and the result rows poisoned (sg_debug_poison), so that a counter word or a sub-row
descriptor no launch of this call wrote shows.

What the shapes are for:
  * the clear of a group's counters runs 2^lg / (NW * 256) passes: NW in {2, 4, 8} x SG_PIPE_LOG2_CNT in {9, 11, 13} is 1/4 of a
    pass (8 x 2^9; a group of 2^8 words: 1/8) up to sixteen (2 x 2^13).  A group takes lg = ceil(log2(buckets needed)) within
    [8, the launch's]: the query "a" has one n-gram, "$a$", which only the document "a" holds — one list of one chunk,
    (7 postings x 255) >> 4 = 111 buckets at the most, lg = 8 below every launch's.  The test asserts that this query is planned
    with one group of one list (pipe_volumes), so the partial pass and the smaller group occur.
  * Cosine >= 0.4 on 2^9 counters with SG_T_FLOOR=2 and filter level 0 makes nearly a group per segment of the window.  Twenty-
    four queries of 38 .. 42 n-grams (three documents end to end, cut to 36 .. 40 bytes: the longest the plan takes here, n-grams
    x (segments of the window + 1) <= 1 280 table words; planned by plan_one_query inside the plan2 launch) then have some
    twenty-five groups of up to 42 lists.  Each is also sent alone (a call of one query is sampled whole), so its lists and rows
    are known exactly:
      - SG_PIPE_DT_BYTES=1024 holds 64 rows: a query of more rows goes through in several windows (the record staged again, the
        cut repeated); one such query at least is required.
      - a query of more than 446 lists (SG_PIPE_REC_LISTS) has an overflow block: groups in the record, groups in the block, and
        one with entries in both unless a group ends at list 446 exactly; one such query at least is required.
    On an MI355X all twenty-four are both (one query more of the batch goes back to the fused kernel there: 1 of 415).
  * an odd number of queries, some of 1 .. 3 n-grams: sg_plan2_kernel's halves without a partner and its reductions with idle
    lanes; calls of a single query likewise.
At most 1 % of a case's queries may go back to the fused kernel: otherwise the comparison says nothing about the stream."""
import numpy as np
import pytest

import oracle
from test_gpu_parity import assert_same

pytestmark = pytest.mark.gpu

REC_LISTS = 446          # SG_PIPE_REC_LISTS: lists of a stream record's head
N_DOCS = 60000
N_LONG = 24
SHORT = [b"a", b"b", b"ab", b"abc", b"q7", b"zzz", b"c"]      # 1 .. 3 n-grams under the "$" wrap; all of them documents too


class World:
    def __init__(self):
        from suggest_amd import NGramIndex, IndexDescription, pack_strings, synth
        blob, offs = synth.make_dict(N_DOCS, seed=5)
        docs = synth.unpack(blob, offs) + SHORT + [b"abcd", b"ab1", b"zzy"]     # (none repeats an n-gram)
        self.blob, self.offs = pack_strings(docs)
        qb, qo = synth.make_queries(384, blob, offs, seed=6)
        qs = synth.unpack(qb, qo)
        # three documents end to end, cut to 36 .. 40 bytes = 38 .. 42 n-grams (module docstring)
        self.long_ones = [(docs[7 * i] + docs[7 * i + 1] + docs[7 * i + 2])[:36 + i % 5] for i in range(N_LONG)]
        for i, s in enumerate(self.long_ones):
            qs.insert(5 + 13 * i, s)
        for i, s in enumerate(SHORT):                          # (in even and odd slots: either half of a plan2 wavefront)
            qs.insert(3 + 11 * i, s)
        assert len(qs) % 2 == 1
        self.queries = qs
        self.qb, self.qo = pack_strings(qs)
        self.gpu = NGramIndex(blob=self.blob, offs=self.offs, description=IndexDescription(**synth.DESCRIPTION))
        self.ora = oracle.OracleIndex(blob=self.blob, offs=self.offs, **synth.DESCRIPTION)
        self.pack = pack_strings
        self._want, self._fused = {}, {}

    def want(self, metric, alpha, k):
        key = (metric, alpha, k)
        if key not in self._want:
            self._want[key] = self.ora.suggest_batch(self.qb, self.qo, metric, alpha, k)
        return self._want[key]

    def fused(self, metric, alpha, k):
        from suggest_amd._lib import poisoned
        key = (metric, alpha, k)
        if key not in self._fused:
            self.gpu.tune(SG_PIPE=0)
            with poisoned(2):
                self._fused[key] = self.gpu.suggest_batch(blob=self.qb, offs=self.qo, metric=metric, similarity=alpha, k=k)
        return self._fused[key]

    def run(self, metric, alpha, k, **knobs):
        """the batch through the three launches under `knobs`, poisoned -> (rows, pipe_stats delta, pipe_volumes delta)"""
        from suggest_amd._lib import poisoned
        fused = self.fused(metric, alpha, k)                   # (before the knobs: it sets SG_PIPE=0)
        base = dict(SG_PIPE=1, SG_PRETOK=1, SG_TIGHTEN=0, SG_PIPE_SUB=4, SG_PIPE_WIDE=0, SG_PIPE_CAND_CAP=64, SG_T_FLOOR=8, SG_FILTER_LEVEL=4, SG_PLAN2=1)
        base.update(knobs)
        self.gpu.tune(**base)
        s0, v0 = self.gpu.pipe_stats(), self.gpu.pipe_volumes()
        with poisoned(1):
            rows = self.gpu.suggest_batch(blob=self.qb, offs=self.qo, metric=metric, similarity=alpha, k=k)
        s1, v1 = self.gpu.pipe_stats(), self.gpu.pipe_volumes()
        d = {x: s1[x] - s0[x] for x in s1}
        v = {x: v1[x] - v0[x] for x in ("sampled", "groups", "lists", "rows", "candidates")}
        print("knobs %s %s>=%s k=%d: stats %s volumes %s" % (knobs, metric, alpha, k, d, v))
        n_q = len(self.queries)
        assert d["queries"] == n_q, d                                           # the batch took the three launches ...
        assert d["unplanned"] + d["overflow"] + d["repeats"] <= n_q // 100, d   # ... and all but 1 % of its queries stayed there
        assert_same(rows, self.want(metric, alpha, k), self.queries)
        assert_same(rows, fused, self.queries)
        return rows, d, v

    def one(self, text, metric, alpha, k):
        """a call of one query (sampled whole: batches up to 1024 are) -> (rows, its groups, lists, rows of 64 lanes)"""
        from suggest_amd._lib import poisoned
        b, o = self.pack([text])
        v0 = self.gpu.pipe_volumes()
        with poisoned(1):
            rows = self.gpu.suggest_batch(blob=b, offs=o, metric=metric, similarity=alpha, k=k)
        v1 = self.gpu.pipe_volumes()
        return rows, v1["sampled"] - v0["sampled"], v1["groups"] - v0["groups"], v1["lists"] - v0["lists"], v1["rows"] - v0["rows"]


@pytest.fixture(scope="module")
def world():
    return World()


@pytest.mark.parametrize("lg", [9, 11, 13])
@pytest.mark.parametrize("nw", [2, 4, 8])
def test_clear_passes_from_a_fraction_to_sixteen(world, nw, lg):
    world.run("jaccard", 0.5, 10, SG_PIPE_NW=nw, SG_PIPE_LOG2_CNT=lg, SG_PIPE_DT_BYTES=4096)
    # a group below the launch's counters: "a" -> one group of one list of one chunk, lg = 8 (module docstring)
    rows, sampled, groups, lists, n_rows = world.one(b"a", "jaccard", 0.5, 10)
    assert (sampled, groups, lists, n_rows) == (1, 1, 1, 1), (sampled, groups, lists, n_rows)
    ids, sc, cnt = rows
    assert int(cnt[0]) == 1 and int(ids[0, 0]) == N_DOCS and float(sc[0, 0]) == 1.0, (cnt, ids, sc)     # the document "a" itself


LOW = dict(SG_PIPE_NW=4, SG_PIPE_LOG2_CNT=9, SG_PIPE_CAND_CAP=4096, SG_T_FLOOR=2, SG_FILTER_LEVEL=0)     # Cosine >= 0.4: nearly a group per segment


def test_queries_of_several_windows(world):
    world.run("cosine", 0.4, 10, SG_PIPE_DT_BYTES=1024, **LOW)
    dt_rows = 1024 // 4 // 4                                  # 4-byte descriptors, four sub-rows of 2^4 chunks to a row: 64 rows
    want = world.want("cosine", 0.4, 10)
    several = 0
    for q in world.long_ones:
        i = world.queries.index(q)
        rows, sampled, groups, lists, n_rows = world.one(q, "cosine", 0.4, 10)
        assert_same(rows, tuple(x[i:i + 1] for x in want[:3]))
        several += sampled == 1 and n_rows > dt_rows
    print("queries of more rows than the table's %d (several windows): %d of %d" % (dt_rows, several, len(world.long_ones)))
    assert several >= 1, several


def test_lists_in_the_record_in_the_block_and_across(world):
    world.run("cosine", 0.4, 10, SG_PIPE_DT_BYTES=4096, **LOW)
    want = world.want("cosine", 0.4, 10)
    over = 0
    for q in world.long_ones:
        i = world.queries.index(q)
        rows, sampled, groups, lists, _ = world.one(q, "cosine", 0.4, 10)
        assert_same(rows, tuple(x[i:i + 1] for x in want[:3]))
        over += sampled == 1 and lists > REC_LISTS
    print("queries with more than %d lists (an overflow block): %d of %d" % (REC_LISTS, over, len(world.long_ones)))
    assert over >= 1, over


def test_wide_descriptors(world):
    _, d, v = world.run("jaccard", 0.5, 10, SG_PIPE_NW=4, SG_PIPE_LOG2_CNT=11, SG_PIPE_DT_BYTES=4096, SG_PIPE_WIDE=1)
    assert world.gpu.pipe_volumes()["wide"]


def test_short_queries_alone_in_an_odd_batch(world):
    """seven queries of 1 .. 3 n-grams and nothing else: every plan2 wavefront holds short queries, the last one a single half"""
    from suggest_amd._lib import poisoned
    b, o = world.pack(SHORT)
    want = world.ora.suggest_batch(b, o, "jaccard", 0.5, 10)
    world.gpu.tune(SG_PIPE=1, SG_PRETOK=1, SG_TIGHTEN=0, SG_PLAN2=1, SG_PIPE_NW=8, SG_PIPE_LOG2_CNT=9, SG_PIPE_DT_BYTES=4096, SG_PIPE_WIDE=0, SG_PIPE_CAND_CAP=64,
                   SG_T_FLOOR=8, SG_FILTER_LEVEL=4)
    s0 = world.gpu.pipe_stats()
    with poisoned(1):
        rows = world.gpu.suggest_batch(blob=b, offs=o, metric="jaccard", similarity=0.5, k=10)
    s1 = world.gpu.pipe_stats()
    assert s1["queries"] - s0["queries"] == len(SHORT) and s1["unplanned"] == s0["unplanned"], (s0, s1)
    assert_same(rows, want, SHORT)
    assert int(np.minimum(rows[2], 10).sum()) >= len(SHORT)        # each finds itself at least
