"""The three outcomes of a query's window — rows, SG_COUNT_REF_DEADLOCK, SG_COUNT_REF_PANIC (query_window, engine.hip;
suggester.go:53-62) — through every planner that states them: the fused kernel, sg_plan2_kernel's halves (|A| <= 32) and
plan_one_query (|A| 33 .. 64, and every query with SG_PLAN2=0).  Counts, docIDs and score bits against the oracle, every row of
every call (tests/window_shapes.py; test_window_shapes_cpu.py pins what the calls give)."""
import numpy as np
import pytest

import oracle
import window_shapes as ws

pytestmark = pytest.mark.gpu

DEFAULTS = dict(SG_LOG2_CNT=11, SG_PIPE=2, SG_TIGHTEN=2, SG_PRETOK=2048, SG_PLAN2=1)
PIPELINE = dict(SG_LOG2_CNT=9, SG_PIPE=1, SG_TIGHTEN=0, SG_PRETOK=1)
# name -> (knobs, takes the pipeline)
LAUNCHES = {
    "fused": (dict(SG_PIPE=0), False),
    "pipeline-plan2": (dict(PIPELINE, SG_PLAN2=1), True),
    "pipeline-plan1": (dict(PIPELINE, SG_PLAN2=0), True),
}


@pytest.fixture(scope="module")
def shapes():
    from suggest_amd import IndexDescription, NGramIndex
    gpu = NGramIndex(ws.DOCS, IndexDescription(**ws.DESC))
    ora = oracle.OracleIndex(ws.DOCS, **ws.DESC)
    packed = oracle.pack_strings(ws.QUERIES)
    want = {c: ora.suggest_batch(*packed, c[0], c[1], ws.K)[:3] for c in ws.CALLS}     # the oracle's rows, once
    yield gpu, packed, want
    gpu.close()


@pytest.mark.parametrize("launch", list(LAUNCHES))
def test_rows_and_flags(shapes, launch):
    gpu, (qb, qo), want = shapes
    knobs, pipeline = LAUNCHES[launch]
    try:
        gpu.tune(**knobs)
        for call in ws.CALLS:
            w_ids, w_sc, w_cnt = want[call]
            before = gpu.pipe_stats()["queries"]
            ids, sc, cnt = gpu.suggest_batch(blob=qb, offs=qo, metric=call[0], similarity=call[1], k=ws.K)[:3]
            assert gpu.pipe_stats()["queries"] - before == (len(ws.QUERIES) if pipeline else 0), (launch, call)
            assert np.array_equal(cnt, w_cnt), (launch, call, "|A| =", (np.nonzero(cnt != w_cnt)[0][:8] + 1).tolist(), cnt.tolist(), w_cnt.tolist())
            assert ws.classes(cnt) == ws.CLASSES[call], (launch, call)
            valid = np.arange(ids.shape[1])[None, :] < np.where(cnt <= ws.K, cnt, 0)[:, None]     # (a flagged query has no rows)
            assert np.array_equal(ids[valid], w_ids[valid]), (launch, call)
            assert np.array_equal(sc.view(np.uint64)[valid], w_sc.view(np.uint64)[valid]), (launch, call)
    finally:
        gpu.tune(**DEFAULTS)
