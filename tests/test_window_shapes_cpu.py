"""The inputs of tests/window_shapes.py against the CPU oracle alone (no GPU): the dictionary is what its header says, and
every call gives rows and both window flags where test_gpu_window_flags.py needs them — in sg_plan2_kernel's range of queries
(|A| <= 32) and in plan_one_query's (33 .. 64).  These are conditions on the inputs, not measurements of the product."""
import pytest

import oracle
import window_shapes as ws


@pytest.fixture(scope="module")
def ora():
    return oracle.OracleIndex(ws.DOCS, **ws.DESC)


def test_the_dictionary_is_what_the_header_says(ora):
    assert len(ws.SYMBOLS) == len(set(ws.SYMBOLS)) == 64 and "~" not in ws.SYMBOLS and " " not in ws.SYMBOLS
    assert len(ws.DOCS) == 2640 == len(set(ws.DOCS)) and len(ws.DOCS) > 4 * 512      # past a counter per document at SG_LOG2_CNT=9
    assert ora.n_segments == 9 and {len(ora.tokenize(d)) for d in ws.DOCS} == set(range(1, 9))
    assert len(ws.QUERIES) == 64 and all(len(ora.tokenize(q)) == a + 1 for a, q in enumerate(ws.QUERIES))


@pytest.mark.parametrize("call", ws.CALLS, ids=lambda c: "%s-%g" % c)
def test_the_oracles_classes(ora, call):
    metric, similarity = call
    qb, qo = oracle.pack_strings(ws.QUERIES)
    cnt = ora.suggest_batch(qb, qo, metric, similarity, ws.K)[2]
    assert ws.classes(cnt) == ws.CLASSES[call], (call, ws.classes(cnt))


def test_both_planners_see_rows_and_both_flags():
    low, high = [tuple(sum(ws.CLASSES[c][h][i] for c in ws.CALLS) for i in range(4)) for h in (0, 1)]
    assert all(n > 0 for n in low[:3]) and all(n > 0 for n in high[:3]), (low, high)
