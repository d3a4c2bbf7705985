"""What the search entry points answer to bad arguments, over an uploaded index (entry_check_cases.py has the table): k = 0 and
k = SG_MAX_TOPK + 1, similarity 0.0 and 1.5, metric 99, each required pointer null in turn, each bad value together with each
null pointer (the value's message wins), a null index — the return code, the exact sg_last_error() text, and output arrays left
as they were.  Every refusal comes before anything is enqueued: the test
launches nothing but the uploads of its fixtures."""
import os

import pytest

import entry_check_cases as ec
from conftest import CARS_DESC, GOLDEN

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def world(cars_lines):
    from suggest_amd import IndexDescription, NGramIndex, _lib
    from suggest_amd.dictionary import DeviceDictionary
    from suggest_amd.metric import JaccardMetric
    from suggest_amd.sharded import ShardedIndex
    from suggest_amd.spell import LanguageModel
    lines, desc = cars_lines[:100], IndexDescription(**CARS_DESC)
    ix = NGramIndex(lines, desc)
    sharded = ShardedIndex(lines, description=desc, n_shards=2)
    dictionary = DeviceDictionary(lines)
    tables = ix.metric_tables(JaccardMetric(), 0.5, 16)
    lm = LanguageModel(os.path.join(GOLDEN, "lm"), 3)
    yield {"index": ix._h, "sharded": sharded._h, "handles": {"lm": lm._h, "dict": dictionary._h, "tables": tables._h},
           "max_topk": _lib.SG_MAX_TOPK}
    for o in (tables, lm, dictionary, sharded, ix):
        o.close()


@pytest.mark.parametrize("entry", ec.ENTRIES, ids=lambda e: e.name)
def test_entry_point_refuses_bad_arguments(world, entry):
    L, bufs = ec.raw_lib(), ec.Buffers()
    cases = ec.value_cases(entry, world["max_topk"]) + ec.pointer_cases(entry) + ec.order_cases(entry, world["max_topk"])
    assert len(cases) >= 2
    for kw, want_rc, want_msg in cases:
        bufs.reset()
        rc, msg = entry.call(L, world[entry.handle], bufs, world["handles"], **kw)
        assert (rc, msg) == (want_rc, want_msg), (entry.name, kw)
        assert bufs.untouched(), (entry.name, kw)
    # a null index is refused before its values are looked at
    bufs.reset()
    rc, msg = entry.call(L, None, bufs, world["handles"], k=0)
    assert (rc, msg) == (ec.SG_E_INVALID, ec.null_handle_message(entry)), entry.name
    assert bufs.untouched(), entry.name
