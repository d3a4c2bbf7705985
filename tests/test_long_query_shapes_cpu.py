"""The inputs of tests/long_query_shapes.py against the CPU oracle alone (no GPU): the dictionaries and queries reach the edges
of the long-query kernel that test_gpu_long_queries.py is about — otherwise a device test could pass over empty rows or never
leave a single 64-lane group.  These are conditions on the inputs, not measurements of the product.

Bounds, and what this generator gives:
  dense():  segments of more than 64 documents            >= 20     92, the largest 442
            lists with raw > 256 and raw != len(stored)   >= 50     686 of 1 759 with raw > 256
            per call of DENSE_CALLS, of the 110 long queries:
              flagged                                      == 0      0, 0, 0, 0, 0
              full rows                                    >= 90 %   100, 105, 102, 102, 110
              rows that hold a docID more than once        >= 5      5, 5, 5, 7, 5
            jaccard 0.95 over 200 queries of 150-2 000 symbols: counts 0xFFFFFFFF and 0xFFFFFFFE both occur   158 and 8
            paging (dice 0.4): candidates 9, 129, 507, 2, 2, 1; five of the six rows repeat a docID; none skipped at page 3
            long prefixes: 10, 10, 1, 1 matches
  limits(): windows at the limit 65 536, one past it 65 537 (q = 3, 2, 1); S between 28 and 1 731
"""
from collections import Counter

import numpy as np
import pytest

import long_query_shapes as lq
import oracle


@pytest.fixture(scope="module")
def dense():
    d = lq.dense()
    ora = oracle.OracleIndex(d["docs"], **lq.DENSE_DESC)
    return d, ora


def test_dense_segments_and_lists(dense):
    d, ora = dense
    assert 19000 <= len(d["docs"]) <= 21000 and all(20 <= len(x) <= 220 and set(x) <= set(b"abcd ") for x in d["docs"])
    per_segment = Counter(len(ora.tokenize(x)) for x in d["docs"])
    assert sum(1 for n in per_segment.values() if n > 64) >= 20, sorted(per_segment.values())[-5:]
    big = [(raw, stored) for raw, stored in ora.lists().values() if raw > 256]
    assert sum(1 for raw, stored in big if raw != len(stored)) >= 50, len(big)


def test_dense_batch_mixes_long_and_short(dense):
    d, ora = dense
    qs = d["queries"]
    long_ = lq.long_set(ora, lq.DENSE_DESC, qs)
    assert len(long_) >= 52 and len(qs) - len(long_) == 100
    assert sum(1 for i in long_ if set(qs[i]) <= set(b"abcd ") and 150 <= len(qs[i]) <= 400) >= 40
    assert sum(1 for i in long_ if qs[i].endswith(b"z") and qs[i][:-1] in {x[:len(qs[i]) - 1] for x in d["docs"] if len(x) >= 200}) >= 12
    runs = sum(1 for i in range(1, len(qs)) if (i in long_) != (i - 1 in long_))
    assert runs >= 40                                            # the two kinds alternate: the hand-over happens all through the batch


@pytest.mark.parametrize("call", lq.DENSE_CALLS)
def test_dense_rows_are_full_and_repeat_documents(dense, call):
    d, ora = dense
    metric, alpha, k = call
    qs = d["queries"]
    long_ = sorted(lq.long_set(ora, lq.DENSE_DESC, qs))
    ids, sc, cnt, _ = ora.suggest_batch(*oracle.pack_strings(qs), metric, alpha, k)
    assert not any(cnt[i] >= 0xFFFFFFF0 for i in long_)
    full = sum(1 for i in long_ if cnt[i] == k)
    repeats = sum(1 for i in long_ if len(set(ids[i, :cnt[i]].tolist())) != cnt[i])
    print(call, "long", len(long_), "full", full, "rows with a repeated docID", repeats)
    assert full >= 0.9 * len(long_), (full, len(long_))
    assert repeats >= 5, repeats


def test_dense_high_similarity_flags_both_ways(dense):
    d, ora = dense
    qs = d["flag_queries"]
    assert len(qs) <= 200 and len(lq.long_set(ora, lq.DENSE_DESC, qs)) == len(qs)
    cnt = ora.suggest_batch(*oracle.pack_strings(qs), *lq.FLAG_CALL)[2]
    print("panic", int((cnt == lq.COUNT_PANIC).sum()), "dead-lock", int((cnt == lq.COUNT_DEADLOCK).sum()))
    assert (cnt == lq.COUNT_PANIC).any() and (cnt == lq.COUNT_DEADLOCK).any()


def test_dense_paging_queries(dense):
    d, ora = dense
    metric, alpha = lq.PAGING
    qs = d["paging"]
    assert len(qs) == 6 and len(lq.long_set(ora, lq.DENSE_DESC, qs)) == 6
    n_repeat = n_page3 = 0
    for q in qs:
        ids, sc, cnt, _ = ora.suggest_batch(*oracle.pack_strings([q]), metric, alpha, 2 * len(d["docs"]))
        n = int(cnt[0])
        assert n < 0xFFFFFFF0
        n_repeat += len(set(ids[0, :n].tolist())) != n
        n_page3 += n >= 1 and n / 3 <= 300
        assert n / 64 <= 300
    assert n_repeat >= 2 and n_page3 >= 4, (n_repeat, n_page3)


def test_dense_long_prefixes(dense):
    d, ora = dense
    ps = d["prefixes"]
    assert len(ps) == 4 and len(lq.long_set(ora, lq.DENSE_DESC, ps, autocomplete=True)) == 4
    assert all(any(x.startswith(p) for x in d["docs"]) for p in ps)
    cnt = ora.autocomplete_batch(*oracle.pack_strings(ps), len(d["docs"]))[1]
    assert (cnt >= 1).all() and (cnt > 7).sum() >= 2, cnt


def test_thread_batch(dense):
    d, ora = dense
    qs = lq.thread_batch(d)
    assert len(qs) == 212 and len(lq.long_set(ora, lq.DENSE_DESC, qs)) == 12


def test_table_dictionary():
    t = lq.table_dictionary()
    ora = oracle.OracleIndex(t["docs"], **lq.DENSE_DESC)
    qs = t["queries"]
    long_ = lq.long_set(ora, lq.DENSE_DESC, qs)
    n_grams = [len(ora.tokenize(q)) for q in qs]
    assert t["over"] in long_ and n_grams[t["over"]] > lq.TABLE_A_MAX
    assert len(long_) >= 13 and all(n_grams[i] <= lq.TABLE_A_MAX for i in range(len(qs)) if i != t["over"])
    assert 0 < t["over"] < len(qs) - 1                           # it has neighbours
    cnt = ora.suggest_batch(*oracle.pack_strings(qs), "jaccard", 0.5, 10)[2]
    assert sum(1 for i in long_ if i != t["over"] and 1 <= cnt[i] <= 10) >= 12


@pytest.mark.parametrize("case", sorted(lq.LIMIT_CASES))
def test_limit_cases(case):
    c = lq.LIMIT_CASES[case]
    L = lq.limits(case)
    desc, qs = L["desc"], L["queries"]
    ora = oracle.OracleIndex(L["docs"], **desc)
    assert ora.n_segments < 2000                                  # (seg_off is dense: n_terms x (S + 1) words)
    for i, w in L["expect_windows"].items():
        assert lq.windows(desc, qs[i]) == w, (i, w)
        assert not any(b == 0x20 for b in qs[i])
    assert sorted(set(L["expect_windows"].values()) & {255, 256, 257, 4095, 4096, 4097, 32767, 32768, 32769}) == \
        [255, 256, 257, 4095, 4096, 4097, 32767, 32768, 32769]
    long_ = lq.long_set(ora, desc, qs)
    assert set(L["expect_windows"]) | set(L["on_document"]) <= long_ and len(qs) - len(long_) >= 3
    if c["answered"] is not None:
        a = L["answered"]
        assert len(qs[a]) == c["answered"] and lq.windows(desc, qs[a]) == lq.runes_of(qs[a]) + 2 - c["q"] + 1
        if c["flagged"] is not None:
            f = L["flagged"]
            assert len(qs[f]) == c["flagged"] and 0 < a < f < len(qs) - 1 and f + 1 in L["on_document"]
            # one side of the limit and the other: 65 536 windows or bytes are taken, one more is not
            assert lq.windows(desc, qs[a]) == lq.LONG_MAX and len(qs[a]) <= lq.LONG_MAX
            assert lq.windows(desc, qs[f]) == lq.LONG_MAX + 1
            assert (len(qs[f]) > lq.LONG_MAX) == (case == "q3_12")      # the byte guard there, the window guard in the others
        if case == "q3_cyr":
            assert lq.runes_of(qs[a]) >= 32768 and any(b >= 0x80 for b in qs[a])
    else:
        assert [len(ora.tokenize(qs[i])) for i in sorted(L["spaces"])] == [1, 0, 0, len(ora.tokenize(qs[sorted(L["spaces"])[3]]))]
        assert len(qs[sorted(L["spaces"])[2]]) == lq.LONG_MAX
    if c.get("doc_65536"):
        assert max(len(x) for x in L["docs"]) == lq.LONG_MAX
    ids, sc, cnt, _ = ora.suggest_batch(*oracle.pack_strings(qs), "cosine", 0.5, 10)
    for i in L["on_document"]:
        assert 1 <= cnt[i] <= 10, (i, cnt[i])
    for i, want in L["spaces"].items():
        assert (cnt[i] == 0) if want == 0 else (1 <= cnt[i] <= 10), (i, cnt[i])
