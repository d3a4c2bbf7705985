"""The crafted Predict model of tests/predict_shapes.py against the CPU oracle alone (no GPU): for every (topK, similarity) the
device tests use, the batch holds queries of every kind those tests are about — otherwise a device test could pass without
ever reaching the path it is named after.  These are conditions on the inputs, not measurements of the product."""
import numpy as np
import pytest

import oracle
import predict_shapes as ps
from test_spell import _assert_same_predictions

AT_LEAST = 3


@pytest.fixture(scope="module")
def crafted(tmp_path_factory):
    m = ps.build(str(tmp_path_factory.mktemp("predict_shapes")))
    lm, ix = ps.open_oracle(m)
    return m, lm, ix


def test_the_model_is_what_the_issue_describes(crafted):
    m, lm, ix = crafted
    assert [g["size"] for g in m["groups"]] == list(ps.GROUP_SIZES)
    assert [len(f["completions"]) for f in m["families"]] == list(ps.FAMILY_COMPLETIONS)
    assert all(len(f["neighbours"]) == 140 for f in m["families"])
    assert sorted(len(c) for k, c in m["lists"].items() if k[1].startswith("cx") and k[1][2:].isdigit()) == list(ps.LIST_LENGTHS[1:])
    assert [len(m["lists"][p]) for p in m["pairs"].values()] == [64, 65]
    assert all(set(c.values()) <= {1, 2, 3} for c in m["lists"].values())
    assert len(m["long_stem"]) == 90 and all(145 <= len(w) <= 440 and w.startswith(m["stem"]) for w in m["long_stem"])
    assert len(m["long_other"]) == 30 and all(130 <= len(w) <= 500 for w in m["long_other"])
    assert len(set(m["vocab"])) == len(m["vocab"]) and m["vocab"] != sorted(m["vocab"])
    words = dict(ps.last_words(m, ix))
    assert len(ix.tokenize(words["long128"])) == 128 and len(ix.tokenize(words["long129"])) == 129
    for f in m["families"]:                                       # 70 of a base's neighbours score Cosine 0.5 against it
        qb, qo = oracle.pack_strings([f["base"]])
        ids, sc, cnt, _ = ix.suggest_batch(qb, qo, "cosine", 0.5, 200)
        assert int(cnt[0]) == 70 and {m["vocab"][i] for i in ids[0, :70]} <= set(f["neighbours"])
    qs = ps.queries(m, ix)
    assert b"" in qs and any(q != q.lower() for q in qs) and any(b"  " in q.strip() for q in qs)


def test_the_constructions_counts_are_the_oracles(crafted):
    """continuation_counts() (what conditions() ranks ties by) against LanguageModel.Next(context).ScoreNext(word) of the
    oracle: a scorer exactly where the construction has a list, -100 exactly where it has no count, and scores ordered as the counts"""
    m, lm, ix = crafted
    qs = ps.queries(m, ix)
    length, cont, last = ps.continuation_counts(m, lm, qs)
    rnd = np.random.RandomState(5)
    n_words = len(ps.last_words(m, ix))
    seen = set()
    for i in list(range(0, len(qs), n_words)) + [len(qs) - j for j in range(1, 9)]:      # a query of every context, and the variants
        ctx = [t.decode() for t in lm.tokenize(qs[i])][:-1]
        if not ctx:                                               # (spellchecker.go:94-107: no context, Next is not asked)
            assert length[i] == 0
            continue
        in_list = np.nonzero(cont[i])[0][:40].tolist()
        scored = []
        for w in in_list + rnd.randint(0, len(m["vocab"]), size=40).tolist():
            status, score = lm.next_score(ctx, m["vocab"][w])
            assert (status == 0) == (length[i] > 0), (qs[i], status)
            if status == 0:
                assert (score == -100.0) == (cont[i][w] == 0), (qs[i], m["vocab"][w])
                scored.append((int(cont[i][w]), score))
        for (c1, s1) in scored:
            for (c2, s2) in scored:
                assert (c1 < c2) == (s1 < s2) and (c1 == c2) == (s1 == s2)
        seen.add(int(length[i]))
    assert seen >= set(ps.LIST_LENGTHS)


@pytest.mark.parametrize("top_k,similarity", ps.GPU_CASES)
def test_conditions_are_not_vacuous(crafted, top_k, similarity):
    m, lm, ix = crafted
    c = ps.conditions(m, lm, ix, top_k, similarity)
    print(top_k, similarity, c)
    need = ["completions_at_least_top_k", "completions_above_top_k", "completions_below_top_k", "full_rows", "ties_nonzero", "ties_zero",
            "long_with_completions", "long_without_completions"]
    if top_k >= 64:
        need += ["rows_above_64", "rows_above_64_list_at_most_64", "rows_above_64_list_above_64"]
    else:
        assert c["rows_above_64"] == 0
    for name in need:
        assert c[name] >= AT_LEAST, (name, c)


def _context_rows(m, ix, oi, oc, context):
    n = len(ps.last_words(m, ix))
    at = m["contexts"].index(context) * n
    return oi[at:at + n], oc[at:at + n]


@pytest.mark.parametrize("top_k", (64, 100))
def test_the_oracles_rows_depend_on_the_re_rank(crafted, top_k):
    """the rows under the contexts of 64 and 65 continuations (one word and two) differ from those under the context never
    seen as one, same last words: a merge step that dropped the re-rank could not pass"""
    m, lm, ix = crafted
    oi, oc = lm.predict_batch(ix, *oracle.pack_strings(ps.queries(m, ix)), top_k, 0.3)
    plain_i, plain_c = _context_rows(m, ix, oi, oc, m["ctx_word"][0] + " ")
    for context in [m["ctx_word"][64] + " ", m["ctx_word"][65] + " "] + ["%s %s " % p for p in m["pairs"].values()]:
        ri, rc = _context_rows(m, ix, oi, oc, context)
        assert np.array_equal(rc, plain_c)                        # the same candidates ...
        assert ((ri != plain_i).any(axis=1)).sum() >= 10, context    # ... in another order


def test_the_row_check_fails_on_two_tied_ids_swapped(crafted):
    m, lm, ix = crafted
    qs = ps.queries(m, ix)
    top_k, sim = 100, 0.3
    oi, oc = lm.predict_batch(ix, *oracle.pack_strings(qs), top_k, sim)
    _assert_same_predictions(ps.Replay(oi, oc), lm, ix, qs, top_k, sim)          # the oracle's own rows pass
    length, cont, _ = ps.continuation_counts(m, lm, qs)
    swapped = 0
    for want in (0, 2):                                           # two candidates without a count; two of count 2
        bad = oi.copy()
        for i in np.nonzero((length > 64) & (oc > 64) & (oc < ps.SPECIAL))[0]:
            c = cont[i][oi[i, :int(oc[i])]]
            j = np.nonzero((c[:-1] == want) & (c[1:] == want))[0]
            if want == 0:
                j = j[j >= 64]                                    # (beyond a wavefront's first pass over the row)
            if j.size:
                bad[i, j[0]], bad[i, j[0] + 1] = oi[i, j[0] + 1], oi[i, j[0]]
                swapped += 1
                break
        with pytest.raises(AssertionError, match="rows differ"):
            _assert_same_predictions(ps.Replay(bad, oc), lm, ix, qs, top_k, sim)
    assert swapped == 2
    with pytest.raises(AssertionError, match="counts differ"):
        _assert_same_predictions(ps.Replay(oi, np.where(oc == top_k + 1, top_k, oc).astype(np.uint32)), lm, ix, qs, top_k, sim)
