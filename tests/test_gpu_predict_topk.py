"""SpellChecker.Predict on the device at topK 32 .. 1023 (the largest sg_spell_predict_batch takes), with last words beyond the
wavefront kernel's 128 n-grams, with its fuzzy top-up going through the plan -> stream -> verify pipeline, and in batches
whose top-k rows pass 1 GiB (launch() cuts them into pieces) — against the CPU oracle, on the crafted model of
tests/predict_shapes.py.  Rows are word ids and counts: compared exactly.  Every test first asserts, from the oracle and the
construction alone (predict_shapes.conditions, held to >= 3 of every kind by tests/test_predict_shapes_cpu.py), that its batch
holds the queries it is about; then it asks the device."""
import numpy as np
import pytest

import oracle
import predict_shapes as ps
from test_gpu_lm_orders import _assert_entry_points_agree
from test_gpu_parity import assert_same
from test_gpu_scratch import _twice
from test_spell import SPELL_INDEX, _assert_same_predictions, _write_lm

pytestmark = pytest.mark.gpu


def _open(directory):
    from suggest_amd import LanguageModel, SpellChecker
    return SpellChecker(LanguageModel(directory, ps.ORDER, alphabet=ps.ALPHA))


@pytest.fixture(scope="module")
def crafted(tmp_path_factory):
    import torch  # noqa: F401  (before the library: both must resolve the same libamdhip64, suggest_amd/_lib.py)
    m = ps.build(str(tmp_path_factory.mktemp("predict_topk")))
    lm, ix = ps.open_oracle(m)
    return m, _open(m["directory"]), lm, ix


def _assert_conditions(m, lm, ix, top_k, similarity):
    c = ps.conditions(m, lm, ix, top_k, similarity)
    for name in ("completions_at_least_top_k", "completions_above_top_k", "completions_below_top_k", "ties_nonzero", "ties_zero",
                 "long_with_completions", "long_without_completions"):
        assert c[name] >= 3, (name, c)
    if top_k >= 32:
        assert c["full_rows"] >= 3, c
    if top_k >= 64:
        assert min(c["rows_above_64"], c["rows_above_64_list_at_most_64"], c["rows_above_64_list_above_64"]) >= 3, c
    return c


def _same_rows(a, b, what):
    """two (ids, counts) of the device: equal counts, equal counted entries"""
    (ai, ac), (bi, bc) = a, b
    assert np.array_equal(ac, bc), (what, "counts differ", np.nonzero(ac != bc)[0][:5])
    valid = (np.arange(ai.shape[1])[None, :] < np.minimum(ac, ai.shape[1])[:, None]) & (ac < ps.SPECIAL)[:, None]
    rows = np.nonzero((valid & (ai != bi)).any(axis=1))[0]
    assert rows.size == 0, (what, "rows differ", rows[:5])


@pytest.mark.parametrize("similarity", ps.SIMILARITIES)
@pytest.mark.parametrize("top_k", ps.LARGE_TOP_KS)
def test_predict_at_large_top_k(crafted, top_k, similarity):
    m, sc, lm, ix = crafted
    _assert_conditions(m, lm, ix, top_k, similarity)
    _assert_same_predictions(sc, lm, ix, ps.queries(m, ix), top_k, similarity)


@pytest.mark.parametrize("top_k", (100, 1023))
def test_device_entry_point_at_large_top_k(crafted, top_k):
    m, sc, lm, ix = crafted
    _assert_conditions(m, lm, ix, top_k, 0.3)
    qb, qo = oracle.pack_strings(ps.queries(m, ix))
    cnt = _assert_entry_points_agree(sc, qb, qo, top_k, 0.3)
    assert np.array_equal(cnt, lm.predict_batch(ix, qb, qo, top_k, 0.3)[1])


def test_top_k_limit(crafted):
    m, sc, lm, ix = crafted
    queries = ps.queries(m, ix)[:40]
    ids, cnt = sc.predict_batch(queries, top_k=1023, similarity=0.3)
    assert ids.shape == (40, 1024) and (cnt > 0).any()
    with pytest.raises(Exception, match="1023"):
        sc.predict_batch(queries, top_k=1024, similarity=0.3)


def _knob(index, name):
    from suggest_amd.index import knobs
    return next(r["value"] for r in knobs(index) if r["name"] == name)


@pytest.mark.parametrize("top_k", (64, 100))
def test_rows_do_not_depend_on_the_counter_knobs_at_large_top_k(crafted, top_k):
    """SG_LOG2_CNT 9, 11, 13: the LDS the counters leave decides between the slim and the full instantiation of the LM
    collector's kernel (LaunchPlan::slim), and at 9 the vocabulary is above the one-counter-per-document size.  Nothing tells
    which instantiation ran: the rows are all there is to assert."""
    m, sc, lm, ix = crafted
    _assert_conditions(m, lm, ix, top_k, 0.2)
    before = _knob(sc.index, "SG_LOG2_CNT")
    try:
        for log2_cnt in (9, 11, 13):
            sc.index.tune(SG_LOG2_CNT=log2_cnt)
            _assert_same_predictions(sc, lm, ix, ps.queries(m, ix), top_k, 0.2)
    finally:
        sc.index.tune(SG_LOG2_CNT=before)


@pytest.mark.parametrize("top_k", (5, 100))
def test_predict_over_8_bit_gaps_at_large_top_k(crafted, monkeypatch, top_k):
    """SG_G8=2 (every term's list in 8-bit gaps): sg_lm_kernel_g8 and the kG8 fuzzy kernel, rows in LDS and in HBM"""
    m, _, lm, ix = crafted
    _assert_conditions(m, lm, ix, top_k, 0.3)
    monkeypatch.setenv("SG_G8", "2")
    sc = _open(m["directory"])
    try:
        _assert_same_predictions(sc, lm, ix, ps.queries(m, ix), top_k, 0.3)
    finally:
        sc.index.close()


def test_large_top_k_rows_do_not_depend_on_the_poison(crafted):
    """topK = 100 under both poison patterns (sg_debug_poison): the HBM top-k rows of both searches and Predict's two id rows"""
    m, sc, lm, ix = crafted
    _assert_conditions(m, lm, ix, 100, 0.3)
    qb, qo = oracle.pack_strings(ps.queries(m, ix))
    got = _twice(lambda: sc.predict_batch(blob=qb, offs=qo, top_k=100, similarity=0.3))
    oi, oc = lm.predict_batch(ix, qb, qo, 100, 0.3)
    assert np.array_equal(got[1], oc)
    _same_rows(got, (oi, oc), "poisoned against the oracle")


# ---- the fuzzy top-up through the pipeline ----
@pytest.fixture(scope="module")
def big_vocabulary(tmp_path_factory):
    """A vocabulary above the one-counter-per-document size (8192 words) and a batch above the tokeniser launch's (2048 queries):
    what pipe_eligible asks of a fuzzy launch.  A third of the queries are typos, a third whole words or long prefixes (few
    completions: the flagged subset), a third prefixes of two letters or the prefix of a family of 400 words added to the
    vocabulary (a dozen completions and 400: not flagged at topK = 5, and the family's not at 100 either)."""
    import torch  # noqa: F401
    from suggest_amd import synth
    tmp = str(tmp_path_factory.mktemp("predict_pipe"))
    blob, offs = synth.make_dict(16000, seed=61, families=3)
    family = ["zzp" + "".join(chr(97 + (i // 26 ** j) % 26) for j in range(3)) for i in range(400)]
    vocab = sorted(set(w.decode() for w in synth.unpack(blob, offs)) | set(family))
    assert len(vocab) >= 12000
    rnd = np.random.RandomState(9)
    sentences = [[vocab[int(i)] for i in rnd.zipf(1.3, size=int(rnd.randint(2, 7))) % len(vocab)] for _ in range(20000)]
    _write_lm(tmp, vocab, 3, sentences)
    queries = []
    for i in range(4200):
        s = sentences[int(rnd.randint(0, len(sentences)))]
        cut = int(rnd.randint(1, len(s) + 1))
        ctx, word = s[max(0, cut - 1 - int(rnd.randint(0, 3))):cut - 1], s[cut - 1]
        if i % 3 == 0 and len(word) > 3:
            p = int(rnd.randint(0, len(word)))
            word = word[:p] + "x" + word[p + 1:]                                 # a typo
        elif i % 3 == 1:
            word = "zzp" if i % 2 else word[:2]                                  # the family's prefix; two letters
        elif i % 2:
            word = word[:max(4, len(word) - 2)]                                  # a long prefix
        queries.append(" ".join(ctx + [word]).encode())
    lm = oracle.OracleLM(tmp, 3, alphabet=ps.ALPHA)
    return _open(tmp), lm, oracle.OracleIndex(lm.words(), **SPELL_INDEX), queries


@pytest.mark.parametrize("top_k", (5, 100))
def test_fuzzy_top_up_takes_the_pipeline(big_vocabulary, top_k):
    sc, lm, ix, queries = big_vocabulary
    n = len(queries)
    assert n >= 4096
    last = [(lm.tokenize(q) or [b""])[-1] for q in queries]
    ac = ix.autocomplete_batch(*oracle.pack_strings(last), top_k)[1]
    flagged = int(((ac < top_k) & np.array([len(w) > 0 for w in last])).sum())
    assert n // 3 <= flagged < n - 100, flagged                  # the top-up's subset: neither empty nor the whole batch
    qb, qo = oracle.pack_strings(queries)
    want = lm.predict_batch(ix, qb, qo, top_k, 0.4)
    before = {name: _knob(sc.index, name) for name in ("SG_PIPE", "SG_TIGHTEN", "SG_PLAN2")}
    try:
        sc.index.tune(SG_PIPE=0, SG_TIGHTEN=0)
        at = sc.index.pipe_stats()["queries"]
        fused = sc.predict_batch(blob=qb, offs=qo, top_k=top_k, similarity=0.4)
        assert sc.index.pipe_stats()["queries"] == at
        _same_rows(fused, want, "fused")
        for plan2 in (1, 0):
            sc.index.tune(SG_PIPE=1, SG_PLAN2=plan2)
            at = sc.index.pipe_stats()["queries"]
            got = sc.predict_batch(blob=qb, offs=qo, top_k=top_k, similarity=0.4)
            assert sc.index.pipe_stats()["queries"] > at, "the top-up did not take the pipeline"
            _same_rows(got, want, "pipeline, SG_PLAN2=%d" % plan2)
            _same_rows(got, fused, "pipeline against SG_PIPE=0")
    finally:
        sc.index.tune(**before)


# ---- batches whose top-k rows pass 1 GiB ----
def test_a_predict_batch_above_one_gib_of_rows(crafted):
    """launch(): `k > SG_K_LDS && n_q * k * 12 > 1 GiB` -> pieces of (1 GiB) / (k * 12) queries, every per-query array re-based.
    At topK = 1023 a piece is 87 466 queries: 737 more make a second, short piece that starts mid-batch — for the LM
    collector's launch and for the flagged fuzzy launch alike."""
    m, sc, lm, ix = crafted
    top_k, sim = 1023, 0.3
    piece = (1 << 30) // (top_k * 12)
    n_q = piece + 737
    assert n_q * top_k * 12 > 1 << 30 and 0 < n_q - piece < piece
    _assert_conditions(m, lm, ix, top_k, sim)
    kinds, words = zip(*ps.last_words(m, ix))
    ctxs = m["contexts"]
    nw, nc = len(words), len(ctxs)
    pairs = [((j // nw + j % nw) % nc, j % nw) for j in range(n_q)]     # the crafted batch cycled, the contexts rotated
    assert len(set(pairs[:nw * nc])) == nw * nc and all(a[0] != b[0] and a[1] != b[1] for a, b in zip(pairs, pairs[1:]))
    # A last word above 128 n-grams costs 2 ms (sg_long_kernel; measured: 14.7 s of this batch's 14.8 s per pass when every cycle
    # kept its long words, 0.08 s without any), so they stay in every eighth cycle and in the cycles around and behind the cut;
    # elsewhere a short last word takes their place.  The query count, which is what reaches the branch, is untouched.
    is_long = [k in ("long128", "long129", "stem", "stem typo") for k in kinds]
    short = [w for w, l in zip(words, is_long) if not l]
    cycle = nw * nc
    keeps = lambda j: (j // cycle) % 8 == 0 or j // cycle >= piece // cycle
    queries = [(ctxs[c] + (words[w] if keeps(j) or not is_long[w] else short[(j // nw) % len(short)])).encode() for j, (c, w) in enumerate(pairs)]
    n_long = np.array([is_long[w] and keeps(j) for j, (c, w) in enumerate(pairs)])
    assert n_long[:piece].sum() >= 500 and n_long[piece:].sum() >= 50
    qb, qo = oracle.pack_strings(queries)
    ids, cnt = sc.predict_batch(blob=qb, offs=qo, top_k=top_k, similarity=sim)
    for lo in range(0, n_q, 8192):                               # below the cut
        hi = min(n_q, lo + 8192)
        assert (hi - lo) * top_k * 12 <= 1 << 30
        _same_rows((ids[lo:hi], cnt[lo:hi]), sc.predict_batch(queries[lo:hi], top_k=top_k, similarity=sim), "calls of 8192, from %d" % lo)
    pick = np.union1d(np.arange(0, n_q, 37), np.arange(piece - 64, n_q))      # every 37th, and all around and behind the cut
    oi, oc = lm.predict_batch(ix, *oracle.pack_strings([queries[i] for i in pick]), top_k, sim)
    assert (oc[pick >= piece] == top_k + 1).any() and (oc[pick < piece] == top_k + 1).any()
    _same_rows((ids[pick], cnt[pick]), (oi, oc), "the sample against the oracle")


def test_suggest_at_the_largest_k_above_one_gib_of_rows():
    """The same cut for the fuzzy search at k = SG_MAX_TOPK (65 536): a piece is 1365 queries; 300 more.  The dictionary is the
    50 000-string synthetic one with Zipf-distributed symbols; every 13th query is a short string over its two commonest
    symbols, which Cosine >= 0.2 matches against thousands of documents."""
    import itertools
    from suggest_amd import IndexDescription, NGramIndex, _lib, synth
    k = _lib.SG_MAX_TOPK
    piece = (1 << 30) // (k * 12)
    n_q = piece + 300
    assert n_q * k * 12 > 1 << 30 and 0 < n_q - piece < piece
    blob, offs = synth.make_dict(50000, seed=1, skewed=True)
    queries = synth.unpack(*synth.make_queries(n_q, blob, offs, seed=12))
    heavy = [b"aabaaa", b"aaabaa", b"aaaabaa", b"aaabaaa", b"aabaaaa", b"aabaaab", b"baabaaa", b"abaaabb"]
    heavy += [("".join(t)).encode() for t in itertools.product("ab", repeat=6)][:27]
    assert len(heavy) == 35                                      # (105 x 13 = the first query of the second piece: heavy[0] again)
    for j, i in enumerate(range(0, n_q, 13)):
        queries[i] = heavy[j % 35]
    qb, qo = oracle.pack_strings(queries)
    gpu = NGramIndex(blob=blob, offs=offs, description=IndexDescription(**synth.DESCRIPTION))
    ora = oracle.OracleIndex(blob=blob, offs=offs, **synth.DESCRIPTION)
    pick = np.array([0, 13, 26, 7, 500, 1001, piece - 1, 104 * 13] + [piece, piece + 1, 106 * 13, 107 * 13, 108 * 13, n_q - 2, n_q - 1, 127 * 13])
    assert len(set(pick.tolist())) == 16 and (pick < piece).sum() == 8 and pick.max() < n_q
    want = ora.suggest_batch(*oracle.pack_strings([queries[i] for i in pick]), "cosine", 0.2, k)
    assert int(want[2][:8].max()) > 2500 and int(want[2][8:].max()) > 2500, want[2]      # rows longer than any tested before, in both pieces
    try:
        ids, sc, cnt = gpu.suggest_batch(blob=qb, offs=qo, metric="cosine", similarity=0.2, k=k)
        assert_same((ids[pick], sc[pick], cnt[pick]), want)
        for lo in range(0, n_q, 500):
            hi = min(n_q, lo + 500)
            assert_same((ids[lo:hi], sc[lo:hi], cnt[lo:hi]), gpu.suggest_batch(queries[lo:hi], metric="cosine", similarity=0.2, k=k))
    finally:
        gpu.close()
