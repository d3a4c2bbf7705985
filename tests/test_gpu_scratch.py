"""Launches that read working memory they did not write this call.  The per-stream scratch blocks (SCRATCH_ROWS, PIPE,
PRETOK, LONG_LIST, PREDICT) and a host-buffer call's result rows are grow-only and reused: a read of a stale word returns an
earlier call's leftover, which usually equals the right answer.  With the test-only poison switch (sg_debug_poison) every call
fills what it is meant to write with a pattern first, so such a read shows as a wrong row.  Bit-exact against the oracle."""
import contextlib
import os
import random

import numpy as np
import pytest

import oracle

pytestmark = pytest.mark.gpu

SPECIAL = 0xFFFFFFF0          # counts at and above: SG_COUNT_TOO_LONG and friends (no row)
ALPHA_DESC = dict(ngram_size=2, wrap=("$", "$"), pad="$", alphabet=("ab", "$"))
# the knob values both unexplained fuzz reports shared
REPORT_KNOBS = dict(SG_G8="2", SG_T_FLOOR="2", SG_FILTER_LEVEL="6", SG_TIGHTEN="0", SG_PIPE="0", SG_ORDER="64")


@contextlib.contextmanager
def _env(**knobs):
    """SG_* knobs for the index built inside (an index reads them once, at its first upload)"""
    old = {k: os.environ.get(k) for k in knobs}
    os.environ.update(knobs)
    try:
        yield
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def _build(docs, desc, **knobs):
    from suggest_amd import IndexDescription, NGramIndex
    with _env(**knobs):
        return NGramIndex(docs, IndexDescription(**desc))


def _alpha_docs(seed, n_docs=3000, n_long=6):
    """tools/fuzz_parity.py's trial shape: a two-letter alphabet, documents drawn from a few bases with mutations (many
    documents repeat a term), a few documents above the wavefront kernel's 128 n-grams"""
    rng = random.Random(seed)
    syms = "ab"
    base = ["".join(rng.choice(syms) for _ in range(rng.randint(0, 30))) for _ in range(n_docs // 4)]
    docs = []
    for _ in range(n_docs):
        w = list(rng.choice(base))
        for _ in range(rng.randint(0, 2)):
            if w:
                w[rng.randrange(len(w))] = rng.choice(syms)
        docs.append("".join(w))
    docs[0] = "abbaab"
    docs += ["".join(rng.choice(syms) for _ in range(rng.randint(150, 400))) for _ in range(n_long)]
    queries = [rng.choice(docs[:n_docs]) for _ in range(120)] + ["".join(rng.choice(syms) for _ in range(rng.randint(0, 36))) for _ in range(60)]
    queries += [d[:rng.randint(0, len(d))] + rng.choice(syms) + d[rng.randint(0, len(d)):] for d in rng.sample(docs[:n_docs], 60)]
    rng.shuffle(queries)
    long_q = [d[:rng.randint(140, len(d))] for d in docs[n_docs:]] + [docs[n_docs][:200].replace("a", "b", 3)]
    return [d.encode() for d in docs], [q.encode() for q in queries], [q.encode() for q in long_q]


@pytest.fixture(scope="module")
def world():
    """Every index of this file, built once: the pipeline's (SG_PIPE=1, tokeniser launch for every batch, query order from 64
    queries), the same with two candidate slots per query (overflow: queries handed back to the fused kernel), plain fused and
    tightening ones, and two over a two-letter alphabet with the reports' knobs and split queries (8-chunk and 1-chunk parts)."""
    from suggest_amd import synth
    blob, offs = synth.make_dict(20000, seed=11)
    sdocs = [bytes(blob[offs[i]:offs[i + 1]]) for i in range(len(offs) - 1)]
    sq = [sdocs[i] for i in range(0, 20000, 97)] + [d[:-2] + b"qz" for d in sdocs[5:20000:131]] + [b"", b"x", sdocs[7][:3]]
    random.Random(3).shuffle(sq)
    adocs, aq, along = _alpha_docs(610200998)
    pipe_knobs = dict(SG_PIPE="1", SG_PRETOK="1", SG_ORDER="64", SG_TIGHTEN="0", SG_SPLIT_CHUNKS="0", SG_G8="0")
    w = dict(
        pipe=_build(sdocs, synth.DESCRIPTION, **pipe_knobs),
        pipe_cap2=_build(sdocs, synth.DESCRIPTION, SG_PIPE_CAND_CAP="2", **pipe_knobs),
        fused=_build(sdocs, synth.DESCRIPTION, SG_PIPE="0", SG_PRETOK="0", SG_ORDER="0", SG_TIGHTEN="0", SG_SPLIT_CHUNKS="0", SG_G8="0"),
        tight=_build(sdocs, synth.DESCRIPTION, SG_PIPE="0", SG_PRETOK="0", SG_TIGHTEN="1", SG_SPLIT_CHUNKS="0", SG_G8="0"),
        split8=_build(adocs, ALPHA_DESC, SG_SPLIT_CHUNKS="8", SG_PRETOK="1", **REPORT_KNOBS),
        split1=_build(adocs, ALPHA_DESC, SG_SPLIT_CHUNKS="1", SG_PRETOK="48", **REPORT_KNOBS),
        ora_s=oracle.OracleIndex(sdocs, **synth.DESCRIPTION), ora_a=oracle.OracleIndex(adocs, **ALPHA_DESC),
        sq=sq, aq=aq, along=along, adocs=adocs)
    yield w
    for name in ("pipe", "pipe_cap2", "fused", "tight", "split8", "split1"):
        w[name].close()


def _word(family):
    from suggest_amd import _lib
    return _lib.POISON_WORD[family]


def _check(gpu, ora, family=None, what=""):
    """gpu == oracle bit for bit on every counted entry; with poison `family` on, every entry past a row's count still holds
    the pattern (nothing wrote there).  gpu: (ids, scores, counts) or (ids, counts)."""
    ids, cnt = gpu[0], gpu[-1]
    sc = gpu[1] if len(gpu) == 3 else None
    oi, os_, oc = (ora[0], ora[1], ora[2]) if sc is not None else (ora[0], None, ora[1])
    bad = np.nonzero(cnt != oc)[0]
    assert bad.size == 0, (what, "counts differ", bad[:5], cnt[bad[:5]], oc[bad[:5]])
    k = ids.shape[1]
    col = np.arange(k)[None, :]
    valid = (col < np.minimum(cnt, k)[:, None]) & (cnt < SPECIAL)[:, None]
    neq = valid & (ids != oi)
    if sc is not None:
        neq |= valid & (sc.view(np.uint64) != os_.view(np.uint64))
    rows = np.nonzero(neq.any(axis=1))[0]
    assert rows.size == 0, (what, "rows differ", rows[:5], ids[rows[:2]], oi[rows[:2]])
    if family:
        tail = (col >= np.minimum(cnt, k)[:, None]) & (cnt < SPECIAL)[:, None]
        w = _word(family)
        assert np.all(ids[tail] == w), (what, "ids written past the count")
        if sc is not None:
            assert np.all(sc.view(np.uint64)[tail] == (w << 32 | w)), (what, "scores written past the count")


def _pack(queries):
    return oracle.pack_strings(queries)


def _take(pool, start, n):
    return [pool[(start + i) % len(pool)] for i in range(n)]


def test_poison_reaches_the_rows_and_the_scratch(world):
    """Positive control: with the switch on, the rows past a query's count hold the id / score pattern of the family chosen
    (0xA5A5A5A5 or 0x5A5A5A5A) on the synchronous and the ticket path, and the split-query queue (SCRATCH_ROWS) and the
    pipeline's fb_list (SCRATCH_PIPE) were poisoned; with it off again the rows past the count are zero."""
    from suggest_amd import _lib
    from suggest_amd.index import pinned_array
    gpu, ora = world["split8"], world["ora_a"]
    qb, qo = _pack(world["aq"][:100])
    n_q, k = 100, 64
    want = ora.suggest_batch(qb, qo, "dice", 0.9, k)
    for family in (1, 2):
        with _lib.poisoned(family):
            got = gpu.suggest_batch(blob=qb, offs=qo, metric="dice", similarity=0.9, k=k)
            st = _lib.poison_stats()
        _check(got, want, family, "split")
        assert (got[2] < k).sum() > 10                          # rows with a tail to look at
        assert st["out_ids"] == n_q * k * 4 and st["out_scores"] == n_q * k * 8 and st["out_counts"] == n_q * 4, st
        assert st["rows"] >= 64 * 1024, st                      # items, slot words, part rows of the split-query queue
        print("poison family %d, split launch: %s" % (family, st))
    # the ticket path (sg_suggest_submit): the slot's device block takes the pattern too
    ids, sc, cnt = pinned_array((n_q, k), np.uint32), pinned_array((n_q, k), np.float64), pinned_array((n_q,), np.uint32)
    with _lib.poisoned(1):
        gpu.suggest_submit(qb, qo, "dice", 0.9, k, ids, sc, cnt).wait()
        st = _lib.poison_stats()
    _check((np.array(ids), np.array(sc), np.array(cnt)), want, 1, "ticket")
    assert st["out_ids"] == n_q * k * 4 and st["rows"] > 0, st
    # the pipeline: its hand-back list
    pq = world["sq"][:300]
    pb, po = _pack(pq)
    before = world["pipe"].pipe_stats()["queries"]
    with _lib.poisoned(1):
        got = world["pipe"].suggest_batch(blob=pb, offs=po, metric="jaccard", similarity=0.5, k=10)
        st = _lib.poison_stats()
    assert world["pipe"].pipe_stats()["queries"] == before + len(pq), "the launch did not take the pipeline"
    _check(got, world["ora_s"].suggest_batch(pb, po, "jaccard", 0.5, 10), 1, "pipeline")
    assert st["pipe"] == (len(pq) + 1) * 4 and st["rows"] >= len(pq) * 4, st    # fb_list; the ordered list (>= 64 queries)
    print("poison family 1, pipeline launch: %s" % st)
    # off: rows past the count are zero again, and nothing is poisoned
    got = gpu.suggest_batch(blob=qb, offs=qo, metric="dice", similarity=0.9, k=k)
    tail = np.arange(k)[None, :] >= got[2][:, None]
    assert np.all(got[0][tail] == 0) and np.all(got[1][tail] == 0)
    assert sum(_lib.poison_stats().values()) == 0


def test_pipeline_and_split_launches_interleaved(world):
    """One thread, one stream, poison on: pipeline launches (SCRATCH_ROWS holding the ordered list, SCRATCH_PIPE the records)
    alternate with split-forced fused launches (the same ROWS block re-carved as items, slot words, part rows), autocomplete
    (limit 7) and k > SG_K_LDS launches (HBM rows, again in ROWS), while k and n_q grow and shrink so that every region moves.
    Dice >= 0.9 at k = 64 is the first report's search."""
    from suggest_amd import _lib
    ks = [1, 5, 64, 10, 65, 300]
    nqs = [7, 47, 48, 63, 64, 200]
    metrics = [("jaccard", 0.5), ("cosine", 0.3), ("dice", 0.9), ("overlap", 0.7), ("jaccard", 0.3), ("cosine", 0.6)]
    sched = list(zip(ks, nqs, metrics))
    sched = sched + sched[::-1]
    w = world
    pipe_before = w["pipe"].pipe_stats()["queries"]
    with _lib.poisoned(1):
        for step, (k, n_q, (metric, alpha)) in enumerate(sched):
            if k == 64:
                metric, alpha = "dice", 0.9
            tag = "step %d k=%d n_q=%d %s %.2f" % (step, k, n_q, metric, alpha)
            sb, so = _pack(_take(w["sq"], step * 11, n_q))
            _check(w["pipe"].suggest_batch(blob=sb, offs=so, metric=metric, similarity=alpha, k=k),
                   w["ora_s"].suggest_batch(sb, so, metric, alpha, k), 1, "pipe " + tag)
            ab, ao = _pack(_take(w["aq"], step * 3, n_q))
            want = w["ora_a"].suggest_batch(ab, ao, metric, alpha, k)
            for name in ("split8", "split1"):
                _check(w[name].suggest_batch(blob=ab, offs=ao, metric=metric, similarity=alpha, k=k), want, 1, name + " " + tag)
            _check(w["split8"].autocomplete_batch(blob=ab, offs=ao, limit=7), w["ora_a"].autocomplete_batch(ab, ao, 7), 1, "autocomplete " + tag)
            if k <= 64:     # (d) a k above SG_K_LDS right behind: HBM rows in the block the split queue just used
                _check(w["split8"].suggest_batch(blob=ab, offs=ao, metric=metric, similarity=alpha, k=k + 100),
                       w["ora_a"].suggest_batch(ab, ao, metric, alpha, k + 100), 1, "big k " + tag)
    assert w["pipe"].pipe_stats()["queries"] > pipe_before


def _twice(run):
    """run() under both pattern families: the counted entries and counts must be byte-identical"""
    from suggest_amd import _lib
    out = []
    for family in (1, 2):
        with _lib.poisoned(family):
            out.append(run())
            _lib.poison_stats()
    a, b = out
    cnt_a, cnt_b = a[-1], b[-1]
    assert np.array_equal(cnt_a, cnt_b), "counts depend on the poison"
    k = a[0].shape[1]
    valid = (np.arange(k)[None, :] < np.minimum(cnt_a, k)[:, None]) & (cnt_a < SPECIAL)[:, None]
    for x, y in zip(a[:-1], b[:-1]):
        x, y = np.asarray(x), np.asarray(y)
        if x.ndim == 2:
            assert np.array_equal(x.view(np.uint8).reshape(x.shape[0], -1)[np.repeat(valid, x.itemsize, axis=1)],
                                  y.view(np.uint8).reshape(y.shape[0], -1)[np.repeat(valid, y.itemsize, axis=1)]), "rows depend on the poison"
    return a


@pytest.mark.parametrize("kind", ["fused", "split", "tight", "g8", "long", "hbm_topk", "pipe_overflow", "autocomplete", "by_doc", "predict"])
def test_rows_do_not_depend_on_the_poison(world, kind, reference_tests):
    """Every launch kind, the same batch under both pattern families: identical rows and counts (a read of an unwritten word
    that the oracle comparison alone could miss), and equal to the oracle."""
    w = world
    sb, so = _pack(w["sq"][:180])
    ab, ao = _pack(w["aq"][:180])
    if kind == "fused":
        got = _twice(lambda: w["fused"].suggest_batch(blob=sb, offs=so, metric="cosine", similarity=0.4, k=20))
        _check(got, w["ora_s"].suggest_batch(sb, so, "cosine", 0.4, 20))
    elif kind == "split":
        got = _twice(lambda: w["split1"].suggest_batch(blob=ab, offs=ao, metric="dice", similarity=0.9, k=64))
        _check(got, w["ora_a"].suggest_batch(ab, ao, "dice", 0.9, 64))
    elif kind == "tight":
        got = _twice(lambda: w["tight"].suggest_batch(blob=sb, offs=so, metric="jaccard", similarity=0.3, k=10))
        _check(got, w["ora_s"].suggest_batch(sb, so, "jaccard", 0.3, 10))
    elif kind == "g8":       # 8-bit gaps for every term (SG_G8=2): the kG8 instantiations of the fused and the parts kernel
        got = _twice(lambda: w["split8"].suggest_batch(blob=ab, offs=ao, metric="jaccard", similarity=0.5, k=5))
        _check(got, w["ora_a"].suggest_batch(ab, ao, "jaccard", 0.5, 5))
    elif kind == "long":     # queries above 128 n-grams: sg_long_kernel
        lb, lo = _pack(w["along"] + w["aq"][:20])
        got = _twice(lambda: w["split8"].suggest_batch(blob=lb, offs=lo, metric="jaccard", similarity=0.5, k=10))
        _check(got, w["ora_a"].suggest_batch(lb, lo, "jaccard", 0.5, 10))
        assert int(got[2][:len(w["along"])].sum()) > 0
    elif kind == "hbm_topk":
        got = _twice(lambda: w["fused"].suggest_batch(blob=sb, offs=so, metric="cosine", similarity=0.2, k=300))
        _check(got, w["ora_s"].suggest_batch(sb, so, "cosine", 0.2, 300))
    elif kind == "pipe_overflow":
        st = w["pipe_cap2"].pipe_stats()
        got = _twice(lambda: w["pipe_cap2"].suggest_batch(blob=sb, offs=so, metric="jaccard", similarity=0.4, k=10))
        _check(got, w["ora_s"].suggest_batch(sb, so, "jaccard", 0.4, 10))
        after = w["pipe_cap2"].pipe_stats()
        assert after["queries"] > st["queries"] and after["overflow"] > st["overflow"], (st, after)
    elif kind == "autocomplete":
        got = _twice(lambda: w["split8"].autocomplete_batch(blob=ab, offs=ao, limit=7))
        _check(got, w["ora_a"].autocomplete_batch(ab, ao, 7))
    elif kind == "by_doc":   # docID-ordered paging: the counted ids are the first `limit` of the oracle's candidates by docID
        got = _twice(lambda: w["fused"].suggest_batch_from(blob=sb, offs=so, metric="dice", similarity=0.5, first_doc=100, limit=16))
        oi, os_, oc = w["ora_s"].suggest_batch(sb, so, "dice", 0.5, 20000)[:3]
        for i in range(len(oc)):
            if oc[i] >= SPECIAL:
                continue
            want = sorted(int(d) for d in oi[i, :int(oc[i])] if d >= 100)[:16]
            assert got[0][i, :int(got[3][i])].tolist() == want, i
    elif kind == "predict":
        from suggest_amd import LanguageModel, SpellChecker
        g = reference_tests["lm"]
        lm_dir = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "lm")
        sc = SpellChecker(LanguageModel(lm_dir, g["order"], g["startSymbol"], g["endSymbol"]))
        queries = [b"i am sa", b"green eg", b"i do", b"sam i am sam i am sa", b"gren egs", b"i an", b"ha", b"", b"I AM SAM", b"eggs and ha", b"sam"]
        qb, qo = _pack(queries)
        got = _twice(lambda: sc.predict_batch(blob=qb, offs=qo, top_k=5, similarity=0.3))
        ora_lm = oracle.OracleLM(lm_dir, g["order"], g["startSymbol"], g["endSymbol"])
        spell_index = dict(ngram_size=3, wrap=("^", "$"), pad="$", alphabet=("english", "russian", "numbers", "$^'"))
        oi, oc = ora_lm.predict_batch(oracle.OracleIndex(ora_lm.words(), **spell_index), qb, qo, 5, 0.3)
        assert np.array_equal(got[1], oc)
        for i in range(len(oc)):
            if oc[i] < SPECIAL:
                assert got[0][i, :int(oc[i])].tolist() == oi[i, :int(oc[i])].tolist(), i
