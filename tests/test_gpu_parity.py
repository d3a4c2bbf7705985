"""Parity of the HIP path (through the C ABI) against the CPU oracle: bit-exact ids, order, scores."""
import os

import numpy as np
import pytest

import oracle
from conftest import CARS_DESC, WORDS_DESC

pytestmark = pytest.mark.gpu

METRICS = [("jaccard", 0.5), ("cosine", 0.4), ("dice", 0.5), ("cosine", 0.7), ("jaccard", 0.8), ("overlap", 0.9),
           ("exact", 1.0)]


def _desc(d):
    from suggest_amd import IndexDescription
    return IndexDescription(ngram_size=d["ngram_size"], wrap=d["wrap"], pad=d["pad"], alphabet=d["alphabet"])


def assert_same(gpu, ora, queries=None):
    ids, sc, cnt = gpu
    oi, os_, oc = ora[:3]
    bad = np.nonzero(cnt != oc)[0]
    assert bad.size == 0, ("counts differ", bad[:5], cnt[bad[:5]], oc[bad[:5]], None if queries is None else [queries[i] for i in bad[:5]])
    k = ids.shape[1]
    valid = np.arange(k)[None, :] < np.minimum(cnt, k)[:, None]
    valid &= (cnt < 0xFFFFFFF0)[:, None]
    neq = valid & ((ids != oi) | (sc.view(np.uint64) != os_.view(np.uint64)))
    rows = np.nonzero(neq.any(axis=1))[0]
    assert rows.size == 0, ("rows differ", rows[:5], ids[rows[:3]], oi[rows[:3]], sc[rows[:3]], os_[rows[:3]],
                            None if queries is None else [queries[i] for i in rows[:5]])


@pytest.fixture(scope="module")
def synth_small():
    from suggest_amd import NGramIndex, IndexDescription, synth
    blob, offs = synth.make_dict(50000, seed=1)
    qb, qo = synth.make_queries(4096, blob, offs, seed=2)
    gpu = NGramIndex(blob=blob, offs=offs, description=IndexDescription(**synth.DESCRIPTION))
    ora = oracle.OracleIndex(blob=blob, offs=offs, **synth.DESCRIPTION)
    return gpu, ora, qb, qo


@pytest.mark.parametrize("metric,alpha", METRICS)
@pytest.mark.parametrize("k", [1, 10, 20])
def test_synthetic_parity(synth_small, metric, alpha, k):
    gpu, ora, qb, qo = synth_small
    assert_same(gpu.suggest_batch(blob=qb, offs=qo, metric=metric, similarity=alpha, k=k),
                ora.suggest_batch(qb, qo, metric, alpha, k))


def test_synthetic_q2_long_lists():
    from suggest_amd import NGramIndex, IndexDescription, synth
    desc = dict(synth.DESCRIPTION, ngram_size=2)
    blob, offs = synth.make_dict(200000, seed=3)
    qb, qo = synth.make_queries(512, blob, offs, seed=4)
    gpu = NGramIndex(blob=blob, offs=offs, description=IndexDescription(**desc))
    ora = oracle.OracleIndex(blob=blob, offs=offs, **desc)
    assert_same(gpu.suggest_batch(blob=qb, offs=qo, metric="dice", similarity=0.5, k=10),
                ora.suggest_batch(qb, qo, "dice", 0.5, 10))


def test_docid_range_passes_on_heavy_segments(monkeypatch):
    """q=2 on 1M strings with the smallest counter array: a segment's postings outnumber what the counters
    resolve, so the kernel streams it in several docID-range passes (engine.hip, n_pass > 1)."""
    from suggest_amd import NGramIndex, IndexDescription, synth
    monkeypatch.setenv("SG_LOG2_CNT", "9")
    desc = dict(synth.DESCRIPTION, ngram_size=2)
    blob, offs = synth.make_dict(1000000, seed=5)
    qb, qo = synth.make_queries(256, blob, offs, seed=6)
    gpu = NGramIndex(blob=blob, offs=offs, description=IndexDescription(**desc))
    ora = oracle.OracleIndex(blob=blob, offs=offs, **desc)
    for metric, alpha in (("dice", 0.5), ("jaccard", 0.4), ("cosine", 0.3)):
        assert_same(gpu.suggest_batch(blob=qb, offs=qo, metric=metric, similarity=alpha, k=10),
                    ora.suggest_batch(qb, qo, metric, alpha, 10))


def test_large_k_uses_hbm_rows(synth_small):
    gpu, ora, qb, qo = synth_small
    assert_same(gpu.suggest_batch(blob=qb[:int(qo[256])], offs=qo[:257], metric="cosine", similarity=0.3, k=200),
                ora.suggest_batch(qb[:int(qo[256])], qo[:257], "cosine", 0.3, 200))


def test_reference_goldens_through_gpu(reference_tests):
    from suggest_amd import IndexDescription, JaccardMetric, CosineMetric, SearchConfig, Service
    coll = reference_tests["small_collection"]
    t = reference_tests["suggest_auto"]
    d = t["description"]
    svc = Service()
    svc.AddIndex("index", coll, IndexDescription(ngram_size=d["nGramSize"], wrap=d["wrap"], pad=d["pad"], alphabet=d["alphabet"]))
    res = svc.Suggest("index", SearchConfig(t["query"], t["topK"], JaccardMetric(), t["similarity"]))
    assert [r.value for r in res] == [coll[i] for i in t["expected_ids"]]       # ngram_index_test.go:15-40
    a = reference_tests["autocomplete"]
    res = svc.Autocomplete("index", a["query"], a["limit"])
    assert [r.value for r in res] == [coll[i] for i in a["expected_ids"]]       # ngram_index_test.go:42-67
    assert all(r.score == 0 for r in res)
    e = reference_tests["example"]
    d = e["description"]
    svc.AddIndex("cars", coll, IndexDescription(ngram_size=d["nGramSize"], wrap=d["wrap"], pad=d["pad"], alphabet=d["alphabet"]))
    res = svc.Suggest("cars", SearchConfig(e["query"], e["topK"], CosineMetric(), e["similarity"]))
    assert [r.value for r in res] == e["expected_values"]                       # example_test.go:14-72
    with pytest.raises(KeyError):
        svc.Suggest("nope", SearchConfig("x", 1, CosineMetric(), 0.5))          # service.go:111-113


def test_service_cars_golden(reference_tests, cars_lines):
    from suggest_amd import CosineMetric, SearchConfig, Service
    svc = Service()
    svc.AddIndex("cars", cars_lines, _desc(CARS_DESC))
    t = reference_tests["service_cars"]
    for q, exp in zip(t["queries"], t["expected_values"]):                      # service_test.go:35,53-59
        res = svc.Suggest("cars", SearchConfig(q, t["topK"], CosineMetric(), t["similarity"]))
        assert [r.value for r in res] == exp, q


@pytest.mark.parametrize("tighten", [0, 1, 2])
def test_cars_all_lines_as_queries(cars_lines, tighten):
    """Every third dictionary line (and edited copies) as a query, several metrics, ALL rows compared — including
    the rows where the reference returns a document twice (documents that repeat a term).  With and
    without threshold tightening (its own kernel instantiation; 2 = picked per launch from what recent queries did)."""
    from suggest_amd import NGramIndex
    gpu = NGramIndex(cars_lines, _desc(CARS_DESC)).tune(SG_TIGHTEN=tighten, SG_ROOMY=(2, 0, 1)[tighten])    # (small queue + slim tables with tightening on)
    ora = oracle.OracleIndex(cars_lines, **CARS_DESC)
    queries = list(cars_lines[::3]) + [l[1:] + b"x" for l in cars_lines[::7]] + [l.lower()[:-2] for l in cars_lines[::11]]
    qb, qo = oracle.pack_strings(queries)
    n_dup_rows = 0
    for metric, alpha, k in [("cosine", 0.5, 5), ("jaccard", 0.5, 10), ("dice", 0.6, 3), ("cosine", 0.3, 40), ("jaccard", 0.2, 100)]:
        g = gpu.suggest_batch(blob=qb, offs=qo, metric=metric, similarity=alpha, k=k)
        o = ora.suggest_batch(qb, qo, metric, alpha, k)
        n_dup_rows += sum(len(set(o[0][i, :o[2][i]].tolist())) != o[2][i] for i in range(len(queries)))
        assert_same(g, o, queries)
    assert n_dup_rows > 50          # the quirk is really exercised


def test_cars_autocomplete_with_repeated_terms(cars_lines):
    from suggest_amd import NGramIndex
    gpu = NGramIndex(cars_lines, _desc(CARS_DESC))
    ora = oracle.OracleIndex(cars_lines, **CARS_DESC)
    queries = [l[:n] for l in cars_lines[::9] for n in (3, 6, 12)] + [b"NISSAN TITAN", b"TITAN", b"AN "]
    qb, qo = oracle.pack_strings(queries)
    for limit in (3, 20):
        ids, cnt = gpu.autocomplete_batch(blob=qb, offs=qo, limit=limit)
        oi, oc, _ = ora.autocomplete_batch(qb, qo, limit)
        assert np.array_equal(cnt, oc)
        valid = np.arange(limit)[None, :] < cnt[:, None]
        assert np.array_equal(ids[valid], oi[valid])


def test_words_parity(words_lines, reference_tests):
    from suggest_amd import NGramIndex
    gpu = NGramIndex(words_lines, _desc(WORDS_DESC))
    ora = oracle.OracleIndex(words_lines, **WORDS_DESC)
    queries = reference_tests["workloads"]["words_cosine_0.5_k5"] + [w for w in words_lines[::997]] + \
        [w[:-1] + b"q" for w in words_lines[5::1999]]
    qb, qo = oracle.pack_strings(queries)
    for metric, alpha, k in [("cosine", 0.5, 5), ("jaccard", 0.4, 10), ("dice", 0.45, 1), ("cosine", 0.3, 3)]:
        want = ora.suggest_batch(qb, qo, metric, alpha, k)
        for tighten in (0, 1):        # both kernel instantiations (threshold tightening off / on)
            gpu.tune(SG_TIGHTEN=tighten)
            assert_same(gpu.suggest_batch(blob=qb, offs=qo, metric=metric, similarity=alpha, k=k), want, queries)


def test_autocomplete_parity(words_lines, cars_lines):
    from suggest_amd import NGramIndex
    gpu = NGramIndex(words_lines, _desc(WORDS_DESC))
    ora = oracle.OracleIndex(words_lines, **WORDS_DESC)
    queries = [w[:4] for w in words_lines[::501]] + [w[:2] for w in words_lines[::4001]] + [b"", b"zzzzqq", b"a"]
    qb, qo = oracle.pack_strings(queries)
    for limit in (1, 5, 50):
        ids, cnt = gpu.autocomplete_batch(blob=qb, offs=qo, limit=limit)
        oi, oc, _ = ora.autocomplete_batch(qb, qo, limit)
        assert np.array_equal(cnt, oc)
        valid = np.arange(limit)[None, :] < cnt[:, None]
        assert np.array_equal(ids[valid], oi[valid])


def test_edge_queries(cars_lines):
    import random
    from suggest_amd import NGramIndex
    gpu = NGramIndex(cars_lines, _desc(CARS_DESC))
    ora = oracle.OracleIndex(cars_lines, **CARS_DESC)
    rng = random.Random(5)
    long_q = "".join(rng.choice("abcdefghijklmnopqrstuvwxyz") for _ in range(120))
    queries = ["", " ", "a", "ab", "  NISSAN  ", "ниссан", "Ёлка ё", "toyota\xff\xfe", "TOYOTA COROLLA", long_q, "İstanbul",
               "$$$", "x" * 100, "NISSAN TITAN"]
    qb, qo = oracle.pack_strings([q.encode("utf-8", "surrogateescape") if isinstance(q, str) else q for q in queries])
    ids, sc, cnt = gpu.suggest_batch(blob=qb, offs=qo, metric="jaccard", similarity=0.5, k=5)
    oi, os_, oc, _ = ora.suggest_batch(qb, qo, "jaccard", 0.5, 5)
    assert np.array_equal(cnt, oc), (cnt, oc)
    assert cnt[0] == 0 and cnt[9] == 0xFFFFFFFF          # empty -> no result; overlong -> reference panics
    assert_same((ids, sc, cnt), (oi, os_, oc))


def test_random_small_dictionaries_property():
    """Randomised parity: tiny alphabets and short strings give many ties, repeated documents, repeated terms after
    normalisation (pad), empty/short queries and cardinality windows that clip at the index edge."""
    import random
    from suggest_amd import NGramIndex, IndexDescription
    rng = random.Random(1234)
    for trial in range(12):
        q = rng.choice([1, 2, 3, 3, 4])
        alpha = rng.choice([("english",), ("english", "numbers"), ("ab", "$"), ("russian", "english", "numbers", "$")])
        wrap = rng.choice([("$", "$"), ("^", "$"), ("", ""), (" ", " ")])
        pad = rng.choice(["$", "_", ""]) if q <= 4 else "$"
        syms = rng.choice(["ab", "abc -", "abcdefgh 12", "абвгд ёab", "AbC.dE f"])
        docs = ["".join(rng.choice(syms) for _ in range(rng.randint(0, 14))) for _ in range(rng.randint(1, 400))]
        if not ora_tokens_ok(docs[0], q, wrap, pad, alpha):
            docs[0] = "abcabcab"            # the reference panics if the FIRST document has no tokens (indexer_writer.go:70)
        desc = dict(ngram_size=q, wrap=wrap, pad=pad, alphabet=alpha)
        gpu = NGramIndex(docs, IndexDescription(**desc))
        ora = oracle.OracleIndex(docs, **desc)
        queries = [rng.choice(docs) for _ in range(40)] + ["".join(rng.choice(syms) for _ in range(rng.randint(0, 18))) for _ in range(60)]
        qb, qo = oracle.pack_strings(queries)
        for metric, a in (("jaccard", rng.choice([0.2, 0.5, 0.9])), ("cosine", rng.choice([0.3, 0.6])), ("dice", 0.4),
                          ("overlap", rng.choice([0.5, 1.0])), ("exact", 1.0)):
            k = rng.choice([1, 3, 10, 70])
            assert_same(gpu.suggest_batch(blob=qb, offs=qo, metric=metric, similarity=a, k=k),
                        ora.suggest_batch(qb, qo, metric, a, k), queries)
        ids, cnt = gpu.autocomplete_batch(blob=qb, offs=qo, limit=7)
        oi, oc, _ = ora.autocomplete_batch(qb, qo, 7)
        assert np.array_equal(cnt, oc), (trial, desc)
        valid = np.arange(7)[None, :] < cnt[:, None]
        assert np.array_equal(ids[valid], oi[valid]), (trial, desc)


@pytest.mark.parametrize("n_docs", [8191, 8192, 8193, 16384])
def test_one_counter_per_document_on_dictionaries_below_the_counter_count(n_docs):
    """A dictionary with at most as many documents as a wavefront has u8 counters (8 192 at the default size) is searched
    without list skipping and without flags on the way: the counters are read out after a group's stream and what
    reaches the threshold is verified (engine.hip, `tiny`).  Sizes on both sides of the switch, near-duplicate families
    (many matches per query, ties), low and high thresholds, the tightening instantiation, autocomplete; SG_LOG2_CNT=12
    moves the switch to 16 384."""
    from suggest_amd import NGramIndex, IndexDescription, synth
    blob, offs = synth.make_dict(n_docs, seed=5, families=3)
    desc = dict(synth.DESCRIPTION)
    gpu = NGramIndex(blob=blob, offs=offs, description=IndexDescription(**desc))
    ora = oracle.OracleIndex(blob=blob, offs=offs, **desc)
    qb, qo = synth.make_queries(3000, blob, offs, seed=6)
    queries = synth.unpack(qb, qo)
    for log2_cnt in ((11, 12) if n_docs > 8192 else (11,)):
        for tighten in (0, 1):
            gpu.tune(SG_LOG2_CNT=log2_cnt, SG_TIGHTEN=tighten)
            for metric, a, k in (("jaccard", 0.5, 10), ("cosine", 0.2, 5), ("dice", 0.8, 3), ("overlap", 0.4, 70)):
                assert_same(gpu.suggest_batch(blob=qb, offs=qo, metric=metric, similarity=a, k=k),
                            ora.suggest_batch(qb, qo, metric, a, k), queries)
    pre = [q[:5] for q in queries[:1500]]
    pb, po = oracle.pack_strings(pre)
    ids, cnt = gpu.autocomplete_batch(blob=pb, offs=po, limit=9)
    oi, oc, _ = ora.autocomplete_batch(pb, po, 9)
    assert np.array_equal(cnt, oc)
    valid = np.arange(9)[None, :] < np.minimum(cnt, 9)[:, None]
    assert np.array_equal(ids[valid], oi[valid])


def ora_tokens_ok(doc, q, wrap, pad, alpha):
    return len(oracle.OracleIndex([doc], ngram_size=q, wrap=wrap, pad=pad, alphabet=alpha).tokenize(doc)) > 0


def test_identity_round_trip_at_1m():
    """Size-independent property at 1 M strings: a dictionary string queried verbatim comes back first with score
    exactly 1.0 (or an identical string with a smaller docID), for every metric."""
    from suggest_amd import NGramIndex, IndexDescription, synth
    blob, offs = synth.make_dict(1000000, seed=1)
    gpu = NGramIndex(blob=blob, offs=offs, description=IndexDescription(**synth.DESCRIPTION))
    pick = np.arange(0, 1000000, 977)[:1024]
    docs = synth.unpack(blob, offs)
    qs = [docs[i] for i in pick]
    qb, qo = oracle.pack_strings(qs)
    for metric, a in (("jaccard", 0.5), ("cosine", 0.4), ("dice", 0.5)):
        ids, sc, cnt = gpu.suggest_batch(blob=qb, offs=qo, metric=metric, similarity=a, k=10)
        assert (cnt >= 1).all()
        assert (sc[:, 0] == 1.0).all()
        assert all(docs[int(ids[r, 0])] == qs[r] and int(ids[r, 0]) <= int(pick[r]) for r in range(len(qs)))
        # scores are non-increasing and ties are ordered by ascending docID
        for r in range(len(qs)):
            c = int(cnt[r])
            assert all(sc[r, j] > sc[r, j + 1] or (sc[r, j] == sc[r, j + 1] and ids[r, j] < ids[r, j + 1]) for j in range(c - 1))


def test_service_disc_driver_golden(reference_tests, golden_dir):
    """TestConcurrencyOnDisc (pkg/suggest/service_test.go:11-80): testdata/config.json verbatim, DISC driver — the index
    files and the CDB dictionary the reference committed are opened directly."""
    import os
    from suggest_amd import CosineMetric, SearchConfig, Service, read_configs
    descriptions = read_configs(os.path.join(golden_dir, "config.json"))
    assert descriptions[0].driver == "DISC"
    svc = Service()
    svc.AddIndexByDescription(descriptions[0])
    t = reference_tests["service_cars"]
    for q, exp in zip(t["queries"], t["expected_values"]):
        res = svc.Suggest("cars", SearchConfig(q, t["topK"], CosineMetric(), t["similarity"]))
        assert [r.value for r in res] == exp, q
    assert svc.GetDictionaries() == ["cars"]


@pytest.mark.parametrize("g8", [0, 1, 2])
def test_dense_terms_with_8_bit_gaps(monkeypatch, cars_lines, g8):
    """The packed store keeps the lists of dense terms as {u32 first, 12 x u8 gaps} chunks (13 postings instead of 7;
    packed_store.inc, knob SG_G8: 0 never, 1 where it saves chunks, 2 every term).  Rows of such lists are decoded and
    counted by their own code (count_row8, flagged8, the overflow pass, the per-list searches of documents that repeat a
    term, the long-query kernel), so: bigram dictionaries (every list dense), plain and in near-duplicate families (queue
    overflow, ties), with the smallest counter array (docID-range passes cut on the chunks' first words), autocomplete,
    queries beyond the wavefront kernel's tables, and the reference's cars dictionary with every term forced to the
    format (gaps above 255 on every other posting: chunks of one or two postings; documents that repeat a term; the
    one-counter-per-document mode).  The rows never depend on the format."""
    from suggest_amd import NGramIndex, IndexDescription, synth
    monkeypatch.setenv("SG_G8", str(g8))
    desc = dict(synth.DESCRIPTION, ngram_size=2)
    bytes_of = {}
    for variant, n_docs, log2_cnt in ((dict(), 200000, None), (dict(families=3), 120000, None), (dict(skewed=True), 300000, "9")):
        if log2_cnt:
            monkeypatch.setenv("SG_LOG2_CNT", log2_cnt)
        blob, offs = synth.make_dict(n_docs, seed=41, **variant)
        qb, qo = synth.make_queries(384, blob, offs, seed=42)
        gpu = NGramIndex(blob=blob, offs=offs, description=IndexDescription(**desc))
        ora = oracle.OracleIndex(blob=blob, offs=offs, **desc)
        bytes_of[n_docs] = gpu.stats()["device_bytes"]
        for metric, alpha, k in (("dice", 0.5, 10), ("jaccard", 0.4, 3), ("cosine", 0.3, 100)):
            assert_same(gpu.suggest_batch(blob=qb, offs=qo, metric=metric, similarity=alpha, k=k), ora.suggest_batch(qb, qo, metric, alpha, k))
        ids, cnt = gpu.autocomplete_batch(blob=qb, offs=qo, limit=30)
        oi, oc, _ = ora.autocomplete_batch(qb, qo, 30)
        assert np.array_equal(cnt, oc)
        valid = np.arange(30)[None, :] < cnt[:, None]
        assert np.array_equal(ids[valid], oi[valid])
        # queries of 150 ... 400 bigrams: sg_long_kernel (ScanCount over the store)
        rnd = np.random.RandomState(7)
        long_q = [bytes(rnd.choice(list(b"abcdefghij0123456789"), size=int(n)).astype(np.uint8)) for n in rnd.randint(150, 400, size=6)]
        lb, lo = oracle.pack_strings(long_q)
        assert_same(gpu.suggest_batch(blob=lb, offs=lo, metric="dice", similarity=0.2, k=10), ora.suggest_batch(lb, lo, "dice", 0.2, 10), long_q)
        monkeypatch.delenv("SG_LOG2_CNT", raising=False)
    if g8 == 0:
        test_dense_terms_with_8_bit_gaps.plain_bytes = bytes_of
    elif getattr(test_dense_terms_with_8_bit_gaps, "plain_bytes", None):
        assert bytes_of[200000] < 0.93 * test_dense_terms_with_8_bit_gaps.plain_bytes[200000]     # the store shrank (postings are ~half of the replica)
    gpu = NGramIndex(cars_lines, _desc(CARS_DESC))
    ora = oracle.OracleIndex(cars_lines, **CARS_DESC)
    queries = list(cars_lines[::3]) + [l[1:] + b"x" for l in cars_lines[::7]]
    qb, qo = oracle.pack_strings(queries)
    for tighten in (0, 1):
        gpu.tune(SG_TIGHTEN=tighten)
        for metric, alpha, k in [("cosine", 0.5, 5), ("jaccard", 0.2, 100)]:
            assert_same(gpu.suggest_batch(blob=qb, offs=qo, metric=metric, similarity=alpha, k=k), ora.suggest_batch(qb, qo, metric, alpha, k), queries)


def test_saturating_bucket_and_candidate_overflow():
    """300 identical documents whose docIDs share their low 12 bits: every posting of a query term lands in the same
    counter bucket (a u8 counter would saturate -> the group is re-run with u32 counters) and the group has far more
    than 64 distinct candidates (-> second pass over the final counters).  Most documents are empty strings."""
    from suggest_amd import NGramIndex, IndexDescription, synth
    docs = [b""] * (300 * 4096)
    for i in range(300):
        docs[i * 4096] = b"saturating bucket"
    docs[0] = b"saturating bucket"
    docs[5] = b"saturating buckets"
    docs[77] = b"saturation bucket"
    desc = dict(synth.DESCRIPTION)
    gpu = NGramIndex(docs, IndexDescription(**desc))
    ora = oracle.OracleIndex(docs, **desc)
    queries = [b"saturating bucket", b"saturatin bucket", b"saturating buckets", b"zzz"]
    qb, qo = oracle.pack_strings(queries)
    for metric, a, k in (("jaccard", 0.5, 10), ("cosine", 0.6, 400), ("dice", 0.9, 1000)):
        assert_same(gpu.suggest_batch(blob=qb, offs=qo, metric=metric, similarity=a, k=k),
                    ora.suggest_batch(qb, qo, metric, a, k), queries)
    ids, cnt = gpu.autocomplete_batch(blob=qb, offs=qo, limit=50)
    oi, oc, _ = ora.autocomplete_batch(qb, qo, 50)
    assert np.array_equal(cnt, oc)
    valid = np.arange(50)[None, :] < cnt[:, None]
    assert np.array_equal(ids[valid], oi[valid])


@pytest.mark.parametrize("knobs", [dict(SG_T_FLOOR="2", SG_FILTER_LEVEL="0", SG_LOG2_CNT="9", SG_SPLIT_CHUNKS="0", SG_TIGHTEN="1", SG_ROOMY="0"),
                                   dict(SG_T_FLOOR="3", SG_FILTER_LEVEL="3", SG_LOG2_CNT="12", SG_SPLIT_CHUNKS="8", SG_TIGHTEN="0", SG_ROOMY="1"),
                                   dict(SG_T_FLOOR="64", SG_FILTER_LEVEL="1", SG_LOG2_CNT="10", SG_SPLIT_CHUNKS="200", SG_TIGHTEN="1", SG_ROOMY="1"),
                                   dict(SG_T_FLOOR="8", SG_FILTER_LEVEL="4", SG_LOG2_CNT="11", SG_TIGHTEN="0", SG_ROOMY="0")])
def test_results_do_not_depend_on_tuning_knobs(monkeypatch, knobs):
    """The lossy counters are only a filter (every flagged doc is verified exactly), so list-skipping depth,
    bucket-table strictness and counter-array size must not change a single output bit (DESIGN.md §4 knobs)."""
    from suggest_amd import NGramIndex, IndexDescription, synth
    for name, v in knobs.items():
        monkeypatch.setenv(name, v)
    desc = dict(synth.DESCRIPTION)
    blob, offs = synth.make_dict(300000, seed=21)
    qb, qo = synth.make_queries(1024, blob, offs, seed=22)
    gpu = NGramIndex(blob=blob, offs=offs, description=IndexDescription(**desc))
    ora = oracle.OracleIndex(blob=blob, offs=offs, **desc)
    for metric, alpha, k in (("jaccard", 0.5, 10), ("cosine", 0.35, 50), ("overlap", 0.6, 5)):
        assert_same(gpu.suggest_batch(blob=qb, offs=qo, metric=metric, similarity=alpha, k=k),
                    ora.suggest_batch(qb, qo, metric, alpha, k))


@pytest.mark.parametrize("variant", [dict(skewed=True), dict(families=3), dict(skewed=True, families=3)])
def test_skewed_and_family_dictionaries(variant):
    """SURVEY.md §8d dictionary variants: Zipf-distributed symbols (long lists) and families of near-duplicates
    (several matches per query: top-k eviction and score ties decided by docID)."""
    from suggest_amd import NGramIndex, IndexDescription, synth
    desc = dict(synth.DESCRIPTION)
    blob, offs = synth.make_dict(200000, seed=31, **variant)
    qb, qo = synth.make_queries(1024, blob, offs, seed=32)
    gpu = NGramIndex(blob=blob, offs=offs, description=IndexDescription(**desc))
    ora = oracle.OracleIndex(blob=blob, offs=offs, **desc)
    for metric, alpha, k in (("jaccard", 0.5, 10), ("jaccard", 0.3, 2), ("cosine", 0.4, 20), ("dice", 0.6, 3)):
        got = gpu.suggest_batch(blob=qb, offs=qo, metric=metric, similarity=alpha, k=k)
        assert_same(got, ora.suggest_batch(qb, qo, metric, alpha, k))
    if variant.get("families"):
        assert (got[2] >= 3).mean() > 0.3          # the variant does what it is for: many queries fill k=3


def test_concurrent_callers_share_one_handle(synth_small):
    """Suggest is called concurrently from arbitrary goroutines on one index; the C ABI must be
    re-entrant on a shared handle (per-call stream and buffers).  ctypes releases the GIL during the call."""
    import threading
    gpu, ora, qb, qo = synth_small
    n = len(qo) - 1
    want = ora.suggest_batch(qb, qo, "jaccard", 0.5, 10)
    errors = []

    def worker(t):
        try:
            for rep in range(4):
                lo, hi = (t * 37 + rep * 11) % (n // 2), n
                sb, so = qb[int(qo[lo]):int(qo[hi])], qo[lo:hi + 1] - qo[lo]
                ids, sc, cnt = gpu.suggest_batch(blob=sb, offs=so, metric="jaccard", similarity=0.5, k=10)
                assert np.array_equal(cnt, want[2][lo:hi])
                valid = np.arange(10)[None, :] < cnt[:, None]
                assert np.array_equal(ids[valid], want[0][lo:hi][valid])
                assert np.array_equal(sc.view(np.uint64)[valid], want[1][lo:hi].view(np.uint64)[valid])
        except BaseException as exc:  # noqa: BLE001
            errors.append(repr(exc))

    threads = [threading.Thread(target=worker, args=(t,)) for t in range(8)]
    [t.start() for t in threads]
    [t.join() for t in threads]
    assert not errors, errors


def test_split_queries_match_unsplit(monkeypatch, cars_lines, words_lines):
    """Heavy queries are cut into parts (ranges of segments) run by other wavefronts and merged by the part that
    finishes last (DESIGN.md §4 "split queries").  With SG_SPLIT_CHUNKS=1 every query with two valid segments is
    split: the cars workload (documents returned twice), autocomplete and the words goldens must
    not change by a bit."""
    from suggest_amd import NGramIndex
    monkeypatch.setenv("SG_SPLIT_CHUNKS", "1")
    gpu = NGramIndex(cars_lines, _desc(CARS_DESC))
    ora = oracle.OracleIndex(cars_lines, **CARS_DESC)
    queries = list(cars_lines[::3]) + [l[1:] + b"x" for l in cars_lines[::7]] + [b"", b"zzzzzz", b"NISSAN"]
    qb, qo = oracle.pack_strings(queries)
    for metric, alpha, k in [("cosine", 0.5, 5), ("jaccard", 0.2, 64), ("dice", 0.6, 3), ("cosine", 0.3, 200)]:
        assert_same(gpu.suggest_batch(blob=qb, offs=qo, metric=metric, similarity=alpha, k=k),
                    ora.suggest_batch(qb, qo, metric, alpha, k), queries)
    aq = [l[:n] for l in cars_lines[::9] for n in (3, 6)] + [b"AN "]
    ab, ao = oracle.pack_strings(aq)
    ids, cnt = gpu.autocomplete_batch(blob=ab, offs=ao, limit=20)
    oi, oc, _ = ora.autocomplete_batch(ab, ao, 20)
    assert np.array_equal(cnt, oc)
    valid = np.arange(20)[None, :] < cnt[:, None]
    assert np.array_equal(ids[valid], oi[valid])
    gpu = NGramIndex(words_lines, _desc(WORDS_DESC))
    ora = oracle.OracleIndex(words_lines, **WORDS_DESC)
    queries = [w for w in words_lines[::499]] + [w[:-1] + b"q" for w in words_lines[5::999]]
    qb, qo = oracle.pack_strings(queries)
    assert_same(gpu.suggest_batch(blob=qb, offs=qo, metric="jaccard", similarity=0.4, k=10),
                ora.suggest_batch(qb, qo, "jaccard", 0.4, 10), queries)


def test_device_index_build_is_identical_to_host_build(cars_lines, words_lines):
    """the index built on the GPU (device tokeniser, device term table, radix sort) has the same CSR —
    array for array (digests of postings, seg_off, list lengths, term numbering, repeated-term table) — as the host
    build, for the reference's dictionaries (cars: 211 documents repeat a term; words), synthetic ones (q = 2, 3) and
    awkward inputs (empty strings, non-ASCII, invalid UTF-8, strings shorter than q)."""
    from suggest_amd import NGramIndex, IndexDescription, synth
    cases = [(cars_lines, _desc(CARS_DESC)), (words_lines, _desc(WORDS_DESC))]
    for n, q, kw in ((200000, 3, {}), (50000, 2, {}), (100000, 3, dict(skewed=True, families=3))):
        blob, offs = synth.make_dict(n, seed=41, **kw)
        cases.append((synth.unpack(blob, offs), IndexDescription(**dict(synth.DESCRIPTION, ngram_size=q))))
    odd = [b"", b"a", b"  ", "Привет мир".encode(), b"\xff\xfe bad \xc3", "İstanbul ǅ".encode(), b"ab", b"x" * 100, b"AAAAAAAA", b"abcabcabc"]
    cases.append((odd * 7, IndexDescription(ngram_size=3, wrap=("$", "$"), pad="$", alphabet=("english", "russian", "numbers", "$"))))
    cases.append((odd * 3, IndexDescription(ngram_size=2, wrap=("^", "$"), pad="_", alphabet=("english", "_^$"))))
    # an empty pad turns n-grams of foreign runes into the EMPTY term (key 0) and makes most documents repeat terms
    cases.append(([b"ab - c", b"--- --", b"a-b", b"   ", b"abc", b"- -", b"cab cab"] * 40,
                  IndexDescription(ngram_size=3, wrap=("", ""), pad="", alphabet=("english", "numbers"))))
    for docs, desc in cases:
        host = NGramIndex(docs, desc, upload=False)
        dev = NGramIndex(docs, desc, upload=False, build="device")
        assert dev.stats() == host.stats()
        assert dev.digest() == host.digest()
    # and it searches like any other index
    blob, offs = synth.make_dict(100000, seed=43)
    qb, qo = synth.make_queries(512, blob, offs, seed=44)
    dev = NGramIndex(blob=blob, offs=offs, description=IndexDescription(**synth.DESCRIPTION), build="device")
    ora = oracle.OracleIndex(blob=blob, offs=offs, **synth.DESCRIPTION)
    assert_same(dev.suggest_batch(blob=qb, offs=qo, metric="jaccard", similarity=0.5, k=10), ora.suggest_batch(qb, qo, "jaccard", 0.5, 10))


def test_device_index_build_takes_long_documents():
    """Writer.AddDocument has no limit on a document's n-grams (indexer_writer.go:66-86): the device builder hands documents
    above the LDS tokeniser's 128 n-grams to its long tokeniser and produces the host builder's arrays; only a document
    above 65 536 bytes is refused (and the host builder takes that one)."""
    from suggest_amd import NGramIndex, IndexDescription, synth
    import random
    rnd = random.Random(5)
    long_doc = bytes(rnd.choice(b"abcdefghijklmnopqrstuvwxyz0123456789") for _ in range(400))
    docs = [b"short", long_doc, long_doc[:129], long_doc[100:300] * 3, b"abc" * 200]
    host = NGramIndex(docs, IndexDescription(**synth.DESCRIPTION), upload=False)
    assert NGramIndex(docs, IndexDescription(**synth.DESCRIPTION), upload=False, build="device").digest() == host.digest()
    huge = long_doc * 170                                               # 68 000 bytes
    with pytest.raises(Exception, match="sg_index_build"):
        NGramIndex([b"short", huge], IndexDescription(**synth.DESCRIPTION), upload=False, build="device")
    NGramIndex([b"short", huge], IndexDescription(**synth.DESCRIPTION), upload=False)             # the host builder takes it


def test_doc_sharded_index_merges_to_the_unsharded_result():
    """SURVEY.md §8e alternative design on one GPU: three docID-range shards (uneven: the last shard has shorter
    documents, so it has to be rebuilt with the global number of segments) searched separately and merged."""
    import torch
    from suggest_amd import NGramIndex, IndexDescription, synth
    from suggest_amd.distributed import merge_topk, shard_bounds
    desc = IndexDescription(**synth.DESCRIPTION)
    blob, offs = synth.make_dict(90000, seed=71, families=3)
    docs = synth.unpack(blob, offs)
    docs[60000:] = [d[:10] for d in docs[60000:]]                    # the last shard only has short documents
    blob, offs = oracle.pack_strings(docs)
    qb, qo = synth.make_queries(512, blob, offs, seed=72)
    full = NGramIndex(blob=blob, offs=offs, description=desc)
    S = full.stats()["n_segments"]
    k = 10
    rows = []
    for r in range(3):
        lo, hi = shard_bounds(len(docs), 3, r)
        sb, so = blob[int(offs[lo]):int(offs[hi])], (offs[lo:hi + 1] - offs[lo]).astype(np.uint64)
        shard = NGramIndex(blob=sb, offs=so, description=desc, min_segments=S, build="device" if r == 1 else "host")
        assert shard.stats()["n_segments"] == S
        ids, sc, cnt = shard.suggest_batch(blob=qb, offs=qo, metric="cosine", similarity=0.4, k=k)
        rows.append((torch.from_numpy(ids.astype(np.int64) + lo), torch.from_numpy(sc), torch.from_numpy(cnt.astype(np.int64))))
    m_ids, m_sc, m_cnt = merge_topk(torch.stack([r[0] for r in rows]), torch.stack([r[1] for r in rows]), torch.stack([r[2] for r in rows]), k)
    merged = (m_ids.numpy().astype(np.uint32), m_sc.numpy(), m_cnt.numpy().astype(np.uint32))
    assert_same(merged, full.suggest_batch(blob=qb, offs=qo, metric="cosine", similarity=0.4, k=k))
    assert (merged[2] > 1).mean() > 0.3


def test_limits_long_ngrams_max_k_and_query_length():
    """The edges of the wavefront kernel: n-grams of 5 and 8 runes (the 64-bit term key is full at 8), k = 1024 and beyond
    (top-k rows in HBM), queries with exactly 128 n-grams (its last) and one more (the first the long-query kernel takes)."""
    import random
    from suggest_amd import NGramIndex, IndexDescription, _lib
    rng = random.Random(77)
    words = ["".join(rng.choice("abcdefgh") for _ in range(rng.randint(4, 24))) for _ in range(3000)]
    for q in (5, 8):
        desc = dict(ngram_size=q, wrap=("$", "$"), pad="$", alphabet=("english", "$"))
        gpu = NGramIndex(words, IndexDescription(**desc))
        ora = oracle.OracleIndex(words, **desc)
        queries = [w[:-1] + "x" for w in words[::30]] + words[:40] + ["abc", "a" * q, "a" * (q - 1)]
        qb, qo = oracle.pack_strings(queries)
        for metric, a, k in (("jaccard", 0.3, 10), ("cosine", 0.5, 1024), ("dice", 0.2, 300), ("cosine", 0.2, 2500)):
            assert_same(gpu.suggest_batch(blob=qb, offs=qo, metric=metric, similarity=a, k=k), ora.suggest_batch(qb, qo, metric, a, k), queries)
    with pytest.raises(Exception):
        gpu.suggest_batch(queries[:1], metric="jaccard", similarity=0.5, k=_lib.SG_MAX_TOPK + 1)
    # query length: q = 3, wrap "$".."$": a string of L distinct-trigram runes has L n-grams
    desc = dict(ngram_size=3, wrap=("$", "$"), pad="$", alphabet=("english", "numbers", "$"))
    base = [bytes(rng.choice(b"abcdefghijklmnopqrstuvwxyz0123456789") for _ in range(rng.randint(100, 140))) for _ in range(300)]
    gpu = NGramIndex(base, IndexDescription(**desc))
    ora = oracle.OracleIndex(base, **desc)
    exact = [d for d in base if len(ora.tokenize(d)) == 128][:5] or [base[0][:128]]
    over = [d for d in base if len(ora.tokenize(d)) == 129][:5] or [base[0] + b"zq7"]
    qb, qo = oracle.pack_strings(exact + over)
    assert all(len(ora.tokenize(q)) <= 128 for q in exact) and all(len(ora.tokenize(q)) > 128 for q in over)
    got = gpu.suggest_batch(blob=qb, offs=qo, metric="jaccard", similarity=0.5, k=5)
    assert_same(got, ora.suggest_batch(qb, qo, "jaccard", 0.5, 5), exact + over)
    assert (got[2] >= 1).all()                                   # every one of them is in the dictionary


def test_long_queries_are_answered_on_the_device():
    """Queries with more than 128 n-grams (the wavefront kernel's tables): the reference has no such limit
    (pkg/suggest/suggester.go:46-59) — sg_long_kernel answers them with HBM working memory: ScanCount per segment, the
    same tokeniser rules (first-occurrence dedup over thousands of grams, non-ASCII runes, wrap), the secondary entries of
    documents that repeat a term, autocomplete, k above the LDS rows, mixed into a batch of ordinary queries."""
    import random
    from suggest_amd import NGramIndex, IndexDescription
    rng = random.Random(5)
    alpha = "abcdefghijklmnopqrstuvwxyz0123456789 "
    desc = dict(ngram_size=3, wrap=("$", "$"), pad="$", alphabet=("english", "russian", "numbers", "$"))

    def text(n, pool=alpha):
        return "".join(rng.choice(pool) for _ in range(n))

    docs = [text(rng.randint(5, 40)) for _ in range(400)]
    docs += [text(rng.randint(150, 900)) for _ in range(250)]                       # long documents (host builder)
    docs += [text(rng.randint(200, 500), "ab ") for _ in range(60)]                  # ... that repeat their terms over and over
    docs += [text(rng.randint(150, 400), "абвгдежз abc") for _ in range(60)]          # ... with non-ASCII runes
    docs += [docs[410] + "x", docs[410][:-3], docs[420][5:] + "tail"]
    gpu = NGramIndex(docs, IndexDescription(**desc))
    ora = oracle.OracleIndex(docs, **desc)
    # the device index builder takes the long documents too (Writer.AddDocument has no limit, indexer_writer.go:66-86):
    # same arrays as the host build, and the same answers from the store it leaves in HBM
    dev_built = NGramIndex(docs, IndexDescription(**desc), build="device")
    assert dev_built.digest() == gpu.digest()

    def edit(s):
        s = list(s)
        for _ in range(rng.randint(1, 6)):
            s[rng.randrange(len(s))] = rng.choice(alpha)
        return "".join(s)

    queries = [edit(d) for d in docs[400:] if len(d) > 130][::3] + docs[400:420] + [edit(d) for d in docs[:30]]
    queries += [text(3000), docs[405] * 3, "ab " * 700, "б" * 300 + docs[715][:200], "x" * 200]
    queries = [q.encode("utf-8") for q in queries]
    queries += [b"\xff\xfe" + docs[430].encode("utf-8"), docs[431][:140].encode("utf-8") + b"\xe2\x82" * 40 + "\u20ac".encode("utf-8") * 20]   # invalid UTF-8
    n_long = sum(1 for q in queries if len(ora.tokenize(q)) > 128)
    assert n_long > 50
    qb, qo = oracle.pack_strings(queries)
    for metric, a, k in (("jaccard", 0.5, 5), ("cosine", 0.3, 10), ("dice", 0.4, 100), ("overlap", 0.6, 7), ("cosine", 0.2, 70)):
        assert_same(gpu.suggest_batch(blob=qb, offs=qo, metric=metric, similarity=a, k=k), ora.suggest_batch(qb, qo, metric, a, k), queries)
    assert_same(dev_built.suggest_batch(blob=qb, offs=qo, metric="cosine", similarity=0.3, k=10), ora.suggest_batch(qb, qo, "cosine", 0.3, 10), queries)
    # autocomplete: every n-gram of the prefix must be in the document
    prefixes = [d[:rng.randint(130, 200)] for d in docs[400:460] if len(d) > 210] + [docs[10][:4], docs[405][:131]]
    pb, po = oracle.pack_strings(prefixes)
    for limit in (3, 80):
        g_ids, g_cnt = gpu.autocomplete_batch(blob=pb, offs=po, limit=limit)
        o_ids, o_cnt = ora.autocomplete_batch(pb, po, limit)[:2]
        assert np.array_equal(g_cnt, o_cnt)
        valid = np.arange(limit)[None, :] < np.minimum(o_cnt, limit)[:, None]
        assert np.array_equal(g_ids[valid], o_ids[valid])
    assert int(g_cnt.sum()) >= len(prefixes) - 2


@pytest.mark.parametrize("seed", [300004, 700812, 610200998, 77700102924])
def test_fuzz_regressions(seed, monkeypatch):
    """Trials of tools/fuzz_parity.py that found bugs: 300004 — device builder and the empty term (empty pad); 700812 — a u8
    counter wrapping within one batch (a query repeating one term 33 times, 2 KB of counters) went unnoticed.  610200998 and
    77700102924: the two reports nobody could replay — run as their hunts ran, behind pipeline launches on the
    same thread and stream, and with the scratch and result rows poisoned (sg_debug_poison), so that a word no launch of the
    trial wrote shows as a wrong row instead of an earlier call's leftover."""
    import importlib.util
    from suggest_amd import _lib
    spec = importlib.util.spec_from_file_location("fuzz_parity", os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools", "fuzz_parity.py"))
    fz = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(fz)
    t = fz.make_trial(seed)
    with _lib.poisoned(1):
        _pipeline_launches_first(monkeypatch)
        for name, value in t["env"].items():
            monkeypatch.setenv(name, value)
        assert fz.run_trial(t) == []


def _pipeline_launches_first(monkeypatch):
    """a pipeline trial on this thread's stream: its SCRATCH_ROWS / PIPE blocks are what the next launches inherit"""
    from suggest_amd import NGramIndex, IndexDescription, synth
    blob, offs = synth.make_dict(12000, seed=5)
    qb, qo = synth.make_queries(300, blob, offs, seed=6)
    for name, value in dict(SG_PIPE="1", SG_PRETOK="1", SG_ORDER="64", SG_TIGHTEN="0", SG_SPLIT_CHUNKS="0", SG_G8="0").items():
        monkeypatch.setenv(name, value)
    gpu = NGramIndex(blob=blob, offs=offs, description=IndexDescription(**synth.DESCRIPTION))
    ora = oracle.OracleIndex(blob=blob, offs=offs, **synth.DESCRIPTION)
    for metric, a, k in (("jaccard", 0.5, 64), ("cosine", 0.3, 10), ("dice", 0.9, 300)):
        assert_same(gpu.suggest_batch(blob=qb, offs=qo, metric=metric, similarity=a, k=k), ora.suggest_batch(qb, qo, metric, a, k))
    assert gpu.pipe_stats()["queries"] >= 3 * 300
    gpu.close()


def test_low_similarity_over_near_duplicates_stays_fast():
    """Fuzz trial 4200037 (scale 10): 200 012 near-duplicate documents over eight letters, Dice >= 0.15 / Overlap >= 0.3,
    97 queries of which 13 are above 128 n-grams.  It took the device 640 s (the CPU oracle: 6 s): the top-k filled with
    the worst admissible documents first and a million postings per query were verified, every document that repeats a
    term through the per-list path.  Thresholds that follow the top-k from the first launch on (similarity < 0.3), the
    segments next to |A| first, and one compare against the k-th best before the per-list path: 1 s.  Parity as ever."""
    import importlib.util, time
    spec = importlib.util.spec_from_file_location("fuzz_parity", os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools", "fuzz_parity.py"))
    fz = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(fz)
    t = fz.make_trial(4200037, 10)
    t["env"] = {}
    from suggest_amd import IndexDescription, NGramIndex
    gpu = NGramIndex(t["docs"], IndexDescription(**t["desc"]), build="host")
    qb, qo = oracle.pack_strings(t["queries"])
    t0 = time.time()
    for metric, a, k in t["searches"]:
        gpu.suggest_batch(blob=qb, offs=qo, metric=metric, similarity=a, k=k)
    gpu.autocomplete_batch(blob=qb, offs=qo, limit=t["limit"])
    took = time.time() - t0
    gpu.close()
    assert took < 30.0, took
    assert fz.run_trial(t) == []


def test_autocomplete_pages_through_every_match(golden_dir):
    """The reference's Autocomplete streams EVERY match to the caller's collector (pkg/suggest/autocomplete.go:40-77); a
    binding gets them all by paging (sg_autocomplete_one_from: the `limit` smallest docIDs >= first_doc)."""
    import lzma
    from conftest import WORDS_DESC
    from suggest_amd import NGramIndex, IndexDescription
    words = lzma.open(os.path.join(golden_dir, "words.dict.xz")).read().splitlines()[:60000]
    gpu = NGramIndex(words, IndexDescription(**WORDS_DESC))
    ora = oracle.OracleIndex(words, **WORDS_DESC)
    for prefix in (b"a", b"un", b"pre", b"zzq", b"inter"):
        qb, qo = oracle.pack_strings([prefix])
        o_ids, o_cnt = ora.autocomplete_batch(qb, qo, len(words))[:2]
        want = o_ids[0, :int(o_cnt[0])].tolist()
        for page in (7, 1000):
            if len(want) / page > 400:
                continue
            assert gpu.autocomplete_all(prefix, page=page) == want
    assert len(ora.autocomplete_batch(*oracle.pack_strings([b"a"]), len(words))[0]) > 0


def test_rows_do_not_depend_on_how_a_batch_is_cut(synth_small):
    """A query's row is the same whatever batch it travels in: one call of 36 867 queries (ordered by length on the
    device, above the 8192-query threshold of the order kernels) against the same queries in calls of 8000, and the
    oracle's rows on a sample."""
    from suggest_amd import synth
    gpu, ora, _, _ = synth_small
    blob, offs = synth.make_dict(50000, seed=1)
    n = 16384 * 2 + 4099                          # uneven pieces
    qb, qo = synth.make_queries(n, blob, offs, seed=5)
    ids, sc, cnt = gpu.suggest_batch(blob=qb, offs=qo, metric="jaccard", similarity=0.5, k=7)
    aid, acnt = gpu.autocomplete_batch(blob=qb, offs=qo, limit=5)
    for lo in range(0, n, 8000):
        hi = min(n, lo + 8000)
        so = (qo[lo:hi + 1] - qo[lo]).astype(np.uint64)
        sb = qb[int(qo[lo]):int(qo[hi])]
        i2, s2, c2 = gpu.suggest_batch(blob=sb, offs=so, metric="jaccard", similarity=0.5, k=7)
        assert_same((ids[lo:hi], sc[lo:hi], cnt[lo:hi]), (i2, s2, c2))
        a2, ac2 = gpu.autocomplete_batch(blob=sb, offs=so, limit=5)
        assert (acnt[lo:hi] == ac2).all()
        valid = np.arange(5)[None, :] < np.minimum(ac2, 5)[:, None]
        assert (aid[lo:hi][valid] == a2[valid]).all()
    pick = np.arange(0, n, 37)
    po = np.zeros(len(pick) + 1, np.uint64)
    po[1:] = np.cumsum(qo[pick + 1] - qo[pick])
    pb = np.concatenate([qb[int(qo[i]):int(qo[i + 1])] for i in pick])
    assert_same((ids[pick], sc[pick], cnt[pick]), ora.suggest_batch(pb, po, "jaccard", 0.5, 7))


def test_rows_above_the_staging_limit_equal_small_calls(synth_small):
    """A call whose rows pass the 64 MB staging limit (6 000 queries x k = 1 100: 79 MB, in HBM rows above SG_K_LDS) copies
    straight to the caller's arrays; a slice of it with offsets that do not start at zero stages only its rebased inputs.
    Both give the rows of the same queries in staged calls of 1 000."""
    from suggest_amd import synth
    gpu, _, _, _ = synth_small
    blob, offs = synth.make_dict(50000, seed=1)
    n, k = 6000, 1100
    qb, qo = synth.make_queries(n, blob, offs, seed=7)
    assert n * k * 12 > 64 << 20
    ids, sc, cnt = gpu.suggest_batch(blob=qb, offs=qo, metric="cosine", similarity=0.3, k=k)
    lo = 500
    si, ss, sn = gpu.suggest_batch(blob=qb, offs=qo[lo:], metric="cosine", similarity=0.3, k=k)
    assert_same((si, ss, sn), (ids[lo:], sc[lo:], cnt[lo:]))
    for a in range(0, n, 1000):
        b = min(n, a + 1000)
        i2, s2, c2 = gpu.suggest_batch(blob=qb, offs=qo[a:b + 1], metric="cosine", similarity=0.3, k=k)
        assert_same((ids[a:b], sc[a:b], cnt[a:b]), (i2, s2, c2))


class _OracleBacked:
    """metric.Metric (pkg/metric/metric.go:7-16) as an opaque implementation: the four methods answer from the ORACLE's
    restatement of pkg/metric/*.go, and nothing tells the engine which metric it is (code None) — it is tabulated."""
    code = None

    def __init__(self, name):
        self.name = name

    def MinY(self, alpha, size): return oracle.metric_min_y(self.name, alpha, size)
    def MaxY(self, alpha, size): return oracle.metric_max_y(self.name, alpha, size)
    def Threshold(self, alpha, a, b): return oracle.metric_threshold(self.name, alpha, a, b)
    def Distance(self, inter, a, b): return 1 - oracle.metric_score(self.name, inter, a, b)     # (only 1 - Distance is tabulated: see below)


@pytest.mark.parametrize("metric,alpha", METRICS)
def test_tabulated_metric_equals_the_native_one(synth_small, metric, alpha):
    """sg_metric_tables_create + sg_suggest_batch_tables: an opaque Metric implementation reaches the engine as tables of its
    four methods; filled from the oracle's own metric functions (scores taken as the oracle computes them) the rows must be
    the native metric's, bit for bit — ids, order, score bits — and so must the Python mirror's own formulas
    (suggest_amd/metric.py)."""
    gpu, ora, qb, qo = synth_small
    want = ora.suggest_batch(qb, qo, metric, alpha, 10)

    class Exact(_OracleBacked):
        pass
    m = Exact(metric)
    tb = gpu.metric_tables(m, alpha, 48)
    # the score table holds what metricScorer.Score returns (scorer.go:29-31); write the oracle's own doubles over the
    # 1 - (1 - x) round trip of the duck above so that the comparison is bit-exact by construction of the TABLE, not of Python
    S = gpu.stats()["n_segments"]
    score = np.zeros((49, S, 49))
    thr = np.zeros((49, S), np.int32)
    mn = np.array([oracle.metric_min_y(metric, alpha, a) for a in range(49)], np.int32)
    mx = np.array([min(oracle.metric_max_y(metric, alpha, a), 2**31 - 1) for a in range(49)], np.int32)
    for a in range(1, 49):
        for b in range(max(0, int(mn[a])), min(S - 1, int(mx[a])) + 1):
            thr[a, b] = oracle.metric_threshold(metric, alpha, a, b)
            for o in range(max(0, int(thr[a, b])), min(a, 48) + 1):
                score[a, b, o] = oracle.metric_score(metric, o, a, b)
    import ctypes as C
    from suggest_amd import _lib
    from suggest_amd.index import MetricTables
    t = C.c_void_p()
    _lib.check(_lib.lib().sg_metric_tables_create(gpu._h, 48, mn.ctypes.data, mx.ctypes.data, thr.ctypes.data, score.ctypes.data, C.byref(t)))
    assert_same(gpu.suggest_batch(blob=qb, offs=qo, k=10, tables=MetricTables(t, 48)), want)
    # the Python mirror of pkg/metric (IEEE doubles, Go's evaluation order) through the same path
    from suggest_amd.metric import resolve

    class Opaque:                                           # a duck: no code, the built-in's four methods
        code = None

        def __init__(self, inner):
            self.MinY, self.MaxY, self.Threshold, self.Distance = inner.MinY, inner.MaxY, inner.Threshold, inner.Distance
    assert_same(gpu.suggest_batch(blob=qb, offs=qo, metric=Opaque(resolve(metric)), similarity=alpha, k=10), want)
    del tb


def test_tabulated_metric_of_the_callers_own(cars_lines):
    """A Metric the engine has never heard of — Tversky-like, asymmetric in |A| and |B| — against a brute-force evaluation of
    the reference's definition of Suggest on the oracle's tokens: every document of cardinality in [MinY, MaxY] whose overlap
    reaches Threshold, scored 1 - Distance, top-k by (score desc, docID asc)."""
    import math
    from suggest_amd import NGramIndex

    class Tversky:
        code = None

        def MinY(self, alpha, size): return int(math.ceil(alpha * size * 0.75))
        def MaxY(self, alpha, size): return int(math.floor(size / alpha * 1.25))
        def Threshold(self, alpha, a, b): return int(math.ceil(alpha * (0.75 * a + 0.25 * b)))
        def Distance(self, inter, a, b): return 1 - inter / (0.75 * a + 0.25 * b)
    docs = [l for l in cars_lines[:1500]]
    gpu = NGramIndex(docs, _desc(CARS_DESC))
    ora = oracle.OracleIndex(docs, **CARS_DESC)
    toks = [ora.tokenize(d) for d in docs]
    m, alpha, k = Tversky(), 0.55, 7
    queries = [docs[i] for i in range(0, 1500, 37)] + [docs[i][1:-1] + b"q" for i in range(5, 1500, 91)]
    ids, sc, cnt = gpu.suggest_batch(queries, m, alpha, k)
    S = gpu.stats()["n_segments"]
    for qi, q in enumerate(queries):
        qt = ora.tokenize(q)
        A = len(qt)
        if A == 0:
            assert cnt[qi] == 0
            continue
        lo, hi = m.MinY(alpha, A), min(m.MaxY(alpha, A), S - 1)
        cands = []
        for d, dt in enumerate(toks):
            B = len(dt)
            if not (lo <= B <= hi) or len(set(dt)) != B:       # (documents that repeat a term have secondary entries: left out of the brute force)
                continue
            T = m.Threshold(alpha, A, B)
            if T == 0 or T > B or T > A:
                continue
            ds = set(dt)
            ov = sum(1 for t in qt if t in ds)
            if ov >= T:
                cands.append((-(1 - m.Distance(ov, A, B)), d))
        cands.sort()
        dup_docs = {d for d, dt in enumerate(toks) if len(set(dt)) != len(dt)}
        got = [(int(ids[qi, j]), float(sc[qi, j])) for j in range(int(cnt[qi]))]
        if any(d in dup_docs for d, _ in got):
            continue
        assert got == [(d, -s) for s, d in cands[:k]], (q, got, cands[:k])


def test_suggest_pages_through_every_candidate(cars_lines):
    """sg_suggest_batch_from: the fuzzy search for ANY collector — every document whose overlap reaches its segment's threshold,
    ascending docID, paged — against the oracle's Suggest with k = the whole dictionary (the same candidates, ordered by
    score): the multisets of (docID, score bits) must be equal, documents that repeat a term (several entries) included, for
    pages that end inside such runs too."""
    from suggest_amd import NGramIndex
    gpu = NGramIndex(cars_lines, _desc(CARS_DESC))
    ora = oracle.OracleIndex(cars_lines, **CARS_DESC)
    queries = [b"Nissan Mar", b"NISSAN TITAN", b"toyota corola", cars_lines[3238], cars_lines[1111][:-3], b"zzzzzz", b"a"]
    # ... and dictionary lines that repeat a term (the reference returns such a document more than once)
    rep = [l for l in cars_lines if len(ora.tokenize(l)) != len(set(ora.tokenize(l)))]
    queries += rep[:3] + rep[len(rep) // 2:len(rep) // 2 + 3]
    n_multi = 0
    for metric, alpha in (("jaccard", 0.3), ("cosine", 0.5), ("dice", 0.4)):
        for q in queries:
            qb, qo = oracle.pack_strings([q])
            oi, os_, oc = ora.suggest_batch(qb, qo, metric, alpha, len(cars_lines) * 2)[:3]
            if oc[0] >= 0xFFFFFFF0:
                continue
            want = sorted((int(oi[0, j]), int(os_.view(np.uint64)[0, j])) for j in range(int(oc[0])))
            n_multi += len(want) != len({d for d, _ in want})
            for page in (3, 64, 5000):
                if len(want) / page > 300:
                    continue
                rows = gpu.suggest_all(q, metric, alpha, page=page)
                ids = [r[0] for r in rows]
                assert ids == sorted(ids)
                got = sorted((r[0], int(np.float64(r[1]).view(np.uint64))) for r in rows)
                assert got == want, (metric, q, page, got[:5], want[:5])
                for d, s, ov, seg in rows:                       # aux: the overlap and segment the score came from
                    assert np.float64(oracle.metric_score(metric, ov, len(ora.tokenize(q)), seg)).view(np.uint64) == np.float64(s).view(np.uint64)
    assert n_multi >= 3      # documents with several entries were among the results
    # batches, and first_doc / limit as given
    qb, qo = oracle.pack_strings(queries)
    ids, sc, aux, cnt = gpu.suggest_batch_from(blob=qb, offs=qo, metric="cosine", similarity=0.5, first_doc=2000, limit=16)
    for i, q in enumerate(queries):
        if cnt[i] >= 0xFFFFFFF0:
            continue
        rows = [r for r in gpu.suggest_all(q, "cosine", 0.5) if r[0] >= 2000][:16]
        assert [r[0] for r in rows] == ids[i, :int(cnt[i])].tolist()
