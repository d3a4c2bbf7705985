"""One batch whose queries differ in metric, similarity and k (sg_suggest_batch_mixed; suggest_amd/csrc/mixed_batch.inc).
Expected rows come from the oracle, run once per config on that config's queries, compared bit for bit — ids, score bit patterns,
counts with every SG_COUNT_* flag — and the ragged rows are compared byte for byte against the same index's plain calls.  The
grouping itself (sg_debug_mixed_last) is held against tests/mixed_shapes.py word for word."""
import ctypes as C
import threading
import time

import numpy as np
import pytest

import mixed_shapes as ms
import oracle
from conftest import CARS_DESC

pytestmark = pytest.mark.gpu

SPECIAL = 0xFFFFFFF0          # counts at and above: SG_COUNT_* flags (no row)
HALF_UP = float(np.nextafter(0.5, 1.0))

# the table the tests draw from: all five metrics, k across the LDS / HBM top-k boundary (64 | 65), autocomplete with and without
# first_doc, two configs a last bit of similarity apart, two equal ones, and one whose window is empty for long queries
CONFIGS = [
    dict(metric="jaccard", similarity=0.5, k=10),
    dict(metric="cosine", similarity=0.4, k=1),
    dict(metric="dice", similarity=0.5, k=64),
    dict(metric="exact", similarity=1.0, k=65),
    dict(metric="overlap", similarity=0.6, k=100),
    dict(autocomplete=1, k=5),
    dict(autocomplete=1, k=7, first_doc=1000),
    dict(metric="jaccard", similarity=HALF_UP, k=10),
    dict(metric="jaccard", similarity=0.5, k=10),
    dict(metric="jaccard", similarity=0.95, k=3),
]


class World:
    def __init__(self, docs, desc):
        from suggest_amd import IndexDescription, NGramIndex
        self.docs = docs
        self.gpu = NGramIndex(docs, IndexDescription(**desc))
        self.ora = oracle.OracleIndex(docs, **desc)
        self.cache = {}

    def close(self):
        self.gpu.close()
        self.ora.close()

    def reference(self, cfg, queries):
        """-> (oracle (ids, scores | None, counts), plain call (ids, scores, counts)) of `queries` under `cfg`, [n, k] rows; computed
        once per (config, queries)"""
        key = (tuple(sorted(cfg.items())), tuple(queries))
        if key not in self.cache:
            self.cache[key] = (self._oracle(cfg, queries), self._plain(cfg, queries))
        return self.cache[key]

    def _oracle(self, cfg, queries):
        qb, qo = oracle.pack_strings(queries)
        k = cfg["k"]
        if not cfg.get("autocomplete"):
            return self.ora.suggest_batch(qb, qo, cfg["metric"], cfg["similarity"], k)[:3]
        first = cfg.get("first_doc", 0)
        if not first:
            ids, cnt, _ = self.ora.autocomplete_batch(qb, qo, k)
            return ids, None, cnt
        # the k smallest docIDs >= first_doc among ALL matches (the oracle lists them ascending)
        all_ids, all_cnt, _ = self.ora.autocomplete_batch(qb, qo, len(self.docs))
        ids = np.zeros((len(queries), k), dtype=np.uint32)
        cnt = np.zeros(len(queries), dtype=np.uint32)
        for i in range(len(queries)):
            if all_cnt[i] >= SPECIAL:
                cnt[i] = all_cnt[i]
                continue
            row = [d for d in all_ids[i, :int(all_cnt[i])].tolist() if d >= first][:k]
            ids[i, :len(row)] = row
            cnt[i] = len(row)
        return ids, None, cnt

    def _plain(self, cfg, queries):
        from suggest_amd import _lib
        k = cfg["k"]
        if not cfg.get("autocomplete"):
            return self.gpu.suggest_batch(queries, cfg["metric"], cfg["similarity"], k)
        qb, qo = oracle.pack_strings(queries)
        ids = np.zeros((len(queries), k), dtype=np.uint32)
        cnt = np.zeros(len(queries), dtype=np.uint32)
        with self.gpu._use() as h:
            _lib.check(_lib.lib().sg_autocomplete_batch_from(h, qb.ctypes.data if qb.size else None, qo.ctypes.data, len(queries),
                                                             int(cfg.get("first_doc", 0)), k, ids.ctypes.data, cnt.ctypes.data))
        return ids, np.zeros((len(queries), k), dtype=np.float64), cnt


@pytest.fixture(scope="module")
def cars(cars_lines):
    w = World(cars_lines, CARS_DESC)
    yield w
    w.close()


@pytest.fixture(scope="module")
def synth20k():
    from suggest_amd import synth
    blob, offs = synth.make_dict(20000, seed=11)
    w = World([bytes(blob[offs[i]:offs[i + 1]]) for i in range(len(offs) - 1)], synth.DESCRIPTION)
    yield w
    w.close()


def _pool(w, n, seed):
    """n queries from the dictionary: entries as they are, with a byte dropped, with two bytes appended, prefixes"""
    rng = np.random.RandomState(seed)
    out = []
    for i in rng.randint(0, len(w.docs), n):
        d = bytes(w.docs[int(i)])
        kind = int(rng.randint(0, 4))
        if kind == 1 and len(d) > 3:
            cut = int(rng.randint(0, len(d)))
            d = d[:cut] + d[cut + 1:]
            d = d.decode("utf-8", "ignore").encode("utf-8")          # (a rune cut in half: dropped whole)
        elif kind == 2:
            d = d + b"qz"
        elif kind == 3:
            d = d.decode("utf-8", "ignore")[:int(rng.randint(1, 8))].encode("utf-8")
        out.append(d)
    return out


def _check(w, queries, configs, config_of, got, family=None, what=""):
    """got = (ids, scores, counts, row_offs) of a mixed call: row_offs by the rules, counts == the oracle's, every counted entry the
    oracle's bit for bit, and the whole ragged arrays the plain calls' byte for byte (poison `family` on: for both alike)"""
    ids, sc, cnt, row_offs = got
    config_of = np.asarray(config_of, dtype=np.uint32)
    ks = [c["k"] for c in configs]
    ms.check_row_offsets(row_offs, config_of, ks)
    assert np.array_equal(row_offs, ms.row_offsets(config_of, ks)), what
    assert ids.shape == sc.shape == (int(row_offs[-1]),) and cnt.shape == (len(queries),), what
    want_ids, want_sc = np.zeros_like(ids), np.zeros_like(sc)
    want_cnt = np.zeros_like(cnt)
    for g, cfg in enumerate(configs):
        members = np.flatnonzero(config_of == g)
        if members.size == 0:
            continue
        (oi, os_, oc), (pi, ps, pc) = w.reference(cfg, [queries[int(i)] for i in members])
        k = cfg["k"]
        for r, i in enumerate(members.tolist()):
            at = int(row_offs[i])
            assert cnt[i] == oc[r], (what, "count differs from the oracle's", i, g, queries[i], int(cnt[i]), int(oc[r]))
            m = 0 if oc[r] >= SPECIAL else min(int(oc[r]), k)
            assert np.array_equal(ids[at:at + m], oi[r, :m]), (what, "ids differ from the oracle's", i, g, queries[i])
            if os_ is not None:
                assert np.array_equal(sc[at:at + m].view(np.uint64), os_[r, :m].view(np.uint64)), (what, "scores differ from the oracle's", i, g, queries[i])
            want_ids[at:at + k], want_sc[at:at + k], want_cnt[i] = pi[r], ps[r], pc[r]
            if family is None:
                assert not ids[at + m:at + k].any() and not sc[at + m:at + k].view(np.uint64).any(), (what, "slots past the count are not zero", i, g)
            else:
                from suggest_amd import _lib
                word = _lib.POISON_WORD[family]
                assert np.all(ids[at + m:at + k] == word), (what, "an id slot past the count lost the pattern", i, g)
                tail = sc[at + m:at + k].view(np.uint64)
                assert np.all(tail == (0 if cfg.get("autocomplete") else (word << 32 | word))), (what, "a score slot past the count lost the pattern", i, g)
    assert np.array_equal(cnt, want_cnt), what
    if family is None:       # (under poison a plain autocomplete call has no score rows to compare; the slots were checked above)
        assert np.array_equal(ids, want_ids) and np.array_equal(sc.view(np.uint64), want_sc.view(np.uint64)), (what, "rows differ from the plain calls'")


def _run(w, queries, configs, config_of):
    return w.gpu.suggest_batch_mixed(queries, configs, np.asarray(config_of, dtype=np.uint32))


def _check_grouping(config_of, n_configs):
    from suggest_amd.index import mixed_last
    perm, start = mixed_last(len(config_of), n_configs)
    want_perm, want_start = ms.permutation(config_of, n_configs)
    ms.check_permutation(perm, start, config_of, n_configs)
    assert np.array_equal(perm, want_perm) and np.array_equal(start, want_start)


def test_group_sizes_across_wavefront_and_workgroup_boundaries(synth20k):
    """0, 1, 63, 64, 65 and 257 queries per config in one call, the configs interleaved"""
    w = synth20k
    base = ms.sizes_batch()
    config_of = base[ms.order(base, "shuffled")]
    queries = _pool(w, len(config_of), 21)
    configs = [CONFIGS[g] for g in (0, 1, 2, 3, 4, 5)]
    _check(w, queries, configs, config_of, _run(w, queries, configs, config_of))
    _check_grouping(config_of, len(configs))
    assert np.diff(ms.permutation(config_of, 6)[1].astype(np.int64)).tolist() == list(ms.GROUP_SIZES)


def test_one_query_and_one_config(cars):
    w = cars
    got = _run(w, [b"nissan ma"], CONFIGS[:3], [2])
    _check(w, [b"nissan ma"], CONFIGS[:3], [2], got)
    _check_grouping(np.array([2]), 3)
    # one config: the plain call, and the permutation is the identity
    queries = _pool(w, 70, 22)
    got = _run(w, queries, [CONFIGS[0]], np.zeros(70, dtype=np.uint32))
    _check(w, queries, [CONFIGS[0]], np.zeros(70, dtype=np.uint32), got)
    pi, ps, pc = w.gpu.suggest_batch(queries, "jaccard", 0.5, 10)
    assert np.array_equal(got[0], pi.ravel()) and np.array_equal(got[1].view(np.uint64), ps.ravel().view(np.uint64)) and np.array_equal(got[2], pc)
    from suggest_amd.index import mixed_last
    perm, start = mixed_last(70, 1)
    assert perm.tolist() == list(range(70)) and start.tolist() == [0, 70]
    # no query at all
    ids, sc, cnt, ro = _run(w, [], CONFIGS[:2], [])
    assert ids.size == 0 and cnt.size == 0 and ro.tolist() == [0]


def test_256_configs_each_used_once_and_one_twice(cars):
    w = cars
    metrics = ("jaccard", "cosine", "dice", "overlap")
    configs = [dict(metric=metrics[g % 4], similarity=0.3 + 0.002 * g, k=g + 1) for g in range(256)]
    c256 = np.concatenate([np.arange(256), [17]]).astype(np.uint32)
    config_of = c256[ms.order(c256, "shuffled", seed=3)]
    queries = _pool(w, 257, 23)
    _check(w, queries, configs, config_of, _run(w, queries, configs, config_of))
    _check_grouping(config_of, 256)


@pytest.mark.parametrize("how", ms.ORDERS)
def test_rows_follow_the_caller_order(cars, how):
    """the same multiset of (query, config) sorted by config, reversed, round-robin and shuffled: row i always answers query i"""
    w = cars
    rng = np.random.RandomState(24)
    sorted_cfg = np.sort(rng.randint(0, len(CONFIGS), 300)).astype(np.uint32)
    sorted_q = _pool(w, 300, 25)
    o = ms.order(sorted_cfg, how)
    config_of, queries = sorted_cfg[o], [sorted_q[int(i)] for i in o]
    _check(w, queries, CONFIGS, config_of, _run(w, queries, CONFIGS, config_of), what=how)
    _check_grouping(config_of, len(CONFIGS))


def _of_bytes(n, lead):
    """a query of exactly n bytes: `lead` ASCII bytes, then two-byte Cyrillic runes (at odd offsets for an odd lead), ASCII to fill"""
    s = b"a" * min(lead, n)
    while len(s) + 2 <= n and len(s) < lead + 8:
        s += "ж".encode("utf-8")
    return s + b"b" * (n - len(s))


def test_query_lengths_and_alignment(cars):
    """0 .. 33 bytes with two-byte runes at odd offsets, an empty query first and last: the gather's alignment cases — source and
    destination 16, 8, 4 bytes apart and not at all, ragged heads and tails"""
    w = cars
    lengths = (0, 1, 2, 3, 4, 5, 15, 16, 17, 31, 32, 33)
    queries = [b""] + [_of_bytes(n, lead) for lead in (1, 0, 3) for n in lengths] + _pool(w, 40, 26)[:40] + [_of_bytes(n, 1) for n in lengths] + [b""]
    assert [len(q) for q in queries[1:13]] == list(lengths) and queries[0] == queries[-1] == b""
    rng = np.random.RandomState(27)
    for trial in range(3):              # three assignments: every query meets other neighbours in its group, other offsets
        config_of = rng.randint(0, len(CONFIGS), len(queries)).astype(np.uint32)
        _check(w, queries, CONFIGS, config_of, _run(w, queries, CONFIGS, config_of), what="trial %d" % trial)


def test_long_queries_and_flagged_rows(cars):
    """one query above 112 bytes and one above 128 n-grams in groups of otherwise short queries (the per-group no_long_queries, the
    long-query kernel), and pairs the plain call flags: SG_COUNT_REF_PANIC and SG_COUNT_REF_DEADLOCK arrive in the caller's order"""
    w = cars
    long112 = (b"toyota land cruiser prado " * 5)[:118]
    long128 = (b"mercedes benz sprinter classic " * 8)[:200]
    text = bytes(np.random.RandomState(40).choice(list(b"abcdefghijklmnopqrstuvwxyz0123456789"), 120).tolist())
    sweep = [text[:n] for n in range(40, 112)]             # distinct n-grams: MinY walks past the last segment (52 of them)
    queries = _pool(w, 60, 28) + [long112] + _pool(w, 30, 29) + [long128] + sweep
    config_of = np.array([(i * 7) % len(CONFIGS) for i in range(len(queries))], dtype=np.uint32)
    config_of[60], config_of[91] = 0, 2                    # the long ones: a jaccard group, a dice group ...
    config_of[92:] = 9                                     # ... and the sweep under jaccard 0.95
    config_of[92::3] = 0
    got = _run(w, queries, CONFIGS, config_of)
    _check(w, queries, CONFIGS, config_of, got)
    flags = set(int(c) for c in got[2] if c >= SPECIAL)
    assert {0xFFFFFFFF, 0xFFFFFFFE} <= flags, flags
    # a group with a long query beside a group without: both at once (config 5, autocomplete, holds only short ones)
    short = [q for q in queries if len(q) <= 112]
    mixed_q = [long128] + short[:20]
    mixed_c = np.array([0] + [5] * 20, dtype=np.uint32)
    _check(w, mixed_q, CONFIGS, mixed_c, _run(w, mixed_q, CONFIGS, mixed_c))


@pytest.mark.parametrize("family", [1, 2])
def test_scratch_reuse_on_one_thread_under_poison(synth20k, family):
    """4 096 queries, then 3, then the 4 096 again with other k's, on one thread (one scratch block, one device block): with the
    poison on, the counted entries equal the unpoisoned run's and every slot past a count holds the pattern"""
    from suggest_amd import _lib, synth
    w = synth20k
    if not hasattr(w, "big"):
        blob, offs = synth.make_dict(20000, seed=11)
        qb, qo = synth.make_queries(4096, blob, offs, seed=31)
        w.big = [bytes(qb[qo[i]:qo[i + 1]]) for i in range(4096)]
        w.big_cfg = np.random.RandomState(32).randint(0, 4, 4096).astype(np.uint32)
    first = [CONFIGS[0], CONFIGS[2], CONFIGS[5], CONFIGS[3]]
    second = [dict(CONFIGS[0], k=3), dict(CONFIGS[2], k=70), dict(CONFIGS[5], k=9), dict(CONFIGS[3], k=2)]
    tiny_q, tiny_c = [b"abcde", b"", w.big[5]], np.array([3, 1, 0], dtype=np.uint32)
    clean = [_run(w, w.big, first, w.big_cfg), _run(w, tiny_q, first, tiny_c), _run(w, w.big, second, w.big_cfg)]
    _check(w, w.big, first, w.big_cfg, clean[0])
    _check(w, tiny_q, first, tiny_c, clean[1])
    _check(w, w.big, second, w.big_cfg, clean[2])
    with _lib.poisoned(family):
        dirty = [_run(w, w.big, first, w.big_cfg), _run(w, tiny_q, first, tiny_c), _run(w, w.big, second, w.big_cfg)]
        stats = _lib.poison_stats()
    assert set(stats) == set(_lib.POISON_REGIONS) and stats["out_ids"] > 0 and stats["rows"] > 0
    for (queries, configs, config_of), c, d in zip(((w.big, first, w.big_cfg), (tiny_q, first, tiny_c), (w.big, second, w.big_cfg)), clean, dirty):
        assert np.array_equal(c[2], d[2]) and np.array_equal(c[3], d[3])
        ks = np.array([cf["k"] for cf in configs])[config_of]
        slot = np.arange(int(c[3][-1])) - np.repeat(c[3][:-1].astype(np.int64), ks)
        counted = slot < np.repeat(np.where(c[2] >= SPECIAL, 0, np.minimum(c[2], ks)), ks)
        assert np.array_equal(c[0][counted], d[0][counted]) and np.array_equal(c[1].view(np.uint64)[counted], d[1].view(np.uint64)[counted])
        _check(w, queries, configs, config_of, d, family=family)
    # off again: zeros past the counts
    again = _run(w, tiny_q, first, tiny_c)
    for a, b in zip(again, clean[1]):
        assert np.array_equal(a.view(np.uint8), b.view(np.uint8))


def test_device_route_on_a_stream_of_its_own(cars):
    """the same inputs resident in HBM, on a non-default stream: every output, row_offs included, equals the host route's byte for
    byte; a config number equal to n_configs is refused by a check on the device, and the index answers the next call"""
    import torch
    from suggest_amd import _lib
    w = cars
    rng = np.random.RandomState(33)
    queries = [b""] + _pool(w, 500, 34) + [b""]
    config_of = rng.randint(0, len(CONFIGS), len(queries)).astype(np.uint32)
    host = _run(w, queries, CONFIGS, config_of)
    _check(w, queries, CONFIGS, config_of, host)
    qb, qo = oracle.pack_strings(queries)
    dev = torch.device("cuda", 0)
    pad = 3                                                   # the blob does not start at an aligned address
    d_blob = torch.zeros(qb.size + pad + 1, dtype=torch.uint8, device=dev)
    d_blob[pad:pad + qb.size] = torch.from_numpy(qb).to(dev)
    d_offs = torch.from_numpy((qo + np.uint64(pad)).view(np.int64)).to(dev)            # absolute offsets into d_blob
    d_cfg = torch.from_numpy(config_of.view(np.int32)).to(dev)
    rows = int(host[3][-1])
    stream = torch.cuda.Stream(device=dev)

    def call(d_config_of, cap=rows):
        out = (torch.full((rows,), -1, dtype=torch.int32, device=dev), torch.full((rows,), -1.0, dtype=torch.float64, device=dev),
               torch.full((len(queries),), -1, dtype=torch.int32, device=dev), torch.full((len(queries) + 1,), -1, dtype=torch.int64, device=dev))
        torch.cuda.synchronize()
        w.gpu.suggest_batch_mixed_device(d_blob.data_ptr(), d_offs.data_ptr(), len(queries), CONFIGS, d_config_of.data_ptr(), cap,
                                         out[0].data_ptr(), out[1].data_ptr(), out[2].data_ptr(), out[3].data_ptr(), stream=stream.cuda_stream)
        stream.synchronize()
        return (out[0].cpu().numpy().view(np.uint32), out[1].cpu().numpy(), out[2].cpu().numpy().view(np.uint32), out[3].cpu().numpy().view(np.uint64))

    got = call(d_cfg)
    for name, a, b in zip(("ids", "scores", "counts", "row_offs"), got, host):
        assert np.array_equal(a.view(np.uint8), b.view(np.uint8)), name
    # rows_cap one short: refused once the device has counted
    with pytest.raises(_lib.SuggestHipError) as e:
        call(d_cfg, cap=rows - 1)
    assert e.value.code == -1 and "rows_cap" in str(e.value)
    # one config number equal to n_configs
    bad = config_of.copy()
    bad[len(bad) // 2] = len(CONFIGS)
    d_bad = torch.from_numpy(bad.view(np.int32)).to(dev)
    with pytest.raises(_lib.SuggestHipError) as e:
        call(d_bad)
    assert e.value.code == -1 and "outside the table" in str(e.value)
    pi, ps, pc = w.gpu.suggest_batch(queries, "jaccard", 0.5, 10)
    oi, os_, oc = w.ora.suggest_batch(qb, qo, "jaccard", 0.5, 10)[:3]
    assert np.array_equal(pc, oc) and np.array_equal(pi, oi) and np.array_equal(ps.view(np.uint64), os_.view(np.uint64))
    again = call(d_cfg)
    for a, b in zip(again, host):
        assert np.array_equal(a.view(np.uint8), b.view(np.uint8))


def test_service_suggest_many(cars):
    from suggest_amd import SearchConfig, Service
    w = cars
    svc = Service()
    svc._install("cars", w.gpu, w.docs)
    try:
        reqs = [SearchConfig(q.decode("utf-8", "ignore"), k, m, s) for q, (m, s, k) in
                zip(_pool(w, 40, 35), [("jaccard", 0.5, 5), ("cosine", 0.4, 10), ("dice", 0.3, 65), ("jaccard", 0.5, 5)] * 10)]
        many = svc.suggest_many("cars", reqs)
        assert len(many) == 40 and sum(len(r) for r in many if r) > 0
        for r, c in zip(many, reqs):
            assert r == svc.suggest_batch("cars", [c.query], c.top_k, c.metric, c.similarity)[0]
        assert svc.suggest_many("cars", []) == []
    finally:
        svc._indexes.clear()              # (the fixture closes the index)


def test_cpp_mirror_suggest_many():
    import os
    import subprocess
    from conftest import GOLDEN, ROOT
    binary = os.path.join(ROOT, "tests", "cpp", "_build", "suggest_many_test")
    if not os.path.exists(binary):
        subprocess.run(["make", "-C", os.path.join(ROOT, "tests", "cpp"), "-f", "mixed.mk", "_build/suggest_many_test"], check=True, capture_output=True)
    r = subprocess.run([binary, GOLDEN], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr


# ---- the coalescer ----

KEYS = [("jaccard", 0.5, 10), ("cosine", 0.4, 3), ("dice", 0.5, 65), ("jaccard", HALF_UP, 10), ("ac", 0, 5), ("ac", 300, 7)]


def _coalescer_stats(ix):
    from suggest_amd import _lib
    out = (C.c_uint64 * 4)()
    with ix._use() as h:
        _lib.check(_lib.lib().sg_debug_coalesce_stats(h, out))
    return [int(x) for x in out]


def _hold(ix, on):
    from suggest_amd import _lib
    with ix._use() as h:
        _lib.check(_lib.lib().sg_debug_coalesce_hold(h, 1 if on else 0))


@pytest.mark.parametrize("mixed", [True, False])
def test_coalescer_answers_several_keys_with_one_mixed_call(cars_lines, mixed):
    """96 single-query callers over 6 keys queue up behind the hold; released, the dispatcher answers them with ONE mixed batch of 6
    groups (switch on) or with 6 batches of one key each (switch off) — and every caller gets the plain batch call's row"""
    from suggest_amd import _lib
    from suggest_amd.metric import resolve
    w = World(cars_lines, CARS_DESC)
    try:
        ix = w.gpu
        L = _lib.lib()
        queries = _pool(w, 96, 36)
        ix.coalesce_mixed(mixed)
        before = _coalescer_stats(ix)
        assert before[0] == 0
        _hold(ix, True)
        results, errors = [None] * 96, []

        def caller(i):
            try:
                m, s, k = KEYS[i % 6]
                q = queries[i]
                ids, sc, cnt = np.zeros(k, np.uint32), np.zeros(k, np.float64), C.c_uint32()
                with ix._use() as h:
                    if m == "ac":
                        _lib.check(L.sg_autocomplete_one_from(h, q, len(q), int(s), k, ids.ctypes.data, C.addressof(cnt)))
                    else:
                        _lib.check(L.sg_suggest_one(h, q, len(q), resolve(m).code, float(s), k, ids.ctypes.data, sc.ctypes.data, C.addressof(cnt)))
                results[i] = (ids, sc, int(cnt.value))
            except Exception as e:      # noqa: BLE001
                errors.append((i, e))

        threads = [threading.Thread(target=caller, args=(i,)) for i in range(96)]
        try:
            for t in threads:
                t.start()
            deadline = time.monotonic() + 60
            while _coalescer_stats(ix)[0] < 96 and time.monotonic() < deadline:
                time.sleep(0.002)
            held = _coalescer_stats(ix)
        finally:
            _hold(ix, False)              # (release before the index goes, whatever happened)
            for t in threads:
                t.join()
        assert not errors, errors
        assert held[0] == 96 and held[1:] == before[1:], (before, held)        # nothing was taken while held
        after = _coalescer_stats(ix)
        assert after[0] == 0
        took = [a - b for a, b in zip(after[1:], before[1:])]
        assert took == ([1, 1, 6] if mixed else [6, 0, 6]), took
        for g, (m, s, k) in enumerate(KEYS):
            members = list(range(g, 96, 6))
            cfg = dict(autocomplete=1, k=k, first_doc=int(s)) if m == "ac" else dict(metric=m, similarity=s, k=k)
            (oi, os_, oc), (pi, ps, pc) = w.reference(cfg, [queries[i] for i in members])
            for r, i in enumerate(members):
                ids, sc, cnt = results[i]
                n = 0 if pc[r] >= SPECIAL else min(int(pc[r]), k)
                assert cnt == int(pc[r]) == int(oc[r]), (i, m, cnt, int(pc[r]))
                assert np.array_equal(ids[:n], pi[r, :n]) and np.array_equal(ids[:n], oi[r, :n]), (i, m)
                if m != "ac":
                    assert np.array_equal(sc[:n].view(np.uint64), ps[r, :n].view(np.uint64)), (i, m)
    finally:
        w.close()
