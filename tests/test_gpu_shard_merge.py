"""A dictionary sharded by docID range behind one handle (sg_sharded, suggest_amd.ShardedIndex) on the GPU: the merge kernel
alone against tests/shard_ref.py, slices, the sharded search against the unsharded index, real data with repeated terms, corners."""
import numpy as np
import pytest

import oracle
import shard_ref
from conftest import CARS_DESC
from test_gpu_parity import assert_same

pytestmark = pytest.mark.gpu

PANIC, DEADLOCK = 0xFFFFFFFF, 0xFFFFFFFE


def _same_rows(got, want, what=""):
    """ids, score bits and counts, every slot (tails and flagged rows are zero on both sides)"""
    g_ids, g_sc, g_cnt = got
    w_ids, w_sc, w_cnt = want
    assert np.array_equal(g_cnt, w_cnt), (what, "counts", np.nonzero(g_cnt != w_cnt)[0][:5])
    bad = np.nonzero((g_ids != w_ids).any(axis=1))[0]
    assert bad.size == 0, (what, "ids", bad[:5], g_ids[bad[:2]], w_ids[bad[:2]])
    if w_sc is not None:
        bad = np.nonzero((g_sc.view(np.uint64) != w_sc.view(np.uint64)).any(axis=1))[0]
        assert bad.size == 0, (what, "scores", bad[:5], g_sc[bad[:2]], w_sc[bad[:2]])


# ---- 1. the kernel alone ---------------------------------------------------------------------------------------------
# Every W of {1, 2, 3, 64}, k of {1, 10, 64, 65, 1024, 5000} and n_q of {1, 63, 257} appears, each W with a k on either side of
# the kernel's paths (several queries per workgroup while W * k <= 128; one workgroup per query; several workgroups per query
# above 4 096 entries), sized so that no case moves more than a few MB.
KERNEL_CASES = [
    # W, n_q, k, flags
    (1, 1, 1, "none"), (1, 257, 1, "one"), (1, 63, 10, "all"), (1, 63, 64, "none"), (1, 257, 65, "one"), (1, 63, 1024, "none"), (1, 1, 5000, "none"),
    (2, 257, 1, "one"), (2, 63, 10, "one"), (2, 257, 64, "all"), (2, 63, 65, "none"), (2, 63, 1024, "one"), (2, 63, 5000, "one"),
    (3, 63, 1, "all"), (3, 257, 10, "one"), (3, 1, 64, "none"), (3, 63, 65, "one"), (3, 63, 1024, "all"), (3, 1, 5000, "none"),
    (64, 257, 1, "one"), (64, 63, 2, "all"), (64, 63, 10, "one"), (64, 1, 64, "none"), (64, 63, 65, "one"), (64, 1, 1024, "none"), (64, 1, 5000, "none"),
]


@pytest.mark.parametrize("W,n,k,flags", KERNEL_CASES)
def test_kernel_equals_shard_ref(W, n, k, flags):
    from suggest_amd.sharded import shard_merge
    ids, sc, cnt, doc_lo = shard_ref.make_case(W, n, k, seed=W * 100003 + n * 101 + k, flags=flags)
    _same_rows(shard_merge(ids, sc, cnt, doc_lo), shard_ref.merge(ids, sc, cnt, doc_lo), "fuzzy")
    _same_rows(shard_merge(ids, None, cnt, doc_lo, autocomplete=True), shard_ref.merge(ids, None, cnt, doc_lo, autocomplete=True), "autocomplete")


def test_kernel_keeps_a_run_of_equal_keys_in_source_order():
    from suggest_amd.sharded import shard_merge
    for W, n, k in ((2, 5, 10), (3, 3, 65), (3, 2, 2000)):
        ids, sc, cnt, doc_lo = shard_ref.make_case(W, n, k, seed=k, dup_run=True)
        assert shard_ref.has_equal_keys(ids, sc, cnt, doc_lo)
        _same_rows(shard_merge(ids, sc, cnt, doc_lo), shard_ref.merge(ids, sc, cnt, doc_lo), (W, n, k))


def test_kernel_returns_ids_above_2_31_as_u32():
    from suggest_amd.sharded import shard_merge
    for n, k, flags in ((63, 10, "one"), (5, 1024, "none")):      # (with "one" four queries are flagged: too few are left at n = 5)
        ids, sc, cnt, doc_lo = shard_ref.make_case(2, n, k, seed=9, doc_lo=[0, 3_000_000_000], flags=flags)
        got = shard_merge(ids, sc, cnt, doc_lo)
        _same_rows(got, shard_ref.merge(ids, sc, cnt, doc_lo))
        assert (got[0] >= 3_000_000_000).any() and got[0].dtype == np.uint32


# ---- 3. end to end against the unsharded index (and 2, slices, on the same dictionary) --------------------------------
@pytest.fixture(scope="module")
def uneven():
    """the dictionary of test_gpu_parity's doc-sharded test: the last third only has short documents, so the last shard has to
    be built again with the dictionary-wide number of segments"""
    from suggest_amd import IndexDescription, NGramIndex, synth
    desc = IndexDescription(**synth.DESCRIPTION)
    blob, offs = synth.make_dict(90000, seed=71, families=3)
    docs = synth.unpack(blob, offs)
    docs[60000:] = [d[:10] for d in docs[60000:]]
    blob, offs = oracle.pack_strings(docs)
    qb, qo = synth.make_queries(512, blob, offs, seed=72)
    full = NGramIndex(blob=blob, offs=offs, description=desc)
    st = full.stats()
    assert st["n_postings_raw"] == st["n_postings"]        # no document repeats a term: the condition under which equality is promised
    want = {(m, a, k): full.suggest_batch(blob=qb, offs=qo, metric=m, similarity=a, k=k) for m, a, k in (("cosine", 0.4, 10), ("jaccard", 0.5, 65))}
    want_ac = full.autocomplete_batch(blob=qb, offs=qo, limit=10)
    return dict(desc=desc, blob=blob, offs=offs, qb=qb, qo=qo, full=full, want=want, want_ac=want_ac, n_docs=len(docs))


def _device_call(sh, qb, qo, metric, similarity, k):
    import torch
    d_q = torch.from_numpy(qb).cuda()
    d_o = torch.from_numpy(qo.view(np.int64)).cuda()
    n_q = len(qo) - 1
    d_ids = torch.full((n_q, k), 0x5A5A5A5A, dtype=torch.int32, device="cuda")          # the call writes every slot itself
    d_sc = torch.full((n_q, k), 7.0, dtype=torch.float64, device="cuda")
    d_cnt = torch.full((n_q,), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
    st = torch.cuda.current_stream()
    sh.suggest_batch_device(d_q.data_ptr(), d_o.data_ptr(), n_q, metric, similarity, k, d_ids.data_ptr(), d_sc.data_ptr(), d_cnt.data_ptr(), st.cuda_stream)
    st.synchronize()
    return d_ids.cpu().numpy().view(np.uint32), d_sc.cpu().numpy(), d_cnt.cpu().numpy().view(np.uint32)


@pytest.mark.parametrize("W,build", [(3, "host"), (4, "device")])
def test_sharded_index_equals_the_unsharded(uneven, W, build):
    from suggest_amd import ShardedIndex
    from suggest_amd.distributed import shard_bounds
    u = uneven
    sh = ShardedIndex(blob=u["blob"], offs=u["offs"], description=u["desc"], n_shards=W, devices=(0,), build=build)
    assert sh.shards() == [(shard_bounds(u["n_docs"], W, s)[0], 0) for s in range(W)]
    for (m, a, k), want in u["want"].items():
        got = sh.suggest_batch(blob=u["qb"], offs=u["qo"], metric=m, similarity=a, k=k)
        assert_same(got, want)
        dev = _device_call(sh, u["qb"], u["qo"], m, a, k)
        assert_same(dev, want)
        _same_rows(dev, got, "device-resident against host-buffer")
        if m == "cosine":
            assert (got[2] > 1).mean() > 0.3          # (as the existing doc-sharded test: most rows really are merged from several entries)
    ids, cnt = sh.autocomplete_batch(blob=u["qb"], offs=u["qo"], limit=10)
    w_ids, w_cnt = u["want_ac"]
    assert np.array_equal(cnt, w_cnt)
    valid = np.arange(10)[None, :] < np.minimum(cnt, 10)[:, None]
    assert np.array_equal(ids[valid], w_ids[valid]) and not ids[~valid].any()
    sh.close()


def test_slices_give_the_unsliced_rows(uneven):
    """257 queries in slices of 128, 128 and 1: the budget holds 128 queries' rows of every shard.  Three shards in one lane;
    four in two lanes, where a lane's copy of slice i + 1 into the merge's block has to wait for the merge of slice i"""
    from suggest_amd import ShardedIndex, _lib
    u = uneven
    qo = u["qo"][:258]
    qb = u["qb"][:int(qo[-1])]
    k = 10
    for W, devices in ((3, (0,)), (4, (0, 0))):
        sh = ShardedIndex(blob=u["blob"], offs=u["offs"], description=u["desc"], n_shards=W, devices=devices)
        whole = sh.suggest_batch(blob=qb, offs=qo, metric="cosine", similarity=0.4, k=k)
        whole_ac = sh.autocomplete_batch(blob=qb, offs=qo, limit=k)
        try:
            _lib.check(_lib.lib().sg_debug_shard_slice_bytes(128 * W * (k * 12 + 4)))
            sliced = sh.suggest_batch(blob=qb, offs=qo, metric="cosine", similarity=0.4, k=k)
            sliced_dev = _device_call(sh, qb, qo, "cosine", 0.4, k)
            _lib.check(_lib.lib().sg_debug_shard_slice_bytes(128 * W * (k * 4 + 4)))
            sliced_ac = sh.autocomplete_batch(blob=qb, offs=qo, limit=k)
        finally:
            _lib.check(_lib.lib().sg_debug_shard_slice_bytes(0))
        _same_rows(sliced, whole, (W, "host-buffer"))
        _same_rows(sliced_dev, whole, (W, "device-resident"))
        assert np.array_equal(sliced_ac[0], whole_ac[0]) and np.array_equal(sliced_ac[1], whole_ac[1]), W
        assert_same(whole, tuple(x[:257] for x in u["want"][("cosine", 0.4, 10)]))
        assert np.array_equal(whole_ac[1], u["want_ac"][1][:257]), W
        sh.close()


def test_devices_0_0_takes_the_path_for_rows_from_another_device(uneven):
    from suggest_amd import ShardedIndex
    u = uneven
    sh = ShardedIndex(blob=u["blob"], offs=u["offs"], description=u["desc"], n_shards=4, devices=(0, 0))
    assert [d for _, d in sh.shards()] == [0, 0, 0, 0]
    for (m, a, k), want in u["want"].items():
        assert_same(sh.suggest_batch(blob=u["qb"], offs=u["qo"], metric=m, similarity=a, k=k), want)
    ids, cnt = sh.autocomplete_batch(blob=u["qb"], offs=u["qo"], limit=10)
    assert np.array_equal(cnt, u["want_ac"][1])
    valid = np.arange(10)[None, :] < np.minimum(cnt, 10)[:, None]
    assert np.array_equal(ids[valid], u["want_ac"][0][valid])
    sh.close()


def _handles(u):
    """one lane and two lanes over the same dictionary"""
    from suggest_amd import ShardedIndex
    return [ShardedIndex(blob=u["blob"], offs=u["offs"], description=u["desc"], n_shards=W, devices=d) for W, d in ((3, (0,)), (4, (0, 0)))]


def test_offsets_that_do_not_start_at_zero(uneven):
    """queries 100 .. 229 as a slice of the whole blob: the offsets are rebased in staging"""
    u = uneven
    offs = u["qo"][100:231]
    assert offs[0] > 0
    for sh in _handles(u):
        for (m, a, k), want in u["want"].items():
            whole = sh.suggest_batch(blob=u["qb"], offs=u["qo"], metric=m, similarity=a, k=k)
            _same_rows(sh.suggest_batch(blob=u["qb"], offs=offs, metric=m, similarity=a, k=k), tuple(x[100:230] for x in whole), (m, a, k))
        whole = sh.autocomplete_batch(blob=u["qb"], offs=u["qo"], limit=10)
        ids, cnt = sh.autocomplete_batch(blob=u["qb"], offs=offs, limit=10)
        assert np.array_equal(ids, whole[0][100:230]) and np.array_equal(cnt, whole[1][100:230])
        sh.close()


def test_threads_on_one_handle(uneven):
    """two threads on a handle with two lanes, which share the lanes' streams and rows and nothing else; a thread on a handle
    with one lane next to a device-resident call on it, which share nothing"""
    import threading
    u = uneven
    one, two = _handles(u)
    got, errors = {}, []

    def host_calls(sh, name):
        try:
            got[name] = [(key, sh.suggest_batch(blob=u["qb"], offs=u["qo"], metric=key[0], similarity=key[1], k=key[2]))
                         for _ in range(2) for key in u["want"]]
        except Exception as e:      # (a thread's exception is the test's)
            errors.append((name, e))

    threads = [threading.Thread(target=host_calls, args=(two, i)) for i in range(2)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    t = threading.Thread(target=host_calls, args=(one, "one lane"))
    t.start()
    dev = [(key, _device_call(one, u["qb"], u["qo"], *key)) for _ in range(2) for key in u["want"]]
    t.join()
    assert not errors, errors
    assert sorted(got, key=str) == [0, 1, "one lane"] and all(len(v) == 4 for v in got.values())
    for name, rows in list(got.items()) + [("device-resident", dev)]:
        for key, r in rows:
            assert_same(r, u["want"][key], (name, key))
    one.close()
    two.close()


def test_poisoned_scratch_leaves_the_rows_as_they_are(uneven):
    """the merge kernel writes every slot of every row, so a host-buffer call does not clear them first: with the scratch and
    the shards' rows poisoned the merged rows are the same, zero past each count"""
    from suggest_amd import _lib
    u = uneven
    for sh in _handles(u):
        for (m, a, k), want in u["want"].items():
            plain = sh.suggest_batch(blob=u["qb"], offs=u["qo"], metric=m, similarity=a, k=k)
            for family in (1, 2):
                with _lib.poisoned(family):
                    ids, sc, cnt = sh.suggest_batch(blob=u["qb"], offs=u["qo"], metric=m, similarity=a, k=k)
                _same_rows((ids, sc, cnt), plain, (m, a, k, family))
                past = np.arange(k)[None, :] >= np.minimum(cnt, k)[:, None]
                assert past.any() and not ids[past].any() and not sc.view(np.uint64)[past].any()
        plain = sh.autocomplete_batch(blob=u["qb"], offs=u["qo"], limit=10)
        for family in (1, 2):
            with _lib.poisoned(family):
                ids, cnt = sh.autocomplete_batch(blob=u["qb"], offs=u["qo"], limit=10)
            assert np.array_equal(ids, plain[0]) and np.array_equal(cnt, plain[1])
            assert not ids[np.arange(10)[None, :] >= np.minimum(cnt, 10)[:, None]].any()
        sh.close()


def test_merged_rows_above_64_mib_are_copied_straight_out(uneven):
    """6 000 queries at k = 1 000: 72 MB of merged rows, past what a host-buffer call stages, from a [shard][query][k] block of
    216 MB — one slice.  Cosine >= 0.1: the threshold at which this dictionary gives rows of more than 64 entries (up to 177)"""
    from suggest_amd import ShardedIndex
    u = uneven
    n, k = 6000, 1000
    reps = -(-n // 512)
    lens = np.tile(np.diff(u["qo"].astype(np.int64)), reps)[:n]
    qo = np.concatenate([[0], np.cumsum(lens)]).astype(np.uint64)
    qb = np.tile(u["qb"][:int(u["qo"][-1])], reps)[:int(qo[-1])]
    assert n * (12 * k + 4) > 64 << 20 and 3 * n * (12 * k + 4) <= 256 << 20
    want = u["full"].suggest_batch(blob=qb, offs=qo, metric="cosine", similarity=0.1, k=k)
    assert (want[2][want[2] < shard_ref.FLAG_MIN] > 64).any()        # rows that long come from the top-k kept in HBM
    sh = ShardedIndex(blob=u["blob"], offs=u["offs"], description=u["desc"], n_shards=3)
    got = sh.suggest_batch(blob=qb, offs=qo, metric="cosine", similarity=0.1, k=k)
    assert_same(got, want)
    assert not got[0][np.arange(k)[None, :] >= np.minimum(got[2], k)[:, None]].any()
    sh.close()


# ---- 4. real data with repeated terms -------------------------------------------------------------------------------
def test_cars_sharded_rows_are_the_merge_of_the_shards_own_rows(cars_lines):
    from suggest_amd import IndexDescription, NGramIndex, ShardedIndex
    from suggest_amd.distributed import shard_bounds
    desc = IndexDescription(**CARS_DESC)
    blob, offs = oracle.pack_strings(cars_lines)
    full = NGramIndex(blob=blob, offs=offs, description=desc, upload=False)
    st = full.stats()
    assert st["n_postings_raw"] > st["n_postings"]          # documents that repeat a term
    S = st["n_segments"]
    queries = [l[:max(3, len(l) - 2)] for l in cars_lines[::7]] + [b"toyota corolla", b"bmw", b"mercedes-benz c"]
    qb, qo = oracle.pack_strings(queries)
    W = 3
    sh = ShardedIndex(blob=blob, offs=offs, description=desc, n_shards=W)
    shards, los = [], []
    for s in range(W):
        lo, hi = shard_bounds(len(cars_lines), W, s)
        shards.append(NGramIndex(blob=blob[int(offs[lo]):int(offs[hi])], offs=(offs[lo:hi + 1] - offs[lo]).astype(np.uint64), description=desc, min_segments=S))
        los.append(lo)
    for metric, a, k in (("cosine", 0.4, 10), ("jaccard", 0.3, 65)):
        rows = [x.suggest_batch(blob=qb, offs=qo, metric=metric, similarity=a, k=k) for x in shards]
        want = shard_ref.merge(np.stack([r[0] for r in rows]), np.stack([r[1] for r in rows]), np.stack([r[2] for r in rows]), los)
        _same_rows(sh.suggest_batch(blob=qb, offs=qo, metric=metric, similarity=a, k=k), want, (metric, a, k))
        answered = want[2] < shard_ref.FLAG_MIN
        assert answered.any() and int(want[2][answered].sum()) > int(answered.sum())
    adopted = ShardedIndex.adopt(shards, los)                # the same shards behind an adopted handle
    rows = [x.autocomplete_batch(blob=qb, offs=qo, limit=10) for x in shards]
    want = shard_ref.merge(np.stack([r[0] for r in rows]), None, np.stack([r[1] for r in rows]), los, autocomplete=True)
    for handle in (sh, adopted):
        ids, cnt = handle.autocomplete_batch(blob=qb, offs=qo, limit=10)
        _same_rows((ids, None, cnt), want, "autocomplete")


# ---- 5. corners -----------------------------------------------------------------------------------------------------
def test_empty_shards_add_nothing():
    from suggest_amd import IndexDescription, NGramIndex, ShardedIndex, synth
    desc = IndexDescription(**synth.DESCRIPTION)
    docs = [b"alpha beta", b"alpha gamma", b"delta"]
    full = NGramIndex(docs, desc)
    sh = ShardedIndex(docs, description=desc, n_shards=5)
    assert sh.shards() == [(0, 0), (1, 0), (2, 0)]
    queries = [b"alpha", b"alpha bet", b"delta", b"zzz"]
    assert_same(sh.suggest_batch(queries, metric="jaccard", similarity=0.3, k=5), full.suggest_batch(queries, metric="jaccard", similarity=0.3, k=5))
    ids, cnt = sh.autocomplete_batch(queries, limit=5)
    w_ids, w_cnt = full.autocomplete_batch(queries, limit=5)
    assert np.array_equal(cnt, w_cnt) and np.array_equal(ids, w_ids)


def test_a_query_with_an_empty_window_stays_flagged(uneven):
    """a window [MinY, MaxY] that the clipping leaves empty: the reference panics or dead-locks (suggester.go:62); every shard
    was built with the dictionary-wide number of segments, so every shard says what the unsharded index says"""
    from suggest_amd import ShardedIndex
    u = uneven
    import random
    rng = random.Random(11)      # strings of 5 .. 160 distinct-ish runes: MinY walks past the last segment one step at a time
    queries = [bytes(rng.choice(b"abcdefghijklmnopqrstuvwxyz0123456789") for _ in range(n)) for n in range(5, 161)] + [b"ab", synth_doc(u, 5)]
    want = u["full"].suggest_batch(queries, metric="jaccard", similarity=0.9, k=10)
    assert {PANIC, DEADLOCK} <= set(want[2].tolist()), sorted(set(want[2].tolist()))[-4:]
    assert (want[2] < shard_ref.FLAG_MIN).any()
    sh = ShardedIndex(blob=u["blob"], offs=u["offs"], description=u["desc"], n_shards=3)
    got = sh.suggest_batch(queries, metric="jaccard", similarity=0.9, k=10)
    assert np.array_equal(got[2], want[2])
    assert_same(got, want)
    flagged = got[2] >= shard_ref.FLAG_MIN
    assert not got[0][flagged].any() and not got[1][flagged].view(np.uint64).any()
    sh.close()


def synth_doc(u, i):
    return bytes(u["blob"][int(u["offs"][i]):int(u["offs"][i + 1])])


def test_adopted_shards_return_ids_above_2_31():
    import random
    from suggest_amd import IndexDescription, NGramIndex, ShardedIndex, _lib, synth
    rng = random.Random(3)
    desc = IndexDescription(**synth.DESCRIPTION)
    docs = ["".join(rng.choice("abcdefgh") for _ in range(12)) for _ in range(200)]
    a, b = NGramIndex(docs[:100], desc), NGramIndex(docs[100:], desc)
    S = max(a.stats()["n_segments"], b.stats()["n_segments"])
    if a.stats()["n_segments"] != b.stats()["n_segments"]:
        with pytest.raises(_lib.SuggestHipError) as e:        # adoption refuses shards that would clip the window differently
            ShardedIndex.adopt([a, b], [0, 4_000_000_000])
        assert e.value.code == -1
        a, b = NGramIndex(docs[:100], desc, min_segments=S), NGramIndex(docs[100:], desc, min_segments=S)
    sh = ShardedIndex.adopt([a, b], [0, 4_000_000_000])
    assert sh.shards() == [(0, 0), (4_000_000_000, 0)]
    queries = [d[:-1] + "x" for d in docs[95:105]]
    ids, sc, cnt = sh.suggest_batch(queries, metric="cosine", similarity=0.5, k=4)
    ra, rb = (x.suggest_batch(queries, metric="cosine", similarity=0.5, k=4) for x in (a, b))
    _same_rows((ids, sc, cnt), shard_ref.merge(np.stack([ra[0], rb[0]]), np.stack([ra[1], rb[1]]), np.stack([ra[2], rb[2]]), [0, 4_000_000_000]))
    for q in range(5, 10):                                      # documents 100 .. 104 live in the second shard
        assert cnt[q] >= 1 and ids[q, 0] == 4_000_000_000 + q - 5, (q, ids[q], cnt[q])
    for q in range(5):
        assert cnt[q] >= 1 and ids[q, 0] == 95 + q
    with pytest.raises(_lib.SuggestHipError) as e:              # an overlap, refused
        ShardedIndex.adopt([a, b], [0, 50])
    assert e.value.code == -1
    with pytest.raises(_lib.SuggestHipError) as e:              # a shard that is not uploaded
        ShardedIndex.adopt([a, NGramIndex(docs[100:], desc, min_segments=S, upload=False)], [0, 100])
    assert e.value.code == -1 and "not uploaded" in str(e.value)
    with pytest.raises(_lib.SuggestHipError) as e:              # descriptions that differ
        ShardedIndex.adopt([a, NGramIndex(docs[100:], IndexDescription(**dict(synth.DESCRIPTION, ngram_size=2)), min_segments=S)], [0, 100])
    assert e.value.code == -1


def test_device_call_needs_every_shard_on_the_buffers_device():
    """One GPU visible: the check is exercised by its arguments alone — buffers that are not device memory of the shards' GPU;
    with a second GPU, buffers that live there"""
    import torch
    from suggest_amd import IndexDescription, NGramIndex, ShardedIndex, _lib, synth
    sh = ShardedIndex([b"alpha", b"beta", b"gamma", b"delta"], description=IndexDescription(**synth.DESCRIPTION), n_shards=2)
    UNSUPPORTED, INVALID = -2, -1
    qb, qo = oracle.pack_strings([b"alpha"])
    ids = np.zeros((1, 3), dtype=np.uint32); sc = np.zeros((1, 3), dtype=np.float64); cnt = np.zeros(1, dtype=np.uint32)
    with pytest.raises(_lib.SuggestHipError) as e:              # host memory: no device owns it
        sh.suggest_batch_device(qb.ctypes.data, qo.ctypes.data, 1, "jaccard", 0.5, 3, ids.ctypes.data, sc.ctypes.data, cnt.ctypes.data)
    assert e.value.code == UNSUPPORTED
    with pytest.raises(_lib.SuggestHipError) as e:
        sh.suggest_batch_device(qb.ctypes.data, None, 1, "jaccard", 0.5, 3, ids.ctypes.data, sc.ctypes.data, cnt.ctypes.data)
    assert e.value.code == INVALID
    with pytest.raises(_lib.SuggestHipError) as e:
        sh.suggest_batch_device(qb.ctypes.data, qo.ctypes.data, 1, "jaccard", 0.5, 0, ids.ctypes.data, sc.ctypes.data, cnt.ctypes.data)
    assert e.value.code == INVALID                              # k == 0
    if torch.cuda.device_count() >= 2:
        d = torch.device("cuda", 1)
        d_q, d_o = torch.from_numpy(qb).to(d), torch.from_numpy(qo.view(np.int64)).to(d)
        d_ids, d_sc, d_cnt = torch.zeros((1, 3), dtype=torch.int32, device=d), torch.zeros((1, 3), dtype=torch.float64, device=d), torch.zeros(1, dtype=torch.int32, device=d)
        with pytest.raises(_lib.SuggestHipError) as e:
            sh.suggest_batch_device(d_q.data_ptr(), d_o.data_ptr(), 1, "jaccard", 0.5, 3, d_ids.data_ptr(), d_sc.data_ptr(), d_cnt.data_ptr())
        assert e.value.code == UNSUPPORTED
        two = ShardedIndex([b"alpha", b"beta", b"gamma", b"delta"], description=IndexDescription(**synth.DESCRIPTION), n_shards=2, devices=(0, 1))
        assert [dv for _, dv in two.shards()] == [0, 1]
        d0 = torch.device("cuda", 0)
        t = [torch.from_numpy(qb).to(d0), torch.from_numpy(qo.view(np.int64)).to(d0), torch.zeros((1, 3), dtype=torch.int32, device=d0),
             torch.zeros((1, 3), dtype=torch.float64, device=d0), torch.zeros(1, dtype=torch.int32, device=d0)]
        with pytest.raises(_lib.SuggestHipError) as e:          # shard 1 is not on device 0
            two.suggest_batch_device(t[0].data_ptr(), t[1].data_ptr(), 1, "jaccard", 0.5, 3, t[2].data_ptr(), t[3].data_ptr(), t[4].data_ptr())
        assert e.value.code == UNSUPPORTED
        assert_same(two.suggest_batch([b"alpha", b"gamm"], metric="jaccard", similarity=0.3, k=3), sh.suggest_batch([b"alpha", b"gamm"], metric="jaccard", similarity=0.3, k=3))
        full = NGramIndex([b"alpha", b"beta", b"gamma", b"delta"], IndexDescription(**synth.DESCRIPTION))
        assert_same(two.suggest_batch([b"alpha", b"gamm", b"delt"], metric="jaccard", similarity=0.3, k=3),
                    full.suggest_batch([b"alpha", b"gamm", b"delt"], metric="jaccard", similarity=0.3, k=3))      # against the unsharded index
