"""The merge of per-shard top-k rows, restated in numpy: what sg_shard_merge_kernel (suggest_amd/csrc/shard_merge.inc) and
distributed.merge_topk compute, written entry by entry so that it shares no code with either.

Rules (include/suggest_hip.h, the sg_sharded section):
  c_s = counts[s][q] if it is below FLAG_MIN, else 0; clamped to k
  any count >= FLAG_MIN (an SG_COUNT_* flag): out_counts[q] = the largest such value, the row zeroed
  else out_counts[q] = min(k, sum c_s); the row = the first out_counts[q] entries of the union ordered by
  (score desc, doc_lo[s] + id asc), entries equal in both keys in source order (shard, then position); the rest zero
  autocomplete: no scores; the order is the shards' rows one after the other, cut at k
"""
import numpy as np

FLAG_MIN = 0xFFFFFFF0
FLAGS = (0xFFFFFFFF, 0xFFFFFFFE, 0xFFFFFFFD, 0xFFFFFFFC)       # SG_COUNT_REF_PANIC, _REF_DEADLOCK, _TOO_LONG, _LM_ERROR


def merge(ids, scores, counts, doc_lo, autocomplete=False):
    """ids [W, n, k] local docIDs, scores [W, n, k] f64 (ignored with autocomplete), counts [W, n], doc_lo [W]
    -> (ids [n, k] u32, scores [n, k] f64 or None, counts [n] u32)"""
    ids = np.asarray(ids)
    counts = np.asarray(counts, dtype=np.uint64)
    W, n, k = ids.shape
    gid = ids.astype(np.uint64) + np.asarray(doc_lo, dtype=np.uint64)[:, None, None]
    bits = None if autocomplete else np.ascontiguousarray(scores, dtype=np.float64).view(np.uint64)
    o_ids = np.zeros((n, k), dtype=np.uint32)
    o_bits = None if autocomplete else np.zeros((n, k), dtype=np.uint64)
    o_cnt = np.zeros(n, dtype=np.uint32)
    for q in range(n):
        col = counts[:, q]
        if (col >= FLAG_MIN).any():
            o_cnt[q] = int(col.max())
            continue
        c = np.minimum(col, k).astype(np.int64)
        s_of = np.repeat(np.arange(W), c)                           # source order: shard, then position
        p_of = np.concatenate([np.arange(x) for x in c]) if len(s_of) else np.zeros(0, dtype=np.int64)
        g = gid[s_of, q, p_of]
        if autocomplete:
            order = np.arange(len(s_of))
        else:
            sc = np.asarray(scores, dtype=np.float64)[s_of, q, p_of]
            order = np.lexsort((np.arange(len(s_of)), g, -sc))      # last key first: score desc, docID asc, source order
        order = order[:k]
        m = len(order)
        o_cnt[q] = m
        assert (g[order] < 2 ** 32).all()
        o_ids[q, :m] = g[order].astype(np.uint32)
        if not autocomplete:
            o_bits[q, :m] = bits[s_of[order], q, p_of[order]]
    return o_ids, (None if autocomplete else o_bits.view(np.float64)), o_cnt


SCORES = np.array([1.0, 0.75, 2.0 / 3.0, 0.5, 1.0 / 3.0])         # five values: ties are the rule


def make_case(W, n, k, seed, doc_lo=None, flags="none", dup_run=False, id_range=None):
    """Crafted shard rows: every row ordered by (score desc, id asc) as a shard leaves it, scores from SCORES, ids from a small
    range so that equal (score, dictionary docID) pairs across shards cannot occur (ranges are disjoint) but equal scores
    abound.  counts run over 0 .. k with 0 and k forced in; flags: "none", "one" (each flag value in one shard of some
    query), "all" (in every shard of some query).  dup_run: a run of equal (score, id) inside a shard's row.
    Entries past a row's count hold junk the merge must not read into its result."""
    rng = np.random.default_rng(seed)
    id_range = id_range or max(4 * k, 64)
    if doc_lo is None:
        doc_lo = np.arange(W, dtype=np.uint64) * np.uint64(id_range)
    ids = np.zeros((W, n, k), dtype=np.uint32)
    sc = np.zeros((W, n, k), dtype=np.float64)
    cnt = rng.integers(0, k + 1, size=(W, n)).astype(np.uint32)
    cnt[0, 0] = k
    cnt[W - 1, n - 1] = 0 if W * n > 1 else k
    if n > 2:
        cnt[:, 1] = k                                               # every shard full
        cnt[:, 2] = 0                                               # every shard empty
    for s in range(W):
        for q in range(n):
            i = np.sort(rng.choice(id_range, size=k, replace=False)) if id_range >= k else np.sort(rng.integers(0, id_range, size=k))
            v = SCORES[rng.integers(0, len(SCORES), size=k)]
            o = np.lexsort((i, -v))
            ids[s, q], sc[s, q] = i[o], v[o]
            c = int(cnt[s, q])
            ids[s, q, c:] = 0xDEADBEEF                              # junk behind the count
            sc[s, q, c:] = 7.0
    if dup_run and k >= 4:
        ids[0, 0, 1:4] = ids[0, 0, 1]                                # three entries equal in (score, id): a document that repeats a term
        sc[0, 0, 1:4] = sc[0, 0, 1]
        o = np.lexsort((ids[0, 0], -sc[0, 0]))
        ids[0, 0], sc[0, 0] = ids[0, 0][o], sc[0, 0][o]
    if flags != "none":
        for j, f in enumerate(FLAGS):
            q = (3 + j) % n
            if flags == "all":
                cnt[:, q] = f
            else:
                cnt[(j + 1) % W, q] = f
        if flags == "all" and n > 1:
            cnt[:, n - 1] = FLAGS[::-1][:W] if W <= len(FLAGS) else np.resize(np.array(FLAGS, dtype=np.uint32), W)   # different flags: the largest wins
    return ids, sc, cnt, np.asarray(doc_lo, dtype=np.uint64)


def has_equal_keys(ids, sc, cnt, doc_lo):
    """True if some query holds two valid entries equal in (score, dictionary docID)"""
    W, n, k = ids.shape
    for q in range(n):
        if (cnt[:, q] >= FLAG_MIN).any():
            continue
        seen = set()
        for s in range(W):
            for p in range(min(int(cnt[s, q]), k)):
                key = (float(sc[s, q, p]), int(ids[s, q, p]) + int(doc_lo[s]))
                if key in seen:
                    return True
                seen.add(key)
    return False
