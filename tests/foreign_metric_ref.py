"""nGramSuggester.Suggest (pkg/suggest/suggester.go:46-131) stated by brute force for ANY metric object — MinY / MaxY / Threshold /
Distance, nothing else — in numpy and plain Python: no library of the project's, no oracle.  For dictionaries whose documents and
queries repeat no term (a document's overlap is then |tokens(query) & tokens(document)|, and it has one entry).

The reference, literally:
  * bMin, bMax = MinY(alpha, |A|), MaxY(alpha, |A|); bMax = min(bMax, S - 1) (lines 54-59), S = the number of length segments;
  * span = bMax - bMin + 1 is a channel's capacity (line 62): negative, the reference panics (PANIC); zero, the producer blocks on
    the first send with no worker started (DEADLOCK).  Both are checked AFTER the clamp;
  * otherwise it sends i = |A|, |A| - 1, ... while i >= bMin and j = |A| + 1, |A| + 2, ... while j <= bMax (lines 113-121): the
    visited sizes are [bMin, |A|] and [|A| + 1, bMax] — [bMin, bMax] only where bMin <= |A| + 1 and bMax >= |A|; a size outside
    [0, S) has no index (indices.Get returns nil, line 82) and is skipped;
  * per size B: T = Threshold(alpha, |A|, B), skipped if T == 0 or T > B or T > |A| (line 76); every document of cardinality B
    with overlap >= T is collected with the score 1 - Distance(overlap, |A|, B) (scorer.go:29-31), a Python float: the double
    a table built from the same object holds;
  * top-k by (score descending, docID ascending) (collector.go:20-26).
The reference also raises the similarity it passes to Threshold as the top-k fills (lines 101-103).  That is an optimisation of
the five metrics of pkg/metric, whose result is the untightened one; this statement has none, and `tightened` below restates the
device's own rule (engine.hip, d_tighten) only so that a test can show what it does to a score that is not monotone."""
import numpy as np

PANIC, DEADLOCK, TOO_LONG = 0xFFFFFFFF, 0xFFFFFFFE, 0xFFFFFFFD


def visited_sizes(metric, alpha, size_a, n_segments, narrow=False):
    """-> PANIC, DEADLOCK or the ascending list of segment sizes the reference searches for a query of size_a tokens.
    narrow=True: [MinY, min(MaxY, S - 1)] instead — what the device took before it was given the reference's walk (a control)."""
    b_min, b_max = metric.MinY(alpha, size_a), metric.MaxY(alpha, size_a)
    if b_max >= n_segments:
        b_max = n_segments - 1
    span = b_max - b_min + 1
    if span < 0:
        return PANIC
    if span == 0:
        return DEADLOCK
    if narrow:
        return [b for b in range(b_min, b_max + 1) if 0 <= b < n_segments]
    sizes, i, j = [], size_a, size_a + 1
    while i >= b_min or j <= b_max:
        if i >= b_min:
            sizes.append(i)
        if j <= b_max:
            sizes.append(j)
        i, j = i - 1, j + 1
    return sorted(b for b in sizes if 0 <= b < n_segments)


def walk_order(metric, alpha, size_a, n_segments):
    """the visited sizes in the order the reference sends them (inside-out from |A|)"""
    b_min, b_max = metric.MinY(alpha, size_a), min(metric.MaxY(alpha, size_a), n_segments - 1)
    sizes, i, j = [], size_a, size_a + 1
    while i >= b_min or j <= b_max:
        if i >= b_min:
            sizes.append(i)
        if j <= b_max:
            sizes.append(j)
        i, j = i - 1, j + 1
    return [b for b in sizes if 0 <= b < n_segments]


class BruteForce:
    """doc_tokens / query_tokens: one collection of tokens per document / query (none repeats a token); n_segments: S."""

    def __init__(self, doc_tokens, query_tokens, n_segments):
        docs = [frozenset(t) for t in doc_tokens]
        assert all(len(d) == len(t) for d, t in zip(docs, doc_tokens)), "a document repeats a term"
        self.S = int(n_segments)
        self.card = np.array([len(d) for d in docs], dtype=np.int64)
        self.size_a = []
        self.overlap = np.zeros((len(query_tokens), len(docs)), dtype=np.int64)
        for qi, t in enumerate(query_tokens):
            q = frozenset(t)
            assert len(q) == len(t), "a query repeats a term"
            self.size_a.append(len(t))
            self.overlap[qi] = [len(q & d) for d in docs]
        self._cache = {}

    def candidates(self, metric, alpha, narrow=False):
        """per query: PANIC / DEADLOCK, or (ids, scores, segments, overlaps) of EVERY collected document, best first"""
        key = (id(metric), repr(alpha), narrow)
        if key in self._cache:
            return self._cache[key][1]
        rows = []
        for qi, size_a in enumerate(self.size_a):
            if size_a == 0:
                rows.append((np.zeros(0, np.int64), np.zeros(0), np.zeros(0, np.int64), np.zeros(0, np.int64)))
                continue
            sizes = visited_sizes(metric, alpha, size_a, self.S, narrow)
            if not isinstance(sizes, list):
                rows.append(sizes)
                continue
            thr = np.full(self.S + 1, 1 << 62, dtype=np.int64)                 # (no size searched: no overlap reaches it)
            for b in sizes:
                t = metric.Threshold(alpha, size_a, b)
                if not (t == 0 or t > b or t > size_a):
                    thr[b] = t
            card = np.minimum(self.card, self.S)
            ids = np.nonzero(self.overlap[qi] >= thr[card])[0]
            seg, ov = self.card[ids], self.overlap[qi][ids]
            score_of = {(b, o): 1 - metric.Distance(o, size_a, b) for b, o in set(zip(seg.tolist(), ov.tolist()))}
            sc = np.array([score_of[b, o] for b, o in zip(seg.tolist(), ov.tolist())], dtype=np.float64)
            order = np.lexsort((ids, -sc))                                      # score descending, docID ascending
            rows.append((ids[order], sc[order], seg[order], ov[order]))
        self._cache[key] = (metric, rows)                                       # (the metric kept alive: its id is the key)
        return rows

    def suggest(self, metric, alpha, k, narrow=False):
        """-> (ids[n_q, k] u32, scores[n_q, k] f64, counts[n_q] u32) as the library's calls return them: row i best first, zeros
        past counts[i]; counts[i] = PANIC / DEADLOCK where the reference fails"""
        rows = self.candidates(metric, alpha, narrow)
        ids = np.zeros((len(rows), k), dtype=np.uint32)
        sc = np.zeros((len(rows), k), dtype=np.float64)
        cnt = np.zeros(len(rows), dtype=np.uint32)
        for qi, r in enumerate(rows):
            if not isinstance(r, tuple):
                cnt[qi] = r
                continue
            n = min(k, len(r[0]))
            ids[qi, :n], sc[qi, :n], cnt[qi] = r[0][:n], r[1][:n], n
        return ids, sc, cnt

    def tightened(self, metric, alpha, k, assume_monotone=False):
        """The same top-k with the thresholds raised as the device raises them, segments in the reference's order: once k documents
        are held, a segment's threshold goes up from T while 1 - Distance(t, |A|, B) is below the k-th best score (d_tighten).
        Every overlap that walk passes is one whose score cannot enter, so the rows are `suggest`'s for ANY score table.
        assume_monotone=True: what a shortcut that trusts the score to grow with the overlap would do instead — skip a segment
        whose highest possible overlap scores below the k-th best.  -> (ids, scores, counts)"""
        ids = np.zeros((len(self.size_a), k), dtype=np.uint32)
        sc = np.zeros((len(self.size_a), k), dtype=np.float64)
        cnt = np.zeros(len(self.size_a), dtype=np.uint32)
        for qi, size_a in enumerate(self.size_a):
            sizes = visited_sizes(metric, alpha, size_a, self.S) if size_a else []
            if not isinstance(sizes, list):
                cnt[qi] = sizes
                continue
            top = []                                                            # (-score, id), sorted
            for b in walk_order(metric, alpha, size_a, self.S) if size_a else []:
                t = metric.Threshold(alpha, size_a, b)
                if t == 0 or t > b or t > size_a:
                    continue
                o_max = min(size_a, b)
                if len(top) == k:
                    worst = -top[-1][0]
                    if assume_monotone:
                        if 1 - metric.Distance(o_max, size_a, b) < worst:
                            continue
                    else:
                        while t <= o_max and 1 - metric.Distance(t, size_a, b) < worst:
                            t += 1
                d = np.nonzero((self.card == b) & (self.overlap[qi] >= t))[0]
                top.extend((-(1 - metric.Distance(int(self.overlap[qi][x]), size_a, b)), int(x)) for x in d)
                top.sort()
                del top[k:]
            n = len(top)
            ids[qi, :n], sc[qi, :n], cnt[qi] = [x for _, x in top], [-s for s, _ in top], n
        return ids, sc, cnt


def differences(got, want, limit=5):
    """two sets of rows (ids, scores, counts) -> what differs, [] if nothing: the counts (flags among them) and, where the counts
    agree, ids and the BITS of the scores of every valid slot, in order"""
    g_ids, g_sc, g_cnt = (np.asarray(x) for x in got[:3])
    w_ids, w_sc, w_cnt = (np.asarray(x) for x in want[:3])
    bad = g_cnt != w_cnt
    out = [("count", int(q), int(g_cnt[q]), int(w_cnt[q])) for q in np.nonzero(bad)[0][:limit]]
    n = np.where((w_cnt >= TOO_LONG) | bad, 0, np.minimum(w_cnt, w_ids.shape[1]))
    valid = np.arange(w_ids.shape[1])[None, :] < n[:, None]
    differ = valid & ((g_ids != w_ids) | (g_sc.view(np.uint64) != w_sc.view(np.uint64)))
    for q in np.nonzero(differ.any(axis=1))[0][:limit]:
        j = int(np.nonzero(differ[q])[0][0])
        out.append(("row", int(q), j, g_ids[q, j:j + 3].tolist(), w_ids[q, j:j + 3].tolist(), g_sc[q, j:j + 3].tolist(), w_sc[q, j:j + 3].tolist()))
    return out
