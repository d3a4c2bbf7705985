"""The complete search by edit distance of DESIGN.md §5e restated in numpy: the two per-document arrays of sg_edit_index, the two
lower bounds they give, and a brute-force search — the distance from a query to EVERY string (tests/edit_ref.py's recurrences, one
numpy row per rune of the documents, vectorised over the documents), a sort by (distance, docID), the histogram.

Semantics are edit_ref's: runes, Go-`range` decoding, folding through oracle.to_lower, levenshtein and osa."""
import numpy as np

import edit_ref as ref

MAX_DISTANCE = 32
MAX_K = 1024
MAX_QUERY_RUNES = 64
TOO_LONG = 0xFFFFFFFD


def sig_bit(r):
    """the bit a rune sets in a signature: (rune * 0x9E3779B1) >> 26, a 32-bit product"""
    return ((r * 0x9E3779B1) & 0xFFFFFFFF) >> 26


def signature(rs):
    s = 0
    for r in rs:
        s |= 1 << sig_bit(r)
    return s


def arrays(lines, fold):
    """-> (runes u32 [n_docs], sig u64 [n_docs])"""
    rs = [ref.runes(l, fold) for l in lines]
    return np.array([len(r) for r in rs], dtype=np.uint32), np.array([signature(r) for r in rs], dtype=np.uint64)


def bounds(qa, da):
    """the two lower bounds on the distance between rune strings qa and da -> (by length, by signature)"""
    sq, sd = signature(qa), signature(da)
    return abs(len(qa) - len(da)), max(bin(sq & ~sd).count("1"), bin(sd & ~sq).count("1"))


def slice_of(doc, n_docs, n_slices):
    """the docID slice a document falls in when the scan is cut into n_slices (include/suggest_hip.h)"""
    return doc // -(-n_docs // n_slices)


class Docs:
    """a dictionary's rune strings as a padded matrix, longest first, for distances_to_all"""

    def __init__(self, lines, fold):
        rs = [ref.runes(l, fold) for l in lines]
        self.n = len(rs)
        self.lens = np.array([len(r) for r in rs], dtype=np.int64)
        self.order = np.argsort(-self.lens, kind="stable")
        width = int(self.lens.max()) if self.n else 0
        self.mat = np.full((self.n, max(width, 1)), -1, dtype=np.int32)
        for row, d in enumerate(self.order):
            self.mat[row, :len(rs[d])] = rs[d]
        self.sorted_lens = self.lens[self.order]


def distances_to_all(qa, docs, mode):
    """distance from the rune string qa to every document -> int64 [n_docs].  edit_ref.distance_vec with one more axis: the
    documents, sorted longest first so that column j runs over the prefix of documents that have a rune j."""
    a = np.asarray(qa, dtype=np.int32)
    m = a.size
    out = np.empty(docs.n, dtype=np.int64)
    if m == 0 or docs.n == 0:
        out[:] = docs.lens
        return out
    ar = np.arange(m + 1, dtype=np.int32)
    res = np.full(docs.n, m, dtype=np.int64)                 # (an empty document: m)
    prev2, prev = None, np.tile(ar, (docs.n, 1))
    for j in range(1, int(docs.sorted_lens[0]) + 1 if docs.n else 1):
        n_j = int(np.searchsorted(-docs.sorted_lens, -j, side="right"))      # documents of j runes at least
        prev = prev[:n_j]
        bj = docs.mat[:n_j, j - 1][:, None]
        t = np.empty((n_j, m + 1), dtype=np.int32)
        t[:, 0] = j
        t[:, 1:] = np.minimum(prev[:, 1:] + 1, prev[:, :-1] + (a[None, :] != bj))
        if mode == "osa" and j > 1 and m > 1:
            bp = docs.mat[:n_j, j - 2][:, None]
            tr = (a[None, 1:] == bp) & (a[None, :-1] == bj)
            t[:, 2:] = np.where(tr, np.minimum(t[:, 2:], prev2[:n_j, :-2] + 1), t[:, 2:])
        cur = np.minimum.accumulate(t - ar, axis=1) + ar
        ends = docs.sorted_lens[:n_j] == j
        res[:n_j][ends] = cur[ends, m]
        prev2, prev = prev, cur
    out[docs.order] = res
    return out


def distance_matrix(queries, lines, mode, fold):
    """-> int64 [n_q, n_docs]; a row of -1 for a query of more than 64 runes"""
    docs = Docs(lines, fold)
    out = np.full((len(queries), len(lines)), -1, dtype=np.int64)
    for i, q in enumerate(queries):
        qa = ref.runes(q, fold)
        if len(qa) <= MAX_QUERY_RUNES:
            out[i] = distances_to_all(qa, docs, mode)
    return out


def search(dm, k, max_distance):
    """the brute-force search over a distance matrix -> (ids [n_q, k], dist [n_q, k], counts [n_q], hist [n_q, max_distance + 1]),
    all u32: row i = the min(k, matches) nearest by (distance, docID), zeroed from the count on"""
    n_q = dm.shape[0]
    ids = np.zeros((n_q, k), dtype=np.uint32)
    dist = np.zeros((n_q, k), dtype=np.uint32)
    counts = np.zeros(n_q, dtype=np.uint32)
    hist = np.zeros((n_q, max_distance + 1), dtype=np.uint32)
    for i in range(n_q):
        row = dm[i]
        if row.size and row[0] < 0:
            counts[i] = TOO_LONG
            continue
        order = np.argsort(row, kind="stable")                 # (stable: docID ascending among equal distances)
        order = order[row[order] <= max_distance]
        hist[i] = np.bincount(row[order], minlength=max_distance + 1)[:max_distance + 1]
        n = min(k, order.size)
        ids[i, :n] = order[:n]
        dist[i, :n] = row[order[:n]]
        counts[i] = n
    return ids, dist, counts, hist
