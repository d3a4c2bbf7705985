"""The edit-distance ranking of DESIGN.md §5d restated in numpy / Python: Go-`range` decoding, case folding through
tests/oracle.py: to_lower, both distances as plain loops and as a row-vectorised form for long strings, a memoised recursive
definition to hold them against, the distances of id rows and the stable re-rank.

Units are runes: an invalid byte is one U+FFFD of width 1; nothing is trimmed, wrapped or mapped through an alphabet.
levenshtein: unit insert, delete, substitute.  osa: the same plus the transposition of two adjacent runes at cost 1 (optimal
string alignment: no substring is edited twice, so ca -> abc is 3).  A slot that holds no entry — past the row's count, in a
flagged row, in no row — and an entry whose id is outside the dictionary have distance NONE."""
import functools
import sys

import numpy as np

import oracle

NONE = 0xFFFFFFFF
COUNT_FLAG_MIN = 0xFFFFFFF0
RUNE_ERROR = 0xFFFD
MODES = ("levenshtein", "osa")
VEC_FROM = 48          # distance(): strings from this many runes on take the row-vectorised form


def decode(b):
    """Go `for _, r := range s` over bytes -> list of runes"""
    b = bytes(b)
    out, i, n = [], 0, len(b)
    while i < n:
        c0 = b[i]
        if c0 < 0x80:
            out.append(c0); i += 1; continue
        if c0 < 0xC2 or c0 > 0xF4:
            out.append(RUNE_ERROR); i += 1; continue
        if c0 < 0xE0:
            if i + 1 < n and b[i + 1] & 0xC0 == 0x80:
                out.append(((c0 & 0x1F) << 6) | (b[i + 1] & 0x3F)); i += 2
            else:
                out.append(RUNE_ERROR); i += 1
            continue
        if c0 < 0xF0:
            lo, hi = (0xA0 if c0 == 0xE0 else 0x80), (0x9F if c0 == 0xED else 0xBF)
            if i + 2 < n and lo <= b[i + 1] <= hi and b[i + 2] & 0xC0 == 0x80:
                out.append(((c0 & 0x0F) << 12) | ((b[i + 1] & 0x3F) << 6) | (b[i + 2] & 0x3F)); i += 3
            else:
                out.append(RUNE_ERROR); i += 1
            continue
        lo, hi = (0x90 if c0 == 0xF0 else 0x80), (0x8F if c0 == 0xF4 else 0xBF)
        if i + 3 < n and lo <= b[i + 1] <= hi and b[i + 2] & 0xC0 == 0x80 and b[i + 3] & 0xC0 == 0x80:
            out.append(((c0 & 0x07) << 18) | ((b[i + 1] & 0x3F) << 12) | ((b[i + 2] & 0x3F) << 6) | (b[i + 3] & 0x3F)); i += 4
        else:
            out.append(RUNE_ERROR); i += 1
    return out


def _b(s):
    return s.encode("utf-8") if isinstance(s, str) else bytes(s)


@functools.lru_cache(maxsize=None)
def _runes(b, fold):
    # (to_lower decodes as Go does and writes an invalid byte as U+FFFD, which decodes to itself)
    return tuple(decode(oracle.to_lower(b)) if fold else decode(b))


def runes(s, fold=True):
    return _runes(_b(s), bool(fold))


def levenshtein(a, b):
    prev = list(range(len(a) + 1))
    for j in range(1, len(b) + 1):
        cur = [j] + [0] * len(a)
        for i in range(1, len(a) + 1):
            cur[i] = min(prev[i] + 1, cur[i - 1] + 1, prev[i - 1] + (a[i - 1] != b[j - 1]))
        prev = cur
    return prev[len(a)]


def osa(a, b):
    prev2, prev = None, list(range(len(a) + 1))
    for j in range(1, len(b) + 1):
        cur = [j] + [0] * len(a)
        for i in range(1, len(a) + 1):
            v = min(prev[i] + 1, cur[i - 1] + 1, prev[i - 1] + (a[i - 1] != b[j - 1]))
            if i > 1 and j > 1 and a[i - 1] == b[j - 2] and a[i - 2] == b[j - 1]:
                v = min(v, prev2[i - 2] + 1)
            cur[i] = v
        prev2, prev = prev, cur
    return prev[len(a)]


def distance_vec(a, b, mode="levenshtein"):
    """The same rows, one numpy row per rune of b: everything but the insert chain is elementwise on the previous rows; the
    chain cur[i] = min(t[i], cur[i - 1] + 1) is minimum.accumulate(t - arange) + arange."""
    a = np.asarray(a, dtype=np.int64)
    m = a.size
    ar = np.arange(m + 1, dtype=np.int64)
    prev2, prev = None, ar.copy()
    for j in range(1, len(b) + 1):
        t = np.empty(m + 1, dtype=np.int64)
        t[0] = j
        t[1:] = np.minimum(prev[1:] + 1, prev[:-1] + (a != b[j - 1]))
        if mode == "osa" and j > 1 and m > 1:
            tr = (a[1:] == b[j - 2]) & (a[:-1] == b[j - 1])
            t[2:] = np.where(tr, np.minimum(t[2:], prev2[:-2] + 1), t[2:])
        cur = np.minimum.accumulate(t - ar) + ar
        prev2, prev = prev, cur
    return int(prev[m])


def distance_recursive(a, b, mode="levenshtein"):
    """The definition: the cheapest edit of the prefixes (memoised; short strings only)"""
    a, b = tuple(a), tuple(b)
    sys.setrecursionlimit(max(sys.getrecursionlimit(), 10000))

    @functools.lru_cache(maxsize=None)
    def d(i, j):
        if i == 0 or j == 0:
            return i + j
        v = min(d(i - 1, j) + 1, d(i, j - 1) + 1, d(i - 1, j - 1) + (a[i - 1] != b[j - 1]))
        if mode == "osa" and i > 1 and j > 1 and a[i - 1] == b[j - 2] and a[i - 2] == b[j - 1]:
            v = min(v, d(i - 2, j - 2) + 1)
        return v
    return d(len(a), len(b))


def distance_runes(a, b, mode="levenshtein"):
    assert mode in MODES
    if max(len(a), len(b)) >= VEC_FROM:
        return distance_vec(a, b, mode)
    return osa(a, b) if mode == "osa" else levenshtein(a, b)


def distance(x, y, mode="levenshtein", fold=True):
    return distance_runes(runes(x, fold), runes(y, fold), mode)


def peq_hash(r):
    """the slot a rune hashes to in the short kernel's Peq table of 128 slots (edit_peq_hash)"""
    return ((r * 0x9E3779B1) & 0xFFFFFFFF) >> 25


def row_bounds(n_rows, row=0, row_offs=None):
    if row_offs is None:
        return [(i * row, row) for i in range(n_rows)]
    ro = [int(x) for x in row_offs]
    return [(ro[i], ro[i + 1] - ro[i]) for i in range(n_rows)]


def edit_rows(queries, ids, counts, lines, row=0, row_offs=None, mode="levenshtein", fold=True):
    """-> (dist[slots] u32, entries with an id outside the dictionary)"""
    flat = np.asarray(ids, dtype=np.uint32).reshape(-1)
    dist = np.full(flat.size, NONE, dtype=np.uint32)
    outside = 0
    memo = {}
    for i, (b, length) in enumerate(row_bounds(len(counts), row, row_offs)):
        c = int(counts[i])
        if c >= COUNT_FLAG_MIN:
            continue
        qa = runes(queries[i], fold)
        for p in range(min(c, length)):
            d = int(flat[b + p])
            if d >= len(lines):
                outside += 1
                continue
            key = (qa, d)
            if key not in memo:
                memo[key] = distance_runes(qa, runes(lines[d], fold), mode)
            dist[b + p] = memo[key]
    return dist, outside


def rerank(ids, scores, dist, counts, row=0, row_offs=None, max_distance=NONE, k_out=None):
    """The stable re-rank -> (ids, scores or None, dist, counts), copies, flat: a row's entries by (distance ascending, the order
    they had); those above max_distance removed; the count = the number kept, at most k_out; the row zeroed from the count on.
    Flagged rows and slots of no row stay as they are."""
    ids = np.array(ids, dtype=np.uint32).reshape(-1)
    dist = np.array(dist, dtype=np.uint32).reshape(-1)
    scores = None if scores is None else np.array(scores, dtype=np.float64).reshape(-1)
    counts = np.array(counts, dtype=np.uint32).reshape(-1)
    for i, (b, length) in enumerate(row_bounds(len(counts), row, row_offs)):
        c = int(counts[i])
        if c >= COUNT_FLAG_MIN:
            continue
        n = min(c, length)
        order = sorted(range(n), key=lambda p: int(dist[b + p]))            # (sorted is stable)
        keep = [p for p in order if int(dist[b + p]) <= max_distance]
        if k_out is not None:
            keep = keep[:k_out]
        for arr in (ids, dist) + (() if scores is None else (scores,)):
            new = np.zeros(length, dtype=arr.dtype)
            new[:len(keep)] = arr[[b + p for p in keep]] if keep else []
            arr[b:b + length] = new
        counts[i] = len(keep)
    return ids, scores, dist, counts
