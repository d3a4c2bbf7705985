"""Metrics that behave differently from the five of pkg/metric, and the dictionaries they are searched on.  Every
class is a plain object with the four methods of metric.Metric and no `code`: it reaches the engine tabulated (SG_TABLE).

  1 Tversky   asymmetric in |A| and |B| (0.75 / 0.25).
  2 Wobbly    a threshold that is NOT monotone in the segment: ceil(alpha min(a, b)) + (b % 3 == 0) — from b >= a on every third
              segment asks one more than its right-hand neighbour, so a group of the plan launch whose first segment is such a
              one has its lowest threshold further in (pipeline.inc takes wave_min over the group for SG_TABLE only).  Its score
              FALLS with the overlap (1 - o / min(a, b)), so the best rows are the documents that just reach their segment's
              threshold — the ones a threshold taken from the wrong segment loses.  The window is |A| -+ 12: 25 segments, which
              the plan launch takes for |A| <= 49 (|A| x 26 table words of 1 280); MinY is negative below 12.
  3 Above     a window above |A|: MinY = a + 2, MaxY = 2 a + 3.  The reference walks j = a + 1, a + 2, ... <= bMax, so it ALSO
              searches a + 1, where the threshold is admissible and the best scores (o / b) lie.
  4 Below     a window below |A|: MinY = ceil(a / 2), MaxY = a - 2.  The reference walks i = a, a - 1, ... >= bMin: it also
              searches a - 1 and a — the query's own text among them.
  5 Edges     MinY negative for a < 5; MaxY = 2^40 at every a = 3 mod 5 (the bindings clamp it to 32 bits); span 0 at every a divisible by 7 and span -1 at every a divisible by 11, measured against
              the CLAMPED bMax = min(MaxY, S - 1) as the reference measures them; thresholds of 0, above |A| and above |B| in
              mid-window ((a + b) % 5 == 0 / == 1).
  6 Coarse    scores outside [0, 1] and heavy ties: 3 floor(8 o / a) / 8 - 1 - a % 4 - (b % 2) / 16, steps of 0.375 within [-1, 2] down
              to [-4, -1] by the query's size: negative doubles in score_bits — the best rows of three queries in four are negative
              — and whole segments of equal scores that the docID must order.
  7 Peak      a score that is not monotone in the overlap: 1 - |o - 0.7 a| / a.  d_tighten walks up from the threshold only
              past overlaps whose own score is below the k-th best, so the rows are the untightened ones under every SG_TIGHTEN;
              a shortcut that judged a segment by its highest overlap would lose rows (`not_monotone` counts them).
A Distance that divides by zero (NaN scores) is out of scope: none of these does inside a searched cell."""
import math

import numpy as np

import foreign_metric_ref as ref
from test_gpu_metric_ladder import DEFAULTS, DESC, DOCS, LAUNCHES, QUERIES, SYMBOLS, _compact  # noqa: F401  (the ladder: reused, not copied)

S_LADDER = 65                                # cardinalities 1 .. 64: segments 0 .. 64
SIMILARITIES = (0.15, 0.5, 0.85)             # low (result sets of hundreds), middle, high
KS = (10, 65, len(DOCS))


class Tversky:
    def MinY(self, alpha, size): return int(math.ceil(alpha * size * 0.75))
    def MaxY(self, alpha, size): return int(math.floor(size / alpha * 1.25))
    def Threshold(self, alpha, a, b): return int(math.ceil(alpha * (0.75 * a + 0.25 * b)))
    def Distance(self, inter, a, b): return 1 - inter / (0.75 * a + 0.25 * b)

    @staticmethod
    def np_threshold(alpha, a, b): return np.ceil(alpha * (0.75 * a + 0.25 * b))
    @staticmethod
    def np_distance(o, a, b): return 1 - o / (0.75 * a + 0.25 * b)


class Wobbly:
    def MinY(self, alpha, size): return size - 12
    def MaxY(self, alpha, size): return size + 12
    def Threshold(self, alpha, a, b): return int(math.ceil(alpha * min(a, b))) + (1 if b % 3 == 0 else 0)
    def Distance(self, inter, a, b): return inter / min(a, b)

    @staticmethod
    def np_threshold(alpha, a, b): return np.ceil(alpha * np.minimum(a, b)) + (b % 3 == 0)
    @staticmethod
    def np_distance(o, a, b): return o / np.minimum(a, b)


class Above:
    def MinY(self, alpha, size): return size + 2
    def MaxY(self, alpha, size): return 2 * size + 3
    def Threshold(self, alpha, a, b): return int(math.ceil(alpha * min(a, b)))
    def Distance(self, inter, a, b): return 1 - inter / b

    @staticmethod
    def np_threshold(alpha, a, b): return np.ceil(alpha * np.minimum(a, b))
    @staticmethod
    def np_distance(o, a, b): return 1 - o / (b + 0 * a)


class Below:
    def MinY(self, alpha, size): return (size + 1) // 2
    def MaxY(self, alpha, size): return size - 2
    def Threshold(self, alpha, a, b): return int(math.ceil(alpha * min(a, b)))
    def Distance(self, inter, a, b): return 1 - inter / max(a, b)


class Edges:
    def __init__(self, n_segments):
        self.S = n_segments

    def MaxY(self, alpha, size): return 1 << 40 if size % 5 == 3 else size + 9

    def MinY(self, alpha, size):
        b_max = min(self.MaxY(alpha, size), self.S - 1)
        if size % 7 == 0:
            return b_max + 1                 # span 0 after the clamp
        if size % 11 == 0:
            return b_max + 2                 # span -1
        return size - 5

    def Threshold(self, alpha, a, b):
        r = (a + b) % 5
        if r == 0:
            return 0
        if r == 1:
            return min(a, b) + 1             # above |A| where a <= b, above |B| where b < a
        return int(math.ceil(alpha * min(a, b)))

    def Distance(self, inter, a, b): return 1 - 2 * inter / (a + b)


class Coarse:
    def MinY(self, alpha, size): return int(math.ceil(alpha * size))
    def MaxY(self, alpha, size): return int(math.floor(size / alpha))
    def Threshold(self, alpha, a, b): return int(math.ceil(alpha * min(a, b) / 2))
    def Distance(self, inter, a, b): return 2 + a % 4 + (b % 2) / 16 - 3 * (8 * inter // a) / 8


class Peak:
    def MinY(self, alpha, size): return int(math.ceil(alpha * size))
    def MaxY(self, alpha, size): return int(math.floor(size / alpha))
    def Threshold(self, alpha, a, b): return int(math.ceil(alpha * min(a, b)))
    def Distance(self, inter, a, b): return abs(inter - 0.7 * a) / a


def family(n_segments=S_LADDER):
    """name -> metric object (one object per name and call: the brute force caches by object)"""
    return dict(tversky=Tversky(), wobbly=Wobbly(), above=Above(), below=Below(), edges=Edges(n_segments), coarse=Coarse(), peak=Peak())


# what `conditions` must count to at least three queries for each metric, at every (similarity, k) the GPU test runs
REQUIRED = dict(
    tversky=("asymmetric",),
    wobbly=("threshold_falls", "min_y_negative"),
    above=("extra_segment",),
    below=("extra_segment",),
    edges=("min_y_negative", "max_y_beyond_int32", "threshold_zero", "threshold_above_a", "threshold_above_b", "deadlock", "panic"),
    coarse=("negative_scores", "scores_above_one", "ties"),
    peak=("not_monotone",),
)


def ladder_tokens():
    """(document tokens, query tokens) of the ladder at q = 1: a symbol is a token (the CPU test holds this against the oracle)"""
    return [list(d.decode()) for d in DOCS], [list(q.decode()) for q in QUERIES]


def conditions(bf, metric, alpha, k):
    """From the brute force alone: how many QUERIES show each property under (metric, alpha, k) -> {property: queries}."""
    out = dict.fromkeys(sum(REQUIRED.values(), ()), 0)
    cands = bf.candidates(metric, alpha)
    mono = bf.tightened(metric, alpha, k, assume_monotone=True) if isinstance(metric, Peak) and k < len(bf.card) else None
    rows = bf.suggest(metric, alpha, k)
    for qi, a in enumerate(bf.size_a):
        c = cands[qi]
        out["max_y_beyond_int32"] += metric.MaxY(alpha, a) > 2**31 - 1
        out["min_y_negative"] += metric.MinY(alpha, a) < 0 and isinstance(c, tuple)
        if not isinstance(c, tuple):
            out["panic"] += c == ref.PANIC
            out["deadlock"] += c == ref.DEADLOCK
            continue
        sizes = ref.visited_sizes(metric, alpha, a, bf.S)
        narrow = set(ref.visited_sizes(metric, alpha, a, bf.S, narrow=True))
        n = min(k, len(c[0]))
        ids, sc, seg, ov = (x[:n] for x in c)
        thr = {b: metric.Threshold(alpha, a, b) for b in sizes}
        mid = sizes[1:-1]
        out["threshold_zero"] += any(thr[b] == 0 for b in mid)
        out["threshold_above_a"] += any(thr[b] > a for b in mid)
        out["threshold_above_b"] += any(a >= thr[b] > b for b in mid)
        ok = [b for b in sizes if not (thr[b] == 0 or thr[b] > b or thr[b] > a)]
        # a searched segment whose right-hand neighbour asks less, and a row of that neighbour below the first one's threshold
        falls = {nb: thr[b] for b, nb in zip(ok, ok[1:]) if nb == b + 1 and thr[b] > thr[nb]}
        out["threshold_falls"] += any(int(s) in falls and int(o) < falls[int(s)] for s, o in zip(seg, ov))
        out["extra_segment"] += any(int(s) not in narrow for s in seg)
        out["asymmetric"] += any(1 - metric.Distance(int(o), a, int(s)) != 1 - metric.Distance(int(o), int(s), a) for s, o in zip(seg, ov) if s != a)
        out["negative_scores"] += bool((sc < 0).sum() >= 2 and len(set(sc[sc < 0].tolist())) >= 2)     # two different negative scores to order
        out["scores_above_one"] += bool((sc > 1).any())
        out["ties"] += bool(n >= 2 and (sc[1:] == sc[:-1]).any())
        if mono is not None:
            out["not_monotone"] += bool(ref.differences((rows[0][qi:qi + 1], rows[1][qi:qi + 1], rows[2][qi:qi + 1]),
                                                        (mono[0][qi:qi + 1], mono[1][qi:qi + 1], mono[2][qi:qi + 1])))
        else:                                   # k = everything, nothing to tighten against: a row where more overlap scored less
            best = {}
            for s, o, x in zip(seg.tolist(), ov.tolist(), sc.tolist()):
                best.setdefault(s, []).append((o, x))
            out["not_monotone"] += any(o1 < o2 and x1 > x2 for v in best.values() for o1, x1 in v[:8] for o2, x2 in v[:8])
    return out


def numpy_tables(metric, alpha, a_max, n_segments):
    """The four arrays of sg_metric_tables_create for a metric with np_threshold / np_distance, every cell filled (the library
    reads the visited ones): the same IEEE operations in the same order as the object's own methods, which the CPU test holds
    cell by cell.  For tables too large for a Python loop (a_max = 200)."""
    n_a = a_max + 1
    i32 = lambda v: int(max(-2**31, min(2**31 - 1, v)))                                  # noqa: E731
    min_y = np.array([i32(metric.MinY(alpha, a)) for a in range(n_a)], dtype=np.int32)
    max_y = np.array([i32(metric.MaxY(alpha, a)) for a in range(n_a)], dtype=np.int32)
    a = np.arange(n_a, dtype=np.float64)[:, None]
    b = np.arange(n_segments, dtype=np.float64)[None, :]
    thr = np.ascontiguousarray(metric.np_threshold(alpha, a, b).astype(np.int32))
    with np.errstate(divide="ignore", invalid="ignore"):
        score = 1 - metric.np_distance(np.arange(n_a, dtype=np.float64)[None, None, :], a[:, :, None], b[:, :, None])
    return min_y, max_y, thr, np.ascontiguousarray(score)


# ---- the long ladder: queries of 129 .. 200 n-grams (sg_long_kernel) -----------------------------------------------------------
def _letters(first, last, skip=()):
    return "".join(chr(c) for c in range(first, last + 1) if chr(c) not in skip)


# the ladder's 64 symbols, then lower-case Cyrillic (а .. я, ѐ .. џ), Greek (α .. ω), Armenian (ա .. ֆ) and Georgian (ა .. ჰ)
LONG_SYMBOLS = SYMBOLS + _letters(0x430, 0x45F) + _letters(0x3B1, 0x3C9) + _letters(0x561, 0x586) + _letters(0x10D0, 0x10F0)
LONG_DESC = dict(ngram_size=1, wrap=("", ""), pad="~", alphabet=(LONG_SYMBOLS,))
LONG_SIZES = tuple(range(96, 201, 8))
LONG_A_MAX = 200
LONG_DOCS = [LONG_SYMBOLS[s:s + b].encode() for b in LONG_SIZES for s in range(0, len(LONG_SYMBOLS) - b + 1)]
LONG_QUERIES = [LONG_SYMBOLS[:a].encode() for a in range(129, 201)]
LONG_OVER = LONG_SYMBOLS[:201].encode()      # one symbol more than the tables hold: SG_COUNT_TOO_LONG
LONG_S = 201


def long_tokens():
    return [list(d.decode()) for d in LONG_DOCS], [list(q.decode()) for q in LONG_QUERIES]
