"""Deterministic inputs that drive the three outcomes of a query's window — rows, the reference's dead-lock, the reference's
panic (query_window, engine.hip; suggester.go:53-62) — through every planner: the fused kernel, sg_plan2_kernel's halves
(|A| <= 32) and plan_one_query (|A| 33 .. 64).

A dictionary of short documents (cardinalities 1 .. 8, so 9 segments) under queries of 1 .. 64 n-grams: where MinY(|A|) passes
the last segment the clipped window has span 0 (dead-lock) or a negative span (panic).  More than 2 048 documents, so a launch
with 512 counter words per wavefront is past the counter-per-document path and may take the pipeline.

Used by test_window_shapes_cpu.py (the oracle alone: the classes below are what the oracle gives) and test_gpu_window_flags.py
(the device against the oracle).  Nothing here touches the GPU.
"""
COUNT_PANIC, COUNT_DEADLOCK = 0xFFFFFFFF, 0xFFFFFFFE

# the 64 symbols of test_gpu_metric_ladder.py: printable ASCII, not upper case, not the space, not '~' (the pad)
SYMBOLS = "".join(chr(c) for c in range(0x21, 0x7B) if not "A" <= chr(c) <= "Z")
DESC = dict(ngram_size=1, wrap=("", ""), pad="~", alphabet=(SYMBOLS,))
# every b-th-of-step run of the symbols, b and step 1 .. 8, first occurrences only
DOCS = list(dict.fromkeys(SYMBOLS[s::step][:b].encode() for step in range(1, 9) for b in range(1, 9) for s in range(64)
                          if s + (b - 1) * step < 64))
QUERIES = [SYMBOLS[:a].encode() for a in range(1, 65)]
K = 10
CALLS = (("jaccard", 0.5), ("jaccard", 0.25), ("dice", 0.5), ("cosine", 0.4))
# (queries with rows, dead-locks, panics, empty rows) over |A| 1 .. 32 (plan2's range) and 33 .. 64 (the one-query planner's)
CLASSES = {
    ("jaccard", 0.5): ((16, 2, 14, 0), (0, 0, 32, 0)),
    ("jaccard", 0.25): ((32, 0, 0, 0), (0, 4, 28, 0)),
    ("dice", 0.5): ((24, 3, 5, 0), (0, 0, 32, 0)),
    ("cosine", 0.4): ((32, 0, 0, 0), (17, 7, 8, 0)),
}


def classes(counts):
    """counts of the 64 queries -> the two cells of CLASSES"""
    def cell(c):
        c = [int(x) for x in c]
        cell = (sum(0 < x <= K for x in c), c.count(COUNT_DEADLOCK), c.count(COUNT_PANIC), c.count(0))
        assert sum(cell) == len(c), c                          # (no other flag, no count above k)
        return cell
    return cell(counts[:32]), cell(counts[32:])
