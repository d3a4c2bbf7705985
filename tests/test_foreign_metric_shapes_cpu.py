"""The brute-force statement of Suggest (foreign_metric_ref.py) proved on the five native metrics against the oracle, the foreign
family's properties counted (foreign_metric_shapes.py), the checker shown to fail where it must, and the bindings' tabulation held
cell by cell against the metric objects — all without a GPU."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import foreign_metric_ref as ref
import foreign_metric_shapes as fm
import oracle
from test_gpu_metric_ladder import SIMILARITIES as LADDER_SIMILARITIES

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def ladder():
    ora = oracle.OracleIndex(fm.DOCS, **fm.DESC)
    docs, queries = fm.ladder_tokens()
    # the ladder's tokens are its symbols, and the overlap is the issue's formula
    assert ora.n_segments == fm.S_LADDER
    assert all(ora.tokenize(q) == [t.encode() for t in toks] for q, toks in zip(fm.QUERIES, queries))
    assert all(ora.tokenize(d) == [t.encode() for t in toks] for d, toks in zip(fm.DOCS[::37], docs[::37]))
    bf = ref.BruteForce(docs, queries, fm.S_LADDER)
    starts = np.array([fm.SYMBOLS.index(d.decode()[0]) for d in fm.DOCS])
    for qi in (0, 1, 30, 63):
        a = qi + 1
        assert (bf.overlap[qi] == np.maximum(0, np.minimum(a, starts + bf.card) - starts)).all()
    return bf, ora


@pytest.mark.parametrize("metric", ["jaccard", "cosine", "dice", "overlap", "exact"])
def test_the_brute_force_is_the_oracle_on_the_native_metrics(ladder, metric):
    from suggest_amd.metric import resolve
    bf, ora = ladder
    qb, qo = oracle.pack_strings(fm.QUERIES)
    m = resolve(metric)
    flagged = 0
    for s in ([1.0] if metric == "exact" else LADDER_SIMILARITIES[::4]):
        for k in (len(fm.DOCS), 10):
            want = ora.suggest_batch(qb, qo, metric, s, k)[:3]
            got = bf.suggest(m, s, k)
            assert not ref.differences(got, want), (metric, s, k, ref.differences(got, want))
            flagged += int((want[2] >= ref.TOO_LONG).sum())
    print(metric, "flagged rows over the sweep:", flagged)


def test_the_five_metrics_never_leave_a_gap():
    """why the device's [b_min, b_max] was the reference's walk for the five: MinY <= a + 1 and min(MaxY, S - 1) >= a wherever the
    span is above zero and a < S — so sg_metric_window changes nothing for them"""
    from suggest_amd.index import metric_window
    from suggest_amd.metric import resolve
    for name in ("jaccard", "cosine", "dice", "overlap", "exact"):
        m = resolve(name)
        for s in LADDER_SIMILARITIES[::4]:
            for a in range(1, 65):
                lo, hi = m.MinY(s, a), m.MaxY(s, a)
                assert metric_window(lo, min(hi, 2**31 - 1), a, 65) == (lo, min(hi, 2**31 - 1) if min(hi, 64) - lo + 1 <= 0 else min(hi, 64)), (name, s, a)


def test_metric_window():
    from suggest_amd import _lib
    from suggest_amd.index import metric_window
    assert metric_window(10, 20, 7, 65) == (8, 20)            # above a: a + 1 joins
    assert metric_window(10, 20, 8, 65) == (9, 20)
    assert metric_window(10, 20, 9, 65) == (10, 20)
    assert metric_window(3, 5, 7, 65) == (3, 7)               # below a: bMax + 1 .. a join
    assert metric_window(3, 6, 7, 65) == (3, 7) and metric_window(3, 7, 7, 65) == (3, 7)
    assert metric_window(-4, 2**31 - 1, 3, 65) == (-4, 64)    # the clamp; a negative MinY stays
    assert metric_window(60, 2**31 - 1, 80, 65) == (60, 80)   # a beyond the index: the kernels clamp again, nothing lies there
    assert metric_window(65, 70, 3, 65) == (65, 70) and metric_window(66, 70, 3, 65) == (66, 70)      # span 0 / -1 after the clamp: raw
    assert metric_window(5, 4, 5, 65) == (5, 4) and metric_window(5, 3, 5, 65) == (5, 3)
    assert metric_window(-2**31, 2**31 - 1, 2**31 - 2, 1) == (-2**31, 2**31 - 2)
    assert _lib.lib().sg_metric_window(1, 2, 3, 4, None) == -1
    # the reference's walk, size by size, is the range
    for lo in range(-3, 12):
        for hi in range(-3, 14):
            for a in range(0, 12):
                class M:
                    def MinY(self, alpha, size): return lo
                    def MaxY(self, alpha, size): return hi
                sizes = ref.visited_sizes(M(), 0.5, a, 9)
                w = metric_window(lo, hi, a, 9)
                if not isinstance(sizes, list):
                    assert w == (lo, hi)
                else:
                    assert sizes == [b for b in range(max(0, w[0]), min(8, w[1]) + 1)], (lo, hi, a, sizes, w)


def test_go_shim_calls_the_window_with_the_headers_arity():
    go = open(os.path.join(ROOT, "go", "suggesthip", "suggesthip.go"), encoding="utf-8").read()
    header = open(os.path.join(ROOT, "include", "suggest_hip.h"), encoding="utf-8").read()
    decl = re.search(r"int sg_metric_window\(([^;]*)\);", header).group(1)
    call = re.search(r"C\.sg_metric_window\(([^\n]*)\)\n", go).group(1)
    depth, n = 0, 1
    for ch in call:
        depth += ch in "([{"
        depth -= ch in ")]}"
        n += ch == "," and depth == 0
    assert n == decl.count(",") + 1 == 5


@pytest.fixture(scope="module")
def family():
    return fm.family()


@pytest.mark.parametrize("name", sorted(fm.REQUIRED))
def test_conditions_hold_where_the_gpu_test_runs(ladder, family, name):
    bf, _ = ladder
    m = family[name]
    for s in fm.SIMILARITIES:
        for k in fm.KS:
            c = fm.conditions(bf, m, s, k)
            print(name, s, k, {p: c[p] for p in fm.REQUIRED[name]})
            assert all(c[p] >= 3 for p in fm.REQUIRED[name]), (name, s, k, c)
            if name == "peak":                                   # d_tighten's own rule loses nothing, whatever the score does
                assert not ref.differences(bf.tightened(m, s, k), bf.suggest(m, s, k)), (s, k)


def test_the_check_fails_on_swapped_ties(ladder, family):
    bf, _ = ladder
    ids, sc, cnt = bf.suggest(family["coarse"], 0.5, 10)
    assert not ref.differences((ids, sc, cnt), (ids, sc, cnt))
    swapped = 0
    for q in range(len(cnt)):
        ties = [j for j in range(int(cnt[q]) - 1) if sc[q, j] == sc[q, j + 1]]
        if ties:
            other = ids.copy()
            j = ties[0]
            other[q, j], other[q, j + 1] = ids[q, j + 1], ids[q, j]
            assert ref.differences((other, sc, cnt), (ids, sc, cnt)), q
            swapped += 1
    assert swapped >= 3
    neg = sc.copy()
    neg[5, 0] = -neg[5, 0] if neg[5, 0] else -0.0               # the bits are compared, not the values
    assert ref.differences((ids, neg, cnt), (ids, sc, cnt))


@pytest.mark.parametrize("name", ["above", "below"])
def test_the_check_fails_on_the_narrowed_window(ladder, family, name):
    bf, _ = ladder
    for s in fm.SIMILARITIES:
        for k in fm.KS:
            d = ref.differences(bf.suggest(family[name], s, k, narrow=True), bf.suggest(family[name], s, k), limit=64)
            assert len(d) >= 3, (name, s, k, d)


@pytest.mark.parametrize("name", sorted(fm.REQUIRED))
def test_tabulate_is_the_metric_cell_by_cell(family, name):
    """suggest_amd.index.tabulate over the VISITED range: MinY / MaxY as the metric gives them (clamped to 32 bits), Threshold at
    every visited size, 1 - Distance from the threshold up, zeros in every cell that is not visited"""
    from suggest_amd.index import tabulate
    m, S, a_max = family[name], fm.S_LADDER, 64
    clamp = lambda v: max(-2**31, min(2**31 - 1, v))                                    # noqa: E731
    for s in fm.SIMILARITIES[::2]:
        mn, mx, thr, score = tabulate(m, s, a_max, S)
        assert thr.shape == (65, S) and score.shape == (65, S, 65) and mn.dtype == mx.dtype == thr.dtype == np.int32
        for a in range(1, a_max + 1):
            assert (mn[a], mx[a]) == (clamp(m.MinY(s, a)), clamp(m.MaxY(s, a)))
            sizes = ref.visited_sizes(m, s, a, S)
            if not isinstance(sizes, list):                      # flagged: the raw window's cells are filled, none is ever read
                continue
            for b in range(S):
                if b not in sizes:
                    assert thr[a, b] == 0 and not score[a, b].any(), (name, s, a, b)
                    continue
                t = m.Threshold(s, a, b)
                assert thr[a, b] == t, (name, s, a, b)
                for o in range(max(t, 0), min(a, b) + 1):
                    assert np.float64(score[a, b, o]).view(np.uint64) == np.float64(1 - m.Distance(o, a, b)).view(np.uint64), (name, s, a, b, o)


def test_the_long_ladder_and_its_numpy_tables():
    """about 200 symbols, each one token that lower-casing leaves alone; the numpy tables of the long ladder hold the metric
    objects' own values over every cell a long query can reach"""
    syms = fm.LONG_SYMBOLS
    assert len(syms) == len(set(syms)) >= 200 and "~" not in syms and " " not in syms
    assert oracle.to_lower(syms.encode()).decode() == syms and syms.lower() == syms
    ora = oracle.OracleIndex(fm.LONG_DOCS, **fm.LONG_DESC)
    assert ora.n_segments == fm.LONG_S
    assert ora.tokenize(syms.encode()) == [c.encode() for c in syms]
    assert len(fm.LONG_DOCS) == len(set(fm.LONG_DOCS)) >= 700 and len(fm.LONG_QUERIES) == 72
    assert len(ora.tokenize(fm.LONG_OVER)) == fm.LONG_A_MAX + 1
    fam = fm.family(fm.LONG_S)
    for name, s in (("tversky", 0.5), ("wobbly", 0.5), ("above", 0.5)):
        m = fam[name]
        mn, mx, thr, score = fm.numpy_tables(m, s, fm.LONG_A_MAX, fm.LONG_S)
        for a in range(129, 201, 7):
            sizes = ref.visited_sizes(m, s, a, fm.LONG_S)
            for b in fm.LONG_SIZES + (a + 1,):
                if b >= fm.LONG_S:
                    continue
                t = m.Threshold(s, a, b)
                assert thr[a, b] == t
                if isinstance(sizes, list) and b in sizes:
                    for o in range(max(t, 0), min(a, b) + 1):
                        assert np.float64(score[a, b, o]).view(np.uint64) == np.float64(1 - m.Distance(o, a, b)).view(np.uint64), (name, a, b, o)
