"""The metric arithmetic of the device — d_min_y, d_max_y, d_threshold and d_score (engine.hip: fp64 ceil, floor, sqrt and
division, pkg/metric/{jaccard,cosine,dice,overlap,exact}.go) — on a dictionary that holds every (|A|, |B|, overlap) cell with
cardinalities 1 .. 64, over 173 similarities chosen for their rounding edges, against the oracle bit for bit.  At k = 2 080 (the
whole dictionary) every member of every result set is in the rows, so a window or a threshold that is off by one at one cell
shows; at k = 10 the order among ties and the kernels' threshold tightening decide the rows."""
import random

import numpy as np
import pytest

import oracle

pytestmark = pytest.mark.gpu

SPECIAL = 0xFFFFFFF0
# 64 printable ASCII symbols: not upper case, not the space, not '~' (the pad)
SYMBOLS = "".join(chr(c) for c in range(0x21, 0x7B) if not "A" <= chr(c) <= "Z")
DESC = dict(ngram_size=1, wrap=("", ""), pad="~", alphabet=(SYMBOLS,))
DOCS = [SYMBOLS[s:s + b].encode() for b in range(1, 65) for s in range(0, 65 - b)]
QUERIES = [SYMBOLS[:a].encode() for a in range(1, 65)]
K_ALL, K_TOP = len(DOCS), 10


def similarities():
    s = {i / 100 for i in range(1, 101)}
    s |= {p / q for q in (3, 6, 7, 9, 11, 12, 13) for p in range(1, q)}
    s |= {float(np.nextafter(x, d)) for x in (0.25, 0.5, 0.75, 1.0) for d in (0.0, 2.0) if np.nextafter(x, d) <= 1.0}
    rnd = random.Random(20261019)
    s |= {rnd.random() for _ in range(24)}
    return sorted(s)


SIMILARITIES = similarities()
METRICS = ("jaccard", "cosine", "dice", "overlap")
DEFAULTS = dict(SG_LOG2_CNT=11, SG_PIPE=2, SG_TIGHTEN=2, SG_PRETOK=2048)
# name -> (knobs, takes the pipeline)
LAUNCHES = {
    "default": (dict(), False),                                                            # 2 080 documents: a counter per document
    "counters-512": (dict(SG_LOG2_CNT=9, SG_PIPE=0), False),                               # 2 080 > 4 x 512: past that path
    "pipeline": (dict(SG_LOG2_CNT=9, SG_PIPE=1, SG_TIGHTEN=0, SG_PRETOK=1), True),         # |A| <= 32: plan2's halves; above: a wavefront each
}


def test_the_ladder_is_what_the_issue_describes():
    assert len(SYMBOLS) == len(set(SYMBOLS)) == 64 and "~" not in SYMBOLS and " " not in SYMBOLS and SYMBOLS == SYMBOLS.lower()
    assert len(DOCS) == 2080 == len(set(DOCS)) and len(QUERIES) == 64 and len(SIMILARITIES) == 173
    assert all(0.0 < s <= 1.0 for s in SIMILARITIES)
    ora = oracle.OracleIndex(DOCS, **DESC)
    assert ora.n_segments == 65
    assert all(len(ora.tokenize(q)) == a + 1 for a, q in enumerate(QUERIES)) and all(len(ora.tokenize(d)) == len(d) for d in DOCS)
    cells = {(a, len(d), len(set(SYMBOLS[:a]) & set(d.decode()))) for a in range(1, 65) for d in DOCS}
    assert cells == {(a, b, o) for a in range(1, 65) for b in range(1, 65) for o in range(0, min(a, b) + 1) if b - o <= 64 - a}


def _compact(rows):
    """(ids, scores, counts) -> (the valid ids, the bits of the valid scores, counts): what two sets of rows must share"""
    ids, sc, cnt = rows[:3]
    assert (cnt < SPECIAL).all()
    valid = np.arange(ids.shape[1])[None, :] < cnt[:, None]
    return ids[valid].copy(), sc.view(np.uint64)[valid].copy(), cnt.copy()


@pytest.fixture(scope="module")
def ladder():
    from suggest_amd import IndexDescription, NGramIndex
    gpu = NGramIndex(DOCS, IndexDescription(**DESC))
    ora = oracle.OracleIndex(DOCS, **DESC)
    yield gpu, ora, oracle.pack_strings(QUERIES)
    gpu.close()


PARTS = 3                                 # a case takes every third similarity: low ones (the large result sets) in every part


@pytest.fixture(scope="module", params=METRICS)
def wanted(request, ladder):
    """the oracle's rows of one metric over the sweep, computed once (one metric's at a time is held)"""
    _, ora, (qb, qo) = ladder
    want = {(s, k): _compact(ora.suggest_batch(qb, qo, request.param, s, k)) for s in SIMILARITIES for k in (K_ALL, K_TOP)}
    assert all((w[2] >= 1).all() for w in want.values())         # (every query is a document: no row is empty)
    return request.param, want


def _sweep(gpu, packed, metric, want, launch):
    """the device's rows under `launch` for every (similarity, k) of `want` -> what differs, every call tried"""
    qb, qo = packed
    knobs, pipeline = LAUNCHES[launch]
    differ = []
    try:
        gpu.tune(**knobs)
        for (s, k), (w_ids, w_bits, w_cnt) in want.items():
            before = gpu.pipe_stats()["queries"]
            ids, bits, cnt = _compact(gpu.suggest_batch(blob=qb, offs=qo, metric=metric, similarity=s, k=k))
            assert gpu.pipe_stats()["queries"] - before == (len(QUERIES) if pipeline else 0), (metric, s, k, launch)
            bad = np.nonzero(cnt != w_cnt)[0]
            if bad.size:
                differ.append(("counts differ", repr(s), k, "|A| =", (bad[:5] + 1).tolist(), cnt[bad[:5]].tolist(), w_cnt[bad[:5]].tolist()))
                continue
            bad = np.nonzero((ids != w_ids) | (bits != w_bits))[0]
            if bad.size:
                row = np.repeat(np.arange(len(cnt)), cnt)
                differ.append(("rows differ", repr(s), k, "|A| =", int(row[bad[0]]) + 1, ids[bad[:3]].tolist(), w_ids[bad[:3]].tolist(),
                               bits[bad[:3]].view(np.float64).tolist(), w_bits[bad[:3]].view(np.float64).tolist()))
    finally:
        gpu.tune(**DEFAULTS)
    return differ


@pytest.mark.parametrize("part", range(PARTS))
@pytest.mark.parametrize("k", (K_ALL, K_TOP))
@pytest.mark.parametrize("launch", list(LAUNCHES))
def test_rows_over_the_sweep(ladder, wanted, launch, k, part):
    gpu, _, packed = ladder
    metric, want = wanted
    mine = {(s, k): want[s, k] for s in SIMILARITIES[part::PARTS]}
    differ = _sweep(gpu, packed, metric, mine, launch)
    assert not differ, (metric, launch, len(differ), "of", len(mine), differ[:10])


@pytest.mark.parametrize("launch", list(LAUNCHES))
def test_exact_rows(ladder, launch):
    gpu, ora, packed = ladder
    want = {(1.0, k): _compact(ora.suggest_batch(*packed, "exact", 1.0, k)) for k in (K_ALL, K_TOP)}
    assert all((w[2] == 1).all() for w in want.values())          # a query's own text, and no other document has its tokens
    differ = _sweep(gpu, packed, "exact", want, launch)
    assert not differ, (launch, differ)
