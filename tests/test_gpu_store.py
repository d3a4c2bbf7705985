"""What an upload derives on the GPU — the segment-major numbering, the packed posting store with its two chunk formats, the rows,
cut_sample and the forward index (packed_store.inc, forward_index.inc) — read back raw (sg_debug_index_array) and compared, word
for word, with the plain restatement of tests/packed_ref.py applied to the host CSR.  Integer equality throughout.

The search tests see these arrays only through the rows of the queries that happen to touch a list at a given place; a wrong count
field, padding gap, cut_sample entry or format changes no row at all.  tests/test_packed_ref_cpu.py shows that the checker fails on
each of them."""
import numpy as np
import pytest

import packed_ref as pr
from conftest import CARS_DESC, WORDS_DESC

pytestmark = pytest.mark.gpu

BREAK = 65536            # the smallest gap a 16-bit chunk cannot hold
CARD = 8                 # every string of the crafted dictionary has 8 characters = 8 trigrams: one segment, x == docID


def _desc(d):
    from suggest_amd import IndexDescription
    return IndexDescription(ngram_size=d["ngram_size"], wrap=d["wrap"], pad=d["pad"], alphabet=d["alphabet"])


def _run(n):
    return [1] * (n - 1)


# family -> the x-gaps of its lists.  A family is one marker string over two letters p, q of k..z that no other string uses, planted
# at the documents that give its eight terms exactly these gaps.
F130 = [256 if i in (63, 64, 100) else 255 if i in (30, 90) else 1 for i in range(1, 130)]
FAMILIES = {
    "gap_65535": [BREAK - 1],                                     # stays in the chunk
    "gap_65536": [BREAK],                                         # a new chunk
    "7_break_7": _run(7) + [BREAK] + _run(7),                     # the forced break falls on a chunk boundary
    "3_break_10": _run(3) + [BREAK] + _run(10),                   # a short chunk in mid-list, 7 + 3 behind it
    "64_break_5": _run(64) + [BREAK] + _run(5),                   # the break at lane 0 of the second batch of 64
    "130_g8": F130,                                               # 8-bit breaks at lanes 63 and 0, a run carried over the batch
}
FAMILIES.update({"len_%d" % n: _run(n) for n in (1, 6, 7, 8, 13, 14, 63, 64, 65, 128, 129)})
LETTERS = b"klmnopqrstuvwxyz"


def _marker(i):
    """pqqppqpq: eight distinct trigrams ($pq pqq qqp qpp ppq pqp qpq pq$), each with both letters — no two pairs share one"""
    p, q = [(p, q) for a, p in enumerate(LETTERS) for q in LETTERS[a + 1:]][i]
    return bytes([p, q, q, p, p, q, p, q])


@pytest.fixture(scope="module")
def crafted():
    """-> (blob, offs, {family: (marker string, docIDs)}): ~66 000 strings of 8 characters over a-j0-9 (the first three over a, b: a
    dozen dense terms, so that SG_G8=1 has something to choose), the markers planted among them; document 0 is a marker of its own."""
    plant, at = {"doc_0": (_marker(0), np.array([0]))}, 1
    for i, (fam, gaps) in enumerate(FAMILIES.items()):
        # a family's block in the numbering with the large gaps taken out: blocks apart there are apart in docIDs too
        plant[fam] = (_marker(i + 1), at + np.concatenate([[0], np.cumsum(gaps, dtype=np.int64)]).astype(np.int64))
        at += sum(g for g in gaps if g < BREAK - 1) + 4
    n = max(int(d.max()) for _, d in plant.values()) + 400
    rnd = np.random.RandomState(17)

    def draw(m):
        sym = rnd.randint(0, 20, size=(m, CARD))
        sym[:, :3] = rnd.randint(0, 2, size=(m, 3))
        return sym

    sym = draw(n)
    while True:     # a string that repeats a trigram has fewer than 8 terms and falls into another segment: draw it again
        tri = np.sort(sym[:, :-2] * 400 + sym[:, 1:-1] * 20 + sym[:, 2:], axis=1)
        again = np.flatnonzero((tri[:, 1:] == tri[:, :-1]).any(axis=1))
        if not again.size:
            break
        sym[again] = draw(again.size)
    rows = np.frombuffer(b"abcdefghij0123456789", dtype=np.uint8)[sym]
    taken = np.concatenate([d for _, d in plant.values()])
    assert len(set(taken.tolist())) == taken.size
    for s, docs in plant.values():
        rows[docs] = np.frombuffer(s, dtype=np.uint8)
    return rows.reshape(-1).copy(), np.arange(n + 1, dtype=np.uint64) * CARD, plant


def _index(monkeypatch, g8, **kw):
    from suggest_amd import NGramIndex
    monkeypatch.setenv("SG_G8", str(g8))
    return NGramIndex(**kw)


@pytest.mark.parametrize("g8,build", [(0, "host"), (1, "host"), (2, "host"), (1, "device")])
def test_crafted_gaps_breaks_and_carries(monkeypatch, crafted, g8, build):
    from suggest_amd import IndexDescription, synth
    blob, offs, plant = crafted
    ix = _index(monkeypatch, g8, blob=blob, offs=offs, description=IndexDescription(**synth.DESCRIPTION), build=build)
    st = ix.stats()
    n_docs, S, n_terms = st["n_docs"], st["n_segments"], st["n_terms"]
    assert 66000 < n_docs < 69000 and S == CARD + 1
    # first: the host CSR holds every intended pattern, as exact gaps in the store's own numbering
    hp, hso = ix.raw_array("host_postings"), ix.raw_array("host_seg_off")
    ref = pr.derive(hp, hso, n_docs, S, n_terms, g8)
    assert np.array_equal(ref.x_of, np.arange(n_docs)) and ref.seg_base.tolist() == [0] * (CARD + 1) + [n_docs]
    term_of = {int(k): t for t, k in enumerate(pr.term_keys(ix))}
    for fam, (s, docs) in plant.items():
        keys = set(ix.tokenize_keys(s))
        assert len(keys) == CARD
        for k in keys:
            x = ref.x[ref.vl == term_of[k] * S + CARD]
            assert np.array_equal(x, docs), fam
            assert np.diff(x).tolist() == FAMILIES.get(fam, []), fam
    first = hp[int(hso[term_of[ix.tokenize_keys(plant["doc_0"][0])[0]] * (S + 1) + CARD]) * 4:][:4]
    assert first.tolist() == [0, 0, 0, 0]                        # the host padding of a list that holds document 0 alone
    # then: what the kernels built
    ref, dev = pr.check_index(ix, g8)
    total = dev.packed.shape[0] - pr.SLACK
    print("crafted dictionary, SG_G8=%d, build=%s: %d chunks with 16-bit gaps throughout, %d in the store, %d terms of %d with 8-bit gaps"
          % (g8, build, ref.s16.sum(), total, ref.want_fmt.sum(), n_terms))
    assert total == (ref.s16.sum() if g8 == 0 else np.where(ref.want_fmt, ref.s8, ref.s16).sum())
    if g8 == 1:     # the mixed store: the dense terms and the long marker runs took 8-bit gaps, the sparse terms did not
        assert 0 < ref.want_fmt.sum() < n_terms
        assert all(ref.want_fmt[term_of[k]] for k in ix.tokenize_keys(plant["130_g8"][0]))
        assert not any(ref.want_fmt[term_of[k]] for k in ix.tokenize_keys(plant["gap_65536"][0]))
    ix.close()


@pytest.mark.parametrize("S", [63, 64])
def test_strided_forward_layout_up_to_63_segments(monkeypatch, S):
    """pack_store lays the forward index out at a fixed stride per segment (fx_base) for dictionaries of at most 63 segments."""
    from suggest_amd import IndexDescription, synth
    blob, offs = synth.make_dict(3000, seed=23)
    ix = _index(monkeypatch, 1, blob=blob, offs=offs, description=IndexDescription(**synth.DESCRIPTION), min_segments=S)
    assert ix.stats()["n_segments"] == S
    assert ix.raw_array("fx_base").size == (S + 1 if S <= 63 else 0)
    ref, _ = pr.check_index(ix, 1)
    assert ref.strided == (S <= 63)
    ix.close()


def test_one_document(monkeypatch):
    from suggest_amd import IndexDescription, synth
    for g8 in (0, 2):
        ix = _index(monkeypatch, g8, docs=[b"hello"], description=IndexDescription(**synth.DESCRIPTION))
        ref, dev = pr.check_index(ix, g8)
        assert dev.orig_of.tolist() == [0] and dev.packed.shape[0] - pr.SLACK == ix.stats()["n_terms"] == 5
        ix.close()


def test_more_lists_than_the_launch_grid(monkeypatch):
    """fwd_walk, pk_pack and pk_finish start at most 2^22 wavefronts and stride over the (term, segment) lists: the lists behind
    the grid once went unwalked (forward_index.inc)."""
    from suggest_amd import IndexDescription, synth
    blob, offs = synth.make_dict(60000, seed=29)
    ix = _index(monkeypatch, 1, blob=blob, offs=offs, description=IndexDescription(**synth.DESCRIPTION), min_segments=100)
    st = ix.stats()
    assert st["n_terms"] * st["n_segments"] > 1 << 22
    ref, _ = pr.check_index(ix, 1)
    assert (ref.vl >= 1 << 22).sum() > 100000                     # postings of lists only the second trip of the loop reaches
    ix.close()


@pytest.mark.parametrize("g8", [0, 2])
@pytest.mark.parametrize("which", ["cars", "words"])
def test_reference_dictionaries(monkeypatch, cars_lines, words_lines, which, g8):
    """Real strings: many cardinality segments, and in cars.dict documents that repeat a term — fewer distinct terms than n-grams,
    which leaves slots of their stride in the forward index empty."""
    lines, desc = (cars_lines, CARS_DESC) if which == "cars" else (words_lines[::8], WORDS_DESC)
    ix = _index(monkeypatch, g8, docs=lines, description=_desc(desc))
    ref, dev = pr.check_index(ix, g8)
    if which == "cars":      # (211 of its strings repeat a trigram once normalised; the words never do)
        assert ((ref.nd < ref.card) & (ref.nd > 0)).sum() > 100
    assert (np.diff(dev.seg_base) > 0).sum() >= 10
    assert bool((dev.seg_off >> 31).any()) == (g8 == 2)
    ix.close()
