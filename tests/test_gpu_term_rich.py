"""A term-rich dictionary (tests/term_rich_shapes.py: 240 000 documents, 691 501 distinct 4-grams) and the device builder's term
table (index_build.inc) on its edges.  Every other dictionary of the suite stays under 37^3 terms: the builder's 2^20-slot table
never passed a load of 5 %, never overflowed, its tokenise pass was never repeated, no probe chain ever wrapped from the last slot
to slot 0, and no term id above 2^19 ever reached the forward index, the packed store, a seg_off row or the verify launch's hash.

The builder's reference is the host build (stats and digest), which tests/test_term_rich_shapes_cpu.py holds against plain numpy;
the search's reference is the CPU oracle, row for row: ids, order, score bits, counts.  sg_debug_index_build_table_bits shrinks the
first table so that dictionaries of a dozen terms stand where 524 289 terms stand by default, and sg_debug_index_build_report says
which path a build took — every case asserts it.

What the cases had to go by in the code:
  * Under the capacity rule (the table starts no smaller than capacity / 16) no dictionary can repeat the pass more than three
    times, and cars.dict or words.dict not even once at 16 slots: the hook names the first table outright (suggest_hip.h).
  * The overflow count includes the empty term, which lives beside the table: the empty-pad dictionary has seven terms and the
    empty one, which 16 slots take in one pass; empty_pad_documents() adds four one-term documents to it.
  * The tokeniser keeps an n-gram of a document once, so "aaaa" repeats no term; the documents of the "repeated terms" refusal are
    "a-a+", whose foreign runes become the pad: $a$ twice.  And a random 65 000-byte document over 36 letters has 35 145 distinct
    trigrams, with 80 000 short documents 3.6 x 10^9 cells, which the builder takes: the long document is over 68 letters.
  * The long tokeniser takes the documents d_tokenize gives up on: above 128 n-grams OR above 144 runes — four of
    long_documents(), of which three have more than 128 n-grams.
"""
import numpy as np
import pytest

import long_query_shapes as lq
import oracle
import packed_ref as pr
import term_rich_shapes as tr
from conftest import CARS_DESC, WORDS_DESC
from test_gpu_parity import assert_same
from test_gpu_tokenizers import DEFAULTS, LAUNCHES

pytestmark = pytest.mark.gpu

SEARCH_LAUNCHES = ("fused", "pipe-plan", "pipe-plan2-natural")


def _desc(d):
    from suggest_amd import IndexDescription
    return IndexDescription(ngram_size=d["ngram_size"], wrap=d["wrap"], pad=d["pad"], alphabet=d["alphabet"])


def _device_build(desc, docs=None, bits=0, **kw):
    """-> (the index built on the device with the first table at 2^bits slots (0: the default), its report); the hook is
    process-wide and restored whatever happens"""
    from suggest_amd import NGramIndex
    from suggest_amd.index import build_report, build_table_bits
    with build_table_bits(bits):                      # (restores the default in a `finally`)
        ix = NGramIndex(docs, _desc(desc), upload=False, build="device", **kw)
        return ix, build_report()


def _same_as_host(desc, docs, bits):
    """the device build at 2^bits slots against the host build: stats and digest -> the report"""
    from suggest_amd import NGramIndex
    host = NGramIndex(docs, _desc(desc), upload=False)
    dev, report = _device_build(desc, docs, bits)
    try:
        assert dev.stats() == host.stats(), report
        assert dev.digest() == host.digest(), report
        assert report["terms"] == host.stats()["n_terms"]
    finally:
        host.close()
        dev.close()
    return report


# ---- the builder's table, small ----------------------------------------------------------------------------------------------------
def test_table_boundary():
    """build_intern flags overflow when the count before its own increment is above mask >> 1: 16 slots take 8 terms, the 9th
    flags and the pass is repeated at 64 slots"""
    assert tr.first_overflow(4) == 9
    below = _same_as_host(tr.TABLE_DESC, tr.one_term_documents(8), 4)
    assert below == dict(passes=1, log2_table=4, terms=8, long_docs=0)
    above = _same_as_host(tr.TABLE_DESC, tr.one_term_documents(9), 4)
    assert above == dict(passes=2, log2_table=6, terms=9, long_docs=0)


@pytest.mark.parametrize("three", ["first", "last"])
def test_probe_chain_wraps_to_slot_0(three):
    """three terms whose home is the last of 16 slots: two of them are interned (build_intern), and found again (build_find, in
    build_assign and build_emit), in slot 0 or behind it, where another term has its home"""
    from suggest_amd import NGramIndex
    probe = NGramIndex([b"abc"], _desc(tr.TABLE_DESC), upload=False)
    last, others = tr.wrap_around(lambda d: probe.tokenize_keys(d)[0])
    home = [tr.mix64(probe.tokenize_keys(d)[0]) & 15 for d in last + others]
    probe.close()
    assert home[:4] == [15, 15, 15, 0] and all(4 <= h <= 11 for h in home[4:])
    docs = last + others if three == "first" else others + last
    assert _same_as_host(tr.TABLE_DESC, docs, 4) == dict(passes=1, log2_table=4, terms=7, long_docs=0)


@pytest.mark.parametrize("which", ["cars", "words"])
def test_many_passes(cars_lines, words_lines, which):
    """16, 64, 256 ... slots: every repeat starts from a fresh table, zeroed counters and the whole dictionary"""
    docs, desc = (cars_lines, CARS_DESC) if which == "cars" else (words_lines[::8], WORDS_DESC)
    report = _same_as_host(desc, docs, 4)
    assert report["passes"] >= 5 and report["log2_table"] == 4 + 2 * (report["passes"] - 1), report
    assert report["terms"] <= 1 << report["log2_table"] >> 1
    small, _ = _device_build(desc, docs, 4)
    default, at_default = _device_build(desc, docs, 0)
    assert at_default["passes"] == 1 and at_default["log2_table"] == 20
    assert small.digest() == default.digest() and small.stats() == default.stats()
    small.close()
    default.close()


def test_long_documents_through_repeated_passes():
    """every pass lists the long documents anew (stats[1], long_docs) and the long tokeniser runs in the last one alone: it took
    each of them once, not once per pass"""
    docs = tr.long_documents()
    ora = oracle.OracleIndex(docs, **tr.LONG_DESC)
    n_long = sum(lq.is_long(ora, tr.LONG_DESC, d) for d in docs)
    assert n_long == 4
    report = _same_as_host(tr.LONG_DESC, docs, 4)
    assert report["passes"] >= 3 and report["long_docs"] == n_long, report


@pytest.mark.parametrize("first", [None, b"---"])
def test_empty_term_through_a_repeated_pass(first):
    """the empty term lives beside the table (zero_term): its first appearance and its count in stats[2] are reset with the
    table; as document 0 it is term 0"""
    docs = ([first] if first else []) + tr.empty_pad_documents()
    report = _same_as_host(tr.EMPTY_PAD_DESC, docs, 4)
    assert report == dict(passes=2, log2_table=6, terms=12, long_docs=0)


# ---- the term-rich dictionary ------------------------------------------------------------------------------------------------------
class _Rich:
    def __init__(self):
        from suggest_amd import NGramIndex
        self.docs = tr.term_rich()
        self.blob, self.offs = tr.pack(self.docs)
        self.ora = oracle.OracleIndex(blob=self.blob, offs=self.offs, **tr.DESC)
        self.queries = tr.queries(self.docs)
        self.packed = oracle.pack_strings(self.queries)
        self.prefixes = tr.prefixes(self.queries)
        self.packed_prefixes = oracle.pack_strings(self.prefixes)
        self.want = {c: self._frozen(self.ora.suggest_batch(*self.packed, *c)[:3]) for c in tr.CALLS}
        self.want_auto = {n: self._frozen(self.ora.autocomplete_batch(*self.packed_prefixes, n)[:2]) for n in (7, 80)}
        self.index = {"host": NGramIndex(blob=self.blob, offs=self.offs, description=_desc(tr.DESC), upload=False)}
        self.stats, self.digest = self.index["host"].stats(), self.index["host"].digest()
        self.index["device"], self.report = _device_build(tr.DESC, blob=self.blob, offs=self.offs)
        self.device_stats, self.device_digest = self.index["device"].stats(), self.index["device"].digest()

    @staticmethod
    def _frozen(arrays):
        for a in arrays:
            a.setflags(write=False)
        return arrays

    def uploaded(self, build):
        return self.index[build].upload()          # (a second upload to the device is a no-op)


@pytest.fixture(scope="module")
def rich():
    r = _Rich()
    yield r
    for ix in r.index.values():
        ix.close()


def test_the_table_grows_once_at_full_size(rich):
    """524 289 terms overflow the 2^20 table: one repeat at 2^22, and the host build's arrays"""
    assert rich.report == dict(passes=2, log2_table=22, terms=691501, long_docs=0)
    assert rich.device_stats == rich.stats and rich.stats["n_terms"] == 691501 and rich.stats["n_segments"] == 10
    assert rich.device_digest == rich.digest


def test_the_companion_fills_the_first_table():
    """516 917 terms: the 2^20 table at load 0.49, probe chains of some length, no growth"""
    from suggest_amd import NGramIndex
    blob, offs = tr.pack(tr.term_rich(120000))
    host = NGramIndex(blob=blob, offs=offs, description=_desc(tr.DESC), upload=False)
    dev, report = _device_build(tr.DESC, blob=blob, offs=offs)
    assert report == dict(passes=1, log2_table=20, terms=516917, long_docs=0)
    assert dev.stats() == host.stats() and dev.digest() == host.digest()
    host.close()
    dev.close()


@pytest.mark.parametrize("g8", [0, 1])
def test_derived_arrays_with_high_term_ids(monkeypatch, rich, g8):
    """numbering, packed store, rows, cut_sample and forward index of the upload, word for word (tests/packed_ref.py)"""
    from suggest_amd import NGramIndex
    monkeypatch.setenv("SG_G8", str(g8))
    ix = NGramIndex(blob=rich.blob, offs=rich.offs, description=_desc(tr.DESC))
    assert ix.digest() == rich.digest
    ref, dev = pr.check_index(ix, g8)
    terms = dev.fwd_terms[dev.fwd_terms != pr.NO_TERM]
    assert int(terms.max()) == rich.stats["n_terms"] - 1 and int((terms >= tr.HIGH_TERM).sum()) > 100000
    ix.close()


@pytest.mark.parametrize("launch", SEARCH_LAUNCHES)
@pytest.mark.parametrize("build", ["host", "device"])
def test_rows_are_the_oracles(rich, build, launch):
    """build_term_table at 2^21 slots and d_term_lookup at that load; term ids above 2^19 through the forward index, the store,
    the rows and the verify launch's hash — 457 to 582 rows of each call hold a document with such a term"""
    knobs, pipeline, _ = LAUNCHES[launch]
    gpu = rich.uploaded(build)
    assert 1 << 20 < 2 * rich.stats["n_terms"] <= 1 << 21            # build_term_table: load <= 0.5, so 2^21 slots
    try:
        gpu.tune(**knobs)
        for call in tr.CALLS:
            before = gpu.pipe_stats()["queries"]
            got = gpu.suggest_batch(blob=rich.packed[0], offs=rich.packed[1], metric=call[0], similarity=call[1], k=call[2])
            grew = gpu.pipe_stats()["queries"] - before
            assert_same(got, rich.want[call], rich.queries)
            assert grew == (len(rich.queries) if pipeline else 0), (build, launch, call)      # the launch ran the path it is here for
        pb, po = rich.packed_prefixes
        for limit in (7, 80):
            ids, cnt = gpu.autocomplete_batch(blob=pb, offs=po, limit=limit)
            oi, oc = rich.want_auto[limit]
            bad = np.nonzero(cnt != oc)[0]
            assert bad.size == 0, (limit, [rich.prefixes[i] for i in bad[:5]], cnt[bad[:5]], oc[bad[:5]])
            valid = np.arange(limit)[None, :] < np.minimum(oc, limit)[:, None]
            rows = np.nonzero((valid & (ids != oi)).any(axis=1))[0]
            assert rows.size == 0, (limit, [rich.prefixes[i] for i in rows[:5]])
    finally:
        gpu.tune(**DEFAULTS)


# ---- refusals ----------------------------------------------------------------------------------------------------------------------
def _builder_still_works():
    docs = tr.one_term_documents(9)
    assert _same_as_host(tr.TABLE_DESC, docs, 0)["passes"] == 1


def test_refuses_terms_x_segments_past_the_sort_key():
    """about 119 000 terms x 41 000 segments: sort keys term * S + segment would wrap"""
    docs = tr.refusal_sort_key()
    with pytest.raises(Exception, match="32-bit sort key"):
        _device_build(tr.SORT_KEY_DESC, docs)
    _builder_still_works()


def test_refuses_more_repeating_documents_than_the_side_list_holds():
    """8 500 000 documents "a-a+" ($a$ a$a $a$ a$$: each repeats a term) against the side list's 2^23 entries.  ("aaaa" repeats
    none: the tokeniser keeps an n-gram once; only normalisation makes two n-grams one term.)"""
    from suggest_amd import synth
    n = 8500000
    assert n > 1 << 23 and len(tr.REPEATS_A_TERM) == 4
    with pytest.raises(Exception, match="repeated terms"):
        _device_build(synth.DESCRIPTION, blob=np.tile(np.frombuffer(tr.REPEATS_A_TERM, dtype=np.uint8), n), offs=np.arange(n + 1, dtype=np.uint64) * 4)
    _builder_still_works()


def test_refuses_2_to_the_26_documents():
    n = 1 << 26
    with pytest.raises(Exception, match=r"2\^26"):
        _device_build(tr.DESC, blob=np.zeros(0, dtype=np.uint8), offs=np.zeros(n + 1, dtype=np.uint64))
    _builder_still_works()
