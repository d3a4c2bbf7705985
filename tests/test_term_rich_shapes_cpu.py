"""The inputs of tests/term_rich_shapes.py against the CPU oracle and plain Python alone (no GPU): the dictionary has the terms,
and the queries the rows, that tests/test_gpu_term_rich.py is about — otherwise the device builder's table would not grow, no
query would touch a term id above 2^19, or a comparison would pass over empty rows.  Then the host build — the reference of the
device builder's tests — against a plain numpy restatement of the CSR, array for array over the whole index.

Bounds, and what this generator gives:
  term_rich(180000): distinct 4-grams >= 600 000 and above the 2^20 table's 524 289      691 501 (a Python set and numpy agree)
                     capacity / 16 < 2^20 (the table starts at 2^20)                    2 039 964 / 16
                     segments == 10                                                      10
  term_rich(120000): 450 000 <= terms <= 524 288 (the 2^20 table takes them)             516 917
  per call of CALLS: rows with an entry >= 0.8                                           0.886, 0.939, 0.886
                     rows with two >= 0.15 / 0.30 / 0.15                                 0.221, 0.420, 0.220
                     flagged == 0                                                        0, 0, 0
  queries whose row holds a document with a term id above 2^19 >= 200                    457, 582, 457
"""
import numpy as np
import pytest

import oracle
import packed_ref as pr
import term_rich_shapes as tr


@pytest.fixture(scope="module")
def docs():
    return tr.term_rich()


@pytest.fixture(scope="module")
def plain(docs):
    ref = tr.plain_csr(docs)
    for a in (ref.postings, ref.seg_off, ref.doc, ref.cell, ref.max_term):
        a.setflags(write=False)
    return ref


@pytest.fixture(scope="module")
def host(docs):
    from suggest_amd import IndexDescription, NGramIndex
    ix = NGramIndex(docs, IndexDescription(**tr.DESC), upload=False)
    yield ix
    ix.close()


def test_the_dictionary_outgrows_the_builders_first_table(docs, plain):
    assert len(docs) == 240000 and all(3 <= len(d) <= 10 for d in docs)
    terms = set()
    for d in docs:
        w = b"$" + d + b"$"
        terms.update(w[i:i + 4] for i in range(len(w) - 3))
    print("documents", len(docs), "distinct 4-grams", len(terms), "capacity", tr.capacity(docs), "segments", plain.S)
    assert len(terms) == plain.n_terms == 691501
    assert len(terms) >= 600000 and len(terms) > tr.first_overflow(tr.DEFAULT_BITS) == (1 << 20 >> 1) + 1
    assert len(terms) <= 1 << 22 >> 1                             # the second table takes them: exactly one growth
    assert tr.capacity(docs) == 2039964 and tr.capacity(docs) // 16 < 1 << tr.DEFAULT_BITS
    assert plain.S == 10
    assert int((plain.max_term >= tr.HIGH_TERM).sum()) > 50000      # documents the forward index gives a term id above 2^19


def test_the_companion_fills_the_first_table_without_growing_it():
    comp = tr.term_rich(120000)
    g = tr.grams(comp)[0]
    n = int(np.unique(g).size)
    print("companion: documents", len(comp), "terms", n)
    assert len(comp) == 160000 and n == 516917
    assert 450000 <= n <= 524288 < tr.first_overflow(tr.DEFAULT_BITS)
    assert tr.capacity(comp) // 16 < 1 << tr.DEFAULT_BITS


def test_oracle_rows_are_worth_comparing(docs, plain):
    ora = oracle.OracleIndex(docs, **tr.DESC)
    assert ora.n_segments == 10
    qs = tr.queries(docs)
    known = set(docs)
    assert len(qs) == tr.N_QUERIES and sum(1 for q in qs if q not in known) >= 600      # (750: the odd picks, less the short and the unchanged)
    qb, qo = oracle.pack_strings(qs)
    for call, min2 in zip(tr.CALLS, tr.MIN_ROWS_2):
        ids, _, cnt, _ = ora.suggest_batch(qb, qo, *call)
        valid = np.arange(call[2])[None, :] < cnt[:, None]
        high = int((valid & (plain.max_term[ids] >= tr.HIGH_TERM)).any(axis=1).sum())
        print(call, "rows >= 1: %.3f" % (cnt >= 1).mean(), "rows >= 2: %.3f" % (cnt >= 2).mean(), "flagged", int((cnt >= 0xFFFFFFF0).sum()),
              "longest", int(cnt.max()), "rows with a term id above 2^19:", high)
        assert not (cnt >= 0xFFFFFFF0).any()
        assert (cnt >= 1).mean() >= 0.8 and (cnt >= 2).mean() >= min2
        assert high >= 200
    pre = tr.prefixes(qs)
    assert len(pre) == 256 and {len(p) for p in pre} == {2, 3, 4, 5}
    cnt = ora.autocomplete_batch(*oracle.pack_strings(pre), 80)[1]
    assert (cnt >= 1).mean() >= 0.7 and (cnt > 7).sum() >= 10       # some rows end at limit 7, none at 80
    assert cnt.max() < 80


def test_host_build_is_the_plain_restatement(host, plain, docs):
    """Term ids by first appearance, every (term, segment) list the ascending docIDs padded to four with the last one, seg_off in
    16-byte chunks: the raw arrays as integers, and the postings packed_ref.derive decodes from them."""
    st = host.stats()
    assert (st["n_docs"], st["n_terms"], st["n_segments"]) == (len(docs), plain.n_terms, plain.S)
    assert st["n_postings"] == st["n_postings_raw"] == plain.doc.size       # (no document repeats a term)
    hp, hso = host.raw_array("host_postings"), host.raw_array("host_seg_off")
    tr.compare_csr(hp, hso, plain)
    ref = pr.derive(hp, hso, len(docs), plain.S, plain.n_terms, 0)
    assert np.array_equal(ref.vp, plain.doc) and np.array_equal(ref.vl, plain.cell)
    assert int(ref.doc_terms[1].max()) == plain.n_terms - 1 and (ref.doc_terms[1] >= tr.HIGH_TERM).sum() > 100000
    # the numbering itself: the keys of the terms in id order are the n-grams in order of first appearance
    keys = pr.term_keys(host)
    g = tr.grams(docs)[0]
    first = g[np.sort(np.unique(g, return_index=True)[1])]
    for t in (0, 1, tr.HIGH_TERM, plain.n_terms - 1):
        assert host.term_string(int(keys[t])) == int(first[t]).to_bytes(4, "big"), t


def test_the_comparison_can_fail(host, plain):
    """one posting moved to a neighbouring list — of the next segment, of the next term — is reported, with its row"""
    hp, hso = host.raw_array("host_postings"), host.raw_array("host_seg_off")
    S = plain.S
    length = np.bincount(plain.cell, minlength=plain.n_terms * S)
    # a list of one posting in front of an empty one of the same term: its chunk handed to the next segment
    one = np.flatnonzero((length[:-1] == 1) & (length[1:] == 0) & (np.arange(length.size - 1) % S != S - 1))
    l = int(one[one >= tr.HIGH_TERM * S][0])
    row = l // S * (S + 1) + l % S + 1
    moved = hso.copy()
    moved[row] -= 1
    with pytest.raises(AssertionError, match=r"seg_off row %d \(term %d, segment %d\)" % (row, l // S, l % S + 1)):
        tr.compare_csr(hp, moved, plain)
    # the last posting of a full chunk exchanged for the first of the next list
    full = np.flatnonzero((length[:-1] == 4) & (length[1:] >= 1))
    at = int(plain.seg_off[full[0] // S * (S + 1) + full[0] % S]) * 4 + 3
    swapped = hp.copy()
    swapped[at], swapped[at + 1] = hp[at + 1], hp[at]
    assert swapped[at] != hp[at]
    with pytest.raises(AssertionError, match=r"posting %d \(chunk %d\)" % (at, at // 4)):
        tr.compare_csr(swapped, hso, plain)
    tr.compare_csr(hp, hso, plain)


def test_small_dictionaries_stand_where_they_are_meant_to():
    """16 slots: eight one-term documents fit, the ninth flags; the long documents; the empty pad's terms"""
    import long_query_shapes as lq
    assert tr.first_overflow(tr.SMALL_BITS) == 9
    for n in (8, 9):
        d = tr.one_term_documents(n)
        ora = oracle.OracleIndex(d, **tr.TABLE_DESC)
        assert len({ora.tokenize(x)[0] for x in d}) == n and all(len(ora.tokenize(x)) == 1 for x in d)
    d = tr.long_documents()
    ora = oracle.OracleIndex(d, **tr.LONG_DESC)
    n_long = sum(lq.is_long(ora, tr.LONG_DESC, x) for x in d)
    assert len(d) == 305 and n_long == 4 and sum(len(ora.tokenize(x)) > 128 for x in d) == 3
    assert len({t for x in d for t in ora.tokenize(x)}) > 1 << 10 >> 1       # 16, 64, 256, 1 024 slots overflow: five passes at least
    d = tr.empty_pad_documents()
    ora = oracle.OracleIndex(d, **tr.EMPTY_PAD_DESC)
    terms = {t for x in d for t in ora.tokenize(x)}
    assert b"" in terms and len(terms) == 12
    assert mix64_is_splitmix()
    big = tr.refusal_sort_key()
    assert len(big) == 80001 and len(big[0]) == 65000 and len(set(big)) == 80001
    ora = oracle.OracleIndex(big[1:4], **tr.SORT_KEY_DESC)

    def windows(x):
        w = "$" + x.decode("utf-8") + "$"
        return {w[i:i + 3].encode("utf-8") for i in range(len(w) - 2)}

    head = big[0][:3000].decode("utf-8", "ignore").encode("utf-8")      # (the oracle's dedup is quadratic: a part of the long one)
    for x in (head, big[1], big[-1]):
        assert set(ora.tokenize(x)) == windows(x) and len(ora.tokenize(x)) == len(windows(x))
    S = len(windows(big[0])) + 1                                        # cardinality = the distinct n-grams
    terms = set().union(*(windows(x) for x in big))
    print("sort-key refusal: terms", len(terms), "segments", S, "product", len(terms) * S)
    assert len(terms) * S >= 0xFFFFFFF0 and S <= 0xFFFF
    ora = oracle.OracleIndex([tr.REPEATS_A_TERM], **tr.LONG_DESC)
    assert ora.tokenize(tr.REPEATS_A_TERM) == [b"$a$", b"a$a", b"$a$", b"a$$"] and len(set(ora.tokenize(b"aaaa"))) == 3 == len(ora.tokenize(b"aaaa"))


def mix64_is_splitmix():
    """the restated hash against the vectorised statement of the same finaliser in suggest_amd/synth.py"""
    from suggest_amd import synth
    xs = [0, 1, 0x6162, 0x24616263, (1 << 64) - 1, 0x0123456789ABCDEF]
    return [tr.mix64(x) for x in xs] == [int(v) for v in synth._mix(np.array(xs, dtype=np.uint64))]
