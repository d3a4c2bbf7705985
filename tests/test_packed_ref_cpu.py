"""The checker of tests/packed_ref.py can fail: a small CSR is encoded with the restatement itself, passes, and is then corrupted
one way at a time — every corruption a subtly wrong build kernel could produce without changing a search row must be reported.
(tests/test_gpu_store.py runs the same checker on what the kernels built.)"""
import copy
import re

import numpy as np
import pytest

import packed_ref as pr

N_DOCS, S, SPLIT = 170000, 4, 100000      # documents below SPLIT have cardinality 2, the others 3: x == docID
T_ALL, T_EDGE, T_RUNS, T_SPARSE, T_ONE = 0, 1, 2, 3, 4
N_TERMS = 5


@pytest.fixture(scope="module")
def csr():
    rnd = np.random.RandomState(5)
    lists = {(T_ALL, 2): range(0, SPLIT), (T_ALL, 3): range(SPLIT, N_DOCS),         # dense: 8-bit gaps pay
             (T_EDGE, 2): [10, 10 + 65535, 20 + 65535], (T_EDGE, 3): [SPLIT, SPLIT + 65536, SPLIT + 65537],
             # 20 at gap 1, then 300 further on 9 more (a forced 8-bit break, none with 16-bit gaps), then gaps of 255 and 256
             (T_RUNS, 2): list(range(1000, 1020)) + list(range(1319, 1328)) + [1327 + 255, 1327 + 255 + 256, 1327 + 255 + 257],
             (T_SPARSE, 2): sorted(rnd.choice(SPLIT, size=150, replace=False).tolist()),
             (T_SPARSE, 3): sorted((SPLIT + rnd.choice(N_DOCS - SPLIT, size=41, replace=False)).tolist()),
             (T_ONE, 2): [0]}
    hp, hso = pr.make_csr(N_TERMS, S, lists)
    return hp, hso


def _store(csr, mode, **kw):
    return pr.derive(csr[0], csr[1], N_DOCS, S, N_TERMS, mode, **kw)


def _check(dev, csr, mode):
    return pr.check(dev, csr[0], csr[1], N_DOCS, S, N_TERMS, mode, term_name=lambda t: "t%d" % t)


def _chunks(st, t, b):
    off = st.seg_off & 0x7FFFFFFF
    return range(int(off[t * (S + 1) + b]), int(off[t * (S + 1) + b + 1]))


@pytest.mark.parametrize("mode", [0, 1, 2])
def test_the_restatement_passes_its_own_checker(csr, mode):
    st = _store(csr, mode)
    ref = _check(st, csr, mode)
    assert np.array_equal(ref.x_of, np.arange(N_DOCS))                       # one numbering here: gaps below are docID gaps
    gaps = np.diff(ref.x[ref.vl == T_EDGE * S + 2]).tolist() + np.diff(ref.x[ref.vl == T_EDGE * S + 3]).tolist()
    assert gaps == [65535, 10, 65536, 1]
    flags = (st.seg_off >> 31).reshape(N_TERMS, S + 1)
    if mode == 0:
        assert not flags.any()
    elif mode == 2:
        assert flags.all()
    else:     # the dense term and the runs gain, the sparse terms would only lose
        assert flags.all(axis=1).tolist() == [True, False, True, False, False]
    # 65 535 stays in its chunk, 65 536 starts one
    assert len(_chunks(st, T_EDGE, 2)) == (1 if mode < 2 else 2) and len(_chunks(st, T_EDGE, 3)) == 2


def test_a_saving_below_three_percent_keeps_one_format():
    # 40 sparse lists and one short dense one: 8-bit gaps would save the dense term 1 chunk of 42
    lists = {(t, 1): [t, 1000 + 300 * t] for t in range(40)}
    lists[(40, 1)] = list(range(500, 510))
    hp, hso = pr.make_csr(41, 2, lists)
    st = pr.derive(hp, hso, 20000, 2, 41, 1)
    assert st.s8[40] < st.s16[40] and not st.want_fmt.any() and not (st.seg_off >> 31).any()
    pr.check(st, hp, hso, 20000, 2, 41, 1)
    st2 = pr.derive(hp, hso, 20000, 2, 41, 1, fmt=np.arange(41) == 40)        # valid, decodable — and not what SG_G8=1 chooses
    with pytest.raises(pr.StoreMismatch, match="format is 8-bit"):
        pr.check(st2, hp, hso, 20000, 2, 41, 1)


def _u16(st, c):
    return st.packed[c:c + 1].view(np.uint16)[0]


def drop_a_posting(st, csr):
    c = _chunks(st, T_SPARSE, 2)[0]                 # a full 16-bit chunk: 7 -> 6 postings
    assert st.packed[c, 0] >> 29 == 6
    st.packed[c, 0] -= 1 << 29
    _u16(st, c)[7] = pr.PAD_GAP


def change_a_gap(st, csr):
    _u16(st, _chunks(st, T_SPARSE, 3)[1])[4] += 1


def count_field_too_large(st, csr):
    c = _chunks(st, T_EDGE, 3)[1]                   # 2 postings
    assert st.packed[c, 0] >> 29 == 1
    st.packed[c, 0] += 1 << 29


def count_field_too_small(st, csr):
    st.packed[_chunks(st, T_EDGE, 3)[1], 0] -= 1 << 29


def padding_gap_of_zero(st, csr):
    _u16(st, _chunks(st, T_EDGE, 3)[1])[7] = 0


def padding_gap_of_zero_8bit(st, csr):
    c = _chunks(st, T_RUNS, 2)[-1]
    assert (st.packed[c, 0] >> 28) < 12
    st.packed[c:c + 1].view(np.uint8)[0, 15] = 0


def cut_sample_shifted(st, csr):
    assert st.packed[17, 0] != st.packed[16, 0]
    st.cut_sample[1] = st.packed[17, 0] & pr.X_MASK8      # (chunks 16, 17: the dense 8-bit term)


def cut_sample_behind_the_store(st, csr):
    st.cut_sample[-1] = 0


def flag_bit_missing(st, csr):
    st.seg_off[T_RUNS * (S + 1) + 3] &= 0x7FFFFFFF


def two_documents_swapped(st, csr):
    st.orig_of[[5, 6]] = st.orig_of[[6, 5]]


def forward_term_replaced(st, csr):
    x = 1005                                         # holds T_ALL and T_RUNS
    w = st.fwd_terms[st.fwd_rec[x, 0]]
    assert sorted(w[:2].tolist()) == [T_ALL, T_RUNS]
    w[1] = T_SPARSE if w[1] == T_RUNS else w[1]
    w[0] = T_SPARSE if w[0] == T_RUNS else w[0]


def forward_padding_overwritten(st, csr):
    st.fwd_terms[st.fwd_rec[77, 0], 3] = T_ONE


def wrong_distinct_count(st, csr):
    st.fwd_rec[1005, 1] += 1 << 16


def wrong_cardinality(st, csr):
    st.fwd_rec[1005, 1] += 1


def wrong_stride_address(st, csr):
    st.fwd_rec[SPLIT + 1, 0] += 1


def slack_row_not_zero(st, csr):
    st.packed[-1, 2] = 7


IN_PLACE = [
    (drop_a_posting, r"t3', segment 2\): 149 postings in the store, 150 in the CSR"),
    (change_a_gap, r"chunk 1 of list \(term 3 't3', segment 3\).*decodes to x = "),
    (count_field_too_large, r"t1', segment 3\): 4 postings in the store, 3 in the CSR"),
    (count_field_too_small, r"chunk 1 of list \(term 1 't1', segment 3\).*padding slot 0 holds a gap of 1, not 41"),
    (padding_gap_of_zero, r"chunk 1 of list \(term 1 't1', segment 3\).*padding slot 5 holds a gap of 0, not 41"),
    (padding_gap_of_zero_8bit, r"list \(term 2 't2', segment 2\).*padding slot 11 holds a gap of 0, not 41"),
    (cut_sample_shifted, r"cut_sample\[1\] = .*the first x of chunk 16 of list \(term 0 't0', segment 2\)"),
    (cut_sample_behind_the_store, r"cut_sample\[\d+\] = 0x0, behind the store"),
    (flag_bit_missing, r"term 2 't2': the 8-bit flag \(bit 31\) is set on 4 of its 5 seg_off entries \(entry of segment 3"),
    (two_documents_swapped, r"orig_of\[5\] = 6, the restatement has 5"),
    (forward_term_replaced, r"forward index, document x = 1005 \(docID 1005\): term ids \[0, 3, "),
    (forward_padding_overwritten, r"forward index, document x = 77 "),
    (wrong_distinct_count, r"document x = 1005 \(docID 1005\): 3 distinct terms, the CSR has it in 2 lists"),
    (wrong_cardinality, r"document x = 1005 \(docID 1005\): cardinality 3, the CSR has it in segment 2"),
    (wrong_stride_address, r"document x = 100001 .*its terms at chunk"),
    (slack_row_not_zero, r"slack row"),
]


@pytest.mark.parametrize("corrupt,message", IN_PLACE, ids=[c.__name__ for c, _ in IN_PLACE])
def test_a_corrupted_store_is_reported(csr, corrupt, message):
    st = copy.deepcopy(_store(csr, 1))
    _check(st, csr, 1)
    corrupt(st, csr)
    with pytest.raises(pr.StoreMismatch) as e:
        _check(st, csr, 1)
    assert re.search(message, str(e.value)), str(e.value)


REENCODED = [
    # valid, decodable stores that are not the format's
    ("a_term_in_the_costlier_format", dict(fmt=[True, False, False, False, False]), r"term 2 't2': format is 16-bit gaps, SG_G8=1 chooses 8-bit \(its chunks: 5 with 16-bit gaps, 4 with 8-bit"),
    ("a_sparse_term_in_the_costlier_format", dict(fmt=[True, False, True, True, False]), r"term 3 't3': format is 8-bit gaps, SG_G8=1 chooses 16-bit"),
    ("an_extra_break_at_65535", dict(gap_max=65534), r"list \(term 1 't1', segment 2\): 2 chunks, the format needs 1"),
    ("a_missing_break_at_65536", dict(gap_max=65536), r"list \(term 1 't1', segment 3\): 1 chunks, the format needs 2"),
    ("an_extra_break_at_255", dict(gap_max8=254), r"list \(term 2 't2', segment 2\): 5 chunks, the format needs 4"),
    ("a_missing_break_at_256", dict(gap_max8=256), r"list \(term 2 't2', segment 2\): 3 chunks, the format needs 4"),
]


@pytest.mark.parametrize("name,how,message", REENCODED, ids=[r[0] for r in REENCODED])
def test_a_store_that_breaks_elsewhere_is_reported(csr, name, how, message):
    st = _store(csr, 1, **how)
    with pytest.raises(pr.StoreMismatch) as e:
        _check(st, csr, 1)
    assert re.search(message, str(e.value)), str(e.value)


def test_a_shifted_boundary_with_the_same_chunk_count_is_reported(csr):
    """The 8-bit run of 20 postings at gap 1 is chunks of 13 + 7.  8 + 12 holds the same postings in as many chunks, every word of
    it well-formed: only the comparison of the boundaries themselves refuses it."""
    st = copy.deepcopy(_store(csr, 1))
    c = _chunks(st, T_RUNS, 2)[0]
    a, b = st.packed[c:c + 1].view(np.uint8)[0], st.packed[c + 1:c + 2].view(np.uint8)[0]
    assert st.packed[c, 0] >> 28 == 12 and st.packed[c + 1, 0] >> 28 == 6 and st.packed[c, 0] & pr.X_MASK8 == 1000
    # move the last five postings of the first chunk into the second: 8 + 12
    st.packed[c, 0] = 1000 | 7 << 28
    a[4 + 7:] = pr.PAD_GAP
    st.packed[c + 1, 0] = 1008 | 11 << 28
    b[4:4 + 11] = 1
    with pytest.raises(pr.StoreMismatch, match=r"chunk boundary before posting 8 of the list"):
        _check(st, csr, 1)


def test_a_wrong_row_offset_is_reported(csr):
    st = copy.deepcopy(_store(csr, 0))
    st.seg_off[T_ONE * (S + 1) + 1] += 1          # an empty row that claims a chunk of its neighbour
    with pytest.raises(pr.StoreMismatch, match=r"list \(term 4 't4', segment 0\): 1 chunks, the format needs 0"):
        _check(st, csr, 0)


def test_more_than_63_segments_take_the_sparse_layout():
    lists = {(0, 70): [0, 2], (1, 70): [1, 2], (2, 3): [3], (0, 3): [3]}
    hp, hso = pr.make_csr(3, 71, lists)
    st = pr.derive(hp, hso, 4, 71, 3, 0)
    assert st.fx_base.size == 0 and not st.strided
    pr.check(st, hp, hso, 4, 71, 3, 0)
    bad = copy.deepcopy(st)
    bad.fwd_rec[2, 0] = bad.fwd_rec[1, 0]
    with pytest.raises(pr.StoreMismatch, match="overlap"):
        pr.check(bad, hp, hso, 4, 71, 3, 0)
    bad = copy.deepcopy(st)
    bad.fwd_rec[3, 0] = 9
    with pytest.raises(pr.StoreMismatch, match="outside fwd_terms"):
        pr.check(bad, hp, hso, 4, 71, 3, 0)
    st63 = pr.derive(hp[:0], np.zeros(2 * 64 + 1, dtype=np.uint32), 1, 63, 2, 0)
    assert st63.strided and st63.fx_base.size == 64


def test_the_read_back_hook_serves_the_host_csr_without_a_gpu(cars_lines):
    """sg_debug_index_array: the host CSR's two arrays need no upload and, read through valid_postings, are the lists that
    sg_index_list hands out one by one; a replica's arrays before an upload and an unknown selector are SG_E_INVALID with a message."""
    import ctypes as C
    from conftest import CARS_DESC
    from suggest_amd import NGramIndex, IndexDescription, _lib
    ix = NGramIndex(cars_lines[:400], IndexDescription(**CARS_DESC), upload=False)
    st = ix.stats()
    S, n_terms = st["n_segments"], st["n_terms"]
    hp, hso = ix.raw_array("host_postings"), ix.raw_array("host_seg_off")
    assert hp.size * 4 == st["posting_bytes"] and hso.size == n_terms * (S + 1) + 1
    vp, vl = pr.valid_postings(hp, hso, n_terms, S)
    keys = pr.term_keys(ix)
    got = {}
    for d, l in zip(vp.tolist(), vl.tolist()):
        got.setdefault((l % S, ix.term_string(int(keys[l // S]))), []).append(d)
    assert got == {k: v[1] for k, v in ix.lists().items()}
    for name in ("packed", "seg_off", "orig_of", "x_of", "seg_base", "cut_sample", "fwd_rec", "fwd_terms", "fx_base"):
        with pytest.raises(_lib.SuggestHipError, match="not uploaded"):
            ix.raw_array(name)
    n, small = C.c_uint64(), np.zeros(4, dtype=np.uint32)
    with ix._use() as h:
        assert _lib.lib().sg_debug_index_array(h, 0, 11, None, 0, C.byref(n)) < 0 and b"unknown array" in _lib.lib().sg_last_error()
        with pytest.raises(_lib.SuggestHipError, match="buffer too small"):
            _lib.check(_lib.lib().sg_debug_index_array(h, 0, 9, small.ctypes.data, small.nbytes, C.byref(n)))
    assert n.value == hp.nbytes and not small.any()
