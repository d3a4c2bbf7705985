"""A second statement of what an upload derives on the GPU from the host CSR, and a checker of a replica's raw arrays against it.

numpy only, vectorised over the flat arrays.  Written from the formats as suggest_amd/csrc/packed_store.inc, forward_index.inc and
the SG_PPC / SG_X_MASK / SG_PAD_GAP lines of engine.hip state them — not from the kernels:

  numbering   orig_of = the documents in stable order of cardinality, x_of its inverse, seg_base[b] = documents of cardinality < b
  store       a list (term, segment) = the valid postings of its host row (the padding repeats the last docID), mapped through x_of;
              a chunk = 16 bytes: {u32 first x | (postings - 1) << 29, 6 x u16 gaps} (7 postings) or, for an 8-bit term,
              {u32 first x | (postings - 1) << 28, 12 x u8 gaps} (13 postings); a new chunk starts at a list's first posting, at a
              gap above 65 535 (255) and after 7 (13) postings of a run — nowhere else; the slots behind the count hold gaps of 41
  seg_off     exclusive scan of the rows' chunk counts (a term has S + 1 rows, the last counts 0), bit 31 on the rows of 8-bit terms
  format      SG_G8 = 0 none, 2 every term with a posting, 1 the terms with fewer 8-bit chunks — unless that saves less than 3 %
  cut_sample  the first x of every 16th chunk, 0xFFFFFFFF behind
  forward     fwd_rec[x] = {first chunk of the document's term ids, cardinality | distinct << 16}; the ids padded with 0xFFFFFFFF;
              at most 63 segments: chunk fx_base[B] + (x - seg_base[B]) * ceil(B / 4), fx_base the scan of the segments' sizes x strides

check() raises StoreMismatch naming the first differing row (term, segment, chunk).  tests/test_packed_ref_cpu.py shows that it
can fail; tests/test_gpu_store.py runs it on what the kernels built.
"""
import sys
from types import SimpleNamespace

import numpy as np

PPC, PPC8 = 7, 13
X_MASK, X_MASK8 = 0x1FFFFFFF, 0x0FFFFFFF
PAD_GAP = 41
GAP_MAX, GAP_MAX8 = 65535, 255
G8_FLAG = 0x80000000
NO_TERM = 0xFFFFFFFF
SLACK = 64          # zeroed chunks behind the store
assert sys.byteorder == "little"      # (the u16 / u8 views of a chunk's words below)


class StoreMismatch(AssertionError):
    pass


def make_csr(n_terms, S, lists):
    """{(term, segment): ascending docIDs} -> (postings, seg_off) in the host format: term-major rows of 4-posting chunks, a list
    padded to a whole chunk with its last docID, seg_off in chunks with S + 1 entries per term (+ one at the end)."""
    seg_off = np.zeros(n_terms * (S + 1) + 1, dtype=np.uint32)
    out, chunk = [], 0
    for t in range(n_terms):
        for b in range(S):
            seg_off[t * (S + 1) + b] = chunk
            docs = list(lists.get((t, b), ()))
            if docs:
                docs += [docs[-1]] * (-len(docs) % 4)
                out.extend(docs)
                chunk += len(docs) // 4
        seg_off[t * (S + 1) + S] = chunk
    seg_off[-1] = chunk
    return np.array(out, dtype=np.uint32), seg_off


def valid_postings(host_postings, host_seg_off, n_terms, S):
    """-> (docIDs, list ids = term * S + segment) of every real posting of the host CSR, in store order"""
    so = host_seg_off[:n_terms * (S + 1)].astype(np.int64).reshape(n_terms, S + 1)
    start, end = so[:, :S].ravel() * 4, so[:, 1:].ravel() * 4
    # (the rows follow each other without a hole: a term's last row ends where the next term begins)
    assert start.size == 0 or (start[0] == 0 and np.array_equal(start[1:], end[:-1])), "host rows are not contiguous"
    list_of = np.repeat(np.arange(n_terms * S, dtype=np.int64), end - start)
    p = host_postings[:list_of.size].astype(np.int64)
    valid = np.ones(p.size, dtype=bool)
    valid[1:] = (list_of[1:] != list_of[:-1]) | (p[1:] != p[:-1])
    return p[valid], list_of[valid]


def numbering(card, S):
    orig_of = np.argsort(card, kind="stable").astype(np.uint32)
    x_of = np.empty(card.size, dtype=np.uint32)
    x_of[orig_of] = np.arange(card.size, dtype=np.uint32)
    seg_base = np.searchsorted(card[orig_of], np.arange(S + 1), side="left").astype(np.uint32)
    return orig_of, x_of, seg_base


def chunk_starts(x, vl, g8, gap_max=GAP_MAX, gap_max8=GAP_MAX8):
    """-> (starts a chunk [n] bool, gap to the previous posting [n]) for the postings x of lists vl, g8 [n] bool: 8-bit gaps"""
    n = x.size
    idx = np.arange(n, dtype=np.int64)
    gap = np.zeros(n, dtype=np.int64)
    gap[1:] = x[1:] - x[:-1]
    brk = np.ones(n, dtype=bool)
    brk[1:] = (vl[1:] != vl[:-1]) | (gap[1:] > np.where(g8[1:], gap_max8, gap_max))
    pos = idx - np.maximum.accumulate(np.where(brk, idx, 0))            # position in the run since the last forced break
    return pos % np.where(g8, PPC8, PPC) == 0, gap


def choose_format(s16, s8, g8_mode, n_docs, n_lists):
    """-> [n_terms] bool: the term's lists take 8-bit gaps (s16 / s8: its chunks either way)"""
    f = np.zeros(s16.size, dtype=bool)
    if g8_mode == 0 or n_lists == 0 or n_docs + PPC8 * PAD_GAP > X_MASK8:
        return f
    f = s8 > 0 if g8_mode == 2 else s8 < s16
    if g8_mode == 1 and float(np.where(f, s8, s16).sum()) > 0.97 * float(s16.sum()):     # saves less than 3 %: one format
        f = np.zeros(s16.size, dtype=bool)
    return f


def encode(x, vl, g8, n_terms, S, fmt, gap_max=GAP_MAX, gap_max8=GAP_MAX8):
    """-> (packed [chunks + SLACK, 4] u32, seg_off [n_terms * (S + 1)] u32 with flags, cut_sample, chunk starts [n] bool)"""
    n = x.size
    cstart, gap = chunk_starts(x, vl, g8, gap_max, gap_max8)
    idx = np.arange(n, dtype=np.int64)
    chunk_of = np.cumsum(cstart) - 1
    total = int(chunk_of[-1]) + 1 if n else 0
    slot = idx - np.maximum.accumulate(np.where(cstart, idx, 0))
    cnt = np.bincount(chunk_of, minlength=total).astype(np.int64)
    g8c = g8[cstart]
    packed = np.zeros((total + SLACK, 4), dtype=np.uint32)
    body = packed[:total]
    b16, b8 = body.view(np.uint16), body.view(np.uint8)
    b16[~g8c, 2:] = PAD_GAP
    b8[g8c, 4:] = PAD_GAP
    m = ~cstart & ~g8
    b16[chunk_of[m], 1 + slot[m]] = (gap[m] & 0xFFFF).astype(np.uint16)
    m = ~cstart & g8
    b8[chunk_of[m], 3 + slot[m]] = (gap[m] & 0xFF).astype(np.uint8)
    body[:, 0] = (x[cstart] | ((cnt - 1) << np.where(g8c, 28, 29))).astype(np.uint32)
    rows = np.zeros((n_terms, S + 1), dtype=np.int64)
    rows[:, :S] = np.bincount(vl[cstart], minlength=n_terms * S).reshape(n_terms, S)
    seg_off = np.zeros(n_terms * (S + 1), dtype=np.int64)
    seg_off[1:] = np.cumsum(rows.ravel())[:-1]
    seg_off |= np.repeat(fmt, S + 1).astype(np.int64) << 31
    cut = np.full(total // 16 + 2, 0xFFFFFFFF, dtype=np.uint32)
    first_x = body[:, 0] & np.where(g8c, X_MASK8, X_MASK).astype(np.uint32)
    cut[:(total + 15) // 16] = first_x[::16]
    return packed, seg_off.astype(np.uint32), cut, cstart


def derive(host_postings, host_seg_off, n_docs, S, n_terms, g8_mode, fmt=None, gap_max=GAP_MAX, gap_max8=GAP_MAX8):
    """The whole resident index from the host CSR.  fmt / gap_max / gap_max8: a store that is NOT the format's (a term forced to
    the other format, breaks at another gap) for the tests of the checker."""
    vp, vl = valid_postings(host_postings, host_seg_off, n_terms, S)
    card = np.zeros(n_docs, dtype=np.int64)
    card[vp] = vl % max(S, 1)
    orig_of, x_of, seg_base = numbering(card, S)
    x, vt = x_of[vp].astype(np.int64), vl // max(S, 1)
    none, every = np.zeros(x.size, dtype=bool), np.ones(x.size, dtype=bool)
    s16 = np.bincount(vt[chunk_starts(x, vl, none)[0]], minlength=n_terms)
    s8 = np.bincount(vt[chunk_starts(x, vl, every)[0]], minlength=n_terms)
    want_fmt = choose_format(s16, s8, g8_mode, n_docs, n_terms * S)
    fmt = want_fmt if fmt is None else np.asarray(fmt, dtype=bool)
    packed, seg_off, cut, cstart = encode(x, vl, fmt[vt] if x.size else none, n_terms, S, fmt, gap_max, gap_max8)
    # forward index: a document's distinct terms = the host CSR inverted
    nd = np.bincount(vp, minlength=n_docs).astype(np.int64)
    order = np.lexsort((vt, x))
    y = (card | (nd << 16))[orig_of]
    B, ndx = y & 0xFFFF, y >> 16
    strided = 0 < n_docs and S <= 63
    if strided:
        stride = (np.arange(S + 1, dtype=np.int64) + 3) >> 2
        fx_base = np.zeros(S + 1, dtype=np.int64)
        fx_base[1:] = np.cumsum(np.diff(seg_base.astype(np.int64)) * stride[:S])
        strided = int(fx_base[S]) < 0xFFFFFFF0
    if strided:
        n_chunks = stride[B]
        at = fx_base[B] + (np.arange(n_docs) - seg_base.astype(np.int64)[B]) * n_chunks
        total = max(int(fx_base[S]), 1)
    else:       # (any disjoint layout will do: here the documents' lists one after the other in docID order)
        fx_base = np.zeros(0, dtype=np.int64)
        n_chunks = (ndx + 3) >> 2
        at_doc = np.zeros(n_docs, dtype=np.int64)
        at_doc[1:] = np.cumsum(n_chunks[x_of])[:-1] if n_docs else 0
        at = at_doc[orig_of]
        total = int(n_chunks.sum())
    fwd_terms = np.full((total, 4), NO_TERM, dtype=np.uint32)
    fx = x[order]
    first = np.zeros(n_docs + 1, dtype=np.int64)
    first[1:] = np.cumsum(ndx)
    fwd_terms.reshape(-1)[at[fx] * 4 + np.arange(fx.size) - first[fx]] = vt[order]
    return SimpleNamespace(packed=packed, seg_off=seg_off, cut_sample=cut, orig_of=orig_of, x_of=x_of, seg_base=seg_base,
                           fwd_rec=np.stack([at, y], axis=1).astype(np.uint32), fwd_terms=fwd_terms, fx_base=fx_base.astype(np.uint32),
                           # the truth the checker compares with (not arrays of the replica)
                           x=x, vl=vl, vp=vp, cstart=cstart, fmt=fmt, want_fmt=want_fmt, s16=s16, s8=s8, card=card, nd=nd,
                           doc_terms=(fx, vt[order], first), strided=bool(strided))


def _first(mask):
    return int(np.flatnonzero(mask.ravel())[0])


def check(dev, host_postings, host_seg_off, n_docs, S, n_terms, g8_mode, term_name=None, packed_chunks=None):
    """dev: the replica's raw arrays (attributes packed, seg_off, orig_of, x_of, seg_base, cut_sample, fwd_rec, fwd_terms, fx_base).
    Raises StoreMismatch at the first difference; returns the restatement (its totals: ref.s16.sum(), ref.packed)."""
    ref = derive(host_postings, host_seg_off, n_docs, S, n_terms, g8_mode)

    def name(t):
        return "term %d%s" % (t, " %r" % (term_name(t),) if term_name else "")

    def lst(l):
        return "%s, segment %d" % (name(int(l) // S), int(l) % S)

    def fail(msg):
        raise StoreMismatch(msg)

    # ---- numbering
    for what in ("orig_of", "x_of", "seg_base"):
        got, want = np.asarray(getattr(dev, what)), getattr(ref, what)
        if got.shape != want.shape:
            fail("%s has %d entries, %d expected" % (what, got.size, want.size))
        if not np.array_equal(got, want):
            i = _first(got != want)
            fail("%s[%d] = %d, the restatement has %d" % (what, i, got[i], want[i]))

    # ---- a term's format, then the rows
    n_rows = n_terms * (S + 1)
    seg_off = np.asarray(dev.seg_off)
    if seg_off.size != n_rows:
        fail("seg_off has %d entries, %d expected" % (seg_off.size, n_rows))
    flags = (seg_off >> 31).astype(bool).reshape(n_terms, S + 1)
    n_flag = flags.sum(axis=1)
    if ((n_flag != 0) & (n_flag != S + 1)).any():
        t = _first((n_flag != 0) & (n_flag != S + 1))
        odd = _first(flags[t] != (n_flag[t] * 2 > S + 1))
        fail("%s: the 8-bit flag (bit 31) is set on %d of its %d seg_off entries (entry of segment %d differs)" % (name(t), n_flag[t], S + 1, odd))
    got_fmt = n_flag > 0
    if not np.array_equal(got_fmt, ref.want_fmt):
        t = _first(got_fmt != ref.want_fmt)
        fail("%s: format is %s gaps, SG_G8=%d chooses %s (its chunks: %d with 16-bit gaps, %d with 8-bit gaps; all terms: %d, chosen %d)" % (
            name(t), "8-bit" if got_fmt[t] else "16-bit", g8_mode, "8-bit" if ref.want_fmt[t] else "16-bit", ref.s16[t], ref.s8[t],
            ref.s16.sum(), np.where(ref.want_fmt, ref.s8, ref.s16).sum()))
    off = (seg_off & 0x7FFFFFFF).astype(np.int64)
    want_off = (ref.seg_off & 0x7FFFFFFF).astype(np.int64)
    total = ref.packed.shape[0] - SLACK
    packed = np.asarray(dev.packed)
    if not np.array_equal(off, want_off):
        got_total = packed.shape[0] - SLACK
        n_got, n_want = np.diff(np.append(off, got_total)), np.diff(np.append(want_off, total))
        if (n_got != n_want).any():
            r = _first(n_got != n_want)
            fail("list (%s, segment %d): %d chunks, the format needs %d" % (name(r // (S + 1)), r % (S + 1), n_got[r], n_want[r]))
        r = _first(off != want_off)
        fail("seg_off row %d (%s, segment %d) = %d, the scan of the chunk counts gives %d" % (r, name(r // (S + 1)), r % (S + 1), off[r], want_off[r]))
    if packed.shape != ref.packed.shape:
        fail("the store holds %d chunks (+ %d of slack), its rows end at %d" % (packed.shape[0] - SLACK, SLACK, total))
    if packed_chunks is not None and packed_chunks != total:
        fail("packed_chunks = %d, the rows end at %d" % (packed_chunks, total))
    if packed[total:].any():
        fail("the slack row behind the store is not zero (chunk %d)" % (total + _first(packed[total:].any(axis=1))))

    # ---- chunk words
    rows = np.repeat(np.arange(n_rows, dtype=np.int64), np.diff(np.append(want_off, total)))
    c_list = rows // (S + 1) * S + rows % (S + 1)                        # the list of every chunk
    c_in_list = np.arange(total, dtype=np.int64) - want_off[rows]

    def chunk(c):
        return "chunk %d of list (%s) [store chunk %d: %s]" % (c_in_list[c], lst(c_list[c]), c, " ".join("%08x" % w for w in packed[c]))

    g8c = ref.want_fmt[c_list // max(S, 1)] if total else np.zeros(0, dtype=bool)
    body = np.ascontiguousarray(packed[:total])
    w0 = body[:, 0].astype(np.int64)
    cnt = np.where(g8c, w0 >> 28, w0 >> 29) + 1
    x0 = w0 & np.where(g8c, X_MASK8, X_MASK)
    ppc = np.where(g8c, PPC8, PPC)
    gaps = np.full((total, PPC8 - 1), -1, dtype=np.int64)
    gaps[~g8c, :PPC - 1] = body.view(np.uint16)[~g8c, 2:]
    gaps[g8c] = body.view(np.uint8)[g8c, 4:]
    if (cnt > ppc).any():
        c = _first(cnt > ppc)
        fail("%s: the count field says %d postings, a chunk holds %d" % (chunk(c), cnt[c], ppc[c]))
    j = np.arange(PPC8 - 1)[None, :]
    real, pad = j < (cnt - 1)[:, None], (j >= (cnt - 1)[:, None]) & (j < (ppc - 1)[:, None])
    if (pad & (gaps != PAD_GAP)).any():
        c, s = divmod(_first(pad & (gaps != PAD_GAP)), PPC8 - 1)
        fail("%s: count field %d, but the padding slot %d holds a gap of %d, not %d" % (chunk(c), cnt[c] - 1, s, gaps[c, s], PAD_GAP))
    if (real & (gaps < 1)).any():
        c, s = divmod(_first(real & (gaps < 1)), PPC8 - 1)
        fail("%s: count field %d, but the gap in slot %d is %d (lists ascend strictly)" % (chunk(c), cnt[c] - 1, s, gaps[c, s]))
    xs = np.concatenate([x0[:, None], x0[:, None] + np.cumsum(np.where(real, gaps, 0), axis=1)], axis=1)
    keep = np.arange(PPC8)[None, :] < cnt[:, None]
    if (xs[keep] >= max(n_docs, 1)).any():
        c = _first((keep & (xs >= n_docs)).any(axis=1))
        fail("%s: decodes to document number %d of %d" % (chunk(c), xs[c][keep[c]].max(), n_docs))
    dec_x, dec_l = xs[keep], np.repeat(c_list, cnt)
    dec_c = np.repeat(np.arange(total, dtype=np.int64), cnt)

    # ---- the postings, in chunk order, are the CSR's mapped through x_of; the chunks break exactly where the format says
    n_lists = n_terms * S
    n_got, n_want = np.bincount(dec_l, minlength=n_lists), np.bincount(ref.vl, minlength=n_lists)
    if not np.array_equal(n_got, n_want):
        l = _first(n_got != n_want)
        fail("list (%s): %d postings in the store, %d in the CSR" % (lst(l), n_got[l], n_want[l]))
    if not np.array_equal(dec_x, ref.x):
        i = _first(dec_x != ref.x)
        fail("%s: posting %d of the list decodes to x = %d, the CSR has x = %d (document %d)" % (
            chunk(dec_c[i]), i - np.searchsorted(ref.vl, ref.vl[i]), dec_x[i], ref.x[i], ref.vp[i]))
    starts = np.zeros(dec_x.size, dtype=bool)
    starts[np.cumsum(cnt) - cnt] = True
    if not np.array_equal(starts, ref.cstart):
        i = _first(starts != ref.cstart)
        fail("%s: chunk boundary %s posting %d of the list (x = %d, gap %d), where the format has %s" % (
            chunk(dec_c[i]), "before" if starts[i] else "missing before", i - np.searchsorted(ref.vl, ref.vl[i]), dec_x[i],
            dec_x[i] - dec_x[i - 1] if i else 0, "none" if starts[i] else "one"))

    # ---- cut_sample
    cut = np.asarray(dev.cut_sample)
    if cut.size < ref.cut_sample.size:
        fail("cut_sample has %d entries, %d chunks need %d" % (cut.size, total, ref.cut_sample.size))
    want_cut = np.full(cut.size, 0xFFFFFFFF, dtype=np.uint32)       # (an allocation may be rounded up: all of it is defined)
    want_cut[:ref.cut_sample.size] = ref.cut_sample
    if not np.array_equal(cut, want_cut):
        m = _first(cut != want_cut)
        fail("cut_sample[%d] = %#x, %s" % (m, cut[m], "the first x of %s is %#x" % (chunk(16 * m), ref.cut_sample[m]) if 16 * m < total
                                           else "behind the store: 0xffffffff expected"))
    if not np.array_equal(packed, ref.packed):      # (nothing above should let this through)
        c = _first((packed != ref.packed).any(axis=1))
        fail("%s differs from the restatement's %s" % (chunk(c), " ".join("%08x" % w for w in ref.packed[c])))

    # ---- forward index
    rec = np.asarray(dev.fwd_rec).astype(np.int64).reshape(-1, 2)
    if rec.shape[0] != n_docs:
        fail("fwd_rec has %d records, %d documents" % (rec.shape[0], n_docs))
    want_y = ref.fwd_rec[:, 1].astype(np.int64)
    doc = ref.orig_of.astype(np.int64)

    def docname(x):
        return "document x = %d (docID %d)" % (x, doc[x])

    if ((rec[:, 1] & 0xFFFF) != (want_y & 0xFFFF)).any():
        x = _first((rec[:, 1] & 0xFFFF) != (want_y & 0xFFFF))
        fail("forward index, %s: cardinality %d, the CSR has it in segment %d" % (docname(x), rec[x, 1] & 0xFFFF, want_y[x] & 0xFFFF))
    if ((rec[:, 1] >> 16) != (want_y >> 16)).any():
        x = _first((rec[:, 1] >> 16) != (want_y >> 16))
        fail("forward index, %s: %d distinct terms, the CSR has it in %d lists" % (docname(x), rec[x, 1] >> 16, want_y[x] >> 16))
    terms = np.asarray(dev.fwd_terms).reshape(-1, 4)
    fx_base = np.asarray(dev.fx_base)
    nd = want_y >> 16
    if ref.strided:
        if fx_base.size != S + 1:
            fail("forward index: %d segments, but fx_base has %d entries" % (S, fx_base.size))
        if not np.array_equal(fx_base, ref.fx_base):
            b = _first(fx_base != ref.fx_base)
            fail("forward index: fx_base[%d] = %d, the scan of the segments' sizes x strides gives %d" % (b, fx_base[b], ref.fx_base[b]))
        if not np.array_equal(rec[:, 0], ref.fwd_rec[:, 0]):
            x = _first(rec[:, 0] != ref.fwd_rec[:, 0])
            fail("forward index, %s: its terms at chunk %d, fx_base[B] + (x - seg_base[B]) * ceil(B / 4) = %d" % (docname(x), rec[x, 0], ref.fwd_rec[x, 0]))
        if terms.shape[0] != ref.fwd_terms.shape[0]:
            fail("forward index: fwd_terms holds %d chunks, the strides add up to %d" % (terms.shape[0], ref.fwd_terms.shape[0]))
        n_chunks = ((want_y & 0xFFFF) + 3) >> 2
    else:
        if fx_base.size:
            fail("forward index: %d segments, but fx_base is present" % S)
        n_chunks = (nd + 3) >> 2
        has = np.flatnonzero(n_chunks > 0)
        has = has[np.argsort(rec[has, 0], kind="stable")]
        lo, hi = rec[has, 0], rec[has, 0] + n_chunks[has]
        if has.size and hi.max() > terms.shape[0]:
            x = has[_first(hi > terms.shape[0])]
            fail("forward index, %s: chunks %d .. %d lie outside fwd_terms (%d chunks)" % (docname(x), rec[x, 0], rec[x, 0] + n_chunks[x], terms.shape[0]))
        if (lo[1:] < hi[:-1]).any():
            i = _first(lo[1:] < hi[:-1])
            fail("forward index: the chunks of %s and of %s overlap" % (docname(has[i]), docname(has[i + 1])))
    # a document's term ids as a sorted set, 0xFFFFFFFF in the rest of its chunks
    lens = n_chunks * 4
    begin = np.zeros(n_docs + 1, dtype=np.int64)
    begin[1:] = np.cumsum(lens)
    owner = np.repeat(np.arange(n_docs, dtype=np.int64), lens)
    got = terms.reshape(-1)[rec[owner, 0] * 4 + np.arange(owner.size) - begin[owner]].astype(np.int64)
    got = np.sort((owner << 32) | got) & 0xFFFFFFFF
    fx, ft, first = ref.doc_terms
    want = np.full(owner.size, NO_TERM, dtype=np.int64)
    want[begin[fx] + np.arange(fx.size) - first[fx]] = ft
    if not np.array_equal(got, want):
        i = _first(got != want)
        x = int(owner[i])
        fail("forward index, %s: term ids %s, the CSR has it in the lists of %s" % (
            docname(x), [int(v) for v in got[begin[x]:begin[x + 1]]], [name(int(v)) if v != NO_TERM else "-" for v in want[begin[x]:begin[x + 1]]]))
    return ref


def read_store(index, replica=0):
    """the raw arrays of an uploaded suggest_amd.NGramIndex (sg_debug_index_array)"""
    return SimpleNamespace(**{k: index.raw_array(k, replica) for k in
                              ("packed", "seg_off", "orig_of", "x_of", "seg_base", "cut_sample", "fwd_rec", "fwd_terms", "fx_base")})


def term_keys(index):
    """-> uint64[n_terms], the key of every term id: sg_index_lists enumerates the non-empty lists term-major, so the keys in
    order of first appearance are the terms in id order — provided every term has a list, which is asserted"""
    from suggest_amd import _lib
    L = _lib.lib()
    with index._use() as h:
        n = L.sg_index_lists(h, None, None, 0)
        segs, keys = np.zeros(n, dtype=np.uint32), np.zeros(n, dtype=np.uint64)
        assert L.sg_index_lists(h, segs.ctypes.data, keys.ctypes.data, n) == n
    first = np.ones(n, dtype=bool)
    first[1:] = keys[1:] != keys[:-1]
    keys = keys[first]
    assert len(keys) == index.stats()["n_terms"] == len(set(keys.tolist())), "a term without a list: term ids cannot be named"
    return keys


def check_index(index, g8_mode, sample=48):
    """The whole checker on an uploaded index + NGramIndex.forward() on a sample of documents.  -> (restatement, raw arrays)"""
    st = index.stats()
    n_docs, S, n_terms = st["n_docs"], st["n_segments"], st["n_terms"]
    hp, hso = index.raw_array("host_postings"), index.raw_array("host_seg_off")
    keys = term_keys(index)
    dev = read_store(index)
    ref = check(dev, hp, hso, n_docs, S, n_terms, g8_mode, term_name=lambda t: index.term_string(int(keys[t])),
                packed_chunks=index.pipe_volumes()["packed_chunks"])
    fx, ft, first = ref.doc_terms
    for lo in sorted({0, max(0, n_docs // 2 - sample // 2), max(0, n_docs - sample)}):
        n = min(sample, n_docs - lo)
        card, nt, got = index.forward(lo, n)
        for i in range(n):
            d = lo + i
            x = int(ref.x_of[d])
            want = ft[first[x]:first[x + 1]]
            if card[i] != ref.card[d] or nt[i] != want.size:
                raise StoreMismatch("forward(): document %d has cardinality %d and %d terms, the CSR %d and %d" % (d, card[i], nt[i], ref.card[d], want.size))
            if sorted(got[i, :nt[i]].tolist()) != sorted(keys[want].tolist()):
                raise StoreMismatch("forward(): the term keys of document %d differ from the lists that hold it" % d)
    return ref, dev
