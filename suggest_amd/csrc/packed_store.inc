// packed_store.inc — the posting store the search kernel streams, derived on the GPU from the u32 CSR (host build, device
// build or a reference-built index: all the same from here on).  Included by engine.hip after capi.inc; tune.inc's add_replica calls it.
//
// The reference keeps a list as varint / roaring bytes and decodes it posting by posting (pkg/index/posting_list.go:24-108,
// pkg/compression/*.go); the u32 CSR of round 1-2 made the stream a plain coalesced read, and the kernel ended up waiting
// for HBM (headline: 0.96 of the achievable bandwidth).  The only way further is fewer bytes per posting:
//
//  * Segment-major document numbering.  A list (term t, segment B) holds only documents of cardinality B.  Documents are
//    renumbered x = seg_base[B] + rank of the document among those of its cardinality (stable: ascending docID inside a
//    segment), so the postings of one list fall into one range of n_docs / S numbers instead of all of [0, n_docs): gaps
//    shrink by the number of populated segments (10 M strings, q = 3: mean gap 58 000 -> 2 300), and a term's lists for
//    consecutive segments still form one ascending run (term-major layout, seg_base ascending).
//    The kernel works in x throughout (counters, candidate queue, forward index, docID-range passes) and maps a document
//    back through orig_of[] only when it enters the top-k — whose order (score desc, docID asc) is by ORIGINAL docID.
//  * 16-byte chunks of SG_PPC = 7 postings: {u32 first x, 6 x u16 gaps}.  A gap above 65 535 starts a new chunk; a list
//    starts on a chunk boundary, so seg_off rows address chunks as before.  4 -> 7 postings per 16-byte lane load, decoded
//    with six adds in registers.  Worst case (every gap above 65 535) is one posting per chunk — lists that sparse are short.
//  * The top three bits of the first word say how many of the seven slots are postings (minus one); the slots behind them
//    are padding with gaps of SG_PAD_GAP (pk_finish).  The stream counts every slot without looking — a phantom posting of
//    a few document numbers further on, each in a bucket of its own (the gap is odd and not 1: the immediate neighbours
//    of a document in a sorted dictionary are the likeliest other matches of the same query, and their buckets are the
//    ones not to disturb), is noise the lossy counters absorb (they are upper bounds: the
//    exact overlap comes from the forward index) — and saves the per-slot "is this padding" instruction that zero gaps
//    cost in round 3's first format.  Everything else (candidate queue, exact per-list searches, the overflow pass, the long-
//    query kernel) masks the padding by the count.  Document numbers therefore stay below 2^29.
//
//  * [r4] Dense terms take 8-bit gaps: {u32 first x, 12 x u8 gaps} = SG_PPC8 = 13 postings per chunk (a gap above 255 starts a new
//    chunk).  In the segment's own numbering the gap of a list is 1 / (share of the segment's documents that hold the term),
//    whatever the size of the dictionary: bigrams (q = 2: a 20-rune string holds 1.5 % of the 1 296 bigrams) and the common
//    n-grams of a skewed alphabet sit at gaps of 30 ... 100, and a query over them is a few MB of postings — the launches
//    that do run at the HBM rate.  The format is chosen PER TERM (all of a term's lists: a row of the stream — 64 consecutive
//    chunks of a term's lists for consecutive segments — stays uniform, so the decode is a wave-uniform branch per row), by
//    counting the term's chunks both ways; an index where that saves less than 3 % keeps 16-bit gaps throughout and runs on
//    the kernels that know nothing of this.  A term's format is bit 31 of its seg_off entries (they cancel in every length);
//    an 8-bit chunk keeps x in 28 bits and its posting count (minus one) in the 4 above.
//
//   pk_keys / radix sort / pk_inverse / pk_seg_base   the numbering: orig_of[x], x_of[doc], seg_base[B]
//   pk_pack<false>   one wavefront per list: chunks it needs (once per format)
//   pk_choose        per term: the format with fewer chunks -> term_fmt[], the rows' chunk counts -> exclusive scan = packed seg_off rows
//   pk_pack<true>    the same walk, writing base words and gaps (the store is zeroed first: unused gaps are 0)
//   pk_finish        per list: posting count into each first word's top bits, padding gaps 0 -> SG_PAD_GAP, cut_sample
//   pk_flag_rows     bit 31 of the seg_off rows of 8-bit terms
//   pk_permute_rec   forward-index records in x order
namespace sg {

__global__ void pk_keys(const uint2* rec, uint32_t n_docs, uint32_t* key, uint32_t* val) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n_docs) { key[i] = rec[i].y & 0xFFFFu; val[i] = i; }
}
__global__ void pk_inverse(const uint32_t* orig_of, uint32_t n_docs, uint32_t* x_of) {
  const uint32_t x = blockIdx.x * blockDim.x + threadIdx.x;
  if (x < n_docs) x_of[orig_of[x]] = x;
}
__global__ void pk_seg_base(const uint32_t* sorted_card, uint32_t n_docs, uint32_t S, uint32_t* seg_base) {
  const uint32_t b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b > S) return;
  uint32_t lo = 0, hi = n_docs;                               // first x whose cardinality is >= b
  while (lo < hi) { const uint32_t mid = lo + ((hi - lo) >> 1); if (sorted_card[mid] < b) lo = mid + 1; else hi = mid; }
  seg_base[b] = lo;
}
__global__ void pk_permute_rec(const uint2* rec, const uint32_t* orig_of, uint32_t n_docs, uint2* out) {
  const uint32_t x = blockIdx.x * blockDim.x + threadIdx.x;
  if (x < n_docs) out[x] = rec[orig_of[x]];
}

// fmt8: count mode — the format to count for (every list alike); write mode — ignored, term_fmt[t] decides (null: 16-bit gaps)
// [r6] forward-index term lists in x order at a fixed stride per cardinality segment: document x of segment B at chunk
// fx_base[B] + (x - seg_base[B]) * ceil(B / 4) — a verifier computes the address from x alone (no record to fetch first)
__global__ void pk_fwd_strided(uint2* rec_x, const uint32_t* __restrict__ old_terms, const uint32_t* __restrict__ seg_base, const uint32_t* __restrict__ fx_base,
                               uint32_t n_docs, uint32_t* __restrict__ new_terms) {
  const uint32_t x = blockIdx.x * blockDim.x + threadIdx.x;
  if (x >= n_docs) return;
  const uint2 r = rec_x[x];
  const uint32_t B = r.y & 0xFFFFu, nd = r.y >> 16, stride = (B + 3u) >> 2;
  const uint32_t at = fx_base[B] + (x - seg_base[B]) * stride;
  for (uint32_t c = 0; c < ((nd + 3u) >> 2) && c < stride; c++) ((uint4*)new_terms)[at + c] = ((const uint4*)old_terms)[r.x + c];
  rec_x[x] = make_uint2(at, r.y);
}

template <bool kWrite>
__global__ __launch_bounds__(64) void pk_pack(const uint32_t* __restrict__ postings, const uint32_t* __restrict__ seg_off, uint32_t S, uint64_t n_lists,
                                              const uint32_t* __restrict__ x_of, uint32_t* counts, const uint32_t* new_off, uint32_t* out,
                                              bool fmt8, const uint8_t* __restrict__ term_fmt) {
  const uint32_t lane = threadIdx.x;
  for (uint64_t list = blockIdx.x; list < n_lists; list += gridDim.x) {      // (grid-stride: see fwd_walk)
  const uint32_t t = (uint32_t)(list / S), b = (uint32_t)(list - (uint64_t)t * S);
  const bool g8 = kWrite ? (term_fmt && term_fmt[t]) : fmt8;
  const uint32_t gap_max = g8 ? 0xFFu : 0xFFFFu, ppc = g8 ? SG_PPC8 : SG_PPC;
  const uint64_t row = (uint64_t)t * (S + 1) + b;
  const uint32_t c0 = seg_off[row], c1 = seg_off[row + 1];
  // (x_of null: the rows are the class store's — document numbers already, offsets in postings, no padding)
  const uint32_t n4 = x_of ? (c1 - c0) * 4u : c1 - c0;
  const uint32_t* p = postings + (x_of ? (uint64_t)c0 * 4u : (uint64_t)c0);
  const uint32_t chunk0 = kWrite ? new_off[row] : 0u;
  uint32_t n_chunks = 0;      // chunks begun so far
  uint32_t run_pos = 0;       // position of lane 0's posting in its run (postings since the last forced break)
  uint32_t prev_x = 0;
  for (uint32_t i0 = 0; i0 < n4; i0 += 64u) {
    const uint32_t i = i0 + lane;
    const uint32_t d = i < n4 ? p[i] : 0u;
    const uint32_t dprev = (i > 0u && i < n4) ? p[i - 1u] : 0u;
    const bool valid = i < n4 && (i == 0u || d != dprev);     // (padding repeats the last docID; lists are strictly ascending)
    const uint32_t x = valid ? (x_of ? x_of[d] : d) : 0u;
    uint32_t xp = (uint32_t)__shfl_up((int)x, 1, 64);
    if (lane == 0u) xp = prev_x;
    const uint32_t gap = x - xp;
    const bool brk = valid && (i == 0u || gap > gap_max);
    int rs = brk ? (int)lane : -1;                               // last forced break at or before this lane
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) { const int o = __shfl_up(rs, off, 64); if ((int)lane >= off) rs = max(rs, o); }
    const uint32_t pos_in_run = rs >= 0 ? lane - (uint32_t)rs : run_pos + lane;
    const uint32_t slot = pos_in_run % ppc;
    const uint64_t sm = __builtin_amdgcn_ballot_w64(valid && slot == 0u);
    if (kWrite && valid) {
      const uint32_t my_chunk = n_chunks + (uint32_t)__builtin_popcountll(sm & ((2ull << lane) - 1ull)) - 1u;
      uint32_t* c = out + (uint64_t)(chunk0 + my_chunk) * 4u;
      if (slot == 0u) c[0] = x;
      else if (g8) ((uint8_t*)(c + 1))[slot - 1u] = (uint8_t)gap;
      else ((uint16_t*)(c + 1))[slot - 1u] = (uint16_t)gap;
    }
    n_chunks += (uint32_t)__builtin_popcountll(sm);
    if (__builtin_amdgcn_ballot_w64(valid) != ~0ull) break;      // the padding (or the end) was reached
    prev_x = (uint32_t)__builtin_amdgcn_readlane((int)x, 63);
    run_pos = (uint32_t)__builtin_amdgcn_readlane((int)pos_in_run, 63) + 1u;
  }
  if (!kWrite && lane == 0u) counts[row] = n_chunks;
  }
}

// Per term: the format that needs fewer chunks (c16 / c8: the rows' chunk counts either way; the last row of a term counts
// 0).  mode 1: 8-bit gaps where they save chunks; 2: wherever possible (tests).  totals[0] += the term's chunks with 16-bit
// gaps, totals[1] += with the format chosen.
__global__ void pk_choose(const uint32_t* c16, const uint32_t* c8, uint32_t n_terms, uint32_t S, int mode, uint8_t* term_fmt, uint32_t* counts,
                          unsigned long long* totals) {
  const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= n_terms) return;
  const uint64_t r0 = (uint64_t)t * (S + 1);
  uint64_t s16 = 0, s8 = 0;
  for (uint32_t b = 0; b < S; b++) { s16 += c16[r0 + b]; s8 += c8[r0 + b]; }
  const bool g8 = mode == 2 ? s8 > 0 : s8 < s16;
  term_fmt[t] = g8 ? 1 : 0;
  for (uint32_t b = 0; b <= S; b++) counts[r0 + b] = g8 ? c8[r0 + b] : c16[r0 + b];
  atomicAdd(totals, (unsigned long long)s16);
  atomicAdd(totals + 1, (unsigned long long)(g8 ? s8 : s16));
}
// A chunk as pk_pack<true> left it: real gaps (>= 1: lists ascend strictly) and then zeros.  The count of postings goes into
// the first word, the zeros become gaps of SG_PAD_GAP; the first x of every 16th chunk of the store goes to cut_sample.
// One wavefront per list (the list's term knows the format).
__global__ __launch_bounds__(64) void pk_finish(uint4* packed, const uint32_t* __restrict__ new_off, uint32_t S, uint64_t n_lists,
                                                const uint8_t* __restrict__ term_fmt, uint32_t* cs) {
  for (uint64_t list = blockIdx.x; list < n_lists; list += gridDim.x) {
    const uint32_t t = (uint32_t)(list / S), b = (uint32_t)(list - (uint64_t)t * S);
    const uint64_t row = (uint64_t)t * (S + 1) + b;
    const bool g8 = term_fmt && term_fmt[t];
    const uint32_t c0 = new_off[row], c1 = new_off[row + 1];
    for (uint32_t c = c0 + threadIdx.x; c < c1; c += 64u) {
      uint4 v = packed[c];
      if (g8) {
        uint32_t g[SG_PPC8 - 1];
        for (int e = 0; e < 4; e++) { g[e] = (v.y >> (8 * e)) & 0xFFu; g[4 + e] = (v.z >> (8 * e)) & 0xFFu; g[8 + e] = (v.w >> (8 * e)) & 0xFFu; }
        uint32_t np = 1;
        while (np < SG_PPC8 && g[np - 1] != 0u) np++;
        for (uint32_t e = np; e < SG_PPC8; e++) g[e - 1] = SG_PAD_GAP;
        v.x = (v.x & SG_X_MASK8) | ((np - 1u) << 28);
        v.y = g[0] | (g[1] << 8) | (g[2] << 16) | (g[3] << 24); v.z = g[4] | (g[5] << 8) | (g[6] << 16) | (g[7] << 24);
        v.w = g[8] | (g[9] << 8) | (g[10] << 16) | (g[11] << 24);
      } else {
        uint32_t g[6] = {v.y & 0xFFFFu, v.y >> 16, v.z & 0xFFFFu, v.z >> 16, v.w & 0xFFFFu, v.w >> 16};
        uint32_t np = 1;
        while (np < SG_PPC && g[np - 1] != 0u) np++;
        for (uint32_t e = np; e < SG_PPC; e++) g[e - 1] = SG_PAD_GAP;
        v.x = (v.x & SG_X_MASK) | ((np - 1u) << 29);
        v.y = g[0] | (g[1] << 16); v.z = g[2] | (g[3] << 16); v.w = g[4] | (g[5] << 16);
      }
      packed[c] = v;
      if ((c & 15u) == 0u) cs[c >> 4] = v.x & (g8 ? SG_X_MASK8 : SG_X_MASK);
    }
  }
}
// bit 31 of every seg_off entry of an 8-bit term (S + 1 entries per term; the flags cancel in every length)
__global__ void pk_flag_rows(uint32_t* new_off, uint32_t n_terms, uint32_t S, const uint8_t* term_fmt) {
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < (uint64_t)n_terms * (S + 1) && term_fmt[i / (S + 1)]) new_off[i] |= 0x80000000u;
}

// [r5 -> r6] The "class store" (the document side of the prefix filter: every list split by the term's tail rank in its
// document) was built, bit-exact and 25 % slower on the headline for 2 % fewer streamed chunks; it was removed in round 6.
// The measurement and the reasoning: DESIGN_history.md R5.7, profiles/r05ze_class_store_ab_headline.txt; the code: git history
// (last in commit 475be11).

}  // namespace sg

namespace {

// u32 CSR + forward index (both already on the device, in r->dix) -> the packed store.  On success r->dix.postings /
// seg_off / fwd_rec / cut_sample are the packed store's, orig_of / seg_base are set and the u32 arrays are freed.
// g8_mode (knob SG_G8): 0 16-bit gaps only, 1 8-bit gaps for the terms they save chunks on, 2 for every term (tests)
int pack_store(const HostIndex& h, Replica* r, int g8_mode) {
  DeviceIndex& d = r->dix;
  const uint32_t n_docs = (uint32_t)h.n_docs, S = h.n_segments, nT = (uint32_t)h.term_key.size();
  int rc;
  if ((uint64_t)h.n_docs + SG_PPC * SG_PAD_GAP > (uint64_t)SG_X_MASK) { set_error("the packed posting store numbers documents below 2^29"); return SG_E_UNSUPPORTED; }
  DeviceBlock& mem = r->mem;
  DeviceBlock scratch;                                          // freed on return: not part of the replica
  uint32_t *orig_of = nullptr, *x_of = nullptr, *seg_base = nullptr;
  if ((rc = mem.alloc(&orig_of, (size_t)n_docs)) || (rc = mem.alloc(&x_of, (size_t)n_docs)) || (rc = mem.alloc(&seg_base, (size_t)S + 2))) return rc;
  const unsigned gd = (n_docs + 255u) / 256u;
  if (n_docs) {
    uint32_t *key_in = nullptr, *key_out = nullptr, *val_in = nullptr;
    if ((rc = scratch.alloc(&key_in, (size_t)n_docs)) || (rc = scratch.alloc(&key_out, (size_t)n_docs)) || (rc = scratch.alloc(&val_in, (size_t)n_docs))) return rc;
    hipLaunchKernelGGL(pk_keys, dim3(gd), dim3(256), 0, 0, d.fwd_rec, n_docs, key_in, val_in);
    HIP_TRY(hipGetLastError());
    if ((rc = device_sort_pairs(scratch, key_in, key_out, val_in, orig_of, n_docs, 0, 16))) return rc;   // stable
    hipLaunchKernelGGL(pk_inverse, dim3(gd), dim3(256), 0, 0, orig_of, n_docs, x_of);
    HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(pk_seg_base, dim3((S + 1 + 255) / 256), dim3(256), 0, 0, key_out, n_docs, S, seg_base);
    HIP_TRY(hipGetLastError());
    uint2* rec_x = nullptr;
    if ((rc = mem.alloc(&rec_x, (size_t)n_docs))) return rc;
    hipLaunchKernelGGL(pk_permute_rec, dim3(gd), dim3(256), 0, 0, d.fwd_rec, orig_of, n_docs, rec_x);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipDeviceSynchronize());
    mem.release(d.fwd_rec);
    d.fwd_rec = rec_x;
    // [r6] the term lists themselves in x order, a segment's documents a fixed stride apart (pk_fwd_strided): where the dictionary
    // has at most 63 segments a verifier's lanes find a document's segment in a table they hold, and its term list with it
    // (pipeline.inc sg_verify_kernel: one memory round trip less per candidate).  A document holds at most as many distinct
    // terms as its cardinality; one that repeats terms leaves slots of its stride empty.
    if (S <= 63u) {
      std::vector<uint32_t> sb((size_t)S + 2), fb((size_t)S + 2, 0u);
      HIP_TRY(hipMemcpy(sb.data(), seg_base, ((size_t)S + 1) * 4, hipMemcpyDeviceToHost));
      uint64_t tot = 0;
      bool ok = true;
      for (uint32_t b = 0; b < S; b++) { fb[b] = (uint32_t)tot; tot += (uint64_t)(sb[b + 1] - sb[b]) * ((b + 3u) >> 2); if (tot >= 0xFFFFFFF0ull) ok = false; }
      fb[S] = (uint32_t)tot;
      if (ok) {
        uint32_t *fx_base = nullptr, *terms_x = nullptr;
        if ((rc = mem.alloc(&fx_base, (size_t)S + 2)) || (rc = mem.alloc(&terms_x, (size_t)std::max<uint64_t>(tot, 1) * 4))) return rc;
        HIP_TRY(hipMemcpy(fx_base, fb.data(), ((size_t)S + 1) * 4, hipMemcpyHostToDevice));
        HIP_TRY(hipMemset(terms_x, 0xFF, (size_t)std::max<uint64_t>(tot, 1) * 16));
        hipLaunchKernelGGL(pk_fwd_strided, dim3(gd), dim3(256), 0, 0, rec_x, d.fwd_terms, (const uint32_t*)seg_base, (const uint32_t*)fx_base, n_docs, terms_x);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipDeviceSynchronize());
        mem.release(d.fwd_terms);
        d.fwd_terms = terms_x;
        d.fx_base = fx_base;
      }
    }
  } else {
    HIP_TRY(hipMemset(seg_base, 0, ((size_t)S + 2) * 4));
  }
  d.orig_of = orig_of; d.seg_base = seg_base; r->x_of = x_of;

  const uint64_t n_lists = (uint64_t)nT * S, n_rows = (uint64_t)nT * (S + 1);
  uint32_t* new_off = nullptr;
  if ((rc = mem.alloc(&new_off, (size_t)std::max<uint64_t>(n_rows, 1)))) return rc;
  uint64_t total_chunks = 0;
  uint8_t* term_fmt = nullptr;                                  // [nT] 1: the term's lists have 8-bit gaps (null: none has)
  const unsigned pk_grid = (unsigned)std::min<uint64_t>(std::max<uint64_t>(n_lists, 1), 1u << 22);
  // 8-bit chunks keep x in 28 bits; the padding's phantom numbers must fit as well
  const bool g8_possible = g8_mode > 0 && n_lists && (uint64_t)h.n_docs + SG_PPC8 * SG_PAD_GAP <= (uint64_t)SG_X_MASK8;
  if (n_lists) {
    if (n_rows >= 0x7FFFFFFFull) { set_error("terms x segments exceeds a launch grid"); return SG_E_UNSUPPORTED; }
    uint32_t *counts = nullptr, *c8 = nullptr;
    if ((rc = scratch.alloc(&counts, (size_t)n_rows))) return rc;
    HIP_TRY(hipMemset(counts, 0, (size_t)n_rows * 4));
    hipLaunchKernelGGL(pk_pack<false>, dim3(pk_grid), dim3(64), 0, 0, d.postings, d.seg_off, S, n_lists, (const uint32_t*)x_of, counts,
                       (const uint32_t*)nullptr, (uint32_t*)nullptr, false, (const uint8_t*)nullptr);
    HIP_TRY(hipGetLastError());
    if (g8_possible) {
      uint32_t* c16 = counts;
      unsigned long long* totals = nullptr;
      if ((rc = scratch.alloc(&c8, (size_t)n_rows))) return rc;
      HIP_TRY(hipMemset(c8, 0, (size_t)n_rows * 4));
      if ((rc = scratch.alloc(&counts, (size_t)n_rows)) || (rc = scratch.alloc(&totals, 2))) return rc;
      HIP_TRY(hipMemset(totals, 0, 16));
      if ((rc = scratch.alloc(&term_fmt, (size_t)nT))) return rc;
      hipLaunchKernelGGL(pk_pack<false>, dim3(pk_grid), dim3(64), 0, 0, d.postings, d.seg_off, S, n_lists, (const uint32_t*)x_of, c8,
                         (const uint32_t*)nullptr, (uint32_t*)nullptr, true, (const uint8_t*)nullptr);
      hipLaunchKernelGGL(pk_choose, dim3((nT + 255) / 256), dim3(256), 0, 0, (const uint32_t*)c16, (const uint32_t*)c8, nT, S, g8_mode, term_fmt, counts, totals);
      HIP_TRY(hipGetLastError());
      unsigned long long tot[2] = {0, 0};
      HIP_TRY(hipMemcpy(tot, totals, 16, hipMemcpyDeviceToHost));
      // an index that gains less than 3 % keeps one format — and the kernels that know of one format only
      if (g8_mode == 1 && (double)tot[1] > 0.97 * (double)tot[0]) { term_fmt = nullptr; counts = c16; }
      else if (tot[1] >= 0x7FFFFFFFull) { set_error("the packed posting store addresses chunks below 2^31"); return SG_E_UNSUPPORTED; }
      if (env_int("SG_VERBOSE", 0, 1, 0)) fprintf(stderr, "[suggest_hip] packed store: %llu chunks with 16-bit gaps, %llu with 8-bit gaps for the dense terms%s\n", tot[0], tot[1],
                                        term_fmt ? "" : " (not taken)");
    }
    if ((rc = device_exclusive_sum(scratch, counts, new_off, (size_t)n_rows))) return rc;
    uint32_t last = 0;                                          // (the last row of a term counts 0: its offset is the total)
    HIP_TRY(hipMemcpy(&last, new_off + (n_rows - 1), 4, hipMemcpyDeviceToHost));
    total_chunks = last;
  } else {
    HIP_TRY(hipMemset(new_off, 0, 4));
  }
  uint32_t* packed = nullptr;
  if ((rc = mem.alloc(&packed, (size_t)total_chunks * 4 + 64 * 4))) return rc;      // (+ a row of slack behind the last chunk)
  HIP_TRY(hipMemset(packed, 0, ((size_t)total_chunks * 4 + 64 * 4) * 4));
  // one sample per 16 chunks of the store: lets a docID-range pass cut its lists without probing them (written by pk_finish)
  const uint64_t n_cs = total_chunks / 16 + 2;
  uint32_t* cs = nullptr;
  if ((rc = mem.alloc(&cs, (size_t)n_cs))) return rc;
  HIP_TRY(hipMemset(cs, 0xFF, std::max<size_t>((size_t)n_cs * 4, 16)));      // (all of the allocation: sg_debug_index_array reads it back whole)
  if (n_lists) {
    hipLaunchKernelGGL(pk_pack<true>, dim3(pk_grid), dim3(64), 0, 0, d.postings, d.seg_off, S, n_lists, (const uint32_t*)x_of, (uint32_t*)nullptr,
                       (const uint32_t*)new_off, packed, false, (const uint8_t*)term_fmt);
    HIP_TRY(hipGetLastError());
    if (total_chunks) {
      hipLaunchKernelGGL(pk_finish, dim3(pk_grid), dim3(64), 0, 0, (uint4*)packed, (const uint32_t*)new_off, S, n_lists, (const uint8_t*)term_fmt, cs);
      HIP_TRY(hipGetLastError());
    }
    if (term_fmt) {
      hipLaunchKernelGGL(pk_flag_rows, dim3((unsigned)((n_rows + 255) / 256)), dim3(256), 0, 0, new_off, nT, S, (const uint8_t*)term_fmt);
      HIP_TRY(hipGetLastError());
    }
  }
  HIP_TRY(hipDeviceSynchronize());
  r->packed_chunks = total_chunks;
  mem.release(d.postings);
  mem.release(d.seg_off);
  d.postings = packed;
  d.seg_off = new_off;
  d.cut_sample = cs;
  d.has_g8 = term_fmt ? 1u : 0u;
  r->packed_chunks = total_chunks;
  HIP_TRY(hipDeviceSynchronize());
  return SG_OK;
}

}  // namespace
