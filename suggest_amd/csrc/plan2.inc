// plan2.inc — [r6] the plan launch with TWO queries per wavefront (included by engine.hip behind pipeline.inc).
//
// sg_plan_kernel (pipeline.inc) is bound by instruction issue — 1 139 vector and 1 328 scalar instructions per query, one of
// each per four cycles and SIMD — with its lanes a third full: a query has ~22 n-grams and ~24 admissible segments.  Here lanes
// 0..31 plan slot 2b and lanes 32..63 slot 2b + 1 of the piece (neighbours in the ordered list: the same length, nearly the
// same control flow).  What was wavefront-uniform — the window, a group's bounds, thresholds, budgets, masks of lists — is
// uniform per HALF and lives in vector registers: the 64-bit scalar mask arithmetic of the one-query kernel becomes 32-bit
// vector arithmetic that serves two queries per instruction, and the scalar pipe is left with the loop control.
//
// It plans the SIMPLE queries — ASCII bytes, at most 32 n-grams before and after the first-occurrence dedup, a window of at most
// 32 segments, a table of at most SG_PLAN2_ROWS offsets, nothing to trim — under a simple description (wrap and pad runes ASCII,
// q <= 3, one pad symbol, one of the five metrics of pkg/metric: the host checks, plan2_usable).  Any other query is listed
// for sg_plan_kernel (slot list), which then runs over that list; records are the same either way (pipeline.inc), and so are
// the rows.  Reference: pkg/suggest/tokenizer.go:9-34, suggester.go:53-76, index/searcher.go:38-58, merger/cp_merge.go:22-31.

#define SG_PLAN2_ROWS_MAX 1056u      // seg_off entries (terms x (segments + 1) <= 32 x 33) of one query's table at most
#define SG_PLAN2_RUNES 48u           // runes of a simple query with its wrap

// ---- half-wavefront primitives: lane = hb + hl, hb = 0 or 32 ----
__device__ __forceinline__ uint32_t h_ballot(bool p, uint32_t hb) {                 // the 32 lanes of my half
  const uint64_t m = ballot(p);
  return hb ? (uint32_t)(m >> 32) : (uint32_t)m;
}
__device__ __forceinline__ uint32_t h_read(uint32_t v, uint32_t idx, uint32_t hb) {  // v of lane idx (0 .. 31) of my half (every lane takes part)
  return (uint32_t)__builtin_amdgcn_ds_bpermute((int)((idx << 2) + (hb << 2)), (int)v);
}
__device__ __forceinline__ uint32_t h_scan_incl(uint32_t v) {                        // inclusive scan inside each half (wave_scan_incl without its last step)
  v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x111, 0xf, 0xf, true);   // row_shr:1
  v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x112, 0xf, 0xf, true);   // row_shr:2
  v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x114, 0xf, 0xf, true);   // row_shr:4
  v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x118, 0xf, 0xf, true);   // row_shr:8
  v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x142, 0xa, 0xf, false);  // row_bcast:15 -> rows 1, 3
  return v;
}
__device__ __forceinline__ uint32_t h_below(uint32_t m, uint32_t hl) { return (uint32_t)__builtin_popcount(m & ((1u << hl) - 1u)); }
__device__ __forceinline__ uint32_t h_ctz(uint32_t m) { return m ? (uint32_t)__builtin_ctz(m) : 32u; }

struct Plan2Args {
  uint32_t rows_cap;     // seg_off entries of a simple query's table: what the launch's metric and similarity can ask of 32 n-grams
                         // (the host works it out: the LDS of the launch, hence its wavefronts per SIMD, follows it)
  uint32_t half_words;   // LDS words per half = rows_cap + 32, at least SG_PIPE_ROWS_WORDS / 2 (the two halves together serve plan_one_query)
};

// (8 wavefronts per SIMD: 64 vector and 80 scalar registers — left alone the compiler takes 79 / 106 for the rarely run one-query
//  path inlined below and the launch runs six; with the cap it spills a hundred scalars into vector lanes and is still 8 % faster:
//  121 -> 111 us on the headline, profiles/r06zy_timeline_*)
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(8, 8), amdgpu_num_sgpr(80))) void sg_plan2_kernel(const BatchArgs a, const PipeArgs p, const Plan2Args p2) {
  extern __shared__ __attribute__((aligned(16))) uint32_t lds[];      // [2 x half_words]
  const uint32_t lane = threadIdx.x, hb = lane & 32u, hl = lane & 31u, half = hb >> 5;
  const DeviceIndex& ix = a.ix;
  uint32_t* rows = lds + half * p2.half_words;
  const uint32_t s = 2u * blockIdx.x + half;
  // this half's query (position b0 + s of the batch / the ordered list)
  uint32_t n_live = p.n;
  if (a.q_sel) { const uint32_t sel_n = rfl(*a.q_sel_n); n_live = sel_n > p.b0 ? min(p.n, sel_n - p.b0) : 0u; }
  bool on = s < n_live;                                        // the half has a query and nothing has been decided about it
  if (!ballot(on)) return;
  const uint32_t m16_lane = kBucketsPer16Postings[a.filter_level][min(lane, 32u)];   // (lanes 0..32 hold the row: read by absolute lane)
  uint32_t qi = 0;
  uint64_t qb = 0, qe = 0;
  if (on) {
    qi = a.q_sel ? a.q_sel[p.b0 + s] : p.b0 + s;
    qb = a.q_offs[qi]; qe = a.q_len ? qb + a.q_len[qi] : a.q_offs[qi + 1];
  }
  uint32_t* rec = p.rec + (uint64_t)s * SG_PIPE_REC_STRIDE;
  uint32_t* vrec = p.vrec + (uint64_t)s * p.vrec_words;
  const bool first = hl == 0u;                                 // the lane that writes a half's scalars
  auto finish = [&](bool which, uint32_t status) { plan_close(a, p, s, qi, rec, vrec, which && first, status); };

  // ---- tokenise (pkg/suggest/tokenizer.go:9-34), the ASCII path of d_tokenize for two queries side by side ----
  const uint32_t n_w0 = ix.n_wrap0, n_w1 = ix.n_wrap1, q_n = ix.q;
  const AsciiTab tab = d_ascii_tab(ix, (int)lane);
  const uint32_t qlen = on ? (uint32_t)(qe - qb) : 0u;
  const uint32_t R = n_w0 + qlen + n_w1;
  uint32_t* runes = rows;                                      // [SG_PLAN2_RUNES]
  uint64_t* keys = (uint64_t*)(rows + SG_PLAN2_RUNES);         // [32]
  uint32_t* term = rows + SG_PLAN2_RUNES + 64u;                // [32]
  bool simple = on && R <= SG_PLAN2_RUNES && qlen <= 32u;
  {
    bool na = false;
    if (simple && hl < qlen) {
      const uint32_t b = a.q_blob[qb + hl];
      na = b >= 0x80u;
      runes[n_w0 + hl] = (b - 'A' < 26u) ? b + 32u : b;
    }
    simple = simple && h_ballot(na, hb) == 0u;
    if (hl < n_w0) { const uint32_t r = ix.wrap0[hl & (SG_WRAP_MAX - 1)]; runes[hl] = (r - 'A' < 26u) ? r + 32u : r; }            // (ASCII wrap runes: plan2_usable)
    if (hl < n_w1 && R <= SG_PLAN2_RUNES) { const uint32_t r = ix.wrap1[hl & (SG_WRAP_MAX - 1)]; runes[n_w0 + qlen + hl] = (r - 'A' < 26u) ? r + 32u : r; }
  }
  __syncthreads();
  // strings.Trim(text, " "): a text that begins or ends with a space is not a simple one
  if (simple && R > 0u) simple = runes[0] != ' ' && runes[R - 1u] != ' ';
  int A = 0;
  bool empty = false;                                          // fewer bytes than q: no n-grams (ngram_tokenizer.go:18) — rows final
  if (simple) {
    if (R < q_n) empty = true;
    else if (R <= q_n || R - q_n + 1u > 32u) simple = false;   // one short gram / more than 32 grams: sg_plan_kernel's
  }
  uint32_t t_mine = kNoTerm;
  {
    const uint32_t G = simple && !empty ? R - q_n + 1u : 0u;
    const bool valid = hl < G;
    uint32_t w[3] = {0u, 0u, 0u};
    for (uint32_t t = 0; t < q_n && t < 3u; t++) w[t] = valid ? runes[hl + t] : 0u;
    const uint32_t fp = w[0] | (w[1] << 7) | (w[2] << 14) | (valid ? 1u << 21 : 0u);
    // appendUnique (ngram_tokenizer.go:46-54): a gram that occurred before is dropped
    const uint32_t G_max = wave_max_u32(G);
    bool dup = false;
    for (uint32_t h = 0; h + 1u < G_max; h++) dup |= h_read(fp, h, hb) == fp && h < hl;
    const bool keep = valid && !dup;
    const uint32_t km = h_ballot(keep, hb);
    const uint64_t key = d_pack_key_ascii(ix, tab, w, q_n);    // (every lane takes part in the lookups)
    __syncthreads();                                           // (the runes have been read: the keys may land on them? no — their own words; the barrier orders the halves' phases)
    if (keep) keys[h_below(km, hl)] = key;
    A = (int)__builtin_popcount(km);
    __syncthreads();
    if (ix.slots && hl < (uint32_t)A) term[hl] = d_term_lookup(ix, keys[hl]);
    else if (hl < (uint32_t)A) term[hl] = kNoTerm;
    __syncthreads();
    if (hl < (uint32_t)A) t_mine = term[hl];
    __syncthreads();
  }
  finish(on && simple && (empty || A == 0), 0u);
  bool act = on && simple && !empty && A > 0;                  // this half still plans its query here
  // ---- window (suggester.go:53-62) ----
  const int S = (int)ix.S;
  int b_min = 0, W = 0;
  if (act) {
    b_min = d_min_y(a.metric, a.alpha, A, a.mt);
    int b_max = d_max_y(a.metric, a.alpha, A, S, a.mt);
    if (b_max >= S) b_max = S - 1;
    const int span = b_max - b_min + 1;                        // suggester.go:62 make(chan int, span)
    const bool panic = span < 0, dead = span == 0;
    finish(act && panic, SG_COUNT_REF_PANIC);
    finish(act && !panic && dead, SG_COUNT_REF_DEADLOCK);
    b_min = max(b_min, 0);
    W = b_max - b_min + 1;
    const bool none = !panic && !dead && W <= 0;
    finish(act && none, 0u);
    if (panic || dead || none) { act = false; on = false; }
  }
  uint32_t stride = (uint32_t)W + 1u;
  if (act && (W > 32 || (uint32_t)A * stride > p2.rows_cap)) simple = false;
  // a query that is not simple is planned by this wavefront alone behind the pair's work (plan_one_query, below)
  const uint64_t slow = ballot(on && !simple);
  act = act && simple;
  if (ballot(act)) {
  if (!act) { W = 0; A = 0; stride = 1u; }

  // ---- chunk offsets of every query term over the window, rows[term * stride + segment - b_min]: read flat, 32 entries of each
  //      half's table per load, eight loads in flight ----
  const uint32_t S1 = (uint32_t)S + 1u;
  const bool t_ok = act && hl < (uint32_t)A && t_mine != kNoTerm;
  const uint32_t base_mine = t_ok ? t_mine * S1 + (uint32_t)b_min : 0xFFFFFFFFu;
  if (act) { vrec[SG_PIPE_VREC_TERMS + hl] = hl < (uint32_t)A ? t_mine : kNoTerm; vrec[SG_PIPE_VREC_TERMS + 32u + hl] = kNoTerm; }
  {
    const uint32_t n_flat = act ? (uint32_t)A * stride : 0u;                   // <= 1056
    const uint32_t n_flat_max = wave_max_u32(n_flat);
    const uint32_t inv20 = ((1u << 20) + stride - 1u) / stride;
    for (uint32_t f0 = 0; f0 < n_flat_max; f0 += 256u) {
      uint32_t so[8];
      const bool more = f0 + 128u < n_flat_max;                // (a table of <= 128 entries — most queries' — issues four loads, not eight)
      auto entry = [&](uint32_t u) {
        const uint32_t f = f0 + u * 32u + hl;
        const uint32_t t = min(__umul24(f, inv20) >> 20, 31u), w = f - __umul24(t, stride);
        const uint32_t bt = h_read(base_mine, t, hb);
        so[u] = ix.seg_off[(f < n_flat && bt != 0xFFFFFFFFu) ? bt + w : 0u];
      };
#pragma unroll
      for (uint32_t u = 0; u < 4u; u++) entry(u);
      if (more) {
#pragma unroll
        for (uint32_t u = 4; u < 8u; u++) entry(u);
      }
#pragma unroll
      for (uint32_t u = 0; u < 4u; u++) { const uint32_t f = f0 + u * 32u + hl; if (f < n_flat) rows[f] = so[u]; }
      if (more) {
#pragma unroll
        for (uint32_t u = 4; u < 8u; u++) { const uint32_t f = f0 + u * 32u + hl; if (f < n_flat) rows[f] = so[u]; }
      }
    }
  }
  __syncthreads();
  // the posting volume and the present terms of a segment, in its lane
  uint32_t seg_tot = 0, seg_ne = 0;
  {
    // (lane = segment; one step per term, the longer of the two queries' term counts: a lane of the other half, or behind its own
    //  window, adds nothing — its reads stay inside the half's table)
    const uint32_t A_max = wave_max_u32((uint32_t)A);
    const uint32_t A_eff = hl < (uint32_t)W ? (uint32_t)A : 0u;
    const uint32_t last = (uint32_t)max(A, 1) * stride - 2u;                  // the last entry with a successor
    uint32_t at = min(hl, (uint32_t)max(W - 1, 0));
    for (uint32_t i = 0; i < A_max; i++) {
      const uint32_t j = min(at, last);
      const uint32_t x = rows[j], nxt = rows[j + 1u];
      const uint32_t len = i < A_eff ? nxt - x : 0u;
      seg_tot += len;
      seg_ne += len ? 1u : 0u;
      at += stride;
    }
  }
  // ---- thresholds, valid segments, the buckets each would need ----
  const uint32_t max_buckets = 1u << p.log2_cnt;
  int seg_T = 0;
  bool seg_valid = false;
  if (act && hl < (uint32_t)W) {
    const int B = b_min + (int)hl;
    seg_T = d_threshold(a.metric, a.alpha, A, B, a.mt);
    seg_valid = segment_admissible(seg_T, B, A) && (int)seg_ne >= seg_T;   // searcher.go:32
  }
  const uint32_t vmask = h_ballot(seg_valid, hb);
  const uint32_t seg_need = segment_need(seg_valid, seg_T, seg_tot, A, a.t_floor, m16_lane);
  const uint32_t P_need = h_scan_incl(min(seg_need, 1u << 24)), P_tot = h_scan_incl(seg_valid ? seg_tot : 0u);

  // ---- the groups: both halves step through their own, side by side, until both are done ----
  const uint32_t sub = p.sub_log2, G = 1u << sub, dpr = 64u >> sub;
  uint32_t n_items = 0, doff = 0, q_chunks = 0, rows_total = 0, ovf_blk = SG_PIPE_NO_OVF;
  uint32_t wnext = 0;
  bool bail = false;
  for (;;) {
    const uint32_t rest = (act && !bail && wnext < 32u) ? vmask & ~((1u << wnext) - 1u) : 0u;
    const bool go = rest != 0u;                                // this half has another group
    if (!ballot(go)) break;
    const uint32_t g0 = go ? (uint32_t)__builtin_ctz(rest) : 0u;
    // the run of valid segments from g0 on, cut where their bucket needs pass the counters (at least g0 itself)
    const uint32_t gm = g0 ? g0 - 1u : 0u;
    const uint32_t pn = h_read(P_need, gm, hb), pt = h_read(P_tot, gm, hb);
    const uint32_t base_need = g0 ? pn : 0u, base_tot = g0 ? pt : 0u;
    const uint32_t run_len = h_ctz(~vmask >> g0);              // (bits above the half's 32 are zero: at most 32 - g0)
    const uint32_t fit = h_ballot(P_need - base_need <= max_buckets, hb);
    const uint32_t fit_len = h_ctz(~(fit >> g0));
    const uint32_t g1 = min(g0 + max(1u, min(run_len, fit_len)) - 1u, 31u);
    const uint32_t L = h_read(P_tot, g1, hb) - base_tot;        // 16-byte chunks of the group
    const int Tmin = (int)h_read((uint32_t)seg_T, g0, hb);      // (the five metrics' thresholds grow with the segment: the group's lowest is its first segment's)
    wnext = go ? g1 + 1u : 32u;                                // (a half without a group left stays finished)
    // the group's lists: lane i <-> query position i, postings of its term over segments g0 .. g1 (one contiguous run)
    uint32_t ls = 0, ln = 0;
    if (go && hl < (uint32_t)A) { const uint32_t r0 = __umul24(hl, stride); ls = rows[r0 + g0]; ln = rows[r0 + g1 + 1u] - ls; }
    // ---- the longest lists go unread (the pigeonhole behind CPMerge, cp_merge.go:22-31): tiers of relative length, longest first ----
    uint32_t skip_m = 0;
    int Teff = Tmin;
    uint32_t Leff = L;
    {
      const uint32_t n_ne = (uint32_t)__builtin_popcount(h_ballot(ln != 0u, hb));
      const uint32_t x0 = __umul24(min(ln, 0xFFFFFFu), n_ne);
      // The one-query kernel takes the tiers one after the other: of the lists above 2 L / n, then 1.25 L / n, L / n, L / 2 n —
      // longest class first, query order inside a class — as many as the budget allows.  The same picks at once: a list's place
      // in that order is the lists of lower classes plus those of its own class before it.
      const int budget = go && Tmin > a.t_floor ? Tmin - a.t_floor : 0;
      const uint32_t tier = x0 > L * 2u ? 0u : x0 > L + (L >> 2) ? 1u : x0 > L ? 2u : x0 > (L >> 1) ? 3u : 4u;
      const uint32_t m0 = h_ballot(tier == 0u, hb), m1 = h_ballot(tier == 1u, hb), m2 = h_ballot(tier == 2u, hb), m3 = h_ballot(tier == 3u, hb);
      const uint32_t mt = tier == 0u ? m0 : tier == 1u ? m1 : tier == 2u ? m2 : m3;
      const uint32_t lower = tier == 0u ? 0u : tier == 1u ? m0 : tier == 2u ? (m0 | m1) : (m0 | m1 | m2);
      const uint32_t place = (uint32_t)__builtin_popcount(lower) + h_below(mt, hl);
      const uint32_t pick = h_ballot(tier < 4u && (int)place < budget, hb);
      const uint32_t skipped = h_read(h_scan_incl(((pick >> hl) & 1u) ? ln : 0u), 31u, hb);
      const int k_skip = (int)__builtin_popcount(pick);
      const int Tk = Tmin - k_skip;
      const uint32_t m16 = (uint32_t)__builtin_amdgcn_ds_bpermute((Tk < 0 ? 0 : (Tk > 32 ? 32 : Tk)) << 2, (int)m16_lane);
      if (pick && ((min(L - skipped, 1u << 21) * (uint32_t)SG_PPC * m16) >> 4) <= max_buckets) { skip_m = pick; Teff = Tk; Leff = L - skipped; }
    }
    const bool streamed = go && ln != 0u && !((skip_m >> hl) & 1u);
    const uint32_t m16e = (uint32_t)__builtin_amdgcn_ds_bpermute((Teff < 0 ? 0 : (Teff > 32 ? 32 : Teff)) << 2, (int)m16_lane);
    const uint32_t need = (min(Leff, 1u << 21) * (uint32_t)SG_PPC * m16e) >> 4;
    // (a single segment whose postings outnumber what the counters resolve, more groups than a record's 64: the fused kernel's)
    bool stop = go && ((g0 == g1 && need > max_buckets * SG_PIPE_LOOSE) || Teff > 256 || n_items == SG_PIPE_ITEMS);
    const uint32_t lg = min(p.log2_cnt, max(8u, 32u - (uint32_t)__builtin_clz(max(need, 2u) - 1u)));
    // ---- the group's streamed lists, one behind the other in query order ----
    const uint32_t rm = h_ballot(streamed, hb);
    const uint32_t pos = h_below(rm, hl), n_l = (uint32_t)__builtin_popcount(rm);
    const uint32_t nd = streamed ? (ln + G - 1u) >> sub : 0u;
    const uint32_t n_sub = h_read(h_scan_incl(nd), 31u, hb), n_rows = (n_sub + dpr - 1u) / dpr;
    stop = stop || (go && (doff + n_l > SG_PIPE_MAX_LISTS || n_rows > p.dt_rows));
    const bool put = go && !stop && n_l != 0u;
    // lists beyond the record's head: an overflow block (taken by the half's first lane, told to the others)
    const bool want_ovf = put && doff + n_l > SG_PIPE_REC_LISTS && ovf_blk == SG_PIPE_NO_OVF;
    uint32_t blk = SG_PIPE_NO_OVF;
    if (want_ovf && first) blk = atomicAdd(p.ovf_n, 1u);
    blk = h_read(blk, 0u, hb);
    if (want_ovf) { if (blk >= p.ovf_cap) stop = true; else ovf_blk = blk; }
    const bool wr = put && !stop;
    if (wr && streamed) {
      const uint32_t li = doff + pos;
      uint32_t* e = li < SG_PIPE_REC_LISTS ? rec + SG_PIPE_REC_HDR + 2u * li
                                           : p.ovf + (uint64_t)(ovf_blk == SG_PIPE_NO_OVF ? 0u : ovf_blk) * SG_PIPE_OVF_WORDS + SG_PIPE_OVF_HDR + 2u * (li - SG_PIPE_REC_LISTS);
      *(uint2*)e = make_uint2(ls, ln);
    }
    if (wr && first) { rec[4u + n_items] = ((uint32_t)Teff - 1u) | (lg << 8) | (n_l << 12); rec[4u + SG_PIPE_ITEMS + n_items] = doff | (n_rows << 16); }
    if (wr) { n_items++; doff += n_l; rows_total += n_rows; q_chunks += Leff; }
    bail = bail || stop;
  }
  plan_hand_back(p, s, qi, rec, vrec, act && bail && first);
  if (act && !bail && first) {
    *(uint4*)rec = make_uint4(n_items, doff, ovf_blk, rows_total);
    *(uint4*)vrec = make_uint4(0u, qi, (uint32_t)A, 0u);
    p.cand_n[s] = 0u;
    if (a.fill_stat && (qi & a.fill_mask) == 0u) atomicAdd((unsigned long long*)(a.fill_stat + SG_STAT_CHUNKS), (unsigned long long)q_chunks);
    if ((qi & p.stat_mask) == 0u) { atomicAdd(p.stat + SG_STAT_PLANNED, 1u); atomicAdd(p.stat + SG_STAT_GROUPS, n_items); atomicAdd(p.stat + SG_STAT_LISTS, doff); atomicAdd(p.stat + SG_STAT_ROWS, rows_total); }
  }
  }
  // ---- the queries that were not simple (non-ASCII text, more than 32 n-grams or segments, a larger table, text to trim): one at
  //      a time by the whole wavefront, as sg_plan_kernel plans them ----
  if (slow) {
    for (uint32_t h = 0; h < 2u; h++) {
      if (!((slow >> (32u * h)) & 1ull)) continue;
      __syncthreads();                                           // (the halves' tables are this query's scratch now)
      plan_one_query(a, p, 2u * blockIdx.x + h, readlane(qi, (int)(32u * h)), lds, (int)lane, m16_lane);
    }
  }
}
