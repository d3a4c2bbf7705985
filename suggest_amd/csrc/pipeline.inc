// pipeline.inc — the search of an ordinary fuzzy batch as three launches instead of one wavefront per query end to end
// (included by engine.hip, inside namespace sg, behind the fused kernel whose helpers it shares).
//
//   sg_plan_kernel    one wavefront per query: window [MinY, MaxY] (suggester.go:53-59), thresholds
//                     (suggester.go:73-76), the chunk offsets of every query term (searcher.go:38-58), groups of cardinality
//                     segments, the lists the pigeonhole argument lets go unread (cp_merge.go:22-31), the counter geometry —
//                     everything the fused kernel works out between its streams, written to HBM as the query's STREAM RECORD:
//                     items (one per group: flag threshold, bucket bits) and the groups' streamed lists {first chunk, chunks}.
//   sg_stream_kernel  one WORKGROUP of several wavefronts per query — the device's version of the reference's workers over a
//                     query's segments (suggester.go:23,70-110).  The wavefronts share ONE counter array in LDS: u32 counters
//                     (a posting slot costs decode + address + atomic + 3/7 max: 2.4 VALU instructions where the u8 counters
//                     of the fused kernel cost 5.4) and as many buckets as the fused kernel's four-per-word bytes, because the
//                     array belongs to four or eight wavefronts instead of one.  The kernel holds nothing but fetch -> decode
//                     -> atomics -> flag -> push: no tile tables, no verification, no top-k.  Flagged postings go to the
//                     query's candidate slots in its VERIFY RECORD.
//   sg_verify_kernel  one wavefront per query over its candidates: the document's own term list
//                     (forward index) against the query-term hash -> overlap, the threshold of the document's own segment,
//                     1 - Distance in IEEE double (scorer.go:29-31), top-k by (score desc, docID asc) (collector.go:20-26,
//                     topk.go:82-147), rows out.
//
// What makes the wavefronts of a stream workgroup independent of each other's progress: a matching document is in >= Teff of
// the streamed lists, so whichever of its postings is counted LAST finds Teff - 1 in its bucket and is flagged — in any order of
// the atomics.  The fused kernel emitted a document once by the order of its lists ("at its occurrence in the last streamed
// list"); here a document may be pushed several times and the top-k insertion is idempotent instead: a document already in the
// top-k is skipped, and one that was rejected or evicted before is rejected again (the k-th best only improves).  The result is
// the same set under a total order: bit-exact whatever the interleaving.
//
// Queries the plan cannot express (more than 64 n-grams, windows of more than 64 segments, a single segment that needs
// docID-range passes, more groups or descriptors than a record holds) and queries whose candidates overflow their slots are
// listed in fb_list and answered by the fused kernel behind the three launches (its kLoop instantiation, a few thousand
// persistent wavefronts that leave at once when the list is empty).  Results never depend on which path ran.
//
// [r6] Records are compact (1.5 KB + 0.6 KB per query where round 5 kept an 8 KB slot) and a batch goes through in pieces of at
// most SG_PIPE_PIECE queries, so the scratch is bounded.  [tried, profiles/r06c_wpc_sweep_*: the plan and verify launches as
// persistent wavefronts, a static stride of the grid apart, the next query's first loads asked for ahead — plan 246 us against
// 206 for a workgroup per query with the same code, verify 162 against 116, worse with fewer wavefronts: the hardware's
// dispatcher balances queries of unequal weight, a static share does not, and the latency the prefetch hides was hidden by the
// other seven wavefronts of the SIMD already.]

#define SG_PIPE_ITEMS 64u            // groups per query (lane i of a stream wavefront holds item i)
#define SG_PIPE_ROWS_WORDS 1280u     // (5 120 B = four LDS allocation granules: 32 plan wavefronts per CU) seg_off entries (terms x (segments + 1)) a plan wavefront keeps in LDS
#define SG_PIPE_LOOSE 4u             // see the plan: how far a single segment may outnumber the counters before the plan hands the query back
#define SG_PIPE_SKIP 0xC0000000u     // candidates pushed: the query's row is final (status written by the plan, or left to the fallback launch)
#define SG_PIPE_LDS_BYTES 40960u     // a stream workgroup's LDS: 32 allocation granules = four workgroups per CU
#define SG_PIPE_PIECE 65536u         // queries per plan -> stream -> verify round: ~345 MB of records
// A query's STREAM RECORD (4 KB apart): what the plan leaves for the stream workgroup.  Its first 1.5 KB — all of an ordinary
// query of the headline kind (5 groups, 84 lists) — are fetched in ONE memory round trip; a query with more than 126 lists (low
// similarities — every segment admissible, little list skipping —: cfg 3 has 217) has the workgroup fetch what is left of its
// lists behind that.
//   words 0..3      {items, lists, overflow block (SG_PIPE_NO_OVF: none), rows}
//   words 4..131    the items (groups), two arrays of 64: flag threshold - 1 | bucket bits << 8 | lists << 12 ;
//                   first list | rows << 16   (a row = 64 lanes = 64 >> sub_log2 sub-rows; a group starts a new row)
//   words 132..1023 the groups' streamed lists {first chunk, chunks}, group after group: the first 446
// The rare query with more lists takes an OVERFLOW BLOCK (a cursor over a pool of n / 8 blocks; pool empty: the fused kernel
// answers): lists 446..957.
#define SG_PIPE_REC_WORDS 1024u
#define SG_PIPE_REC_FIRST 384u       // words of a record every stream workgroup stages at once
#define SG_PIPE_REC_STRIDE SG_PIPE_REC_WORDS
#define SG_PIPE_REC_HDR 132u
#define SG_PIPE_REC_LISTS ((SG_PIPE_REC_WORDS - SG_PIPE_REC_HDR) / 2u)
#define SG_PIPE_OVF_WORDS 1024u
#define SG_PIPE_OVF_HDR 0u
#define SG_PIPE_MAX_LISTS (SG_PIPE_REC_LISTS + (SG_PIPE_OVF_WORDS - SG_PIPE_OVF_HDR) / 2u)
#define SG_PIPE_NO_OVF 0xFFFFFFFFu
// A query's VERIFY RECORD: whole 128-byte lines, adjacent —
//   line 0          {-, query, n-grams, -, candidates 0..27}   (how many were pushed: PipeArgs::cand_n)
//   lines 1..2      the query's term ids (<= 64)
//   lines 3..       candidates 28 .. cand_cap - 1
#define SG_PIPE_VREC_CAND0 4u
#define SG_PIPE_VREC_HEAD_CANDS 28u
#define SG_PIPE_VREC_TERMS 32u
#define SG_PIPE_VREC_CAND1 96u
__host__ __device__ inline uint32_t sg_pipe_vrec_words(uint32_t cand_cap) {
  return SG_PIPE_VREC_CAND1 + ((cand_cap > SG_PIPE_VREC_HEAD_CANDS ? cand_cap - SG_PIPE_VREC_HEAD_CANDS : 0u) + 31u) / 32u * 32u;
}
__device__ __forceinline__ uint32_t pipe_cand_word(uint32_t c) { return c < SG_PIPE_VREC_HEAD_CANDS ? SG_PIPE_VREC_CAND0 + c : SG_PIPE_VREC_CAND1 - SG_PIPE_VREC_HEAD_CANDS + c; }

struct PipeArgs {
  uint32_t* rec;      // [n][SG_PIPE_REC_WORDS] stream records
  uint32_t* ovf;      // [ovf_cap][SG_PIPE_OVF_WORDS] overflow blocks
  uint32_t* ovf_n;    // blocks taken (zeroed per piece)
  uint32_t* vrec;     // [n][vrec_words] verify records
  uint32_t* cand_n;   // [n] candidates pushed (SG_PIPE_SKIP: nothing to verify) — a dense array of its own: the stream workgroups' fetch-adds
                      // wait for their return, and these lines stay in the L2 where a verify record's first line does not
  uint32_t* fb_n;     // queries listed for the fused kernel (its q_sel_n) ...
  uint32_t* fb_list;  // ... and their indices (its q_sel)
  uint32_t b0, n;     // this round's piece of the batch: positions b0 .. b0 + n - 1 (of the ordered list, or of the batch itself)
  uint32_t ovf_cap, vrec_words;
  uint32_t cand_cap;
  uint32_t sub_log2;  // the stream cuts a list into sub-rows of 2^sub_log2 chunks: a row of 64 lanes = 64 >> sub_log2 of them, so a lane
                      // behind the end of a list idles for 2^sub_log2 - 1 chunks at most
  uint32_t log2_cnt;  // u32 counters of a stream workgroup = buckets a group may use
  uint32_t dt_rows;   // rows (of 64 >> sub_log2 sub-row descriptors) a stream workgroup's LDS table holds: a query's groups together
  // the pipeline's own counters in the replica's statistics block (always on, whatever the tightening sampler does): what it
  // handed back (SG_STAT_UNPLANNED / _OVERFLOW / _REPEATS) and its volumes over the sampled queries ((query & stat_mask) == 0),
  // SG_STAT_PLANNED .. SG_STAT_CANDS
  uint32_t* stat;
  uint32_t stat_mask;
};

// (SG_PHASE_TIMING builds only — tools/gpu_job.sh plan_stages: the plan / verify launch cut short behind stage n, SG_DEBUG_SKIP = n << 20 /
//  n << 24; rows are wrong when set.  PLAN_STAGE stands in plan_one_query alone and closes the slot with that function's `done`; sg_plan2_kernel's
//  own path has no stages, so such a run sets SG_PLAN2=0)
#ifdef SG_PHASE_TIMING
#define PLAN_STAGE(n) if (((a.dbg_skip >> 20) & 15u) == (n)) { done(0u); return; }
#define VERIFY_STAGE(n) if (((a.dbg_skip >> 24) & 15u) == (n)) return;
#else
#define PLAN_STAGE(n)
#define VERIFY_STAGE(n)
#endif
__device__ __forceinline__ uint32_t rfl(uint32_t v) { return (uint32_t)__builtin_amdgcn_readfirstlane((int)v); }
// ------------------------------------------------------------------------------------------
// plan: one wavefront per query slot (slot s of the piece = position b0 + s of the batch / the ordered list)
// ------------------------------------------------------------------------------------------
// ---- how both plan launches close a slot without a plan (`writer`: lane 0 in plan_one_query, the first lane of a half in sg_plan2_kernel) ----
// nothing to stream, nothing to verify: empty records, the candidate count says so
__device__ __forceinline__ void plan_skip_slot(const PipeArgs& p, uint32_t s, uint32_t qi, uint32_t* rec, uint32_t* vrec) {
  p.cand_n[s] = SG_PIPE_SKIP; *(uint4*)vrec = make_uint4(0u, qi, 0u, 0u); *(uint4*)rec = make_uint4(0u, 0u, SG_PIPE_NO_OVF, 0u);
}
// the query's row is final: its count, or the flag of its window or of its length
__device__ __forceinline__ void plan_close(const BatchArgs& a, const PipeArgs& p, uint32_t s, uint32_t qi, uint32_t* rec, uint32_t* vrec, bool writer, uint32_t status) {
  if (writer) { a.out_counts[qi] = status; plan_skip_slot(p, s, qi, rec, vrec); }
}
// the fused kernel answers this query
__device__ __forceinline__ void plan_hand_back(const PipeArgs& p, uint32_t s, uint32_t qi, uint32_t* rec, uint32_t* vrec, bool writer) {
  if (writer) { p.fb_list[atomicAdd(p.fb_n, 1u)] = qi; plan_skip_slot(p, s, qi, rec, vrec); atomicAdd(p.stat + SG_STAT_UNPLANNED, 1u); }
}
// One query planned by one wavefront: slot s of the piece (rows: SG_PIPE_ROWS_WORDS words of LDS; m16_lane: the launch's row of
// kBucketsPer16Postings, lane t holds entry min(t, 32)).  sg_plan_kernel is this and nothing else; sg_plan2_kernel (plan2.inc) calls
// it for the queries its two-per-wavefront path does not take.
__device__ __forceinline__ void plan_one_query(const BatchArgs& a, const PipeArgs& p, const uint32_t s, const uint32_t qi, uint32_t* rows, const int lane, const uint32_t m16_lane) {
  const DeviceIndex& ix = a.ix;
  const uint64_t qb = a.q_offs[qi], qe = a.q_len ? qb + a.q_len[qi] : a.q_offs[qi + 1];
  uint32_t* rec = p.rec + (uint64_t)s * SG_PIPE_REC_STRIDE;
  uint32_t* vrec = p.vrec + (uint64_t)s * p.vrec_words;
  // tokenise (pkg/suggest/tokenizer.go:9-34; the scratch is the segment table's LDS, idle until the term ids are known)
  int A;
  uint32_t t_mine = kNoTerm;
  {
    uint32_t* runes = rows;
    uint64_t* keys = (uint64_t*)(rows + SG_MAX_RUNES);
    uint32_t* term = rows + SG_MAX_RUNES + 2 * SG_MAX_A;
    A = d_tokenize(a, a.q_blob + qb, (uint32_t)(qe - qb), runes, keys, term, lane);
    if (lane < A) t_mine = term[lane];                          // (A > 64: left to the fused kernel below)
    __syncthreads();
  }
  auto done = [&](uint32_t status) { plan_close(a, p, s, qi, rec, vrec, lane == 0, status); };
  auto fallback = [&]() { plan_hand_back(p, s, qi, rec, vrec, lane == 0); };
  PLAN_STAGE(1u)
  if (A < 0) {                                               // beyond the wavefront kernels' tables: sg_long_kernel
    if (lane == 0 && a.long_list) a.long_list[1u + atomicAdd(a.long_list, 1u)] = qi;
    done(SG_COUNT_TOO_LONG);
    return;
  }
  if (A == 0) { done(0u); return; }
  if (a.metric == SG_TABLE && (uint32_t)A > a.mt.a_max) { done(SG_COUNT_TOO_LONG); return; }
  if (A > 64) { fallback(); return; }
  const int S = (int)ix.S;
  int b_min = d_min_y(a.metric, a.alpha, A, a.mt);
  int b_max = d_max_y(a.metric, a.alpha, A, S, a.mt);        // suggester.go:54-59
  if (b_max >= S) b_max = S - 1;
  {
    const int span = b_max - b_min + 1;                      // suggester.go:62 make(chan int, span)
    if (span < 0) { done(SG_COUNT_REF_PANIC); return; }
    if (span == 0) { done(SG_COUNT_REF_DEADLOCK); return; }
  }
  b_min = max(b_min, 0);
  const int W = b_max - b_min + 1;
  if (W <= 0) { done(0u); return; }
  const uint32_t stride = (uint32_t)W + 1u;
  if (W > 63 || (uint32_t)A * stride > SG_PIPE_ROWS_WORDS) { fallback(); return; }

  // ---- chunk offsets of every query term over the window (searcher.go:38-58), rows[term * stride + segment - b_min].  The
  //      table is read FLAT: lane l of load j fetches entry f = 64 j + l — term f / stride, segment f % stride — so a query's
  //      whole table (22 terms x 21 segments: eight loads) is in flight at once: one memory round trip where a load per term,
  //      eight terms at a time, took three.  A term that is not in the dictionary reads entry 0 for every segment: equal
  //      offsets, empty lists. ----
  const uint32_t S1 = (uint32_t)S + 1u;
  const bool t_ok = lane < A && t_mine != kNoTerm;
  const uint32_t base_mine = t_ok ? t_mine * S1 + (uint32_t)b_min : 0xFFFFFFFFu;
  vrec[SG_PIPE_VREC_TERMS + (uint32_t)lane] = lane < A ? t_mine : kNoTerm;    // the term ids, for the verify launch (two whole lines)
  {
    const uint32_t n_flat = (uint32_t)A * stride;                             // <= 1280: f * inv20 stays below 2^32, and (f * inv20) >> 20 == f / stride
    const uint32_t inv20 = ((1u << 20) + stride - 1u) / stride;
    for (uint32_t f0 = 0; f0 < n_flat; f0 += 512u) {
      uint32_t so[8];
#pragma unroll
      for (uint32_t u = 0; u < 8u; u++) {
        const uint32_t f = f0 + u * 64u + (uint32_t)lane;
        const uint32_t t = min(__umul24(f, inv20) >> 20, 63u), w = f - __umul24(t, stride);     // (24-bit operands: v_mul_lo_u32 runs at a quarter of the rate)
        const uint32_t bt = (uint32_t)__builtin_amdgcn_ds_bpermute((int)(t << 2), (int)base_mine);      // (every lane takes part)
        so[u] = ix.seg_off[(f < n_flat && bt != 0xFFFFFFFFu) ? bt + w : 0u];
      }
#pragma unroll
      for (uint32_t u = 0; u < 8u; u++)
        if (f0 + u * 64u < n_flat) rows[f0 + u * 64u + (uint32_t)lane] = so[u];      // (uniform; the table's 1280 words are whole loads)
    }
  }
  __syncthreads();
  PLAN_STAGE(2u)
  // the posting volume and the present terms of a segment, in its lane
  uint32_t seg_tot = 0, seg_ne = 0;
  {
    const uint32_t* r = rows + min(lane, W - 1);
    for (int i = 0; i < A; i++) {
      const uint32_t x = r[(uint32_t)i * stride], nxt = r[(uint32_t)i * stride + 1u];
      const uint32_t len = lane < W ? nxt - x : 0u;
      seg_tot += len;
      seg_ne += len ? 1u : 0u;
    }
  }
  __syncthreads();
  PLAN_STAGE(3u)

  // ---- thresholds, valid segments, the buckets each would need (as the fused kernel: equal-length estimate of what list
  //      skipping leaves) ----
  const uint32_t max_buckets = 1u << p.log2_cnt;
  int seg_T = 0;
  bool seg_valid = false;
  if (lane < W) {
    const int B = b_min + lane;
    seg_T = d_threshold(a.metric, a.alpha, A, B, a.mt);
    seg_valid = segment_admissible(seg_T, B, A) && (int)seg_ne >= seg_T;   // searcher.go:32
  }
  const uint64_t vmask = ballot(seg_valid);
  const uint32_t seg_need = segment_need(seg_valid, seg_T, seg_tot, A, a.t_floor, m16_lane);
  const uint32_t P_need = wave_scan_incl(min(seg_need, 1u << 24), lane), P_tot = wave_scan_incl(seg_valid ? seg_tot : 0u, lane);
  PLAN_STAGE(4u)

  const uint32_t sub = p.sub_log2, G = 1u << sub, dpr = 64u >> sub;
  uint32_t n_items = 0, doff = 0, q_chunks = 0, rows_total = 0, ovf_blk = SG_PIPE_NO_OVF;
  uint32_t* ovf = nullptr;
  bool bail = false;
  int wnext = 0;
  while (wnext < W) {
    const uint64_t rest = (vmask >> wnext) << wnext;
    if (!rest) break;
    const int g0 = __builtin_ctzll(rest);
    // the run of valid segments from g0 on, cut where their bucket needs pass the counters (at least g0 itself)
    const uint32_t base_need = g0 ? readlane(P_need, g0 - 1) : 0u, base_tot = g0 ? readlane(P_tot, g0 - 1) : 0u;
    const uint64_t inv = ~vmask >> g0;
    const int run_len = inv ? __builtin_ctzll(inv) : 64 - g0;
    const uint64_t unfit = ~(ballot(P_need - base_need <= max_buckets) >> g0);
    const int fit_len = unfit ? __builtin_ctzll(unfit) : 64;
    const int g1 = g0 + max(1, min(run_len, fit_len)) - 1;
    const uint32_t L = readlane(P_tot, g1) - base_tot;        // 16-byte chunks of the group
    // (the thresholds of the five metrics of pkg/metric grow with the segment: the group's lowest is its first segment's; a
    //  tabulated metric may do anything)
    const int Tmin = a.metric == SG_TABLE ? wave_min_i32((lane >= g0 && lane <= g1) ? seg_T : 0x7FFFFFFF) : (int)readlane((uint32_t)seg_T, g0);
    wnext = g1 + 1;
    // the group's lists: lane i <-> query position i, postings of its term over segments g0 .. g1 (one contiguous run)
    uint32_t ls = 0, ln = 0;
    if (lane < A) { const uint32_t r0 = __umul24((uint32_t)lane, stride); ls = rows[r0 + (uint32_t)g0]; ln = rows[r0 + (uint32_t)g1 + 1u] - ls; }
    // ---- the longest lists go unread (the pigeonhole behind CPMerge, cp_merge.go:22-31): a document in >= T of the n lists
    //      is in >= T - k of any n - k of them.  Tiers of relative length, longest first, as the fused kernel. ----
    uint64_t skip_m = 0;
    int Teff = Tmin;
    uint32_t Leff = L;
    if (Tmin > a.t_floor) {
      const uint32_t n_ne = popc64(ballot(ln != 0u));
      const uint32_t th[4] = {L * 2u, L + (L >> 2), L, L >> 1};
      uint64_t pick = 0;
      int budget = Tmin - a.t_floor;
      const uint32_t x0 = __umul24(min(ln, 0xFFFFFFu), n_ne);     // (which lists go unread never shows in the rows: a list of 2^24 chunks and more is ranked as one of 2^24 - 1)
#pragma unroll
      for (int f = 0; f < 4; f++) {
        if (budget > 0) {
          const uint64_t m = ballot(x0 > th[f]) & ~pick;
          const uint32_t rank = lane_rank(m);
          const uint64_t keep = m & ballot((int)rank < budget);        // (mask arithmetic is scalar: no per-lane test of m's bit)
          pick |= keep;
          budget -= (int)popc64(keep);
        }
      }
      if (pick) {
        const uint32_t skipped = readlane(wave_scan_incl(((pick >> lane) & 1ull) ? ln : 0u, lane), 63);
        const int k_skip = (int)popc64(pick);
        if (buckets_needed(min(L - skipped, 1u << 21) * (uint32_t)SG_PPC, Tmin - k_skip, m16_lane) <= max_buckets) { skip_m = pick; Teff = Tmin - k_skip; Leff = L - skipped; }
      }
    }
    const bool streamed = ln != 0u && !((skip_m >> lane) & 1ull);
    const uint32_t need = buckets_needed(min(Leff, 1u << 21) * (uint32_t)SG_PPC, Teff, m16_lane);
    // A single segment whose postings outnumber what the counters resolve: the fused kernel streams it in docID-range passes.
    // Here up to SG_PIPE_LOOSE x the buckets the filter table asks for are let through on the full array — the table is about
    // how many flagged postings are no matches, never about matches: the verify launch sorts them out, and a query that
    // overflows its candidate slots goes to the fused kernel like any other.  Beyond that: the fused kernel's business.
    if ((g0 == g1 && need > max_buckets * SG_PIPE_LOOSE) || Teff > 256) { bail = true; break; }
    const uint32_t lg = min(p.log2_cnt, max(8u, 32u - (uint32_t)__builtin_clz(max(need, 2u) - 1u)));   // smallest power of two >= need, within [2^8, the array]
    if (n_items == SG_PIPE_ITEMS) { bail = true; break; }
    // ---- the group's streamed lists, one behind the other in query order (the stream workgroup cuts them into sub-rows of
    //      2^sub chunks — rows of 64 lanes, a group starts a new row — and keeps the sub-rows of ALL the query's groups in LDS) ----
    const uint64_t rm = ballot(streamed);
    const uint32_t pos = lane_rank(rm), n_l = popc64(rm);
    const uint32_t nd = streamed ? (ln + G - 1u) >> sub : 0u;
    const uint32_t n_sub = readlane(wave_scan_incl(nd, lane), 63), n_rows = (n_sub + dpr - 1u) / dpr;
    if (doff + n_l > SG_PIPE_MAX_LISTS || n_rows > p.dt_rows) { bail = true; break; }     // (a group's sub-rows fit the stream workgroup's table; a query's need not: windows)
    if (n_l) {
      if (doff + n_l > SG_PIPE_REC_LISTS && ovf_blk == SG_PIPE_NO_OVF) {       // lists beyond the record's head: an overflow block
        uint32_t blk = 0;
        if (lane == 0) blk = atomicAdd(p.ovf_n, 1u);
        blk = rfl(blk);
        if (blk >= p.ovf_cap) { bail = true; break; }
        ovf_blk = blk;
        ovf = p.ovf + (uint64_t)blk * SG_PIPE_OVF_WORDS;
      }
      if (doff + n_l <= SG_PIPE_REC_LISTS) {                       // (uniform: the whole group in the record's head — all of an ordinary query)
        if (streamed) *(uint2*)(rec + SG_PIPE_REC_HDR + 2u * (doff + pos)) = make_uint2(ls, ln);
      } else if (streamed) {
        const uint32_t li = doff + pos;
        uint32_t* e = li < SG_PIPE_REC_LISTS ? rec + SG_PIPE_REC_HDR + 2u * li : ovf + SG_PIPE_OVF_HDR + 2u * (li - SG_PIPE_REC_LISTS);
        *(uint2*)e = make_uint2(ls, ln);
      }
      if (lane == 0) {
        const uint32_t w1 = ((uint32_t)Teff - 1u) | (lg << 8) | (n_l << 12), w2 = doff | (n_rows << 16);
        rec[4u + n_items] = w1; rec[4u + SG_PIPE_ITEMS + n_items] = w2;
      }
      n_items++;
      doff += n_l;
      rows_total += n_rows;
      q_chunks += Leff;
    }
  }
  if (bail) { fallback(); return; }
  if (lane == 0) {
    *(uint4*)rec = make_uint4(n_items, doff, ovf_blk, rows_total);
    *(uint4*)vrec = make_uint4(0u, qi, (uint32_t)A, 0u);
    p.cand_n[s] = 0u;
    if (a.fill_stat && (qi & a.fill_mask) == 0u) atomicAdd((unsigned long long*)(a.fill_stat + SG_STAT_CHUNKS), (unsigned long long)q_chunks);
    if ((qi & p.stat_mask) == 0u) { atomicAdd(p.stat + SG_STAT_PLANNED, 1u); atomicAdd(p.stat + SG_STAT_GROUPS, n_items); atomicAdd(p.stat + SG_STAT_LISTS, doff); atomicAdd(p.stat + SG_STAT_ROWS, rows_total); }
  }
}

__global__ __launch_bounds__(64) __attribute__((amdgpu_num_sgpr(80))) void sg_plan_kernel(const BatchArgs a, const PipeArgs p) {   // (80: see sg_stream_kernel)
  __shared__ __attribute__((aligned(16))) uint32_t rows[SG_PIPE_ROWS_WORDS];
  const int lane = threadIdx.x;
  const uint32_t s = blockIdx.x;
  uint32_t qi = p.b0 + s;
  if (a.q_sel) {                                             // (both loads issued together: one memory round trip at the head of every query)
    const uint32_t sel_n = *a.q_sel_n, sel_q = a.q_sel[p.b0 + s];
    if (p.b0 + s >= rfl(sel_n)) return;
    qi = rfl(sel_q);
  }
  const uint32_t m16_lane = kBucketsPer16Postings[a.filter_level][min(lane, 32)];   // (a load from memory: asked for here, used behind the tokeniser's round trips)
  plan_one_query(a, p, s, qi, rows, lane, m16_lane);
}

// ------------------------------------------------------------------------------------------
// stream: one workgroup of NW wavefronts per query slot
// ------------------------------------------------------------------------------------------
// Counts one row: an LDS atomic per posting slot on a u32 counter (padding included: phantom postings in buckets of their own,
// packed_store.inc), issued back to back and waited for once.  A lane behind the end of its sub-row holds a copy of its last
// chunk: it adds 0, to counter word `lane` (a bank of its own).  Returns the ballot of lanes that met a count >= Tm1.
__device__ __forceinline__ uint64_t pipe_count_row(const uint4& v, uint32_t live, uint32_t amask, uint32_t cbase, uint32_t lane4, uint32_t Tm1,
                                                   uint32_t (&pp)[SG_PPC], uint32_t (&old)[SG_PPC]) {
  const uint32_t g[SG_PPC] = {0u, v.y & 0xFFFFu, v.y >> 16, v.z & 0xFFFFu, v.z >> 16, v.w & 0xFFFFu, v.w >> 16};
  const uint32_t am = live ? amask : 0u;
  const uint32_t cb = cbase | (live ? 0u : lane4);                  // (the counters are aligned to their size, as counter_word has it: | is +, and folds where cbase is 0)
  uint32_t d = v.x & SG_X_MASK;
#pragma unroll
  for (int e = 0; e < SG_PPC; e++) {
    if (e) d += g[e];
    pp[e] = d;
    old[e] = __hip_atomic_fetch_add(counter_word(d, am, cb), live, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
  }
  __builtin_amdgcn_s_waitcnt(0xC07F);   // lgkmcnt(0): one wait for all the returns
  uint32_t mu = 0;
#pragma unroll
  for (int e = 0; e < SG_PPC; e++) mu = max(mu, old[e]);
  return ballot(live && mu >= Tm1);
}

// A workgroup barrier that waits for this wavefront's LDS operations only — __syncthreads() carries a fence that also waits for
// the row loads in flight (vmcnt(0)), which is exactly what the stream must not do at a group boundary.
__device__ __forceinline__ void pipe_lds_barrier() { asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory"); }

// sub-row descriptors of the stream workgroup's LDS table: {first chunk | chunks << 26} in 4 bytes, or — kWide: stores of 2^26
// chunks (1 GiB) and more — {first chunk, chunks} in 8
template <bool kWide> struct PipeDesc;
template <> struct PipeDesc<false> {
  typedef uint32_t T;
  static __device__ __forceinline__ T make(uint32_t chunk, uint32_t n) { return chunk | (n << 26); }
  static __device__ __forceinline__ uint32_t chunk(T d) { return d & 0x3FFFFFFu; }
  static __device__ __forceinline__ uint32_t n(T d) { return d >> 26; }
};
template <> struct PipeDesc<true> {
  typedef uint2 T;
  static __device__ __forceinline__ T make(uint32_t chunk, uint32_t n) { return make_uint2(chunk, n); }
  static __device__ __forceinline__ uint32_t chunk(T d) { return d.x; }
  static __device__ __forceinline__ uint32_t n(T d) { return d.y; }
};

// One workgroup of NW wavefronts per query slot.  LDS: the counters | (in the counters' words, before the first group clears
// them) the staged stream record | the sub-row table of the query's groups | a dead descriptor.
// amdgpu_num_sgpr(80): at 82 .. 96 scalar registers the hardware admits 7 wavefronts per SIMD, not the 8 the compiler reports
// (MI355X_MICROARCH.md, "Residency") — three workgroups of eight wavefronts per CU instead of four.
// [tried, profiles/r05n_*: persistent workgroups that prefetch the next query's record and keep a row load in flight across
//  queries — the compiler moves a register whose load is in flight at every control-flow merge, whatever the asm constraints
//  (plain, tied, physical): correct only by luck of the allocation, and with the hardware balancing one workgroup per query the
//  launch is 12 % faster than a static share and as fast as a dynamic one.]
template <int NW, bool kWide>
__global__ __launch_bounds__(NW * 64) __attribute__((amdgpu_num_sgpr(80))) void sg_stream_kernel(const BatchArgs a, const PipeArgs p) {
  extern __shared__ __attribute__((aligned(16))) uint32_t smem[];
  typedef PipeDesc<kWide> PD;
  typedef typename PD::T Desc;
  const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = rfl(tid >> 6);
  const uint32_t s = blockIdx.x;
  if (a.q_sel && p.b0 + s >= rfl(*a.q_sel_n)) return;
  const uint32_t cnt_words = 1u << p.log2_cnt;
  uint32_t* cnt = smem;
  const uint32_t cbase = (uint32_t)(uintptr_t)(lds_u32*)cnt;
  uint32_t* S = cnt;                                            // (the staged record lies in the counters' words: read before the first group clears them)
  const uint32_t sub = p.sub_log2, G = 1u << sub, dpr = 64u >> sub, dcap = p.dt_rows * dpr;
  Desc* D = (Desc*)(cnt + max(cnt_words, SG_PIPE_REC_WORDS));   // [dcap], then the dead descriptor
  const uint32_t my_sub = lane >> sub, my_off = lane & (G - 1u);
  const uint4* __restrict__ post4 = (const uint4*)a.ix.postings;
  const uint32_t* rec = p.rec + (uint64_t)s * SG_PIPE_REC_STRIDE;
  // ---- the stream record: one round trip (two for a query whose lists pass the first 1.5 KB) ----
  auto stage = [&]() {
    for (uint32_t w = tid; w < SG_PIPE_REC_FIRST / 2u; w += NW * 64u) ((uint2*)S)[w] = ((const uint2*)rec)[w];
    __syncthreads();
    const uint32_t end = min(SG_PIPE_REC_WORDS, SG_PIPE_REC_HDR + 2u * rfl(S[1]));       // (words 0 .. end of the record are in use)
    if (end > SG_PIPE_REC_FIRST) {
      for (uint32_t w = SG_PIPE_REC_FIRST / 2u + tid; w < (end + 1u) / 2u; w += NW * 64u) ((uint2*)S)[w] = ((const uint2*)rec)[w];
      __syncthreads();
    }
  };
  if (tid == 0u) D[dcap] = PD::make(0u, 0u);
  stage();
  const uint32_t n_items = rfl(S[0]);
  if (n_items == 0u) return;
  const uint32_t ovf_blk = rfl(S[2]);
  const uint32_t* ovf = p.ovf + (uint64_t)(ovf_blk == SG_PIPE_NO_OVF ? 0u : ovf_blk) * SG_PIPE_OVF_WORDS;
  // lane i of every wavefront: item i
  uint32_t w1_mine = 0u, w2_mine = 0u;
  if (lane < n_items) { w1_mine = S[4u + lane]; w2_mine = S[4u + SG_PIPE_ITEMS + lane]; }
  const uint32_t rows_mine = w2_mine >> 16;
  const uint32_t r_incl = wave_scan_incl(rows_mine, (int)lane);                // rows of the query's groups up to and with this one
  uint32_t* vrec = p.vrec + (uint64_t)s * p.vrec_words;
  typedef u32x4v u32x4;
  uint32_t it_on = 0xFFFFFFFFu, Tm1 = 0, amask = 0;

  // [r6] The LDS table holds the sub-rows of a WINDOW of consecutive groups — all of an ordinary query's; a query that streams
  // more rows than the table holds (dictionaries of tens of millions of strings) goes through in several windows: the
  // table is cut anew (the record staged again: its words were the counters'), the row loop runs over the window's groups and
  // drains.  The plan lets no single group pass the table.
  uint32_t win_lo = 0u;
  while (win_lo < n_items) {
    const uint32_t r_base = win_lo ? readlane(r_incl, (int)win_lo - 1) : 0u;
    const uint32_t win_hi = win_lo + max(1u, popc64(ballot(lane >= win_lo && lane < n_items && r_incl - r_base <= p.dt_rows)));
    const uint32_t r0_mine = r_incl - rows_mine - r_base;                      // first row of this lane's group inside the window's table
    if (win_lo) { __syncthreads(); stage(); }                                 // (everybody has counted the window before)
    // ---- the window's groups cut into sub-rows {first chunk, chunks}: wavefront w cuts groups w, w + NW, ...; lane l the group's
    //      list l (a group has a list per query position at most), its first sub-row by a scan over the lists before it ----
    for (uint32_t it = win_lo + wave; it < win_hi; it += NW) {
      const uint32_t w1 = readlane(w1_mine, (int)it), w2 = readlane(w2_mine, (int)it);
      const uint32_t n_l = w1 >> 12, loff = w2 & 0xFFFFu, D0 = readlane(r0_mine, (int)it) * dpr, n_d = (w2 >> 16) * dpr;
      // the list's entry {first chunk, chunks}: an LDS read where the whole group lies in the staged record (every group of a
      // query without an overflow block), else the record's entries from LDS and the block's from memory — never a flat load
      u32x2v e = {0u, 0u};
      const uint32_t li = loff + lane;
      const lds_u32x2* e_rec = (const lds_u32x2*)(lds_u32*)(S + SG_PIPE_REC_HDR) + li;
      if (__builtin_expect(loff + n_l <= SG_PIPE_REC_LISTS, 1)) {
        if (lane < n_l) e = *e_rec;
      } else {
        const glb_u32x2* e_ovf = (const glb_u32x2*)(ovf + SG_PIPE_OVF_HDR) + (li - SG_PIPE_REC_LISTS);
        if (lane < n_l && li < SG_PIPE_REC_LISTS) e = *e_rec;
        if (lane < n_l && li >= SG_PIPE_REC_LISTS) e = *e_ovf;
        asm volatile("" : "+v"(e));                                        // (the block's entries waited for here: the record's path waits for its LDS read alone)
      }
      uint32_t ls = e.x, ln = e.y;
      const uint32_t nd = (ln + G - 1u) >> sub;
      const uint32_t incl = wave_scan_incl(nd, (int)lane), total = readlane(incl, 63);
      for (uint32_t d = D0 + incl - nd; ln; d++) {                        // (the lanes with sub-rows left to write: no bound over the wavefront)
        const uint32_t n = min(G, ln);
        D[d] = PD::make(ls, n);
        ls += G; ln -= n;
      }
      if (total + lane < n_d) D[D0 + total + lane] = PD::make(0u, 0u);   // what is left of the group's last row
    }
    __syncthreads();

    // ---- the rows: wavefront w takes rows w, w + NW, ... of every group, one after the other, the next row's load in flight while
    //      one is counted — across group boundaries too: loads do not touch the counters.  A group is entered by all wavefronts
    //      together (barrier, counters cleared, barrier), whether they have rows in it or not. ----
    u32x4 v, vn;
    uint32_t live = 0, liven = 0;
    auto seek = [&](uint32_t& it, uint32_t& r) { while (it < win_hi && r >= readlane(rows_mine, (int)it)) { it++; r = wave; } };
    auto fetch = [&](uint32_t it, uint32_t r, u32x4& vv, uint32_t& lv) {
      const uint32_t j_d = it < win_hi ? (readlane(r0_mine, (int)it) + r) * dpr + my_sub : dcap;   // (dcap: the dead descriptor)
      const Desc dsc = D[j_d];
      const uint32_t n = PD::n(dsc);
      lv = my_off < n ? 1u : 0u;
      const uint32_t ci = PD::chunk(dsc) + min(my_off, n ? n - 1u : 0u);
      if (kWide) {                                                   // (a 64-bit address per lane: the byte offset passes 2^32)
        const uint64_t addr = (uint64_t)(uintptr_t)post4 + ((uint64_t)ci << 4);
        asm volatile("global_load_dwordx4 %0, %1, off" : "=&v"(vv) : "v"(addr) : "memory");
      } else {
        const uint32_t boff = ci << 4;                               // (the store is below 2^26 chunks: the host picks kWide otherwise)
        asm volatile("global_load_dwordx4 %0, %1, %2" : "=&v"(vv) : "v"(boff), "s"(post4) : "memory");
      }
    };
    auto enter = [&](uint32_t it) {                                 // all wavefronts, once per group, in order
      while ((int32_t)it_on < (int32_t)it) {
        it_on++;
        const uint32_t pk = readlane(w1_mine, (int)it_on), lg = (pk >> 8) & 15u;
        pipe_lds_barrier();                                         // everybody has counted the group before
        for (uint32_t w = tid * 4u; w < (1u << lg); w += NW * 256u) *(uint4*)(cnt + w) = make_uint4(0u, 0u, 0u, 0u);
        pipe_lds_barrier();
        Tm1 = pk & 255u; amask = ((1u << lg) - 1u) << 2;
      }
    };
    auto count = [&](u32x4& qv, uint32_t pl) {
      asm volatile("s_waitcnt vmcnt(1)" : "+v"(qv) :: "memory");
      const uint4 pv = make_uint4(qv.x, qv.y, qv.z, qv.w);
      uint32_t pp[SG_PPC], old[SG_PPC];
      if (pipe_count_row(pv, pl, amask, cbase, lane << 2, Tm1, pp, old)) {
        // the flagged postings (real ones: the slots behind a chunk's last posting are padding) go to the query's candidate
        // slots: one fetch-add on its counter for the row.  (A matching document is flagged at every one of its postings counted
        // behind the (Teff - 1)-th — half a dozen pushes per match; the verify launch takes each distinct document once.
        // [tried, profiles/r06q_*: a 64-entry LDS table of the documents pushed lately to leave the repeats out — 10.7 -> 6.5
        // pushes per headline query, verify 75 -> 72 us, and the seven extra LDS reads of a flagged row cost the stream more.])
        uint32_t mine_bits = 0;
#pragma unroll
        for (int e = 0; e < SG_PPC; e++)
          if (pl && old[e] >= Tm1 && (uint32_t)e <= (pv.x >> 29)) mine_bits |= 1u << e;
        const uint32_t mine_n = (uint32_t)__builtin_popcount(mine_bits);
        const uint32_t incl = wave_scan_incl(mine_n, (int)lane), n_push = readlane(incl, 63);
        if (n_push) {
          uint32_t base = 0;
          if (lane == 0u) base = atomicAdd(p.cand_n + s, n_push);
          base = rfl(base);
          uint32_t pos = base + incl - mine_n;
#pragma unroll
          for (int e = 0; e < SG_PPC; e++)
            if ((mine_bits >> e) & 1u) { if (pos < p.cand_cap) vrec[pipe_cand_word(pos)] = pp[e]; pos++; }
        }
      }
    };
    uint32_t c_it = win_lo, c_r = wave;
    seek(c_it, c_r);
    fetch(c_it, c_r, v, live);
    while (c_it < win_hi) {
      uint32_t n_it = c_it, n_r = c_r + NW;
      seek(n_it, n_r);
      fetch(n_it, n_r, vn, liven);
      enter(c_it);
      count(v, live);
      if (n_it >= win_hi) break;
      c_it = n_it; c_r = n_r + NW;
      seek(c_it, c_r);
      fetch(c_it, c_r, v, live);
      enter(n_it);
      count(vn, liven);
    }
    // The dead-row prefetch: nothing may be in flight into v / vn once the compiler takes them for dead — the barriers below clear
    // counters out of whatever registers it likes (seen in the ISA: v[0:3] as the zero vector with a load into v[2:5] in flight; the
    // counters of the last groups were "cleared" with postings).  The row registers are operands of the wait: live until here.
    asm volatile("s_waitcnt vmcnt(0)" : "+v"(v), "+v"(vn) :: "memory");
    enter(win_hi - 1u);                                             // (the groups behind this wavefront's last row: their barriers)
    win_lo = win_hi;
  }
}

// ------------------------------------------------------------------------------------------
// verify + score + top-k: one wavefront per query slot
// ------------------------------------------------------------------------------------------
#define SG_PIPE_QH 160u   // slots of the query-term hash (A <= 64 occurrences)
// kBigK: k above SG_K_LDS — the top-k working rows live in HBM (BatchArgs::scratch_s / scratch_id, as the fused kernel's).  Its own
// instantiation: with one kernel for both, the rows' pointers are generic and every access of the LDS rows a flat one
// (verify 77 -> 87 us on cfg 2, profiles/r06f_timeline_cfg2.txt).
// One query verified by one wavefront: slot s of the piece.  LDS: the query-term hash, the top-k rows (k <= SG_K_LDS; kBigK: rows in
// HBM), seg_base / fx_base (64 entries each).  sg_verify_kernel_t is this and nothing else.  [tried, profiles/r06z6_*, r06z7_*: two
// queries per wavefront as in the plan launch (a candidate's terms across 32 lanes, top-k rows in registers; the kernel is kept as
// profiles/r06z7_verify2_two_queries_per_wavefront.inc.txt) — bit-exact and not a microsecond faster: this launch was bound by its
// vector instructions, not its scalar ones, and the half-wavefront form turns the scalar work into more of the former.]
template <bool kBigK>
__device__ __forceinline__ void verify_one_query(const BatchArgs& a, const PipeArgs& p, const uint32_t s, const int lane, uint32_t* qh_key, uint32_t* tk_id_lds,
                                                 uint64_t* tk_s_lds, uint32_t* sb_lds, uint32_t* fb_lds) {
  const DeviceIndex& ix = a.ix;
  const uint32_t k = a.k;
  const int S = (int)ix.S;
  // [r6] a candidate's term list by address arithmetic (packed_store.inc pk_fwd_strided): its segment from seg_base — a table
  // this wavefront loads beside the verify record —, its list at fx_base[B] + (x - seg_base[B]) * ceil(B / 4); without the
  // table (more than 63 segments) the document's forward-index record is fetched first, a memory round trip more
  const bool strided = ix.fx_base != nullptr;
  uint32_t sb_load = 0u, fb_load = 0u;
  if (strided && lane <= S) { sb_load = ix.seg_base[lane]; fb_load = ix.fx_base[lane]; }
  // everything the wavefront needs first is in the query's verify record: ONE memory round trip (header, term ids, candidates)
  const uint32_t* vr = p.vrec + (uint64_t)s * p.vrec_words;
  const uint32_t sel_n = a.q_sel ? *a.q_sel_n : a.n_q;
  struct First { uint32_t h, t, c; } f;
  const uint32_t n_c_v = p.cand_n[s];
  f.h = vr[lane & 3];
  f.t = vr[SG_PIPE_VREC_TERMS + (uint32_t)lane];
  f.c = (uint32_t)lane < p.cand_cap ? vr[pipe_cand_word((uint32_t)lane)] : 0u;
  if (p.b0 + s >= rfl(sel_n)) return;
  const uint32_t n_c = rfl(n_c_v), qi = readlane(f.h, 1);
  if (n_c >= SG_PIPE_SKIP) return;                            // status written by the plan / the fused kernel answers
  if (n_c > p.cand_cap) {                                     // more flagged postings than the slots hold: the fused kernel answers
    if (lane == 0) { p.fb_list[atomicAdd(p.fb_n, 1u)] = qi; atomicAdd(p.stat + SG_STAT_OVERFLOW, 1u); }
    return;
  }
  const bool sampled = a.fill_stat && (qi & a.fill_mask) == 0u;
  if (lane == 0 && n_c && (qi & p.stat_mask) == 0u) atomicAdd(p.stat + SG_STAT_CANDS, n_c);
  if (n_c == 0u) {
    if (lane == 0) { a.out_counts[qi] = 0u; if (sampled) atomicAdd(a.fill_stat + SG_STAT_SAMPLED, 1u); }
    return;
  }
  VERIFY_STAGE(1u)
  const int A = (int)readlane(f.h, 2);                         // 1 .. 64 (the plan let it through)
  const uint32_t t_mine = lane < A ? f.t : kNoTerm;
  for (uint32_t i = lane; i < SG_PIPE_QH; i += 64) qh_key[i] = kNoTerm;                           // the query-term hash (d_qhash)
  if (strided) { sb_lds[lane] = lane <= S ? sb_load : 0xFFFFFFFFu; fb_lds[lane] = fb_load; }      // (S <= 63: entries 0 .. S, then sentinels)
  __syncthreads();
  if (t_mine != kNoTerm)
    for (uint32_t h = d_qhash<SG_PIPE_QH>(t_mine);; h = d_qnext<SG_PIPE_QH>(h))
      if (atomicCAS(qh_key + h, kNoTerm, t_mine) == kNoTerm) break;
  __syncthreads();
  // (No window test here: a candidate is a posting of a list the plan streamed, and the plan streams lists of admissible
  //  segments only — MinY <= B <= MaxY, 0 < T(B) <= min(A, B), suggester.go:53-59,76 — so its document's segment is one of them.)
  VERIFY_STAGE(2u)
  TopK tk;
  if (kBigK) topk_begin(tk, a.scratch_s + (uint64_t)qi * k, a.scratch_id + (uint64_t)qi * k, k);
  else topk_begin(tk, tk_s_lds, tk_id_lds, k);
  bool give_up = false;
  for (uint32_t base = 0; base < n_c && !give_up; base += 64) {
    const uint32_t n_raw = min(64u, n_c - base);
    uint32_t my_doc = (uint32_t)lane < n_raw ? (base == 0u ? f.c : vr[pipe_cand_word(base + (uint32_t)lane)]) : 0xFFFFFFFFu;
    // [r6] A matching document is pushed by every one of its postings counted behind the (Teff - 1)-th: half a dozen slots per
    // match (11 slots for 1 result on the headline).  Each distinct document once: the first occurrences, moved to the front.
    uint32_t n = n_raw;
    if (n_raw > 1u) {
      bool dup = false;
      for (uint32_t i = 0; i + 1u < n_raw; i++) dup |= readlane(my_doc, (int)i) == my_doc && i < (uint32_t)lane;
      const uint64_t keep = ballot((uint32_t)lane < n_raw && !dup);
      const uint32_t to = lane_rank(keep);
      const bool mine = (keep >> lane) & 1ull;
      my_doc = (uint32_t)__builtin_amdgcn_ds_permute((int)((mine ? to : 63u) << 2), (int)my_doc);   // (lanes that send nothing aim at lane 63: it holds a first occurrence only if all 64 are distinct, and then sends to itself)
      n = popc64(keep);
      if ((uint32_t)lane >= n) my_doc = 0xFFFFFFFFu;
    }
    uint2 rec = make_uint2(0u, 0u);
    uint32_t my_orig = 0u;
    if ((uint32_t)lane < n) {
      my_orig = ix.orig_of[my_doc];
      if (strided) {
        // the segment B with seg_base[B] <= x < seg_base[B + 1]: the last table entry <= x (entries behind S are sentinels)
        uint32_t B = 0u;                                           // (seg_base[0] = 0, seg_base[S] = documents > x)
#pragma unroll
        for (uint32_t step = 32u; step; step >>= 1) { const uint32_t t = B + step; if (sb_lds[t & 63u] <= my_doc && t < 64u) B = t; }
        rec = make_uint2(fb_lds[B] + (my_doc - sb_lds[B]) * ((B + 3u) >> 2), B | (B << 16));      // (distinct terms <= B; empty slots hold kNoTerm)
      } else rec = ix.fwd_rec[my_doc];
    }
    const uint32_t nd_max = wave_max_u32(rec.y >> 16);
    const int lgs = nd_max <= 8u ? 3 : nd_max <= 16u ? 4 : nd_max <= 32u ? 5 : 6, gsz = 1 << lgs, ngrp = 64 >> lgs;
    const int gi = lane >> lgs, ti = lane & (gsz - 1);
    const uint64_t gmask = gsz == 64 ? ~0ull : ((1ull << gsz) - 1ull) << (gi << lgs);
    // lanes are (candidate, term slot) pairs, 64 / gsz candidates side by side; the next iteration's term loads are issued
    // before this one's are used
    auto fetch_terms = [&](uint32_t c0, uint32_t s0, uint32_t& x_nd) -> uint32_t {
      const uint32_t cc = c0 + (uint32_t)gi;
      const int src = (int)(min(cc, 63u) << 2);
      uint32_t x_off = (uint32_t)__builtin_amdgcn_ds_bpermute(src, (int)rec.x);
      const uint32_t ry = (uint32_t)__builtin_amdgcn_ds_bpermute(src, (int)rec.y);
      asm volatile("" : "+v"(x_off) : "v"(ry));                  // (the permutes stay unpredicated: a switched-off source lane returns 0)
      x_nd = cc < n ? ry >> 16 : 0u;
      const uint32_t slot = s0 + (uint32_t)ti;
      return slot < x_nd ? ix.fwd_terms[(uint64_t)x_off * 4u + slot] : kNoTerm;
    };
    const uint32_t rounds = (nd_max + (uint32_t)gsz - 1u) >> lgs;            // 1 unless a document has more than 64 distinct terms
    uint32_t n_nd;
    uint32_t x_next = fetch_terms(0u, 0u, n_nd);
    uint32_t my_ov = 0;                                          // lane c <- overlap of candidate c
    for (uint32_t c0 = 0; c0 < n; c0 += (uint32_t)ngrp) {
      int ov = 0;
      for (uint32_t rd = 0; rd < rounds; rd++) {
        const uint32_t x = x_next;
        const bool last_rd = rd + 1u == rounds;
        if (!last_rd || c0 + (uint32_t)ngrp < n) x_next = fetch_terms(last_rd ? c0 + (uint32_t)ngrp : c0, last_rd ? 0u : (rd + 1u) * (uint32_t)gsz, n_nd);
        uint32_t mult = 0;
        if (x != kNoTerm)
          for (uint32_t h = d_qhash<SG_PIPE_QH>(x);; h = d_qnext<SG_PIPE_QH>(h)) {
            const uint32_t kx = qh_key[h];
            if (kx == kNoTerm) break;
            if (kx == x) mult++;
          }
        const uint64_t mm = ballot(mult != 0u);
        ov += (int)popc64(mm & gmask);
        uint64_t m2 = ballot(mult > 1u);                         // a query that repeats a term: the extra occurrences
        while (m2) {
          const int l = __builtin_ctzll(m2);
          m2 &= m2 - 1;
          const uint32_t extra = readlane(mult, l) - 1u;
          if ((l >> lgs) == gi) ov += (int)extra;
        }
      }
      // the group's overlap -> the candidate's own lane
#pragma unroll 1
      for (int g = 0; g < ngrp; g++) {
        const uint32_t o = readlane((uint32_t)ov, g << lgs);
        if ((uint32_t)lane == c0 + (uint32_t)g) my_ov = o;
      }
    }
    VERIFY_STAGE(3u)
    // lane c <-> candidate c: the threshold of the document's own segment, the top-k key
    const int B = (int)(rec.y & 0xFFFFu);
    bool pass = false;
    uint64_t key = 0;
    if ((uint32_t)lane < n) {
      const int T = d_threshold(a.metric, a.alpha, A, B, a.mt);
      pass = (int)my_ov >= T;
      if (pass) key = score_bits(d_score(a.metric, (int)my_ov, A, B, a.mt));
    }
    // a document that repeats a term has secondary entries (SURVEY.md §A.3): the fused kernel's per-list view
    if (ix.n_dup_docs) {
      const bool dupd = pass && ((ix.dup_bits[my_orig >> 5] >> (my_orig & 31u)) & 1u);
      if (ballot(dupd)) { give_up = true; break; }
    }
    uint64_t m = ballot(pass);
    while (m) {
      if (tk.n == k) { m &= ballot(better(key, my_orig, tk.worst_s, tk.worst_id)); if (!m) break; }
      const int l = __builtin_ctzll(m);
      m &= m - 1;
      const uint32_t d = readlane(my_orig, l);
      // idempotent: a document already in the top-k was pushed before (by another of its postings)
      __syncthreads();
      bool held = false;
      for (uint32_t i = (uint32_t)lane; i < tk.n; i += 64u) held |= tk.id[i] == d;
      if (ballot(held)) continue;
      const uint64_t ks = (uint64_t)readlane((uint32_t)key, l) | ((uint64_t)readlane((uint32_t)(key >> 32), l) << 32);
      topk_insert(tk, ks, d, lane);
    }
    __syncthreads();
  }
  if (give_up) {
    if (lane == 0) { p.fb_list[atomicAdd(p.fb_n, 1u)] = qi; atomicAdd(p.stat + SG_STAT_REPEATS, 1u); }
    return;
  }
  VERIFY_STAGE(4u)
  // ---- GetCandidates (topk.go:127-147): best first (rank sort, out of place) ----
  __syncthreads();
  uint32_t* out_ids = a.out_ids + (uint64_t)qi * k;
  double* out_scores = a.out_scores ? a.out_scores + (uint64_t)qi * k : nullptr;
  const uint32_t n = tk.n;
  for (uint32_t i = (uint32_t)lane; i < n; i += 64u) {
    const uint64_t sc = tk.s[i];
    const uint32_t d = tk.id[i];
    uint32_t rank = 0;
    for (uint32_t j = 0; j < n; j++) {
      const uint64_t sj = tk.s[j];
      const uint32_t dj = tk.id[j];
      rank += (better(sj, dj, sc, d) || (sj == sc && dj == d && j < i)) ? 1u : 0u;
    }
    out_ids[rank] = d;
    if (out_scores) out_scores[rank] = bits_score(sc);
  }
  if (lane == 0) {
    a.out_counts[qi] = n;
    if (sampled) { atomicAdd(a.fill_stat + SG_STAT_SAMPLED, 1u); if (n == k) atomicAdd(a.fill_stat + SG_STAT_FULL, 1u); if (n) atomicAdd(a.fill_stat + SG_STAT_RESULTS, n); }
  }
}

template <bool kBigK>
__global__ __launch_bounds__(64) __attribute__((amdgpu_num_sgpr(80))) void sg_verify_kernel_t(const BatchArgs a, const PipeArgs p) {   // (80: see sg_stream_kernel)
  __shared__ uint32_t qh_key[SG_PIPE_QH];
  __shared__ uint32_t tk_id_lds[SG_K_LDS];
  __shared__ uint64_t tk_s_lds[SG_K_LDS];
  __shared__ uint32_t sb_lds[64], fb_lds[64];                 // seg_base / fx_base, entries 0 .. S (dictionaries of <= 63 segments)
  verify_one_query<kBigK>(a, p, blockIdx.x, (int)threadIdx.x, qh_key, tk_id_lds, tk_s_lds, sb_lds, fb_lds);
}
#define sg_verify_kernel sg_verify_kernel_t<false>
#define sg_verify_kernel_bigk sg_verify_kernel_t<true>
