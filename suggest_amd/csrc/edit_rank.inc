// edit_rank.inc — result rows ranked by edit distance against the dictionary held in HBM (include/suggest_hip.h; DESIGN.md §5d),
// included by engine.hip after dict_rows.inc (it uses its DictView, sg_dictionary, dict_check_geometry and t_dict, host_call.inc's
// run_host_call / IoCall / search_io, search_api.inc's search_req and no_long_queries, handles.inc's open_search, capi.inc's
// launch, stream_scratch, Carve and the poison, d_next_rune, d_lower_pairs, kCountFlagMin, HIP_TRY).
//
// The second stage of the classical q-gram count filter: the rows a search returned are verified and ranked by Levenshtein or
// optimal-string-alignment distance between the query and each candidate's string.  The result is the exact top-k by edit distance
// AMONG THE CANDIDATES THE Q-GRAM SEARCH RETURNED, not over the whole dictionary.
//   distances  edit_short_kernel: a wavefront per row, four rows per workgroup.  The row's query (<= 64 runes) becomes Myers' Peq in
//              LDS — an open-addressed table of 128 slots keyed by rune — then a lane per candidate decodes its string from the
//              dictionary rune by rune and advances the Myers / Hyyrö bit-vector recurrence on one 64-bit (Pv, Mv) pair in
//              registers.  A query of more than 64 runes is put on the call's list of long rows (a flag per row, no host round trip).
//              edit_long_kernel: a workgroup per long row out of a fixed grid, each with a region of the call's scratch: the query's
//              (rune, position) pairs sorted there, from them Peq as a sorted list of the distinct runes plus w = ceil(m / 64) masks
//              per rune, looked up by binary search (a query whose masks pass the region's share — 65 536 distinct runes would take
//              512 MiB — walks the sorted pairs instead), and the blocked recurrence with w words per candidate laid out
//              [block][lane], the horizontal carry running block to block inside the lane.  The number of regions follows a byte
//              budget (kEditSliceBytes; sg_debug_edit_slice_bytes): the grid's workgroups take the long rows in slices of that many.
//   re-rank    edit_rerank_kernel: rows of a fixed stride of <= 1 024 slots, a workgroup per row, ranks counted in LDS:
//              rank(p) = #{j : d_j < d_p} + #{j < p : d_j = d_p} — distinct, so no two lanes store to one slot (the argument of
//              sg_shard_merge_kernel).  Wider and ragged rows: one stable radix sort of (row, distance) keys over the call's slots
//              and a scatter.  Either way the permuted row is complete in LDS / scratch before a slot of it is written.
// Scratch: one block of the calling thread's per-stream scratch (SCRATCH_EDIT).  The _device entry points write nothing of any handle.

namespace sg {

constexpr uint32_t kEditNone = 0xFFFFFFFFu;           // the distance of a slot that holds no entry, of an id outside the dictionary
constexpr uint32_t kEditRowsPerGroup = 4;             // rows (wavefronts) of an edit_short_kernel workgroup
constexpr uint32_t kEditPeqSlots = 128;               // slots of a row's Peq table: <= 64 keys
constexpr uint32_t kEditShortBytes = 256;             // 64 runes are 256 bytes at most
constexpr uint32_t kEditMaxQueryBytes = 65536;        // the engine's limit of a query
constexpr uint32_t kEditRankSlots = 1024;             // widest row edit_rerank_kernel ranks in LDS
constexpr uint64_t kEditSliceBytes = (uint64_t)64 << 20;   // budget of the long kernel's regions
constexpr uint64_t kEditMaskWords = (uint64_t)2 << 20;     // words of Peq masks a region holds at most (16 MiB): distinct runes x blocks

struct EditLower { const uint32_t* lower_from; const uint32_t* lower_to; uint32_t n_lower; };   // as d_lower_pairs reads it

// ---- the recurrence, one statement for both kernels and the host check (sg_debug_edit_bitvector) ----

// Hash of a rune into the Peq table (tests/edit_ref.py: peq_hash restates it to choose colliding runes)
__host__ __device__ inline uint32_t edit_peq_hash(uint32_t r) { return (r * 0x9E3779B1u) >> 25; }
__host__ __device__ inline void edit_peq_insert(uint32_t* keys, uint64_t* masks, uint32_t r, uint64_t bit) {
  uint32_t h = edit_peq_hash(r);
  while (keys[h] != kEditNone && keys[h] != r) h = (h + 1u) & (kEditPeqSlots - 1u);
  keys[h] = r; masks[h] |= bit;
}
__host__ __device__ inline uint64_t edit_peq_find(const uint32_t* keys, const uint64_t* masks, uint32_t r) {   // an absent rune: 0
  uint32_t h = edit_peq_hash(r);
  for (;;) {
    const uint32_t k = keys[h];
    if (k == r) return masks[h];
    if (k == kEditNone) return 0;
    h = (h + 1u) & (kEditPeqSlots - 1u);
  }
}

// One 64-row block of one column of Hyyrö's formulation of Myers' recurrence (D0 = the diagonal zero deltas), with his term for a
// transposition of two adjacent runes under osa.  eq / eqp: the block's match masks of this column's rune and of the previous one.
// hp_c / hn_c: the horizontal deltas shifted in at bit 0 (the block below's bit 63; the first block's: +1, 0), tr_c: bit 63 of the
// block below's ~D0_old & eq.  hp / hn: the block's horizontal deltas before the shift (the score is read from them).
__host__ __device__ inline void edit_block_step(bool osa, uint64_t eq, uint64_t eqp, uint64_t& pv, uint64_t& mv, uint64_t& d0, uint64_t& hp_c,
                                                uint64_t& hn_c, uint64_t& tr_c, uint64_t& hp, uint64_t& hn) {
  const uint64_t x = eq | hn_c;
  uint64_t nd0 = (((x & pv) + pv) ^ pv) | x | mv;
  if (osa) { const uint64_t t = ~d0 & eq; nd0 |= ((t << 1) | tr_c) & eqp; tr_c = t >> 63; }
  hp = mv | ~(nd0 | pv); hn = nd0 & pv;
  const uint64_t hps = (hp << 1) | hp_c, hns = (hn << 1) | hn_c;
  hp_c = hp >> 63; hn_c = hn >> 63;
  pv = hns | ~(nd0 | hps); mv = hps & nd0; d0 = nd0;
}

// the first of srt[0 .. n) (ascending rune << 32 | position) whose rune is >= r
__host__ __device__ inline uint32_t edit_srt_lower(const uint64_t* srt, uint32_t n, uint32_t r) {
  const uint64_t key = (uint64_t)r << 32;
  uint32_t lo = 0, hi = n;
  while (lo < hi) { const uint32_t mid = lo + (hi - lo) / 2u; if (srt[mid] < key) lo = mid + 1u; else hi = mid; }
  return lo;
}
// Where a pair's (Pv, Mv, D0) words lie: word k of block b at p[k * plane + b * stride] — the kernel: stride = lanes, the host: 1
struct EditState { uint64_t* p; uint64_t stride, plane; __host__ __device__ uint64_t& at(uint32_t k, uint32_t b) const { return p[k * plane + b * stride]; } };
// One column of the blocked recurrence over a query of m runes (w blocks): rune c after rune cp (kEditNone: the first column).
// A block's masks are gathered from the runs of c and cp in the sorted pairs, whose positions ascend.
__host__ __device__ inline void edit_long_column(bool osa, const uint64_t* srt, uint32_t n_srt, uint32_t c, uint32_t cp, uint32_t m, uint32_t w,
                                                 const EditState& st, uint32_t& score) {
  uint32_t cur = edit_srt_lower(srt, n_srt, c), pcur = (osa && cp != kEditNone) ? edit_srt_lower(srt, n_srt, cp) : n_srt;
  uint64_t hp_c = 1, hn_c = 0, tr_c = 0, hp = 0, hn = 0;
  for (uint32_t b = 0; b < w; b++) {
    const uint64_t end = ((uint64_t)c << 32) | ((uint64_t)b * 64u + 64u), pend = ((uint64_t)cp << 32) | ((uint64_t)b * 64u + 64u);
    uint64_t eq = 0, eqp = 0;
    while (cur < n_srt && srt[cur] < end) { eq |= 1ull << (srt[cur] & 63u); cur++; }
    if (osa) while (pcur < n_srt && srt[pcur] < pend) { eqp |= 1ull << (srt[pcur] & 63u); pcur++; }
    edit_block_step(osa, eq, eqp, st.at(0, b), st.at(1, b), st.at(2, b), hp_c, hn_c, tr_c, hp, hn);
  }
  const uint32_t last = (m - 1u) & 63u;
  score += (uint32_t)((hp >> last) & 1u);
  score -= (uint32_t)((hn >> last) & 1u);
}
// The same column where the query's Peq fits the region as whole words: drune[0 .. n_d) the query's distinct runes, ascending, and
// masks[rank * w + b] the match mask of rune `rank` in block b.  rk / rkp: the ranks of the column's rune and of the previous one
// (edit_rune_rank; kEditNone: not a rune of the query, or no previous column) — one load per block instead of a walk over the pairs.
__host__ __device__ inline uint32_t edit_rune_rank(const uint32_t* drune, uint32_t n_d, uint32_t r) {
  uint32_t lo = 0, hi = n_d;
  while (lo < hi) { const uint32_t mid = lo + (hi - lo) / 2u; if (drune[mid] < r) lo = mid + 1u; else hi = mid; }
  return lo < n_d && drune[lo] == r ? lo : kEditNone;
}
__host__ __device__ inline void edit_long_column_dense(bool osa, const uint64_t* masks, uint32_t rk, uint32_t rkp, uint32_t m, uint32_t w, const EditState& st,
                                                       uint32_t& score) {
  uint64_t hp_c = 1, hn_c = 0, tr_c = 0, hp = 0, hn = 0;
  for (uint32_t b = 0; b < w; b++) {
    const uint64_t eq = rk != kEditNone ? masks[(uint64_t)rk * w + b] : 0ull, eqp = osa && rkp != kEditNone ? masks[(uint64_t)rkp * w + b] : 0ull;
    edit_block_step(osa, eq, eqp, st.at(0, b), st.at(1, b), st.at(2, b), hp_c, hn_c, tr_c, hp, hn);
  }
  const uint32_t last = (m - 1u) & 63u;
  score += (uint32_t)((hp >> last) & 1u);
  score -= (uint32_t)((hn >> last) & 1u);
}

// ---- the kernels ----

struct EditArgs {
  DictView d;
  EditLower low;
  const uint8_t* q_blob; const uint64_t* q_offs;     // row i belongs to query i
  const uint32_t* ids; const uint32_t* counts; const uint64_t* row_offs;   // row_offs null: rows of `row` slots
  uint32_t n_rows, row;
  uint32_t* dist;                                    // [slots], filled with kEditNone before the launch
  unsigned long long* info;                          // [1]: entries with an id outside the dictionary
  uint32_t* long_list;                               // [0] how many rows are long (zeroed per call), then their numbers
  int osa, fold;
  // the long kernel's regions: region g = [sorted pairs: long_pairs u64 | state: 3 planes of long_w blocks x 64 lanes u64 | distinct
  // runes: long_pairs u32 | masks: long_mask_words u64]
  uint8_t* long_mem; uint64_t long_region, long_mask_words; uint32_t long_pairs, long_w;
};

__device__ __forceinline__ void edit_row_geometry(const EditArgs& a, uint32_t i, uint64_t* begin, uint32_t* n_ent) {
  const uint64_t b = a.row_offs ? a.row_offs[i] : (uint64_t)i * a.row, len = a.row_offs ? a.row_offs[i + 1] - b : (uint64_t)a.row;
  const uint32_t c = a.counts[i];
  *begin = b;
  *n_ent = c >= kCountFlagMin ? 0u : (len < (uint64_t)c ? (uint32_t)len : c);
}
__device__ __forceinline__ uint32_t edit_upto4(uint64_t n) { return n < 4u ? (uint32_t)n : 4u; }   // the bytes d_next_rune may look at
__device__ __forceinline__ uint32_t edit_fold(const EditArgs& a, uint32_t r) { return a.fold ? d_lower_pairs(a.low, r) : r; }

__global__ __launch_bounds__(64 * kEditRowsPerGroup) void edit_short_kernel(const EditArgs a) {
  __shared__ uint64_t s_mask[kEditRowsPerGroup][kEditPeqSlots];
  __shared__ uint32_t s_key[kEditRowsPerGroup][kEditPeqSlots];
  __shared__ uint32_t s_m[kEditRowsPerGroup];
  __shared__ uint8_t s_q[kEditRowsPerGroup][kEditShortBytes];
  const uint32_t wv = threadIdx.x / 64u, lane = threadIdx.x % 64u;
  for (uint64_t base = (uint64_t)blockIdx.x * kEditRowsPerGroup; base < a.n_rows; base += (uint64_t)gridDim.x * kEditRowsPerGroup) {
    const uint64_t i64 = base + wv;
    const uint32_t i = (uint32_t)i64;
    uint64_t begin = 0, qlen = 0;
    uint32_t n_ent = 0;
    const uint8_t* q = nullptr;
    if (i64 < a.n_rows) {
      edit_row_geometry(a, i, &begin, &n_ent);
      q = a.q_blob + a.q_offs[i];
      qlen = a.q_offs[i + 1] - a.q_offs[i];
    }
    const bool is_short = n_ent != 0u && qlen <= kEditShortBytes;
    if (is_short) {
      for (uint32_t t = lane; t < (uint32_t)qlen; t += 64u) s_q[wv][t] = q[t];
      for (uint32_t t = lane; t < kEditPeqSlots; t += 64u) { s_key[wv][t] = kEditNone; s_mask[wv][t] = 0; }
    }
    __syncthreads();
    if (lane == 0u) {                                 // Peq: the distinct folded runes and the bit mask of each one's positions
      uint32_t m = n_ent != 0u && !is_short ? 65u : 0u;
      if (is_short) {
        uint32_t p = 0;
        while (p < (uint32_t)qlen) {
          uint32_t adv;
          const uint32_t r = edit_fold(a, d_next_rune(&s_q[wv][p], (uint32_t)qlen - p, &adv));
          p += adv;
          if (m == 64u) { m = 65u; break; }
          edit_peq_insert(s_key[wv], s_mask[wv], r, 1ull << m);
          m++;
        }
      }
      s_m[wv] = m;
      if (m > 64u) a.long_list[1u + atomicAdd(a.long_list, 1u)] = i;
    }
    __syncthreads();
    const uint32_t m = s_m[wv];
    if (n_ent != 0u && m <= 64u) {
      const uint64_t last = m ? 1ull << (m - 1u) : 0ull;
      for (uint32_t pos = lane; pos < n_ent; pos += 64u) {      // a lane per candidate; wider rows are strided over
        const uint64_t s = begin + pos;
        const uint32_t id = a.ids[s];
        if (id >= a.d.n_docs) { atomicAdd(a.info + 1, 1ull); continue; }
        const uint64_t from = a.d.doc_offs[id], to = a.d.doc_offs[(uint64_t)id + 1];
        uint64_t pv = ~0ull, mv = 0, d0 = 0, eqp = 0;
        uint32_t score = m;
        for (uint64_t at = from; at < to;) {
          uint32_t adv;
          const uint32_t r = edit_fold(a, d_next_rune(a.d.blob + at, edit_upto4(to - at), &adv));
          at += adv;
          if (m == 0u) { score++; continue; }           // an empty query: the candidate's rune count
          const uint64_t eq = edit_peq_find(s_key[wv], s_mask[wv], r);
          uint64_t hp_c = 1, hn_c = 0, tr_c = 0, hp, hn;
          edit_block_step(a.osa != 0, eq, eqp, pv, mv, d0, hp_c, hn_c, tr_c, hp, hn);
          score += (hp & last) != 0ull;
          score -= (hn & last) != 0ull;
          eqp = eq;
        }
        a.dist[s] = score;
      }
    }
    __syncthreads();                                   // (the next group of rows rebuilds the tables)
  }
}

// A workgroup of one wavefront per long row, out of a grid of as many workgroups as there are regions.
__global__ __launch_bounds__(64) void edit_long_kernel(const EditArgs a) {
  __shared__ uint8_t s_buf[64 + 4];
  __shared__ uint32_t s_ctl[2];                        // bytes the decoder took of the chunk; runes so far
  const uint32_t lane = threadIdx.x;
  const uint32_t n_long = min(a.long_list[0], a.n_rows);
  uint64_t* srt = (uint64_t*)(a.long_mem + (uint64_t)blockIdx.x * a.long_region);
  const EditState st{srt + a.long_pairs + lane, 64u, (uint64_t)a.long_w * 64u};
  uint32_t* drune = (uint32_t*)(srt + a.long_pairs + 3ull * a.long_w * 64u);
  uint64_t* masks = (uint64_t*)(drune + a.long_pairs);
  for (uint32_t li = blockIdx.x; li < n_long; li += gridDim.x) {
    const uint32_t i = a.long_list[1u + li];
    uint64_t begin;
    uint32_t n_ent;
    edit_row_geometry(a, i, &begin, &n_ent);
    const uint8_t* q = a.q_blob + a.q_offs[i];
    const uint64_t qlen = a.q_offs[i + 1] - a.q_offs[i];
    if (qlen > (uint64_t)a.long_pairs) {               // beyond the regions (a query above the engine's limit): no distance, counted
      if (lane == 0u) atomicAdd(a.info + 1, (unsigned long long)n_ent);
      continue;
    }
    // the query's folded runes as rune << 32 | position, decoded from 64-byte pieces in LDS (a rune may reach 3 bytes past one)
    if (lane == 0u) s_ctl[1] = 0u;
    for (uint64_t base = 0; base < qlen;) {
      __syncthreads();
      if (base + lane < qlen) s_buf[lane] = q[base + lane];
      if (lane < 4u && base + 64u + lane < qlen) s_buf[64u + lane] = q[base + 64u + lane];
      __syncthreads();
      if (lane == 0u) {
        uint32_t p = 0, m = s_ctl[1];
        while (p < 64u && base + p < qlen) {
          uint32_t adv;
          const uint32_t r = edit_fold(a, d_next_rune(&s_buf[p], edit_upto4(qlen - base - p), &adv));
          p += adv;
          srt[m] = ((uint64_t)r << 32) | m;
          m++;
        }
        s_ctl[0] = p; s_ctl[1] = m;
      }
      __syncthreads();
      base += s_ctl[0];
    }
    __syncthreads();
    const uint32_t m = s_ctl[1];
    uint32_t P = 64u;
    while (P < m) P <<= 1;
    for (uint32_t t = m + lane; t < P; t += 64u) srt[t] = ~0ull;
    __syncthreads();
    for (uint32_t k = 2u; k <= P; k <<= 1) {           // bitonic sort of the P pairs (distinct keys)
      for (uint32_t j = k >> 1; j > 0u; j >>= 1) {
        for (uint32_t t = lane; t < P / 2u; t += 64u) {
          const uint32_t lo = ((t & ~(j - 1u)) << 1) | (t & (j - 1u)), hi = lo | j;
          const uint64_t x = srt[lo], y = srt[hi];
          if ((x > y) == ((lo & k) == 0u)) { srt[lo] = y; srt[hi] = x; }
        }
        __syncthreads();
      }
    }
    const uint32_t w = (m + 63u) / 64u;
    // Peq as whole words where it fits the region: the distinct runes in order (the first pair of every run, ranked by a ballot
    // scan), then every pair ORs its bit into its rune's row of w masks
    uint32_t n_d = 0;
    for (uint32_t base = 0; base < m; base += 64u) {
      const uint32_t t = base + lane;
      const bool first = t < m && (t == 0u || (uint32_t)(srt[t] >> 32) != (uint32_t)(srt[t - 1u] >> 32));
      const uint64_t bal = ballot(first);
      if (first) drune[n_d + popc64(bal & ((1ull << lane) - 1ull))] = (uint32_t)(srt[t] >> 32);
      n_d += popc64(bal);
    }
    const bool dense = (uint64_t)n_d * w <= a.long_mask_words;
    if (dense) for (uint64_t t = lane; t < (uint64_t)n_d * w; t += 64u) masks[t] = 0ull;
    __syncthreads();
    if (dense) for (uint32_t t = lane; t < m; t += 64u) {
      const uint64_t key = srt[t];
      const uint32_t at = (uint32_t)key;
      atomicOr((unsigned long long*)&masks[(uint64_t)edit_rune_rank(drune, n_d, (uint32_t)(key >> 32)) * w + (at >> 6)], 1ull << (at & 63u));
    }
    __syncthreads();
    for (uint32_t pos = lane; pos < n_ent; pos += 64u) {
      const uint64_t s = begin + pos;
      const uint32_t id = a.ids[s];
      if (id >= a.d.n_docs) { atomicAdd(a.info + 1, 1ull); continue; }
      const uint64_t from = a.d.doc_offs[id], to = a.d.doc_offs[(uint64_t)id + 1];
      for (uint32_t b = 0; b < w; b++) { st.at(0, b) = ~0ull; st.at(1, b) = 0; st.at(2, b) = 0; }
      uint32_t score = m, prev = kEditNone, prev_rk = kEditNone;
      for (uint64_t at = from; at < to;) {
        uint32_t adv;
        const uint32_t r = edit_fold(a, d_next_rune(a.d.blob + at, edit_upto4(to - at), &adv));
        at += adv;
        if (dense) {
          const uint32_t rk = edit_rune_rank(drune, n_d, r);
          edit_long_column_dense(a.osa != 0, masks, rk, prev_rk, m, w, st, score);
          prev_rk = rk;
        } else edit_long_column(a.osa != 0, srt, m, r, prev, m, w, st, score);
        prev = r;
      }
      a.dist[s] = score;
    }
    __syncthreads();                                   // (the next row sorts into the same region)
  }
}

// The stable re-rank of rows of a fixed stride of <= kEditRankSlots slots: a workgroup per row, 4 slots per thread at most.
__global__ __launch_bounds__(256) void edit_rerank_kernel(uint32_t* __restrict__ ids, double* __restrict__ scores, uint32_t* __restrict__ dist,
                                                          uint32_t* __restrict__ counts, uint32_t n_rows, uint32_t row, uint32_t max_distance, uint32_t k_out) {
  __shared__ uint32_t s_d[kEditRankSlots];
  for (uint32_t i = blockIdx.x; i < n_rows; i += gridDim.x) {
    const uint32_t c = counts[i];
    if (c >= kCountFlagMin) continue;                  // a flagged row passes through untouched (uniform: no barrier is skipped by some)
    const uint32_t n_ent = min(c, row);
    const uint64_t begin = (uint64_t)i * row;
    uint32_t my_id[4], my_d[4];
    double my_s[4];
#pragma unroll
    for (uint32_t u = 0; u < 4u; u++) {
      const uint32_t p = threadIdx.x + u * blockDim.x;
      my_id[u] = 0; my_d[u] = kEditNone; my_s[u] = 0;
      if (p < n_ent) { my_id[u] = ids[begin + p]; my_d[u] = dist[begin + p]; if (scores) my_s[u] = scores[begin + p]; }
      if (p < row) s_d[p] = my_d[u];
    }
    __syncthreads();
    uint32_t rank[4] = {0, 0, 0, 0}, kept = 0;
    for (uint32_t j = 0; j < n_ent; j++) {
      const uint32_t dj = s_d[j];
      kept += dj <= max_distance;
#pragma unroll
      for (uint32_t u = 0; u < 4u; u++) rank[u] += dj < my_d[u] || (dj == my_d[u] && j < threadIdx.x + u * blockDim.x);
    }
    const uint32_t newc = min(kept, k_out);
    __syncthreads();                                   // (every slot of the row is in registers or LDS: now it may be written)
#pragma unroll
    for (uint32_t u = 0; u < 4u; u++) {
      const uint32_t p = threadIdx.x + u * blockDim.x;
      if (p < n_ent && rank[u] < newc) { ids[begin + rank[u]] = my_id[u]; dist[begin + rank[u]] = my_d[u]; if (scores) scores[begin + rank[u]] = my_s[u]; }
      if (p >= newc && p < row) { ids[begin + p] = 0; dist[begin + p] = 0; if (scores) scores[begin + p] = 0; }
    }
    if (threadIdx.x == 0u) counts[i] = newc;
    __syncthreads();
  }
}

// ---- wider and ragged rows: (row, distance) keys over the call's slots, a stable sort, a scatter ----

// the row a slot lies in: *rk = row + 1 (a slot behind row r's last and before the next row's first: r + 1 too; before the first
// row: 0; behind the last fixed-stride row: n_rows + 1), true when the slot is one of the row's
__device__ __forceinline__ bool edit_slot_row(const uint64_t* row_offs, uint32_t n_rows, uint32_t row, uint64_t s, uint32_t* rk, uint32_t* i, uint64_t* pos,
                                              uint64_t* row_len) {
  *rk = 0; *i = 0; *pos = 0; *row_len = 0;
  if (!n_rows) return false;
  if (row_offs) {
    uint32_t lo = 0, hi = n_rows;
    while (hi - lo > 1u) { const uint32_t mid = lo + (hi - lo) / 2u; if (row_offs[mid] <= s) lo = mid; else hi = mid; }
    const uint64_t b = row_offs[lo], e = row_offs[lo + 1];
    if (s < b) return false;
    *rk = lo + 1u; *i = lo; *pos = s - b; *row_len = e - b;
    return s < e;
  }
  if (!row) return false;
  const uint64_t r = s / row;
  if (r >= n_rows) { *rk = n_rows + 1u; return false; }
  *rk = (uint32_t)r + 1u; *i = (uint32_t)r; *pos = s - r * row; *row_len = row;
  return true;
}

__global__ __launch_bounds__(256) void edit_keys_kernel(const uint32_t* __restrict__ dist, const uint32_t* __restrict__ counts, const uint64_t* __restrict__ row_offs,
                                                        uint32_t n_rows, uint32_t row, uint64_t slots, uint32_t max_distance, uint64_t* __restrict__ keys,
                                                        uint32_t* __restrict__ vals, uint32_t* __restrict__ kept) {
  for (uint64_t s = (uint64_t)blockIdx.x * 256u + threadIdx.x; s < slots; s += (uint64_t)gridDim.x * 256u) {
    uint32_t rk, i;
    uint64_t pos, row_len;
    uint32_t dk = kEditNone;
    if (edit_slot_row(row_offs, n_rows, row, s, &rk, &i, &pos, &row_len)) {
      const uint32_t c = counts[i];
      if (c >= kCountFlagMin) dk = 0;                  // a flagged row: equal keys, the sort leaves it as it is
      else if (pos < c) { dk = dist[s]; if (dk <= max_distance) atomicAdd(kept + i, 1u); }
    } else if (rk == 0u) dk = 0;
    keys[s] = ((uint64_t)rk << 32) | dk;
    vals[s] = (uint32_t)s;
  }
}

// sorted position j takes what slot src[j] held; a row's slots from its new count on are zeroed; what lies in no row, and a flagged
// row, is copied as it is
__global__ __launch_bounds__(256) void edit_scatter_kernel(const uint32_t* __restrict__ src, const uint32_t* __restrict__ ids, const double* __restrict__ scores,
                                                           const uint32_t* __restrict__ dist, const uint32_t* __restrict__ counts, const uint64_t* __restrict__ row_offs,
                                                           uint32_t n_rows, uint32_t row, uint64_t slots, const uint32_t* __restrict__ kept, uint32_t k_out,
                                                           uint32_t* __restrict__ t_ids, double* __restrict__ t_scores, uint32_t* __restrict__ t_dist) {
  for (uint64_t j = (uint64_t)blockIdx.x * 256u + threadIdx.x; j < slots; j += (uint64_t)gridDim.x * 256u) {
    uint32_t rk, i;
    uint64_t pos, row_len;
    uint64_t from = src[j];
    bool zero = false;
    if (edit_slot_row(row_offs, n_rows, row, j, &rk, &i, &pos, &row_len) && counts[i] < kCountFlagMin) zero = pos >= min(kept[i], k_out);
    else from = j;
    t_ids[j] = zero ? 0u : ids[from];
    t_dist[j] = zero ? 0u : dist[from];
    if (scores) t_scores[j] = zero ? 0.0 : scores[from];
  }
}

__global__ __launch_bounds__(256) void edit_counts_kernel(uint32_t* __restrict__ counts, const uint32_t* __restrict__ kept, uint32_t n_rows, uint32_t k_out) {
  for (uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x; i < n_rows; i += (uint64_t)gridDim.x * 256u)
    if (counts[i] < kCountFlagMin) counts[i] = min(kept[i], k_out);
}

// sg_suggest_batch_edit: the first k slots of every row of k_candidates
__global__ __launch_bounds__(256) void edit_take_kernel(const uint32_t* __restrict__ c_ids, const double* __restrict__ c_scores, const uint32_t* __restrict__ c_dist,
                                                        const uint32_t* __restrict__ c_counts, uint32_t n_q, uint32_t kc, uint32_t k, uint32_t* __restrict__ ids,
                                                        double* __restrict__ scores, uint32_t* __restrict__ dist, uint32_t* __restrict__ counts) {
  const uint64_t n = (uint64_t)n_q * k;
  for (uint64_t t = (uint64_t)blockIdx.x * 256u + threadIdx.x; t < n; t += (uint64_t)gridDim.x * 256u) {
    const uint64_t i = t / k, from = i * kc + (t - i * k);
    ids[t] = c_ids[from]; scores[t] = c_scores[from]; dist[t] = c_dist[from];
    if (t - i * k == 0u) counts[i] = c_counts[i];
  }
}

}  // namespace sg

namespace {

std::atomic<uint64_t> g_edit_slice_bytes{0};           // sg_debug_edit_slice_bytes (0: kEditSliceBytes)

// ---- the host-resident handle: the plain loop ----

void edit_host_runes(const uint8_t* s, size_t n, bool fold, std::vector<uint32_t>& out) {
  out.clear();
  for (size_t at = 0; at < n;) {
    size_t adv = 1;
    const uint32_t r = host_next_rune(s + at, n - at, &adv);
    at += adv;
    out.push_back(fold ? host_lower_rune(r) : r);
  }
}
// two rows of the dynamic programme, a third for the transposition
uint32_t edit_host_distance(const std::vector<uint32_t>& a, const std::vector<uint32_t>& b, bool osa, std::vector<uint32_t>& work) {
  const size_t m = a.size();
  work.assign(3 * (m + 1), 0);
  uint32_t *prev2 = work.data(), *prev = prev2 + m + 1, *cur = prev + m + 1;
  for (size_t i = 0; i <= m; i++) prev[i] = (uint32_t)i;
  for (size_t j = 1; j <= b.size(); j++) {
    cur[0] = (uint32_t)j;
    for (size_t i = 1; i <= m; i++) {
      uint32_t v = std::min(std::min(prev[i] + 1u, cur[i - 1] + 1u), prev[i - 1] + (a[i - 1] != b[j - 1] ? 1u : 0u));
      if (osa && i > 1 && j > 1 && a[i - 1] == b[j - 2] && a[i - 2] == b[j - 1]) v = std::min(v, prev2[i - 2] + 1u);
      cur[i] = v;
    }
    uint32_t* t = prev2; prev2 = prev; prev = cur; cur = t;
  }
  return prev[m];
}

// distances of the rows, and where `rerank` the stable re-rank, on the host; *outside: entries with an id outside the dictionary
void edit_host_rows(const sg_dictionary* dict, const sg_edit_config& cfg, const uint8_t* q, const uint64_t* q_offs, uint32_t* ids, double* scores,
                    uint32_t* counts, const uint64_t* row_offs, uint32_t n_rows, uint32_t row, uint64_t slots, uint32_t* dist, bool rerank, uint32_t k_out,
                    uint64_t* outside) {
  for (uint64_t s = 0; s < slots; s++) dist[s] = kEditNone;
  std::vector<uint32_t> qa, ca, work;
  std::vector<uint32_t> order, t_id, t_d;
  std::vector<double> t_s;
  for (uint32_t i = 0; i < n_rows; i++) {
    const uint64_t b = row_offs ? row_offs[i] : (uint64_t)i * row, len = row_offs ? row_offs[i + 1] - b : (uint64_t)row;
    if (counts[i] >= kCountFlagMin) continue;
    const uint32_t n = (uint32_t)std::min<uint64_t>(counts[i], len);
    if (n) edit_host_runes(q + q_offs[i], (size_t)(q_offs[i + 1] - q_offs[i]), cfg.fold_case != 0, qa);
    for (uint32_t p = 0; p < n; p++) {
      const uint32_t id = ids[b + p];
      if (id >= dict->n_docs) { (*outside)++; continue; }
      edit_host_runes(dict->h_blob.data() + dict->h_offs[id], (size_t)(dict->h_offs[(size_t)id + 1] - dict->h_offs[id]), cfg.fold_case != 0, ca);
      dist[b + p] = edit_host_distance(qa, ca, cfg.mode == SG_EDIT_OSA, work);
    }
    if (!rerank) continue;
    order.resize(n);
    for (uint32_t p = 0; p < n; p++) order[p] = p;
    std::stable_sort(order.begin(), order.end(), [&](uint32_t x, uint32_t y) { return dist[b + x] < dist[b + y]; });
    uint32_t kept = 0;
    for (uint32_t p = 0; p < n; p++) kept += dist[b + p] <= cfg.max_distance;
    const uint32_t newc = std::min(kept, k_out);
    t_id.resize(newc); t_d.resize(newc); t_s.resize(newc);
    for (uint32_t p = 0; p < newc; p++) { t_id[p] = ids[b + order[p]]; t_d[p] = dist[b + order[p]]; if (scores) t_s[p] = scores[b + order[p]]; }
    for (uint64_t p = 0; p < len; p++) {
      ids[b + p] = p < newc ? t_id[p] : 0u; dist[b + p] = p < newc ? t_d[p] : 0u;
      if (scores) scores[b + p] = p < newc ? t_s[p] : 0.0;
    }
    counts[i] = newc;
  }
}

// ---- the device routes ----

// The SCRATCH_EDIT block of a call: the list of long rows, the long kernel's regions, and — a re-rank by sort — keys, slot numbers,
// the rows' kept counts, the permuted rows and the sort's working memory; sg_suggest_batch_edit: the candidate rows besides.
struct EditLayout {
  size_t long_list = 0, long_mem = 0, keys_in = 0, keys_out = 0, vals_in = 0, vals_out = 0, kept = 0, t_ids = 0, t_scores = 0, t_dist = 0, tmp = 0,
         c_ids = 0, c_scores = 0, c_counts = 0, c_dist = 0, bytes = 0;
  size_t tmp_bytes = 0;
  uint64_t long_region = 0, long_mask_words = 0; uint32_t long_pairs = 0, long_w = 0, long_grid = 0;
  bool sort = false;
};
// max_q_bytes: the longest query where the caller knows it (host buffers), else kEditMaxQueryBytes.  cand_rows: n_rows rows of `row`
int edit_layout(uint32_t n_rows, uint32_t row, bool ragged, uint64_t slots, uint64_t max_q_bytes, bool rerank, bool cand_rows, EditLayout* out) {
  EditLayout L;
  Carve c;
  L.long_list = c.take(((size_t)n_rows + 1) * 4);
  const uint64_t cap = std::max<uint64_t>(std::min<uint64_t>(max_q_bytes, kEditMaxQueryBytes), 64);
  uint32_t P = 64;
  while (P < cap) P <<= 1;
  L.long_pairs = P; L.long_w = P / 64u;
  const uint64_t budget = g_edit_slice_bytes.load(std::memory_order_relaxed) ? g_edit_slice_bytes.load(std::memory_order_relaxed) : kEditSliceBytes;
  // (a region's masks take a 32nd of the budget at most — 2 MiB of the default 64 — so that the budget still buys a dozen regions
  //  where a region is sized for the longest query there can be; a query whose masks need more walks the sorted pairs, which needs none)
  L.long_mask_words = std::min<uint64_t>(std::min<uint64_t>((uint64_t)P * L.long_w, kEditMaskWords), budget / (8u * 32u));
  L.long_region = (uint64_t)P * 8u + 3ull * L.long_w * 64u * 8u + (uint64_t)P * 4u + L.long_mask_words * 8u;
  L.long_grid = (uint32_t)std::min<uint64_t>(std::max<uint64_t>(budget / L.long_region, 1), std::min<uint64_t>(256, std::max<uint32_t>(n_rows, 1u)));
  L.long_mem = c.take((size_t)(L.long_region * L.long_grid), 256);
  L.sort = rerank && (ragged || row > kEditRankSlots);
  if (L.sort) {
    HIP_TRY(hipcub::DeviceRadixSort::SortPairs(nullptr, L.tmp_bytes, (const uint64_t*)nullptr, (uint64_t*)nullptr, (const uint32_t*)nullptr, (uint32_t*)nullptr,
                                               (int)slots, 0, 64, (hipStream_t) nullptr));
    L.keys_in = c.take((size_t)slots * 8); L.keys_out = c.take((size_t)slots * 8); L.vals_in = c.take((size_t)slots * 4); L.vals_out = c.take((size_t)slots * 4);
    L.kept = c.take((size_t)n_rows * 4); L.t_ids = c.take((size_t)slots * 4); L.t_scores = c.take((size_t)slots * 8); L.t_dist = c.take((size_t)slots * 4);
    L.tmp = c.take(L.tmp_bytes, 256);
  }
  if (cand_rows) {
    L.c_scores = c.take((size_t)slots * 8); L.c_ids = c.take((size_t)slots * 4); L.c_dist = c.take((size_t)slots * 4); L.c_counts = c.take((size_t)n_rows * 4);
  }
  L.bytes = c.size();
  *out = L;
  return SG_OK;
}

struct EditRows {            // device pointers of a call's rows
  const uint8_t* q; const uint64_t* q_offs;
  uint32_t* ids; double* scores; uint32_t* counts; const uint64_t* row_offs;
  uint32_t n_rows, row; uint64_t slots;
  uint32_t* dist; uint64_t* info;
};

// distances of the rows on `st` (the caller has made dict->device current): dist[slots], info[0] = 0, info[1] = entries outside
int edit_dist_enqueue(const sg_dictionary* dict, const sg_edit_config& cfg, const EditRows& r, const EditLayout& L, char* blk, hipStream_t st) {
  HIP_TRY(hipMemsetAsync(r.info, 0, 16, st));
  if (r.slots) HIP_TRY(hipMemsetAsync(r.dist, 0xFF, (size_t)r.slots * 4, st));
  if (!r.n_rows) return SG_OK;
  HIP_TRY(hipMemsetAsync(blk + L.long_list, 0, 4, st));
  EditArgs a{};
  a.d = dict->view; a.low = EditLower{dict->d_lower_from, dict->d_lower_to, dict->n_lower};
  a.q_blob = r.q; a.q_offs = r.q_offs; a.ids = r.ids; a.counts = r.counts; a.row_offs = r.row_offs; a.n_rows = r.n_rows; a.row = r.row;
  a.dist = r.dist; a.info = (unsigned long long*)r.info; a.long_list = (uint32_t*)(blk + L.long_list);
  a.osa = cfg.mode == SG_EDIT_OSA; a.fold = cfg.fold_case != 0;
  a.long_mem = (uint8_t*)(blk + L.long_mem); a.long_region = L.long_region; a.long_mask_words = L.long_mask_words; a.long_pairs = L.long_pairs; a.long_w = L.long_w;
  const uint32_t groups = (uint32_t)std::min<uint64_t>(((uint64_t)r.n_rows + kEditRowsPerGroup - 1) / kEditRowsPerGroup, 16384u);
  hipLaunchKernelGGL(edit_short_kernel, dim3(groups), dim3(64 * kEditRowsPerGroup), 0, st, a);
  HIP_TRY(hipGetLastError());
  hipLaunchKernelGGL(edit_long_kernel, dim3(L.long_grid), dim3(64), 0, st, a);
  HIP_TRY(hipGetLastError());
  return SG_OK;
}

// the stable re-rank of the rows by r.dist, in place, behind edit_dist_enqueue on `st`
int edit_rerank_enqueue(const sg_edit_config& cfg, const EditRows& r, uint32_t k_out, const EditLayout& L, char* blk, hipStream_t st) {
  if (!r.n_rows || !r.slots) return SG_OK;
  if (!L.sort) {
    if (!r.row) return SG_OK;
    const uint32_t threads = r.row <= 256u ? (r.row + 63u) / 64u * 64u : 256u;
    hipLaunchKernelGGL(edit_rerank_kernel, dim3(std::min<uint32_t>(r.n_rows, 65536u)), dim3(threads), 0, st, r.ids, r.scores, r.dist, r.counts, r.n_rows, r.row,
                       cfg.max_distance, k_out);
    HIP_TRY(hipGetLastError());
    return SG_OK;
  }
  uint64_t *keys_in = (uint64_t*)(blk + L.keys_in), *keys_out = (uint64_t*)(blk + L.keys_out);
  uint32_t *vals_in = (uint32_t*)(blk + L.vals_in), *vals_out = (uint32_t*)(blk + L.vals_out), *kept = (uint32_t*)(blk + L.kept);
  uint32_t *t_ids = (uint32_t*)(blk + L.t_ids), *t_dist = (uint32_t*)(blk + L.t_dist);
  double* t_scores = (double*)(blk + L.t_scores);
  HIP_TRY(hipMemsetAsync(kept, 0, (size_t)r.n_rows * 4, st));
  const uint32_t blocks = (uint32_t)std::min<uint64_t>((r.slots + 255) / 256, 4096u);
  hipLaunchKernelGGL(edit_keys_kernel, dim3(blocks), dim3(256), 0, st, r.dist, r.counts, r.row_offs, r.n_rows, r.row, r.slots, cfg.max_distance, keys_in, vals_in, kept);
  HIP_TRY(hipGetLastError());
  size_t tb = L.tmp_bytes;
  HIP_TRY(hipcub::DeviceRadixSort::SortPairs(blk + L.tmp, tb, (const uint64_t*)keys_in, keys_out, (const uint32_t*)vals_in, vals_out, (int)r.slots, 0, 64, st));
  hipLaunchKernelGGL(edit_scatter_kernel, dim3(blocks), dim3(256), 0, st, vals_out, r.ids, r.scores, r.dist, r.counts, r.row_offs, r.n_rows, r.row, r.slots, kept,
                     k_out, t_ids, t_scores, t_dist);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipMemcpyAsync(r.ids, t_ids, (size_t)r.slots * 4, hipMemcpyDeviceToDevice, st));
  HIP_TRY(hipMemcpyAsync(r.dist, t_dist, (size_t)r.slots * 4, hipMemcpyDeviceToDevice, st));
  if (r.scores) HIP_TRY(hipMemcpyAsync(r.scores, t_scores, (size_t)r.slots * 8, hipMemcpyDeviceToDevice, st));
  hipLaunchKernelGGL(edit_counts_kernel, dim3((r.n_rows + 255u) / 256u), dim3(256), 0, st, r.counts, kept, r.n_rows, k_out);
  HIP_TRY(hipGetLastError());
  return SG_OK;
}

int edit_check_config(const sg_edit_config* cfg) {
  if (!cfg) { set_error("null argument"); return SG_E_INVALID; }
  if (cfg->mode != SG_EDIT_LEVENSHTEIN && cfg->mode != SG_EDIT_OSA) { set_error("unknown edit mode"); return SG_E_INVALID; }
  return SG_OK;
}
int edit_check_rows_args(const sg_dictionary* dict, const sg_edit_config* cfg, const void* q_offs, const void* ids, const void* counts, const void* row_offs,
                         uint32_t n_rows, uint32_t row, uint64_t slots, const void* dist) {
  if (!dict) { set_error("null dictionary"); return SG_E_INVALID; }
  if (int rc = edit_check_config(cfg)) return rc;
  if ((slots && !dist) || (n_rows && (!counts || !q_offs)) || (slots && n_rows && !ids)) { set_error("null argument"); return SG_E_INVALID; }
  if (n_rows > 0x7FFFFFF0u) { set_error("edit rows: too many rows for one call"); return SG_E_INVALID; }
  return dict_check_geometry(row_offs, n_rows, row, slots);
}

// sg_edit_rows_device / sg_edit_rerank_device
int edit_device_call(sg_dictionary* dict, const sg_edit_config* cfg, const void* d_q, const void* d_q_offs, void* d_ids, void* d_scores, void* d_counts,
                     const void* d_row_offs, uint32_t n_rows, uint32_t row, uint64_t slots, void* d_dist, void* d_info, bool rerank, uint32_t k_out, void* stream) {
  if (int rc = edit_check_rows_args(dict, cfg, d_q_offs, d_ids, d_counts, d_row_offs, n_rows, row, slots, d_dist)) return rc;
  if (!d_info) { set_error("null argument"); return SG_E_INVALID; }
  if (rerank && k_out == 0) { set_error("k_out should be greater or equal to 1"); return SG_E_INVALID; }
  if (dict->device < 0) { set_error("a host-resident dictionary cannot serve a device call"); return SG_E_UNSUPPORTED; }
  DeviceGuard dg;
  HIP_TRY(dg.set(dict->device));
  hipStream_t st = (hipStream_t)stream;
  EditLayout L;
  if (int rc = edit_layout(n_rows, row, d_row_offs != nullptr, slots, kEditMaxQueryBytes, rerank, false, &L)) return rc;
  void* blk = nullptr;
  if (int rc = stream_scratch(dict->device, st, L.bytes, &blk, SCRATCH_EDIT)) return rc;
  if (poison_mode()) { if (int rc = poison_fill(blk, L.bytes, PZ_ROWS, st)) return rc; }
  const EditRows r{(const uint8_t*)d_q, (const uint64_t*)d_q_offs, (uint32_t*)d_ids, (double*)d_scores, (uint32_t*)d_counts, (const uint64_t*)d_row_offs,
                   n_rows, row, slots, (uint32_t*)d_dist, (uint64_t*)d_info};
  if (int rc = edit_dist_enqueue(dict, *cfg, r, L, (char*)blk, st)) return rc;
  return rerank ? edit_rerank_enqueue(*cfg, r, k_out, L, (char*)blk, st) : SG_OK;
}

// The regions of sg_edit_rows / sg_edit_rerank on a device handle.  Out: the distances (the step fills every slot) and its info
// words.  The rows go in, and come back where they are re-ranked.  In: the queries and the row offsets (null: an empty region).
enum { ER_DIST = 0, ER_INFO, ER_SCORES, ER_IDS, ER_COUNTS, ER_Q_OFFS, ER_Q, ER_ROW_OFFS };
IoCall edit_rows_io(const uint8_t* q, const uint64_t* q_offs, uint32_t* ids, double* scores, uint32_t* counts, const uint64_t* row_offs, uint32_t n_rows,
                    uint64_t slots, uint32_t* dist, uint64_t* info, bool rerank) {
  const IoDir rows_dir = rerank ? IO_BOTH : IO_IN;
  return IoCall().add(IO_OUT, dist, (size_t)slots * 4, 16, false, PZ_OUT_IDS).add(IO_OUT, info, 16, 8)
      .add(rows_dir, scores, scores ? (size_t)slots * 8 : 0, 8).add(rows_dir, ids, (size_t)slots * 4, 4).add(rows_dir, counts, (size_t)n_rows * 4, 4)
      .add_window(q_offs, n_rows, q, 1, false).add(IO_IN, row_offs, row_offs ? ((size_t)n_rows + 1) * 8 : 0, 16);
}

// sg_edit_rows / sg_edit_rerank: host buffers
int edit_host_call(sg_dictionary* dict, const sg_edit_config* cfg, const uint8_t* q, const uint64_t* q_offs, uint32_t* ids, double* scores, uint32_t* counts,
                   const uint64_t* row_offs, uint32_t n_rows, uint32_t row, uint64_t slots, uint32_t* dist, bool rerank, uint32_t k_out) {
  if (int rc = edit_check_rows_args(dict, cfg, q_offs, ids, counts, row_offs, n_rows, row, slots, dist)) return rc;
  if (rerank && k_out == 0) { set_error("k_out should be greater or equal to 1"); return SG_E_INVALID; }
  uint64_t max_q = 0;
  for (uint32_t i = 0; i < n_rows; i++) {
    if (q_offs[i + 1] < q_offs[i]) { set_error("query offsets must not decrease"); return SG_E_INVALID; }
    if (row_offs && row_offs[i + 1] < row_offs[i]) { set_error("row offsets must not decrease"); return SG_E_INVALID; }
    max_q = std::max(max_q, q_offs[i + 1] - q_offs[i]);
  }
  if (row_offs && n_rows && row_offs[n_rows] > slots) { set_error("edit rows: slots is below the last row offset"); return SG_E_INVALID; }
  if (max_q > kEditMaxQueryBytes) { set_error("a query of more than 65536 bytes"); return SG_E_INVALID; }
  if (n_rows && !q && q_offs[n_rows] != q_offs[0]) { set_error("null query buffer"); return SG_E_INVALID; }
  uint64_t outside = 0;
  if (dict->device < 0) {
    edit_host_rows(dict, *cfg, q, q_offs, ids, scores, counts, row_offs, n_rows, row, slots, dist, rerank, k_out, &outside);
  } else if (n_rows == 0 || slots == 0) {
    std::fill(dist, dist + slots, kEditNone);                      // (no slot holds an entry)
  } else {
    uint64_t info[2] = {0, 0};
    const int rc = run_host_call(dict->device, edit_rows_io(q, q_offs, ids, scores, counts, row_offs, n_rows, slots, dist, info, rerank), [&](const IoCall& io, hipStream_t st) -> int {
      EditLayout L;
      if (int rc2 = edit_layout(n_rows, row, row_offs != nullptr, slots, max_q, rerank, false, &L)) return rc2;
      void* blk = nullptr;
      if (int rc2 = stream_scratch(dict->device, st, L.bytes, &blk, SCRATCH_EDIT)) return rc2;
      if (poison_mode()) { if (int rc2 = poison_fill(blk, L.bytes, PZ_ROWS, st)) return rc2; }
      const EditRows r{io.at<uint8_t>(ER_Q), io.at<uint64_t>(ER_Q_OFFS), io.at<uint32_t>(ER_IDS), scores ? io.at<double>(ER_SCORES) : nullptr, io.at<uint32_t>(ER_COUNTS),
                       row_offs ? io.at<uint64_t>(ER_ROW_OFFS) : nullptr, n_rows, row, slots, io.at<uint32_t>(ER_DIST), io.at<uint64_t>(ER_INFO)};
      if (int rc2 = edit_dist_enqueue(dict, *cfg, r, L, (char*)blk, st)) return rc2;
      return rerank ? edit_rerank_enqueue(*cfg, r, k_out, L, (char*)blk, st) : SG_OK;
    });
    if (rc) return rc;
    outside = info[1];
  }
  if (outside) { set_error("docID outside the dictionary"); return SG_E_INVALID; }
  return SG_OK;
}

}  // namespace

extern "C" {

int sg_edit_rows_device(sg_dictionary* dict, const sg_edit_config* cfg, const void* d_q_blob, const void* d_q_offs, const void* d_ids, const void* d_counts,
                        const void* d_row_offs, uint32_t n_rows, uint32_t row, uint64_t slots, void* d_dist, void* d_info, void* stream) {
  SG_GUARD_BEGIN
  return edit_device_call(dict, cfg, d_q_blob, d_q_offs, (void*)d_ids, nullptr, (void*)d_counts, d_row_offs, n_rows, row, slots, d_dist, d_info, false, 0, stream);
  SG_GUARD_END(SG_RC)
}

int sg_edit_rows(sg_dictionary* dict, const sg_edit_config* cfg, const uint8_t* q, const uint64_t* q_offs, const uint32_t* ids, const uint32_t* counts,
                 const uint64_t* row_offs, uint32_t n_rows, uint32_t row, uint64_t slots, uint32_t* dist) {
  SG_GUARD_BEGIN
  return edit_host_call(dict, cfg, q, q_offs, (uint32_t*)ids, nullptr, (uint32_t*)counts, row_offs, n_rows, row, slots, dist, false, 0);
  SG_GUARD_END(SG_RC)
}

int sg_edit_rerank_device(sg_dictionary* dict, const sg_edit_config* cfg, const void* d_q_blob, const void* d_q_offs, void* d_ids, void* d_scores,
                          void* d_counts, const void* d_row_offs, uint32_t n_rows, uint32_t row, uint64_t slots, uint32_t k_out, void* d_dist, void* d_info,
                          void* stream) {
  SG_GUARD_BEGIN
  return edit_device_call(dict, cfg, d_q_blob, d_q_offs, d_ids, d_scores, d_counts, d_row_offs, n_rows, row, slots, d_dist, d_info, true, k_out, stream);
  SG_GUARD_END(SG_RC)
}

int sg_edit_rerank(sg_dictionary* dict, const sg_edit_config* cfg, const uint8_t* q, const uint64_t* q_offs, uint32_t* ids, double* scores, uint32_t* counts,
                   const uint64_t* row_offs, uint32_t n_rows, uint32_t row, uint64_t slots, uint32_t k_out, uint32_t* dist) {
  SG_GUARD_BEGIN
  return edit_host_call(dict, cfg, q, q_offs, ids, scores, counts, row_offs, n_rows, row, slots, dist, true, k_out);
  SG_GUARD_END(SG_RC)
}

int sg_suggest_batch_edit(sg_index* index, const uint8_t* q, const uint64_t* offs, uint32_t n_q, int metric, double similarity, uint32_t k_candidates,
                          sg_dictionary* dict, const sg_edit_config* cfg, uint32_t k, uint32_t* out_ids, double* out_scores, uint32_t* out_dist,
                          uint32_t* out_counts) {
  SG_GUARD_BEGIN
  const SearchKey c = fuzzy_key(metric, similarity, k_candidates);
  if (int rc = open_search(index, c, true, {offs, out_ids, out_scores, out_counts, out_dist})) return rc;
  if (!dict) { set_error("null dictionary"); return SG_E_INVALID; }
  if (int rc = edit_check_config(cfg)) return rc;
  if (k == 0) { set_error("topK should be greater or equal to 1"); return SG_E_INVALID; }
  if (k > k_candidates) { set_error("k above k_candidates"); return SG_E_INVALID; }
  if (dict->device < 0) { set_error("a host-resident dictionary cannot serve a device call"); return SG_E_UNSUPPORTED; }
  Replica* rep = find_replica(index, -1);
  if (dict->device != rep->device) { set_error("the dictionary is not on the device of the index's primary replica"); return SG_E_UNSUPPORTED; }
  const uint64_t slots = (uint64_t)n_q * k_candidates;
  if (int rc = dict_check_geometry(nullptr, n_q, k_candidates, slots)) return rc;
  if (n_q == 0) return SG_OK;
  uint64_t max_q = 0;
  for (uint32_t i = 0; i < n_q; i++) {
    if (offs[i + 1] < offs[i]) { set_error("query offsets must not decrease"); return SG_E_INVALID; }
    max_q = std::max(max_q, offs[i + 1] - offs[i]);
  }
  if (max_q > kEditMaxQueryBytes) { set_error("a query of more than 65536 bytes"); return SG_E_INVALID; }
  const LaunchReq req = search_req(c);
  IoCall call = search_io(q, offs, n_q, (uint64_t)n_q * k, out_ids, out_scores, out_counts, out_dist, true);   // (aux: the distances)
  uint64_t info[2] = {0, 0};
  const int io_info = (int)call.add(IO_OUT, info, 16, 8).n - 1;      // (the step's info words come back with the rows)
  const sg_edit_config config = *cfg;
  const int rc = run_host_call(rep->device, call, [&](const IoCall& io, hipStream_t st) -> int {
    EditLayout L;
    if (int rc2 = edit_layout(n_q, k_candidates, false, slots, max_q, true, true, &L)) return rc2;
    void* blkv = nullptr;
    if (int rc2 = stream_scratch(rep->device, st, L.bytes, &blkv, SCRATCH_EDIT)) return rc2;
    char* blk = (char*)blkv;
    if (poison_mode()) { if (int rc2 = poison_fill(blk, L.bytes, PZ_ROWS, st)) return rc2; }
    else {
      HIP_TRY(hipMemsetAsync(blk + L.c_scores, 0, (size_t)slots * 8, st));
      HIP_TRY(hipMemsetAsync(blk + L.c_ids, 0, (size_t)slots * 4, st));
    }
    LaunchReq r = req;
    r.q = io.at<char>(IO_Q); r.offs = io.at<char>(IO_OFFS); r.n_q = n_q; r.stream = st; r.no_long_queries = no_long_queries(offs, n_q);
    r.ids = blk + L.c_ids; r.scores = blk + L.c_scores; r.counts = blk + L.c_counts;
    if (int rc2 = launch(index, rep, r)) return rc2;
    const EditRows rows{io.at<uint8_t>(IO_Q), io.at<uint64_t>(IO_OFFS), (uint32_t*)(blk + L.c_ids), (double*)(blk + L.c_scores),
                        (uint32_t*)(blk + L.c_counts), nullptr, n_q, k_candidates, slots, (uint32_t*)(blk + L.c_dist), io.at<uint64_t>(io_info)};
    if (int rc2 = edit_dist_enqueue(dict, config, rows, L, blk, st)) return rc2;
    if (int rc2 = edit_rerank_enqueue(config, rows, k, L, blk, st)) return rc2;
    const uint32_t blocks = (uint32_t)std::min<uint64_t>(((uint64_t)n_q * k + 255) / 256, 4096u);
    hipLaunchKernelGGL(edit_take_kernel, dim3(blocks), dim3(256), 0, st, rows.ids, rows.scores, rows.dist, rows.counts, n_q, k_candidates, k,
                       io.at<uint32_t>(IO_IDS), io.at<double>(IO_SCORES), io.at<uint32_t>(IO_AUX), io.at<uint32_t>(IO_COUNTS));
    HIP_TRY(hipGetLastError());
    return SG_OK;
  });
  if (rc) return rc;
  if (info[1]) { set_error("docID outside the dictionary"); return SG_E_INVALID; }
  return SG_OK;
  SG_GUARD_END(SG_RC)
}

// Test hook (no GPU needed; here, behind the last kind's declaring function): the regions a host-buffer call of `kind` declares — by
// the function its call site uses — and the block lay() makes of them.  Of the arrays only the offsets' first and last word are read.
int sg_debug_io_layout(uint32_t kind, uint32_t n, uint32_t k, uint32_t flags, uint64_t blob_bytes, uint64_t rows, uint64_t out[45]) {
  SG_GUARD_BEGIN
  if (!out || n == 0 || kind > 8u) { set_error("bad argument"); return SG_E_INVALID; }
  static uint64_t w[2];
  uint8_t* p8 = (uint8_t*)w; uint32_t* p32 = (uint32_t*)w; double* pd = (double*)w;
  const bool f0 = flags & 1u, f1 = flags & 2u, ragged = flags & 4u;
  std::vector<uint64_t> offs((size_t)n + 1, 0);
  offs[n] = kind == 8 ? blob_bytes / 4 : blob_bytes;
  std::fill(out, out + 45, 0);
  IoCall io;
  if (kind <= 2) io = search_io(p8, offs.data(), n, kind == 2 ? rows : (uint64_t)n * k, p32, f0 || kind == 2 ? pd : nullptr, p32, kind == 0 && f1 ? p32 : nullptr,
                                kind != 2, kind == 1 ? w : nullptr, kind == 2 ? p32 : nullptr);
  else if (kind == 3) io = search_io(p8, offs.data(), n, (uint64_t)n * (k + 1), p32, nullptr, p32, nullptr, false);
  else if (kind == 4) io = dict_rows_io(p32, p32, ragged ? w : nullptr, n, rows, w);
  else if (kind <= 6) io = edit_rows_io(p8, offs.data(), p32, f0 ? pd : nullptr, p32, ragged ? w : nullptr, n, rows, p32, w, kind == 6);
  else io = lm_score_io(p8, kind == 8 ? 4 : 1, offs.data(), n, pd, kind == 7 && f0 ? p32 : nullptr, kind == 7 && f1 ? p32 : nullptr);
  io.lay();
  for (uint64_t v : {(uint64_t)io.n, (uint64_t)io.out_hi, (uint64_t)io.in_lo, (uint64_t)io.in_hi, (uint64_t)io.total}) *out++ = v;
  for (uint32_t i = 0; i < io.n; i++) for (uint64_t v : {(uint64_t)io.r[i].off, (uint64_t)io.r[i].bytes, (uint64_t)io.r[i].align, (uint64_t)io.r[i].dir}) *out++ = v;
  return SG_OK;
  SG_GUARD_END(SG_RC)
}

int sg_debug_edit_slice_bytes(uint64_t bytes) {
  g_edit_slice_bytes.store(bytes, std::memory_order_relaxed);
  return SG_OK;
}

// Test hook (no GPU needed): the kernels' own statement of the recurrence — edit_block_step with the Peq table for a query of <= 64
// runes, edit_long_column over the sorted pairs above — run on the host over two rune strings.
int sg_debug_edit_bitvector(int mode, const uint32_t* a, uint32_t n_a, const uint32_t* b, uint32_t n_b, uint32_t* out) {
  SG_GUARD_BEGIN
  if (!out || (n_a && !a) || (n_b && !b) || (mode != SG_EDIT_LEVENSHTEIN && mode != SG_EDIT_OSA)) { set_error("null argument"); return SG_E_INVALID; }
  const bool osa = mode == SG_EDIT_OSA;
  uint32_t score = n_a;
  if (n_a == 0) score = n_b;
  else if (n_a <= 64) {
    std::vector<uint32_t> keys(kEditPeqSlots, kEditNone);
    std::vector<uint64_t> masks(kEditPeqSlots, 0);
    for (uint32_t i = 0; i < n_a; i++) edit_peq_insert(keys.data(), masks.data(), a[i], 1ull << i);
    const uint64_t last = 1ull << (n_a - 1);
    uint64_t pv = ~0ull, mv = 0, d0 = 0, eqp = 0;
    for (uint32_t j = 0; j < n_b; j++) {
      const uint64_t eq = edit_peq_find(keys.data(), masks.data(), b[j]);
      uint64_t hp_c = 1, hn_c = 0, tr_c = 0, hp, hn;
      edit_block_step(osa, eq, eqp, pv, mv, d0, hp_c, hn_c, tr_c, hp, hn);
      score += (hp & last) != 0;
      score -= (hn & last) != 0;
      eqp = eq;
    }
  } else {
    std::vector<uint64_t> srt(n_a);
    for (uint32_t i = 0; i < n_a; i++) srt[i] = ((uint64_t)a[i] << 32) | i;
    std::sort(srt.begin(), srt.end());
    const uint32_t w = (n_a + 63) / 64;
    std::vector<uint64_t> state(3 * (size_t)w, 0);
    for (uint32_t k = 0; k < w; k++) state[k] = ~0ull;
    const EditState st{state.data(), 1, w};
    uint32_t prev = kEditNone;
    for (uint32_t j = 0; j < n_b; j++) { edit_long_column(osa, srt.data(), n_a, b[j], prev, n_a, w, st, score); prev = b[j]; }
    // ... and over Peq as whole words: both forms must agree
    std::vector<uint32_t> drune;
    for (uint64_t key : srt) if (drune.empty() || drune.back() != (uint32_t)(key >> 32)) drune.push_back((uint32_t)(key >> 32));
    const uint32_t n_d = (uint32_t)drune.size();
    std::vector<uint64_t> masks((size_t)n_d * w, 0);
    for (uint64_t key : srt) masks[(size_t)edit_rune_rank(drune.data(), n_d, (uint32_t)(key >> 32)) * w + ((uint32_t)key >> 6)] |= 1ull << (key & 63u);
    std::fill(state.begin(), state.end(), 0);
    for (uint32_t k = 0; k < w; k++) state[k] = ~0ull;
    uint32_t score2 = n_a, prev_rk = kEditNone;
    for (uint32_t j = 0; j < n_b; j++) {
      const uint32_t rk = edit_rune_rank(drune.data(), n_d, b[j]);
      edit_long_column_dense(osa, masks.data(), rk, prev_rk, n_a, w, st, score2);
      prev_rk = rk;
    }
    if (score2 != score) { set_error("the two forms of the blocked recurrence differ"); return SG_E_INVALID; }
  }
  *out = score;
  return SG_OK;
  SG_GUARD_END(SG_RC)
}

}  // extern "C"
