// edit_search.inc — a complete search of a dictionary held in HBM by edit distance (include/suggest_hip.h; DESIGN.md §5e), included
// by engine.hip after edit_rank.inc (it uses its edit_peq_* / edit_block_step / EditLower / edit_upto4 / edit_host_runes /
// edit_host_distance / edit_check_config and kEditRankSlots, dict_rows.inc's DictView, sg_dictionary and dict_check_geometry,
// host_call.inc's run_host_call / IoCall, capi.inc's stream_scratch, Carve and the poison, d_next_rune, d_lower_pairs, HIP_TRY).
//
// Every string within max_distance edits of the query, the k nearest returned, ties by docID — over the WHOLE dictionary, not over
// the candidates of a q-gram search.  What decides which strings are looked at is a per-document record that needs no q-gram index:
//   build      edit_sig_kernel: a thread per document decodes its string once: runes[d] = its rune count, sig[d] = the OR over its
//              (folded) runes of bit (rune * 0x9E3779B1) >> 26.  One edit removes at most one rune and adds at most one, a
//              transposition neither, so distance >= max(popcount(sigQ & ~sigD), popcount(sigD & ~sigQ)) and >= |runesQ - runesD|.
//   scan       edit_scan_kernel<emit>: a workgroup owns a tile of kEsTile queries — each one's Peq table in LDS, built as
//              edit_short_kernel builds it, its signature and rune count beside it — and each of its four wavefronts a contiguous
//              docID slice.  A lane per document strides over the slice's (sig, runes) records in docID order and tests each loaded
//              record against every query of the tile; only a surviving pair is decoded and run through the one-word recurrence.
//              Pass 1 (emit = false) counts hist[q][distance] — in LDS, one global atomic per non-empty bin at the end.
//              Pass 2 (emit = true) first turns each histogram into the cut-off d* (the first distance at which the running sum
//              reaches k) and the number r still wanted at d*, then repeats the scan with the tighter bound min(d*, max_distance):
//              every pair below d* is appended to segment 0 of the query's row (fewer than k in all), and of each slice the first r
//              pairs at d* in docID order go to the slice's own segment — ordered compaction by ballot and prefix.
//   rank       edit_search_rank_kernel: a workgroup per query.  Segment 0 is ranked by (distance, docID) in LDS — distinct keys, so
//              distinct ranks and no two lanes store to one slot — and the slices' segments follow in slice order, which IS docID
//              order, until k is reached.  A query of more than 64 runes is flagged SG_COUNT_TOO_LONG here.
// Memory is bounded whatever the number of matches: a row of (1 + n_slices) * k slots per query, a batch whose rows pass the budget
// (kEsRowBytes; sg_debug_edit_search_bytes) is enqueued in query chunks.  No host round trip inside the device call.
// Scratch: one block of the calling thread's per-stream scratch (SCRATCH_EDIT_SEARCH).  sg_edit_search_device writes nothing of any handle.

namespace sg {

constexpr uint32_t kEsTile = 16;                      // queries of a scan workgroup
constexpr uint32_t kEsWaves = 4;                      // its wavefronts: a docID slice each
constexpr uint32_t kEsBins = SG_EDIT_SEARCH_MAX_DISTANCE + 1u;   // words of a query's histogram at most
constexpr uint32_t kEsMaxSlices = 1024;
constexpr uint32_t kEsWantWaves = 8192;               // the scan fills the device from this many wavefronts on (32 per CU)
constexpr uint32_t kEsMaxChunk = 1u << 19;            // queries of one chunk at most (the scan's grid: a tile per blockIdx.y)
constexpr uint64_t kEsRowBytes = (uint64_t)256 << 20; // budget of a chunk's rows

// the bit a rune sets in a signature; the two bounds (tests/edit_search_ref.py restates both)
__host__ __device__ inline uint64_t edit_sig_bit(uint32_t r) { return 1ull << ((r * 0x9E3779B1u) >> 26); }
__host__ __device__ inline bool edit_sig_pass(uint64_t sig_q, uint32_t m_q, uint64_t sig_d, uint32_t m_d, uint32_t bound) {
  const uint32_t dl = m_q > m_d ? m_q - m_d : m_d - m_q;
  return dl <= bound && (uint32_t)__builtin_popcountll(sig_q & ~sig_d) <= bound && (uint32_t)__builtin_popcountll(sig_d & ~sig_q) <= bound;
}

__global__ __launch_bounds__(256) void edit_sig_kernel(const DictView d, const EditLower low, int fold, uint32_t* __restrict__ runes, uint64_t* __restrict__ sig) {
  for (uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x; i < d.n_docs; i += (uint64_t)gridDim.x * 256u) {
    const uint64_t to = d.doc_offs[i + 1];
    uint32_t n = 0;
    uint64_t s = 0;
    for (uint64_t at = d.doc_offs[i]; at < to;) {
      uint32_t adv;
      uint32_t r = d_next_rune(d.blob + at, edit_upto4(to - at), &adv);
      if (fold) r = d_lower_pairs(low, r);
      at += adv;
      s |= edit_sig_bit(r); n++;
    }
    runes[i] = n; sig[i] = s;
  }
}

struct EsArgs {
  DictView d;
  EditLower low;
  const uint32_t* runes; const uint64_t* sig;        // the index's two arrays
  const uint8_t* q_blob; const uint64_t* q_offs;
  uint32_t q_first, n_q;                             // the chunk: queries [q_first, q_first + n_q) of the call
  uint32_t k, max_distance, n_slices, per_slice;     // slice s: docs [s * per_slice, (s + 1) * per_slice)
  int osa, fold;
  uint32_t* hist;                                    // [the call's queries][max_distance + 1], zeroed per call
  uint32_t* row_n;                                   // [n_q][1 + n_slices] entries of a row's segments, zeroed per chunk
  uint32_t* row_ids; uint32_t* row_dist;             // [n_q][1 + n_slices][k]
  uint32_t* ids; uint32_t* dist; uint32_t* counts;   // the call's result rows
};

__device__ __forceinline__ uint32_t es_fold(const EsArgs& a, uint32_t r) { return a.fold ? d_lower_pairs(a.low, r) : r; }

template <bool kEmit>
__global__ __launch_bounds__(64 * kEsWaves) void edit_scan_kernel(const EsArgs a) {
  __shared__ uint64_t s_mask[kEsTile][kEditPeqSlots];
  __shared__ uint32_t s_key[kEsTile][kEditPeqSlots];
  __shared__ uint8_t s_q[kEsTile][kEditShortBytes];
  __shared__ uint64_t s_sig[kEsTile];
  __shared__ uint32_t s_m[kEsTile], s_bound[kEsTile], s_cut[kEsTile], s_want[kEsTile];
  __shared__ uint32_t s_hist[kEsTile][kEsBins];        // pass 1
  __shared__ uint32_t s_taken[kEsWaves][kEsTile];      // pass 2: pairs at d* the wavefront's slice has emitted
  const uint32_t wv = threadIdx.x / 64u, lane = threadIdx.x % 64u;
  const uint32_t tile0 = blockIdx.y * kEsTile;
  const uint32_t n_t = min(kEsTile, a.n_q - tile0);
  const uint32_t bins = a.max_distance + 1u;
  for (uint32_t t = 0; t < n_t; t++) {
    const uint64_t qi = (uint64_t)a.q_first + tile0 + t;
    const uint64_t b = a.q_offs[qi], len = a.q_offs[qi + 1] - b;
    if (len <= kEditShortBytes) for (uint32_t x = threadIdx.x; x < (uint32_t)len; x += 64u * kEsWaves) s_q[t][x] = a.q_blob[b + x];
  }
  for (uint32_t x = threadIdx.x; x < kEsTile * kEditPeqSlots; x += 64u * kEsWaves) { (&s_key[0][0])[x] = kEditNone; (&s_mask[0][0])[x] = 0; }
  for (uint32_t x = threadIdx.x; x < kEsTile * kEsBins; x += 64u * kEsWaves) (&s_hist[0][0])[x] = 0;
  for (uint32_t x = threadIdx.x; x < kEsWaves * kEsTile; x += 64u * kEsWaves) (&s_taken[0][0])[x] = 0;
  __syncthreads();
  if (threadIdx.x < n_t) {                             // a thread per query: Peq, signature, rune count (65: too long); pass 2: the cut
    const uint32_t t = threadIdx.x;
    const uint64_t qi = (uint64_t)a.q_first + tile0 + t;
    const uint64_t len = a.q_offs[qi + 1] - a.q_offs[qi];
    uint32_t m = 65u;
    uint64_t sg = 0;
    if (len <= kEditShortBytes) {
      m = 0;
      for (uint32_t p = 0; p < (uint32_t)len;) {
        uint32_t adv;
        const uint32_t r = es_fold(a, d_next_rune(&s_q[t][p], (uint32_t)len - p, &adv));
        p += adv;
        if (m == 64u) { m = 65u; break; }
        edit_peq_insert(s_key[t], s_mask[t], r, 1ull << m);
        sg |= edit_sig_bit(r);
        m++;
      }
    }
    uint32_t cut = bins, want = 0;                      // cut = max_distance + 1: fewer than k matches, every one is "below"
    if (kEmit && m <= 64u) {
      const uint32_t* h = a.hist + qi * bins;
      uint64_t sum = 0;
      for (uint32_t b = 0; b < bins; b++) {
        const uint64_t c = h[b];
        if (sum + c >= a.k) { cut = b; want = (uint32_t)(a.k - sum); break; }
        sum += c;
      }
    }
    s_m[t] = m; s_sig[t] = sg; s_cut[t] = cut; s_want[t] = want; s_bound[t] = min(cut, a.max_distance);
  }
  __syncthreads();
  const uint32_t slice = blockIdx.x * kEsWaves + wv;
  const uint64_t begin = (uint64_t)slice * a.per_slice, end = min(begin + a.per_slice, (uint64_t)a.d.n_docs);
  const uint64_t lt = (1ull << lane) - 1ull;
  if (slice < a.n_slices) for (uint64_t base = begin; base < end; base += 64u) {     // (uniform in the wavefront; no barrier inside)
    const uint64_t doc = base + lane;
    const bool live = doc < end;
    uint64_t sig_d = 0;
    uint32_t m_d = 0;
    if (live) { sig_d = a.sig[doc]; m_d = a.runes[doc]; }
    for (uint32_t t = 0; t < n_t; t++) {
      const uint32_t m = s_m[t];
      if (m > 64u) continue;
      const bool surv = live && edit_sig_pass(s_sig[t], m, sig_d, m_d, s_bound[t]);
      if (!ballot(surv)) continue;
      uint32_t score = kEditNone;
      if (surv) {
        score = m_d;                                   // an empty query: the document's rune count
        if (m != 0u) {
          const uint64_t to = a.d.doc_offs[doc + 1], last = 1ull << (m - 1u);
          uint64_t pv = ~0ull, mv = 0, d0 = 0, eqp = 0;
          score = m;
          for (uint64_t at = a.d.doc_offs[doc]; at < to;) {
            uint32_t adv;
            const uint32_t r = es_fold(a, d_next_rune(a.d.blob + at, edit_upto4(to - at), &adv));
            at += adv;
            const uint64_t eq = edit_peq_find(s_key[t], s_mask[t], r);
            uint64_t hp_c = 1, hn_c = 0, tr_c = 0, hp, hn;
            edit_block_step(a.osa != 0, eq, eqp, pv, mv, d0, hp_c, hn_c, tr_c, hp, hn);
            score += (hp & last) != 0ull;
            score -= (hn & last) != 0ull;
            eqp = eq;
          }
        }
      }
      if (!kEmit) {
        if (score <= a.max_distance) atomicAdd(&s_hist[t][score], 1u);
        continue;
      }
      const uint32_t cut = s_cut[t];
      const uint64_t row = ((uint64_t)tile0 + t) * (1ull + a.n_slices);      // the query's first segment
      const bool below = score < cut;                  // (cut <= max_distance + 1; a pair that did not survive scores kEditNone)
      const uint64_t bb = ballot(below);
      if (bb) {                                        // segment 0, any order: the rank kernel sorts it
        uint32_t at0 = 0;
        if (lane == 0u) at0 = atomicAdd(&a.row_n[row], popc64(bb));
        at0 = (uint32_t)__shfl((int)at0, 0);
        const uint32_t pos = at0 + popc64(bb & lt);
        if (below && pos < a.k) { a.row_ids[row * a.k + pos] = (uint32_t)doc; a.row_dist[row * a.k + pos] = score; }
      }
      const bool at_cut = cut <= a.max_distance && score == cut;
      const uint64_t ba = ballot(at_cut);
      if (ba) {                                        // the slice's own segment: its first `want` pairs at d*, in docID order
        const uint32_t took = s_taken[wv][t], want = s_want[t];
        const uint32_t pos = took + popc64(ba & lt);
        if (at_cut && pos < want) { a.row_ids[(row + 1u + slice) * a.k + pos] = (uint32_t)doc; a.row_dist[(row + 1u + slice) * a.k + pos] = score; }
        s_taken[wv][t] = min(took + popc64(ba), want);  // (every lane stores the same word: each reads back what it wrote itself)
      }
    }
  }
  __syncthreads();
  if (!kEmit) {
    for (uint32_t x = threadIdx.x; x < n_t * kEsBins; x += 64u * kEsWaves) {
      const uint32_t t = x / kEsBins, b = x % kEsBins, v = s_hist[t][b];
      if (v != 0u && b < bins) atomicAdd(&a.hist[((uint64_t)a.q_first + tile0 + t) * bins + b], v);
    }
  } else if (slice < a.n_slices && lane < n_t) {       // what the slice emitted at d*: the count of its segment
    a.row_n[((uint64_t)tile0 + lane) * (1ull + a.n_slices) + 1u + slice] = s_taken[wv][lane];
  }
}

// A workgroup per query of the chunk: the row's segments become the result row of k slots.
__global__ __launch_bounds__(256) void edit_search_rank_kernel(const EsArgs a) {
  __shared__ uint64_t s_k[kEditRankSlots];
  __shared__ uint32_t s_long;
  for (uint32_t i = blockIdx.x; i < a.n_q; i += gridDim.x) {
    const uint64_t qi = (uint64_t)a.q_first + i;
    if (threadIdx.x == 0u) {                           // more than 64 runes?
      const uint64_t b = a.q_offs[qi], len = a.q_offs[qi + 1] - b;
      uint32_t m = 65u;
      if (len <= kEditShortBytes) {
        m = 0;
        for (uint32_t p = 0; p < (uint32_t)len; m++) { uint32_t adv; (void)d_next_rune(a.q_blob + b + p, (uint32_t)len - p, &adv); p += adv; }
      }
      s_long = m > 64u;
    }
    __syncthreads();
    uint32_t* o_ids = a.ids + qi * a.k;
    uint32_t* o_dist = a.dist + qi * a.k;
    uint32_t total = 0;
    if (!s_long) {
      const uint32_t* n = a.row_n + (uint64_t)i * (1ull + a.n_slices);
      const uint64_t row = (uint64_t)i * (1ull + a.n_slices);
      const uint32_t n_below = min(n[0], min(a.k, kEditRankSlots));
      uint64_t my[4];
#pragma unroll
      for (uint32_t u = 0; u < 4u; u++) {
        const uint32_t p = threadIdx.x + u * 256u;
        my[u] = ~0ull;
        if (p < n_below) { my[u] = ((uint64_t)a.row_dist[row * a.k + p] << 32) | a.row_ids[row * a.k + p]; s_k[p] = my[u]; }
      }
      __syncthreads();
      uint32_t rank[4] = {0, 0, 0, 0};
      for (uint32_t j = 0; j < n_below; j++) {
        const uint64_t kj = s_k[j];
#pragma unroll
        for (uint32_t u = 0; u < 4u; u++) rank[u] += kj < my[u];
      }
#pragma unroll
      for (uint32_t u = 0; u < 4u; u++)
        if (threadIdx.x + u * 256u < n_below) { o_ids[rank[u]] = (uint32_t)my[u]; o_dist[rank[u]] = (uint32_t)(my[u] >> 32); }
      total = n_below;
      for (uint32_t s = 0; s < a.n_slices && total < a.k; s++) {          // slice order is docID order
        const uint32_t ns = min(n[1u + s], a.k - total);
        for (uint32_t j = threadIdx.x; j < ns; j += 256u) {
          o_ids[total + j] = a.row_ids[(row + 1u + s) * a.k + j]; o_dist[total + j] = a.row_dist[(row + 1u + s) * a.k + j];
        }
        total += ns;
      }
    }
    for (uint32_t p = total + threadIdx.x; p < a.k; p += 256u) { o_ids[p] = 0; o_dist[p] = 0; }
    if (threadIdx.x == 0u) a.counts[qi] = s_long ? SG_COUNT_TOO_LONG : total;
    __syncthreads();                                   // (the next query rewrites s_long and s_k)
  }
}

}  // namespace sg

struct sg_edit_index {
  std::atomic<int> refs{1};
  sg_dictionary* dict = nullptr;       // retained
  int fold = 0;
  std::vector<uint32_t> h_runes;       // host-resident dictionary: the two arrays
  std::vector<uint64_t> h_sig;
  DeviceBlock mem;                     // device-resident: owns them
  const uint32_t* d_runes = nullptr; const uint64_t* d_sig = nullptr;
};

namespace {

std::atomic<uint32_t> g_es_slices{0};                  // sg_debug_edit_search_slices (0: automatic)
std::atomic<uint64_t> g_es_bytes{0};                   // sg_debug_edit_search_bytes (0: kEsRowBytes)

int es_check(const sg_edit_index* ix, const sg_edit_config* cfg, const void* q_offs, uint32_t n_q, uint32_t k, const void* ids, const void* dist,
             const void* counts) {
  if (!ix) { set_error("null edit index"); return SG_E_INVALID; }
  if (int rc = edit_check_config(cfg)) return rc;
  if ((cfg->fold_case != 0) != (ix->fold != 0)) { set_error("edit search: fold_case differs from the index's"); return SG_E_INVALID; }
  if (cfg->max_distance > SG_EDIT_SEARCH_MAX_DISTANCE) { set_error("edit search: max_distance above 32"); return SG_E_INVALID; }
  if (k == 0 || k > kEditRankSlots) { set_error("edit search: k should be in 1 .. 1024"); return SG_E_INVALID; }
  if (n_q && (!q_offs || !ids || !dist || !counts)) { set_error("null argument"); return SG_E_INVALID; }
  return dict_check_geometry(nullptr, n_q, k, (uint64_t)n_q * k);
}

// the host-resident handle: the plain loop, through the same filter
int es_host(const sg_edit_index* ix, const sg_edit_config& cfg, const uint8_t* q, const uint64_t* q_offs, uint32_t n_q, uint32_t k, uint32_t* ids,
            uint32_t* dist, uint32_t* counts, uint32_t* hist) {
  const sg_dictionary* d = ix->dict;
  const uint32_t bins = cfg.max_distance + 1u;
  std::vector<uint32_t> qa, ca, work;
  std::vector<uint64_t> found;
  for (uint32_t i = 0; i < n_q; i++) {
    std::fill(ids + (size_t)i * k, ids + (size_t)(i + 1) * k, 0u);
    std::fill(dist + (size_t)i * k, dist + (size_t)(i + 1) * k, 0u);
    if (hist) std::fill(hist + (size_t)i * bins, hist + (size_t)(i + 1) * bins, 0u);
    edit_host_runes(q + q_offs[i], (size_t)(q_offs[i + 1] - q_offs[i]), ix->fold != 0, qa);
    if (qa.size() > 64) { counts[i] = SG_COUNT_TOO_LONG; continue; }
    uint64_t sig_q = 0;
    for (uint32_t r : qa) sig_q |= edit_sig_bit(r);
    found.clear();
    for (uint32_t doc = 0; doc < d->n_docs; doc++) {
      if (!edit_sig_pass(sig_q, (uint32_t)qa.size(), ix->h_sig[doc], ix->h_runes[doc], cfg.max_distance)) continue;
      edit_host_runes(d->h_blob.data() + d->h_offs[doc], (size_t)(d->h_offs[(size_t)doc + 1] - d->h_offs[doc]), ix->fold != 0, ca);
      const uint32_t s = edit_host_distance(qa, ca, cfg.mode == SG_EDIT_OSA, work);
      if (s > cfg.max_distance) continue;
      if (hist) hist[(size_t)i * bins + s]++;
      found.push_back(((uint64_t)s << 32) | doc);
    }
    const size_t n = std::min<size_t>(found.size(), k);
    std::partial_sort(found.begin(), found.begin() + (long)n, found.end());
    for (size_t p = 0; p < n; p++) { ids[(size_t)i * k + p] = (uint32_t)found[p]; dist[(size_t)i * k + p] = (uint32_t)(found[p] >> 32); }
    counts[i] = (uint32_t)n;
  }
  return SG_OK;
}

// The search on `st` (the caller has made the dictionary's device current): device pointers; hist null: kept in the scratch block.
int es_enqueue(const sg_edit_index* ix, const sg_edit_config& cfg, const uint8_t* q, const uint64_t* q_offs, uint32_t n_q, uint32_t k, uint32_t* ids,
               uint32_t* dist, uint32_t* counts, uint32_t* hist, hipStream_t st) {
  if (!n_q) return SG_OK;
  const sg_dictionary* d = ix->dict;
  const uint32_t bins = cfg.max_distance + 1u;
  // slices: enough wavefronts to fill the device from a small batch, 64 documents a slice at least
  const uint32_t tiles_all = (n_q + kEsTile - 1u) / kEsTile;
  uint32_t n_slices = g_es_slices.load(std::memory_order_relaxed);
  if (!n_slices) n_slices = std::max(1u, std::min((kEsWantWaves + tiles_all - 1u) / tiles_all, (uint32_t)(((uint64_t)d->n_docs + 63u) / 64u)));
  n_slices = std::min(n_slices, kEsMaxSlices);
  const uint32_t per_slice = (uint32_t)(((uint64_t)d->n_docs + n_slices - 1u) / n_slices);
  // chunks: the rows of a chunk's queries within the budget, a query at least
  const uint64_t budget = g_es_bytes.load(std::memory_order_relaxed) ? g_es_bytes.load(std::memory_order_relaxed) : kEsRowBytes;
  const uint64_t per_query = (1ull + n_slices) * ((uint64_t)k * 8u + 4u);
  uint32_t chunk = (uint32_t)std::min<uint64_t>(std::max<uint64_t>(budget / per_query, 1), std::min(n_q, kEsMaxChunk));
  if (chunk > kEsTile) chunk -= chunk % kEsTile;
  Carve c;
  const size_t o_hist = c.take(hist ? 0 : (size_t)n_q * bins * 4), o_n = c.take((size_t)chunk * (1u + n_slices) * 4);
  const size_t o_ids = c.take((size_t)chunk * (1u + n_slices) * k * 4), o_dist = c.take((size_t)chunk * (1u + n_slices) * k * 4);
  void* blkv = nullptr;
  if (int rc = stream_scratch(d->device, st, c.size(), &blkv, SCRATCH_EDIT_SEARCH)) return rc;
  char* blk = (char*)blkv;
  if (poison_mode()) { if (int rc = poison_fill(blk, c.size(), PZ_ROWS, st)) return rc; }
  EsArgs a{};
  a.d = d->view; a.low = EditLower{d->d_lower_from, d->d_lower_to, d->n_lower}; a.runes = ix->d_runes; a.sig = ix->d_sig;
  a.q_blob = q; a.q_offs = q_offs; a.k = k; a.max_distance = cfg.max_distance; a.n_slices = n_slices; a.per_slice = per_slice;
  a.osa = cfg.mode == SG_EDIT_OSA; a.fold = ix->fold != 0;
  a.hist = hist ? hist : (uint32_t*)(blk + o_hist);
  a.row_n = (uint32_t*)(blk + o_n); a.row_ids = (uint32_t*)(blk + o_ids); a.row_dist = (uint32_t*)(blk + o_dist);
  a.ids = ids; a.dist = dist; a.counts = counts;
  HIP_TRY(hipMemsetAsync(a.hist, 0, (size_t)n_q * bins * 4, st));
  for (uint32_t first = 0; first < n_q; first += chunk) {
    a.q_first = first; a.n_q = std::min(chunk, n_q - first);
    HIP_TRY(hipMemsetAsync(a.row_n, 0, (size_t)a.n_q * (1u + n_slices) * 4, st));
    const dim3 grid((n_slices + kEsWaves - 1u) / kEsWaves, (a.n_q + kEsTile - 1u) / kEsTile);
    hipLaunchKernelGGL(edit_scan_kernel<false>, grid, dim3(64 * kEsWaves), 0, st, a);
    HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(edit_scan_kernel<true>, grid, dim3(64 * kEsWaves), 0, st, a);
    HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(edit_search_rank_kernel, dim3(std::min(a.n_q, 65536u)), dim3(256), 0, st, a);
    HIP_TRY(hipGetLastError());
  }
  return SG_OK;
}

// The regions of sg_edit_search on a device index.  Out: the rows, the counts and the histograms (hist null: the region lives in
// the block alone); every word of them is written by the step.  In: the queries.
enum { ES_IDS = 0, ES_DIST, ES_COUNTS, ES_HIST, ES_Q_OFFS, ES_Q };
IoCall edit_search_io(const uint8_t* q, const uint64_t* q_offs, uint32_t n_q, uint32_t k, uint32_t bins, uint32_t* ids, uint32_t* dist, uint32_t* counts,
                      uint32_t* hist) {
  return IoCall().add(IO_OUT, ids, (size_t)n_q * k * 4, 16, false, PZ_OUT_IDS).add(IO_OUT, dist, (size_t)n_q * k * 4, 4, false, PZ_OUT_IDS)
      .add(IO_OUT, counts, (size_t)n_q * 4, 4, false, PZ_OUT_COUNTS).add(IO_OUT, hist, (size_t)n_q * bins * 4, 4).add_window(q_offs, n_q, q);
}

}  // namespace

extern "C" {

int sg_edit_index_create(sg_dictionary* dict, int fold_case, sg_edit_index** out) {
  SG_GUARD_BEGIN
  if (!out) { set_error("null argument"); return SG_E_INVALID; }
  if (!dict) { set_error("null dictionary"); return SG_E_INVALID; }
  std::unique_ptr<sg_edit_index> ix(new sg_edit_index);
  ix->fold = fold_case != 0;
  if (dict->device < 0) {
    ix->h_runes.resize(dict->n_docs); ix->h_sig.resize(dict->n_docs);
    std::vector<uint32_t> ra;
    for (uint32_t i = 0; i < dict->n_docs; i++) {
      edit_host_runes(dict->h_blob.data() + dict->h_offs[i], (size_t)(dict->h_offs[(size_t)i + 1] - dict->h_offs[i]), ix->fold != 0, ra);
      uint64_t s = 0;
      for (uint32_t r : ra) s |= edit_sig_bit(r);
      ix->h_runes[i] = (uint32_t)ra.size(); ix->h_sig[i] = s;
    }
  } else {
    DeviceGuard dg;
    HIP_TRY(dg.set(dict->device));
    uint32_t* runes = nullptr;
    uint64_t* sig = nullptr;
    if (int rc = ix->mem.alloc(&runes, dict->n_docs)) return rc;
    if (int rc = ix->mem.alloc(&sig, dict->n_docs)) return rc;
    if (dict->n_docs) {
      const uint32_t blocks = (uint32_t)std::min<uint64_t>(((uint64_t)dict->n_docs + 255u) / 256u, 16384u);
      hipLaunchKernelGGL(edit_sig_kernel, dim3(blocks), dim3(256), 0, (hipStream_t) nullptr, dict->view, EditLower{dict->d_lower_from, dict->d_lower_to, dict->n_lower},
                         ix->fold, runes, sig);
      HIP_TRY(hipGetLastError());
      HIP_TRY(hipStreamSynchronize(nullptr));
    }
    ix->d_runes = runes; ix->d_sig = sig;
  }
  sg_dictionary_retain(dict);
  ix->dict = dict;
  *out = ix.release();
  return SG_OK;
  SG_GUARD_END(SG_RC)
}

void sg_edit_index_retain(sg_edit_index* ix) { if (ix) ix->refs.fetch_add(1); }
void sg_edit_index_release(sg_edit_index* ix) {
  if (!ix) return;
  if (ix->refs.fetch_sub(1) != 1) return;
  sg_dictionary* d = ix->dict;
  delete ix;                                               // the DeviceBlock frees its HBM
  sg_dictionary_release(d);
}

int sg_edit_search_device(sg_edit_index* ix, const sg_edit_config* cfg, const void* d_q_blob, const void* d_q_offs, uint32_t n_q, uint32_t k, void* d_ids,
                          void* d_dist, void* d_counts, void* d_hist, void* stream) {
  SG_GUARD_BEGIN
  if (int rc = es_check(ix, cfg, d_q_offs, n_q, k, d_ids, d_dist, d_counts)) return rc;
  if (ix->dict->device < 0) { set_error("a host-resident dictionary cannot serve a device call"); return SG_E_UNSUPPORTED; }
  DeviceGuard dg;
  HIP_TRY(dg.set(ix->dict->device));
  return es_enqueue(ix, *cfg, (const uint8_t*)d_q_blob, (const uint64_t*)d_q_offs, n_q, k, (uint32_t*)d_ids, (uint32_t*)d_dist, (uint32_t*)d_counts,
                    (uint32_t*)d_hist, (hipStream_t)stream);
  SG_GUARD_END(SG_RC)
}

int sg_edit_search(sg_edit_index* ix, const sg_edit_config* cfg, const uint8_t* q, const uint64_t* q_offs, uint32_t n_q, uint32_t k, uint32_t* ids,
                   uint32_t* dist, uint32_t* counts, uint32_t* hist) {
  SG_GUARD_BEGIN
  if (int rc = es_check(ix, cfg, q_offs, n_q, k, ids, dist, counts)) return rc;
  for (uint32_t i = 0; i < n_q; i++)
    if (q_offs[i + 1] < q_offs[i]) { set_error("query offsets must not decrease"); return SG_E_INVALID; }
  if (n_q && !q && q_offs[n_q] != q_offs[0]) { set_error("null query buffer"); return SG_E_INVALID; }
  if (!n_q) return SG_OK;
  if (ix->dict->device < 0) return es_host(ix, *cfg, q, q_offs, n_q, k, ids, dist, counts, hist);
  const sg_edit_config config = *cfg;
  return run_host_call(ix->dict->device, edit_search_io(q, q_offs, n_q, k, config.max_distance + 1u, ids, dist, counts, hist), [&](const IoCall& io, hipStream_t st) -> int {
    return es_enqueue(ix, config, io.at<uint8_t>(ES_Q), io.at<uint64_t>(ES_Q_OFFS), n_q, k, io.at<uint32_t>(ES_IDS), io.at<uint32_t>(ES_DIST),
                      io.at<uint32_t>(ES_COUNTS), io.at<uint32_t>(ES_HIST), st);
  });
  SG_GUARD_END(SG_RC)
}

// Test hook: one of the index's two arrays as it lies in memory — which 0: runes (u32 per document), 1: sig (u64 per document).
// out null: *out_bytes alone.
int sg_debug_edit_index_array(sg_edit_index* ix, uint32_t which, void* out, uint64_t cap_bytes, uint64_t* out_bytes) {
  SG_GUARD_BEGIN
  if (!ix || !out_bytes) { set_error("null argument"); return SG_E_INVALID; }
  if (which > 1u) { set_error("sg_debug_edit_index_array: unknown array"); return SG_E_INVALID; }
  const uint64_t bytes = (uint64_t)ix->dict->n_docs * (which ? 8u : 4u);
  *out_bytes = bytes;
  if (!out) return SG_OK;
  if (cap_bytes < bytes) { set_error("sg_debug_edit_index_array: buffer too small"); return SG_E_INVALID; }
  if (!bytes) return SG_OK;
  if (ix->dict->device < 0) { memcpy(out, which ? (const void*)ix->h_sig.data() : (const void*)ix->h_runes.data(), (size_t)bytes); return SG_OK; }
  DeviceGuard dg;
  HIP_TRY(dg.set(ix->dict->device));
  HIP_TRY(hipMemcpy(out, which ? (const void*)ix->d_sig : (const void*)ix->d_runes, (size_t)bytes, hipMemcpyDeviceToHost));
  return SG_OK;
  SG_GUARD_END(SG_RC)
}

int sg_debug_edit_search_slices(uint32_t n) {
  g_es_slices.store(n, std::memory_order_relaxed);
  return SG_OK;
}
int sg_debug_edit_search_bytes(uint64_t bytes) {
  g_es_bytes.store(bytes, std::memory_order_relaxed);
  return SG_OK;
}

}  // extern "C"
