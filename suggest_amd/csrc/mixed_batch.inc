// mixed_batch.inc — one batch whose queries differ in metric, similarity and k (sg_suggest_batch_mixed, include/suggest_hip.h;
// DESIGN.md §5b), included by engine.hip after the host files (it uses capi.inc's launch(), stream_scratch and poison_fill,
// host_call.inc's run_host_call and search_io, index_api.inc's replica_of_pointer, handles.inc's check_search_values).
// The search kernels keep one (metric, similarity, k) per launch: a mixed call is one enqueue step, mixed_enqueue, around the launch() of every group —
//   count     mixed_count_kernel: every config number checked against n_configs (a bad one raises the call's error word and is
//             counted nowhere), a histogram over the configs, the queries' byte lengths, the sort's keys and values;
//   permute   a stable radix sort of the query numbers by the 8-bit config number (hipcub, as device_sort_pairs): within a group
//             the queries keep the caller's order — results cannot depend on the order, a deterministic one is what lets
//             sg_debug_mixed_last be held against tests/mixed_shapes.py word for word;
//   gather    mixed_lengths_kernel + an exclusive sum give ONE array of n_q + 1 grouped offsets, mixed_gather_kernel copies every
//             query's bytes to its grouped position; the search kernels read q_blob[q_offs[i] .. q_offs[i + 1]) with absolute
//             offsets, so group g is (offsets + group_start[g], n_g queries) over the same blob, a dense launch of its own;
//   scatter   mixed_scatter_kernel copies every group row (n_g x k_g, dense, zeroed or poisoned before its launch as a plain
//             call's rows are) to the caller's ragged row and the count to the caller's order.  It copies all k_g slots, so the
//             slots past a row's count carry what the plain call leaves there; an autocomplete row's score slots are written zero.
// The host-buffer route is host_call.inc's run_host_call around the step: it knows the group sizes from config_of in host memory.  The
// device route reads the n_configs counters (and the error word, and the queries' bytes in all) back through pinned memory with
// ONE wait on the caller's stream — the one place where a device call is not asynchronous.
// The call's own device memory is two blocks of the calling thread's per-stream scratch (SCRATCH_MIXED: lists and offsets, sized by
// n_q; SCRATCH_MIXED_ROWS: the grouped blob and the groups' rows, sized once the group sizes are known).

namespace sg {

constexpr uint32_t kMixedThreads = 256;
static_assert(kMixedThreads == SG_MAX_MIXED_CONFIGS, "mixed_count_kernel: a thread per histogram word");
constexpr uint32_t kMixedSub = 16;                     // lanes that copy one query's bytes / one row
constexpr uint32_t kMixedAutocomplete = 0x80000000u;   // MixedK::k: the config is an autocomplete one (k <= SG_MAX_TOPK below it)

struct MixedK { uint32_t k[SG_MAX_MIXED_CONFIGS]; };   // per config: k | kMixedAutocomplete (a kernel argument: 1 KiB)

// the control words of a call, zeroed before the counting launch; the device route copies them to the host
struct MixedCtl {
  uint32_t hist[SG_MAX_MIXED_CONFIGS];   // queries per config
  uint32_t bad;                          // != 0: a config number >= n_configs was seen
  uint32_t pad_;
  uint64_t q_bytes;                      // q_offs[n_q] - q_offs[0]
};
// what the scatter reads per config (mixed_table_kernel derives it from the histogram; the host derives the same for its launches)
struct MixedTable {
  uint64_t row_base[SG_MAX_MIXED_CONFIGS];   // first slot of the group's rows in the grouped ids / scores
  uint32_t start[SG_MAX_MIXED_CONFIGS];      // first grouped position of the group
};
// a group's rows start at a multiple of four slots (16 bytes of ids, 32 of scores)
__host__ __device__ inline uint64_t mixed_rows_of(uint32_t n, uint32_t k) { return ((uint64_t)n * k + 3u) & ~(uint64_t)3u; }

// One thread per query; thread n_q closes the two scan inputs with a zero.  key / idx: the sort's input (a bad config number sorts
// as config 0 — the call fails before anything reads the result); slots[i]: the row's k, the scan's input for row_offs.
__global__ __launch_bounds__(kMixedThreads) void mixed_count_kernel(const uint32_t* __restrict__ config_of, const uint64_t* __restrict__ q_offs,
                                                                     uint32_t n_q, uint32_t n_configs, const MixedK kt, MixedCtl* ctl,
                                                                     uint32_t* __restrict__ key, uint32_t* __restrict__ idx,
                                                                     uint32_t* __restrict__ len, uint64_t* __restrict__ slots) {
  __shared__ uint32_t s_hist[SG_MAX_MIXED_CONFIGS];
  __shared__ uint32_t s_bad;
  const uint32_t tid = threadIdx.x;
  s_hist[tid] = 0u;                                      // (kMixedThreads == SG_MAX_MIXED_CONFIGS)
  if (tid == 0) s_bad = 0u;
  __syncthreads();
  for (uint64_t i = (uint64_t)blockIdx.x * kMixedThreads + tid; i <= n_q; i += (uint64_t)gridDim.x * kMixedThreads) {
    if (i == n_q) { slots[i] = 0ull; if (n_q) ctl->q_bytes = q_offs[n_q] - q_offs[0]; continue; }
    const uint32_t c = config_of[i];
    const bool ok = c < n_configs;
    if (ok) atomicAdd(&s_hist[c], 1u); else s_bad = 1u;
    key[i] = ok ? c : 0u;
    idx[i] = (uint32_t)i;
    len[i] = (uint32_t)(q_offs[i + 1] - q_offs[i]);
    slots[i] = ok ? (uint64_t)(kt.k[c] & ~kMixedAutocomplete) : 0ull;
  }
  __syncthreads();
  if (s_hist[tid]) atomicAdd(&ctl->hist[tid], s_hist[tid]);
  if (tid == 0 && s_bad) atomicOr(&ctl->bad, 1u);
}

// the groups' first positions and first row slots, from the histogram: 256 additions by one thread.  ONE rule, stated three
// times that must stay in step: group g begins at the sum of the sizes before it, its rows at the sum of mixed_rows_of(size, k)
// before it — here for the scatter, in mixed_enqueue's host loop (start[], row_base[]) for the groups' launches, and the
// caller's row_offs (Σ k_j) by the device scan over `slots` as well as, on the host route, by mixed_host_call for the caller.
__global__ __launch_bounds__(64) void mixed_table_kernel(const MixedCtl* __restrict__ ctl, uint32_t n_configs, const MixedK kt, MixedTable* t) {
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  uint32_t start = 0;
  uint64_t base = 0;
  for (uint32_t g = 0; g < n_configs; g++) {
    t->start[g] = start; t->row_base[g] = base;
    const uint32_t n = ctl->hist[g];
    start += n; base += mixed_rows_of(n, kt.k[g] & ~kMixedAutocomplete);
  }
}

// glen[j] = the bytes of the query at grouped position j; glen[n_q] = 0 (the scan's last input)
__global__ __launch_bounds__(kMixedThreads) void mixed_lengths_kernel(const uint32_t* __restrict__ perm, const uint32_t* __restrict__ len,
                                                                       uint32_t n_q, uint64_t* __restrict__ glen) {
  for (uint64_t j = (uint64_t)blockIdx.x * kMixedThreads + threadIdx.x; j <= n_q; j += (uint64_t)gridDim.x * kMixedThreads)
    glen[j] = j < n_q ? (uint64_t)len[perm[j]] : 0ull;
}

// kMixedSub lanes per query: the bytes q[q_offs[perm[j]] ..) go to gq[goffs[j] ..) by d_copy_bytes (engine.hip: pieces of 16, 8 or
// 4 bytes where source and destination share their position within one, the ragged ends byte by byte).  gq_bytes: the room of gq.
__global__ __launch_bounds__(kMixedThreads) void mixed_gather_kernel(const uint8_t* __restrict__ q, const uint64_t* __restrict__ q_offs,
                                                                      const uint32_t* __restrict__ perm, const uint64_t* __restrict__ goffs,
                                                                      uint8_t* __restrict__ gq, uint64_t gq_bytes, uint32_t n_q) {
  const uint32_t sub = threadIdx.x % kMixedSub;
  const uint64_t per = kMixedThreads / kMixedSub;
  for (uint64_t j = (uint64_t)blockIdx.x * per + threadIdx.x / kMixedSub; j < n_q; j += (uint64_t)gridDim.x * per) {
    const uint64_t from = q_offs[perm[j]], to = goffs[j];
    const uint32_t n = (uint32_t)(goffs[j + 1] - to);
    if (to + n > gq_bytes) continue;          // (offsets that do not ascend: the lengths add up to more than the blob — nothing is written past it)
    d_copy_bytes(gq + to, q + from, n, sub, kMixedSub);
  }
}

// kMixedSub lanes per grouped position j: the group's row j - start[g] goes to the caller's row of query perm[j], all k slots of it;
// an autocomplete row's score slots are written zero (g_scores is not read for it)
__global__ __launch_bounds__(kMixedThreads) void mixed_scatter_kernel(const uint32_t* __restrict__ perm, const uint32_t* __restrict__ key,
                                                                       const MixedTable* __restrict__ t, const MixedK kt,
                                                                       const uint32_t* __restrict__ g_ids, const uint64_t* __restrict__ g_scores,
                                                                       const uint32_t* __restrict__ g_counts, const uint64_t* __restrict__ row_offs,
                                                                       uint32_t* __restrict__ out_ids, uint64_t* __restrict__ out_scores,
                                                                       uint32_t* __restrict__ out_counts, uint32_t n_q) {
  const uint32_t sub = threadIdx.x % kMixedSub;
  const uint64_t per = kMixedThreads / kMixedSub;
  for (uint64_t j = (uint64_t)blockIdx.x * per + threadIdx.x / kMixedSub; j < n_q; j += (uint64_t)gridDim.x * per) {
    const uint32_t g = key[j], i = perm[j];
    const uint32_t kw = kt.k[g], k = kw & ~kMixedAutocomplete;
    const bool scores = (kw & kMixedAutocomplete) == 0u;
    const uint64_t from = t->row_base[g] + (uint64_t)(j - t->start[g]) * k, to = row_offs[i];
    if (sub == 0) out_counts[i] = g_counts[j];
    for (uint32_t s = sub; s < k; s += kMixedSub) {
      out_ids[to + s] = g_ids[from + s];
      out_scores[to + s] = scores ? g_scores[from + s] : 0ull;     // (bit for bit: no arithmetic touches a score)
    }
  }
}

}  // namespace sg

namespace {

// the SCRATCH_MIXED block: everything sized by n_q (and the sort's and the scans' working memory)
struct MixedLayout {
  size_t ctl = 0, table = 0, key_in = 0, key = 0, idx = 0, perm = 0, len = 0, glen = 0, goffs = 0, slots = 0, row_offs = 0, tmp = 0, tmp_bytes = 0, bytes = 0;
};
int mixed_layout(uint32_t n_q, MixedLayout* out) {
  MixedLayout L;
  size_t sort_tmp = 0, scan_tmp = 0;
  HIP_TRY(hipcub::DeviceRadixSort::SortPairs(nullptr, sort_tmp, (const uint32_t*)nullptr, (uint32_t*)nullptr, (const uint32_t*)nullptr, (uint32_t*)nullptr,
                                             (int)n_q, 0, 8, (hipStream_t) nullptr));
  HIP_TRY(hipcub::DeviceScan::ExclusiveSum(nullptr, scan_tmp, (const uint64_t*)nullptr, (uint64_t*)nullptr, (int)n_q + 1, (hipStream_t) nullptr));
  Carve c;
  L.ctl = c.take(sizeof(MixedCtl)); L.table = c.take(sizeof(MixedTable));
  L.key_in = c.take((size_t)n_q * 4); L.key = c.take((size_t)n_q * 4); L.idx = c.take((size_t)n_q * 4); L.perm = c.take((size_t)n_q * 4);
  L.len = c.take((size_t)n_q * 4);
  L.glen = c.take(((size_t)n_q + 1) * 8); L.goffs = c.take(((size_t)n_q + 1) * 8);
  L.slots = c.take(((size_t)n_q + 1) * 8); L.row_offs = c.take(((size_t)n_q + 1) * 8);
  L.tmp_bytes = std::max(sort_tmp, scan_tmp);
  L.tmp = c.take(L.tmp_bytes, 256);
  L.bytes = c.size();
  *out = L;
  return SG_OK;
}

// What a thread keeps between its mixed calls: the pinned words the device route's counters come back through, and where the
// last call's permutation lies (sg_debug_mixed_last reads it from the scratch block, which the thread's next mixed call on that
// stream overwrites).  A thread that ends hands the pinned block back (the main thread's is left to process exit, as its other
// blocks are).
struct MixedThread {
  GrowBlock pin{true};
  hipEvent_t ev[6] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};   // sg_debug_mixed_timing
  int device = -1;
  hipStream_t stream = nullptr;
  const void* perm = nullptr;
  uint32_t n_q = 0;
  std::vector<uint32_t> group_start;    // n_configs + 1
  double ms[5] = {0, 0, 0, 0, 0};
  ~MixedThread() {
    if (on_main_thread()) return;
    pin.release();
    for (hipEvent_t e : ev) if (e) (void)hipEventDestroy(e);
  }
};
thread_local MixedThread t_mixed;
std::atomic<int> g_mixed_timing{0};

// Everything a mixed call is checked for before the index is looked at: the table, the pointers, and — on the host route, where
// config_of is readable — the config numbers and rows_cap.  counts: queries per config (host route only).
int mixed_check_configs(const sg_search_config* configs, uint32_t n_configs) {
  if (!configs) { set_error("null argument"); return SG_E_INVALID; }
  if (n_configs == 0 || n_configs > SG_MAX_MIXED_CONFIGS) { set_error("mixed batch: n_configs outside 1 .. SG_MAX_MIXED_CONFIGS"); return SG_E_INVALID; }
  for (uint32_t g = 0; g < n_configs; g++) {
    const sg_search_config& c = configs[g];
    if (c.autocomplete != 0 && c.autocomplete != 1) { set_error("mixed batch: autocomplete is 0 or 1"); return SG_E_INVALID; }
    if (int rc = check_search_values(c.k, c.autocomplete == 0, c.similarity, c.metric)) return rc;
    if (!c.autocomplete && c.first_doc != 0) { set_error("mixed batch: first_doc with a fuzzy config"); return SG_E_INVALID; }
  }
  return SG_OK;
}
int mixed_check_index(sg_index* index) {
  if (!index->uploaded.load(std::memory_order_acquire)) { set_error("index not uploaded: call sg_index_upload first"); return SG_E_NOT_UPLOADED; }
  return SG_OK;
}

struct MixedIo {          // device pointers of a call
  const uint8_t* q; const uint64_t* offs; const uint32_t* config_of;
  uint32_t* ids; uint64_t* scores; uint32_t* counts; uint64_t* row_offs;   // row_offs null: kept in the scratch block
};

// The enqueue step.  host_counts: the queries per config where the caller knows them (the host route; with host_q_bytes, the
// queries' bytes in all, and no_long[g], LaunchReq::no_long_queries of group g); null: they are read back from the device, with the
// error word, behind one wait on `st`, and rows_cap is checked then.
int mixed_enqueue(sg_index* index, Replica* rep, const MixedIo& io, uint32_t n_q, const sg_search_config* configs, uint32_t n_configs,
                  const uint32_t* host_counts, uint64_t host_q_bytes, const uint8_t* no_long, uint64_t rows_cap, hipStream_t st) {
  if (n_q > 0x7FFFFFF0u) { set_error("mixed batch: too many queries for one call"); return SG_E_INVALID; }   // (hipcub counts in int)
  DeviceGuard dg;
  HIP_TRY(dg.set(rep->device));
  MixedLayout L;
  if (int rc = mixed_layout(n_q, &L)) return rc;
  void* blk = nullptr;
  if (int rc = stream_scratch(rep->device, st, L.bytes, &blk, SCRATCH_MIXED)) return rc;
  char* b = (char*)blk;
  MixedThread& T = t_mixed;
  T.perm = nullptr;
  const bool timing = !host_counts && g_mixed_timing.load(std::memory_order_relaxed) != 0;
  if (timing) for (hipEvent_t& e : T.ev) if (!e) HIP_TRY(hipEventCreate(&e));
  auto stamp = [&](int i) -> int { if (timing) HIP_TRY(hipEventRecord(T.ev[i], st)); return SG_OK; };
  const bool poison = poison_mode() != 0;
  if (poison) {   // lists of query numbers and offsets: 0, a query of every batch and an offset inside every blob (see poison_fill)
    if (int rc = poison_words(b + L.key_in, (L.tmp - L.key_in) / 4, 0u, PZ_ROWS, st)) return rc;
  }
  MixedK kt{};
  for (uint32_t g = 0; g < n_configs; g++) kt.k[g] = configs[g].k | (configs[g].autocomplete ? kMixedAutocomplete : 0u);
  MixedCtl* ctl = (MixedCtl*)(b + L.ctl);
  MixedTable* table = (MixedTable*)(b + L.table);
  uint32_t *key_in = (uint32_t*)(b + L.key_in), *key = (uint32_t*)(b + L.key), *idx = (uint32_t*)(b + L.idx), *perm = (uint32_t*)(b + L.perm);
  uint32_t* len = (uint32_t*)(b + L.len);
  uint64_t *glen = (uint64_t*)(b + L.glen), *goffs = (uint64_t*)(b + L.goffs), *slots = (uint64_t*)(b + L.slots);
  uint64_t* row_offs = io.row_offs ? io.row_offs : (uint64_t*)(b + L.row_offs);
  const uint32_t blocks = (uint32_t)std::min<uint64_t>(((uint64_t)n_q + kMixedThreads) / kMixedThreads, 2048u);
  const uint32_t sub_blocks = (uint32_t)std::min<uint64_t>(((uint64_t)n_q * kMixedSub + kMixedThreads - 1) / kMixedThreads, 4096u);
  // ---- count ----
  if (int rc = stamp(0)) return rc;
  HIP_TRY(hipMemsetAsync(ctl, 0, sizeof(MixedCtl), st));
  hipLaunchKernelGGL(mixed_count_kernel, dim3(blocks), dim3(kMixedThreads), 0, st, io.config_of, io.offs, n_q, n_configs, kt, ctl, key_in, idx, len, slots);
  HIP_TRY(hipGetLastError());
  hipLaunchKernelGGL(mixed_table_kernel, dim3(1), dim3(64), 0, st, (const MixedCtl*)ctl, n_configs, kt, table);
  HIP_TRY(hipGetLastError());
  // the group sizes: the caller's, or the device's through pinned memory (the one wait of the device route)
  std::vector<uint32_t> n_of(n_configs);
  uint64_t q_bytes = host_q_bytes;
  if (host_counts) std::copy(host_counts, host_counts + n_configs, n_of.begin());
  else {
    if (int rc = T.pin.grow(sizeof(MixedCtl))) return rc;
    HIP_TRY(hipMemcpyAsync(T.pin.p, ctl, sizeof(MixedCtl), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    const MixedCtl* h = (const MixedCtl*)T.pin.p;
    if (h->bad) { set_error("mixed batch: config_of holds a number outside the table"); return SG_E_INVALID; }
    std::copy(h->hist, h->hist + n_configs, n_of.begin());
    q_bytes = h->q_bytes;
  }
  std::vector<uint32_t> start(n_configs + 1, 0);
  std::vector<uint64_t> row_base(n_configs + 1, 0);
  uint64_t need = 0;
  for (uint32_t g = 0; g < n_configs; g++) {                  // (mixed_table_kernel's rule, for the launches below)
    start[g + 1] = start[g] + n_of[g];
    row_base[g + 1] = row_base[g] + mixed_rows_of(n_of[g], configs[g].k);
    need += (uint64_t)n_of[g] * configs[g].k;
  }
  if (start[n_configs] != n_q) { set_error("mixed batch: the group sizes do not add up to the batch"); return SG_E_INVALID; }
  if (need > rows_cap) { set_error("mixed batch: rows_cap is below the sum of the queries' k"); return SG_E_INVALID; }
  if (int rc = stamp(1)) return rc;
  // ---- permute ----
  size_t tmp_bytes = L.tmp_bytes;
  HIP_TRY(hipcub::DeviceRadixSort::SortPairs(b + L.tmp, tmp_bytes, (const uint32_t*)key_in, key, (const uint32_t*)idx, perm, (int)n_q, 0, 8, st));
  if (int rc = stamp(2)) return rc;
  // ---- gather: the grouped offsets, the caller's row offsets, the grouped blob ----
  Carve c;
  const size_t R = (size_t)row_base[n_configs];
  const size_t o_sc = c.take(R * 8), o_id = c.take(R * 4), o_cnt = c.take((size_t)n_q * 4), o_q = c.take((size_t)q_bytes, 16);
  void* rows_blk = nullptr;
  if (int rc = stream_scratch(rep->device, st, c.size(), &rows_blk, SCRATCH_MIXED_ROWS)) return rc;
  char* rb = (char*)rows_blk;
  uint64_t* g_scores = (uint64_t*)(rb + o_sc);
  uint32_t *g_ids = (uint32_t*)(rb + o_id), *g_counts = (uint32_t*)(rb + o_cnt);
  uint8_t* gq = (uint8_t*)(rb + o_q);
  hipLaunchKernelGGL(mixed_lengths_kernel, dim3(blocks), dim3(kMixedThreads), 0, st, (const uint32_t*)perm, (const uint32_t*)len, n_q, glen);
  HIP_TRY(hipGetLastError());
  tmp_bytes = L.tmp_bytes;
  HIP_TRY(hipcub::DeviceScan::ExclusiveSum(b + L.tmp, tmp_bytes, (const uint64_t*)glen, goffs, (int)n_q + 1, st));
  tmp_bytes = L.tmp_bytes;
  HIP_TRY(hipcub::DeviceScan::ExclusiveSum(b + L.tmp, tmp_bytes, (const uint64_t*)slots, row_offs, (int)n_q + 1, st));
  if (poison) { if (int rc = poison_fill(gq, (size_t)q_bytes, PZ_ROWS, st)) return rc; }
  hipLaunchKernelGGL(mixed_gather_kernel, dim3(sub_blocks), dim3(kMixedThreads), 0, st, io.q, io.offs, (const uint32_t*)perm, (const uint64_t*)goffs, gq, q_bytes, n_q);
  HIP_TRY(hipGetLastError());
  if (int rc = stamp(3)) return rc;
  // ---- the groups: rows zeroed (poisoned) as a host-buffer call's, then the ordinary launch of the group's config ----
  if (poison) {
    if (int rc = poison_fill(g_scores, R * 8, PZ_OUT_SCORES, st)) return rc;
    if (int rc = poison_fill(g_ids, R * 4, PZ_OUT_IDS, st)) return rc;
    if (int rc = poison_fill(g_counts, (size_t)n_q * 4, PZ_OUT_COUNTS, st)) return rc;
  } else HIP_TRY(hipMemsetAsync(rb, 0, o_id + R * 4, st));
  for (uint32_t g = 0; g < n_configs; g++) {
    if (n_of[g] == 0) continue;
    const sg_search_config& cf = configs[g];
    LaunchReq r;
    r.q = gq; r.offs = goffs + start[g]; r.n_q = n_of[g]; r.k = cf.k; r.stream = st;
    if (cf.autocomplete) { r.autocomplete = 1; r.ac_first = cf.first_doc; }
    else { r.metric = cf.metric; r.similarity = cf.similarity; r.scores = g_scores + row_base[g]; }
    r.ids = g_ids + row_base[g]; r.counts = g_counts + start[g];
    r.no_long_queries = no_long && no_long[g];
    if (int rc = launch(index, rep, r)) return rc;
  }
  if (int rc = stamp(4)) return rc;
  // ---- scatter ----
  hipLaunchKernelGGL(mixed_scatter_kernel, dim3(sub_blocks), dim3(kMixedThreads), 0, st, (const uint32_t*)perm, (const uint32_t*)key, (const MixedTable*)table, kt,
                     (const uint32_t*)g_ids, (const uint64_t*)g_scores, (const uint32_t*)g_counts, (const uint64_t*)row_offs, io.ids, io.scores, io.counts, n_q);
  HIP_TRY(hipGetLastError());
  if (int rc = stamp(5)) return rc;
  if (timing) {
    HIP_TRY(hipEventSynchronize(T.ev[5]));
    for (int i = 0; i < 5; i++) { float ms = 0; HIP_TRY(hipEventElapsedTime(&ms, T.ev[i], T.ev[i + 1])); T.ms[i] = ms; }
  }
  T.device = rep->device; T.stream = st; T.perm = perm; T.n_q = n_q; T.group_start = start;
  return SG_OK;
}

}  // namespace

// The host-buffer route on `rep`: arguments checked here (the coalescer's dispatchers call it too), the group sizes, the row
// offsets and each group's longest query taken from the caller's arrays, then one staging in, mixed_enqueue, one copy out.
static int mixed_host_call(sg_index* index, Replica* rep, const uint8_t* q, const uint64_t* offs, uint32_t n_q, const sg_search_config* configs,
                           uint32_t n_configs, const uint32_t* config_of, uint64_t rows_cap, uint32_t* ids, double* scores, uint32_t* counts,
                           uint64_t* row_offs) {
  if (!index) { set_error("null index"); return SG_E_INVALID; }
  if (int rc = mixed_check_configs(configs, n_configs)) return rc;
  if (!row_offs) { set_error("null argument"); return SG_E_INVALID; }
  if (n_q == 0) { row_offs[0] = 0; return SG_OK; }
  if (!offs || !config_of || !ids || !scores || !counts) { set_error("null argument"); return SG_E_INVALID; }
  std::vector<uint32_t> n_of(n_configs, 0);
  std::vector<uint8_t> no_long(n_configs, 1);
  uint64_t rows = 0;
  for (uint32_t i = 0; i < n_q; i++) {
    const uint32_t g = config_of[i];
    if (g >= n_configs) { set_error("mixed batch: config_of holds a number outside the table"); return SG_E_INVALID; }
    n_of[g]++;
    if (offs[i + 1] - offs[i] > 112) no_long[g] = 0;       // (no_long_queries, per group)
    row_offs[i] = rows;
    rows += configs[g].k;
  }
  row_offs[n_q] = rows;
  if (rows > rows_cap) { set_error("mixed batch: rows_cap is below the sum of the queries' k"); return SG_E_INVALID; }
  if (int rc = mixed_check_index(index)) return rc;
  if (!rep) rep = find_replica(index, -1);
  // a search's regions with ragged rows, not cleared (the scatter writes every slot of every row), and the config numbers behind the queries
  return run_host_call(rep->device, search_io(q, offs, n_q, rows, ids, scores, counts, nullptr, false, nullptr, config_of), [&](const IoCall& io, hipStream_t st) {
    const MixedIo m{io.at<uint8_t>(IO_Q), io.at<uint64_t>(IO_OFFS), io.at<uint32_t>(IO_SEL),
                    io.at<uint32_t>(IO_IDS), io.at<uint64_t>(IO_SCORES), io.at<uint32_t>(IO_COUNTS), nullptr};
    return mixed_enqueue(index, rep, m, n_q, configs, n_configs, n_of.data(), io.r[IO_Q].bytes, no_long.data(), rows, st);
  });
}

extern "C" {

int sg_suggest_batch_mixed(sg_index* index, const uint8_t* q, const uint64_t* offs, uint32_t n_q, const sg_search_config* configs, uint32_t n_configs,
                           const uint32_t* config_of, uint64_t rows_cap, uint32_t* ids, double* scores, uint32_t* counts, uint64_t* row_offs) {
  SG_GUARD_BEGIN
  return mixed_host_call(index, nullptr, q, offs, n_q, configs, n_configs, config_of, rows_cap, ids, scores, counts, row_offs);
  SG_GUARD_END(SG_RC)
}

int sg_suggest_batch_mixed_device(sg_index* index, const void* d_q, const void* d_offs, uint32_t n_q, const sg_search_config* configs,
                                  uint32_t n_configs, const void* d_config_of, uint64_t rows_cap, void* d_ids, void* d_scores, void* d_counts,
                                  void* d_row_offs, void* stream) {
  SG_GUARD_BEGIN
  if (!index) { set_error("null index"); return SG_E_INVALID; }
  if (int rc = mixed_check_configs(configs, n_configs)) return rc;
  if (!d_row_offs) { set_error("null argument"); return SG_E_INVALID; }
  if (n_q && (!d_offs || !d_config_of || !d_ids || !d_scores || !d_counts)) { set_error("null argument"); return SG_E_INVALID; }
  if (int rc = mixed_check_index(index)) return rc;
  Replica* rep = replica_of_pointer(index, d_offs);
  if (n_q == 0) {
    DeviceGuard dg;
    HIP_TRY(dg.set(rep->device));
    HIP_TRY(hipMemsetAsync(d_row_offs, 0, 8, (hipStream_t)stream));
    return SG_OK;
  }
  const MixedIo m{(const uint8_t*)d_q, (const uint64_t*)d_offs, (const uint32_t*)d_config_of, (uint32_t*)d_ids, (uint64_t*)d_scores,
                  (uint32_t*)d_counts, (uint64_t*)d_row_offs};
  return mixed_enqueue(index, rep, m, n_q, configs, n_configs, nullptr, 0, nullptr, rows_cap, (hipStream_t)stream);
  SG_GUARD_END(SG_RC)
}

int sg_coalesce_mixed(sg_index* index, int on) {
  SG_GUARD_BEGIN
  if (!index) { set_error("null index"); return SG_E_INVALID; }
  if (int rc = mixed_check_index(index)) return rc;
  Coalescer* c = coalescer_of(index);
  { std::lock_guard<std::mutex> lock(c->mu); c->mixed = on != 0; }
  return SG_OK;
  SG_GUARD_END(SG_RC)
}

int sg_debug_coalesce_hold(sg_index* index, int on) {
  SG_GUARD_BEGIN
  if (!index) { set_error("null index"); return SG_E_INVALID; }
  if (int rc = mixed_check_index(index)) return rc;
  Coalescer* c = coalescer_of(index);
  { std::lock_guard<std::mutex> lock(c->mu); c->hold = on != 0; }
  if (!on) c->cv.notify_all();
  return SG_OK;
  SG_GUARD_END(SG_RC)
}

int sg_debug_coalesce_stats(sg_index* index, uint64_t out[4]) {
  SG_GUARD_BEGIN
  if (!index || !out) { set_error("null argument"); return SG_E_INVALID; }
  if (int rc = mixed_check_index(index)) return rc;
  Coalescer* c = coalescer_of(index);
  { std::lock_guard<std::mutex> lock(c->mu); out[0] = c->pending.size(); }
  out[1] = c->n_batches.load(std::memory_order_relaxed); out[2] = c->n_mixed.load(std::memory_order_relaxed);
  out[3] = c->n_groups.load(std::memory_order_relaxed);
  return SG_OK;
  SG_GUARD_END(SG_RC)
}

int sg_debug_mixed_last(uint32_t* perm, uint32_t cap, uint32_t* group_start, uint32_t n_configs) {
  SG_GUARD_BEGIN
  const MixedThread& T = t_mixed;
  if (!perm || !group_start) { set_error("null argument"); return SG_E_INVALID; }
  if (!T.perm) { set_error("sg_debug_mixed_last: this thread has no mixed call to show"); return SG_E_INVALID; }
  if (T.group_start.size() != (size_t)n_configs + 1 || cap < T.n_q) { set_error("sg_debug_mixed_last: not the last call's sizes"); return SG_E_INVALID; }
  bool there = false;     // (the block may have gone to another stream's launch since)
  for (const auto& x : t_scratch) if (x.device == T.device && x.stream == T.stream && x.tag == SCRATCH_MIXED && x.blk.p && (const char*)T.perm >= (const char*)x.blk.p && (const char*)T.perm + (size_t)T.n_q * 4 <= (const char*)x.blk.p + x.blk.cap) there = true;
  if (!there) { set_error("sg_debug_mixed_last: the call's block has been reused"); return SG_E_INVALID; }
  DeviceGuard dg;
  HIP_TRY(dg.set(T.device));
  HIP_TRY(hipStreamSynchronize(T.stream));
  HIP_TRY(hipMemcpy(perm, T.perm, (size_t)T.n_q * 4, hipMemcpyDeviceToHost));
  std::copy(T.group_start.begin(), T.group_start.end(), group_start);
  return SG_OK;
  SG_GUARD_END(SG_RC)
}

int sg_debug_mixed_timing(int on) {
  g_mixed_timing.store(on != 0, std::memory_order_relaxed);
  return SG_OK;
}

int sg_debug_mixed_times(double out_ms[5]) {
  if (!out_ms) { set_error("null argument"); return SG_E_INVALID; }
  for (int i = 0; i < 5; i++) out_ms[i] = t_mixed.ms[i];
  return SG_OK;
}

}  // extern "C"
