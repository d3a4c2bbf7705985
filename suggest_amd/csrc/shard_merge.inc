// shard_merge.inc — a dictionary sharded by docID range behind one handle (sg_sharded, include/suggest_hip.h), included by
// engine.hip after the host files (it uses capi.inc's launch(), stream_scratch and GrowBlock, index_api.inc's build_any(), tune.inc's
// add_replica(), host_call.inc's run_host_call and IoCall, handles.inc's open_search, host_base.inc's
// DeviceGuard, HIP_TRY).  A sharded search is one enqueue step, sharded_enqueue: the device-resident call is that step on the
// caller's stream, a host-buffer call is host_call.inc's run_host_call around it, as every other host-buffer call is around its own.
// SURVEY.md §8(e) / DESIGN.md §5: every shard indexes the documents [doc_lo, doc_lo + n) under local docIDs, built with the
// dictionary-wide number of cardinality segments; a call searches the whole batch on every shard and sg_shard_merge_kernel
// merges the per-shard top-k rows on the device under the reference's total order (score desc, docID asc; collector.go:20-26).
// The rules of the merge restate suggest_amd/distributed.py::merge_topk; tests/shard_ref.py is the numpy statement the kernel
// is held against.
//
// The kernel ranks by search, with no sort: the lane that owns entry p of shard s's row counts the entries of every other row
// that go in front of it — an upper bound of its key in the rows of shards t < s, a lower bound in those of t > s, so that equal
// keys order by shard, then position — and stores its entry at p + the sum, if that is below k.  Every entry's rank is distinct,
// the ranks below min(k, total) are all taken, the slots from there on are zeroed by the lanes that own them: no two lanes
// store to one slot, nothing is read back.  Autocomplete rows carry no scores and shards own ascending docID ranges, so the
// rank is the position in the concatenation.

namespace sg {

constexpr uint32_t kShardSliceBytes = 256u << 20;    // the [shard][query][k] block of a slice of queries (as kGmSliceBytes)
constexpr uint32_t kMergeThreads = 256;
constexpr uint32_t kMergeItems = 4096;               // entries a workgroup walks when one query's W * k entries pass a workgroup
constexpr uint32_t kCountFlagMin = 0xFFFFFFF0u;      // out_counts values from here up are SG_COUNT_* flags

static thread_local double t_shard_merge_ms = 0;      // the launch of the calling thread's last sg_debug_shard_merge (sg_debug_shard_merge_time)
static std::atomic<uint32_t> g_shard_slice_bytes{0};   // sg_debug_shard_slice_bytes (0: kShardSliceBytes)
static inline uint32_t shard_slice_budget() {
  const uint32_t v = g_shard_slice_bytes.load(std::memory_order_relaxed);
  return v ? v : kShardSliceBytes;
}

struct ShardMergeArgs {
  const uint32_t* ids; const uint64_t* scores; const uint32_t* counts;   // [W][n_q][k] local docIDs, [W][n_q][k] score bits (null: autocomplete), [W][n_q]
  uint32_t* out_ids; uint64_t* out_scores; uint32_t* out_counts;         // [n_q][k], [n_q][k] (null: autocomplete), [n_q]
  uint32_t W, n_q, k;
  uint32_t per_block;     // queries a workgroup answers (W * k <= 128: 256 / (W * k), else 1)
  uint32_t chunks;        // per_block == 1: workgroups per query, kMergeItems entries each
  uint64_t doc_lo[SG_MAX_SHARDS];
};

__global__ __launch_bounds__(kMergeThreads) void sg_shard_merge_kernel(const ShardMergeArgs a) {
  __shared__ uint32_t s_c[kMergeThreads];        // [query of the block][shard] count, flags taken out, clamped to k
  __shared__ uint32_t s_f[kMergeThreads];        // [query of the block][shard] the flag, or 0
  __shared__ uint32_t s_tot[kMergeThreads];      // [query of the block] min(k, sum of the counts)
  __shared__ uint32_t s_flag[kMergeThreads];     // [query of the block] the largest flag, or 0
  __shared__ uint64_t s_lo[SG_MAX_SHARDS];
  const uint32_t tid = threadIdx.x, W = a.W, k = a.k, G = a.per_block;
  const uint32_t E = W * k;                      // (at most 64 * 65 536)
  uint64_t q0;
  uint32_t chunk = 0;
  if (G > 1) q0 = (uint64_t)blockIdx.x * G;
  else { q0 = blockIdx.x / a.chunks; chunk = blockIdx.x % a.chunks; }
  if (tid < W) s_lo[tid] = a.doc_lo[tid];
  for (uint32_t i = tid; i < G * W; i += kMergeThreads) {      // (G * W <= 256)
    const uint32_t g = i / W, s = i - g * W;
    uint32_t c = 0, f = 0;
    if (q0 + g < a.n_q) {
      const uint32_t raw = a.counts[(uint64_t)s * a.n_q + q0 + g];
      if (raw >= kCountFlagMin) f = raw; else c = min(raw, k);
    }
    s_c[i] = c; s_f[i] = f;
  }
  __syncthreads();
  if (tid < G) {
    uint32_t tot = 0, flag = 0;
    for (uint32_t s = 0; s < W; s++) { tot += s_c[tid * W + s]; flag = max(flag, s_f[tid * W + s]); }
    s_tot[tid] = min(tot, k); s_flag[tid] = flag;
  }
  __syncthreads();
  uint32_t g = 0, e_begin, e_end;
  if (G > 1) { g = tid / E; e_begin = tid - g * E; e_end = g < G ? e_begin + 1u : e_begin; }
  else { e_begin = chunk * kMergeItems + tid; e_end = min(E, (chunk + 1u) * kMergeItems); }
  const uint64_t q = q0 + g;
  if (g >= G || q >= a.n_q) return;
  const uint32_t tot = s_tot[g], flag = s_flag[g];
  const uint32_t* cs = s_c + g * W;
  const uint64_t out_row = q * k;
  for (uint32_t e = e_begin; e < e_end; e += kMergeThreads) {
    if (e < k) {                                               // slot e of the merged row
      if (e == 0) a.out_counts[q] = flag ? flag : tot;
      if (flag || e >= tot) { a.out_ids[out_row + e] = 0u; if (a.out_scores) a.out_scores[out_row + e] = 0ull; }
    }
    if (flag) continue;
    const uint32_t s = e / k, p = e - s * k;                   // entry p of shard s's row
    if (p >= cs[s]) continue;
    const uint64_t row = ((uint64_t)s * a.n_q + q) * k;
    const uint64_t gid = s_lo[s] + a.ids[row + p];             // dictionary docID (sg_sharded_adopt: below 2^32)
    uint32_t rank = p;
    uint64_t bits = 0;
    if (!a.scores) {
      for (uint32_t t = 0; t < s; t++) rank += cs[t];
    } else {
      bits = a.scores[row + p];
      const double sc = __longlong_as_double((long long)bits);
      for (uint32_t t = 0; t < W && rank < k; t++) {
        const uint32_t ct = cs[t];
        if (t == s || ct == 0u) continue;
        const uint64_t rt = ((uint64_t)t * a.n_q + q) * k;
        const uint64_t lo_t = s_lo[t];
        uint32_t lo = 0, hi = ct;                              // the entries of row t in front of this one: [0, lo)
        while (lo < hi) {
          const uint32_t mid = lo + ((hi - lo) >> 1);
          const double x = __longlong_as_double((long long)a.scores[rt + mid]);
          bool front;
          if (x != sc) front = x > sc;
          else {
            const uint64_t xg = lo_t + a.ids[rt + mid];
            front = t < s ? xg <= gid : xg < gid;
          }
          if (front) lo = mid + 1u; else hi = mid;
        }
        rank += lo;
      }
    }
    if (rank < k) {
      a.out_ids[out_row + rank] = (uint32_t)gid;
      if (a.out_scores) a.out_scores[out_row + rank] = bits;   // (bit for bit: no arithmetic touches a score)
    }
  }
}

// the launch: ids / scores / counts / out_* / W / n_q / k / doc_lo of `a` set by the caller
static int enqueue_shard_merge(ShardMergeArgs a, hipStream_t st) {
  if (a.n_q == 0) return SG_OK;
  const uint64_t E = (uint64_t)a.W * a.k;
  a.per_block = E <= kMergeThreads / 2 ? (uint32_t)(kMergeThreads / E) : 1u;
  a.chunks = (uint32_t)((E + kMergeItems - 1) / kMergeItems);
  const uint64_t blocks = a.per_block > 1 ? ((uint64_t)a.n_q + a.per_block - 1) / a.per_block : (uint64_t)a.n_q * a.chunks;
  if (blocks > 0x7FFFFFFFull) { set_error("shard merge: too many queries for one launch"); return SG_E_INVALID; }
  hipLaunchKernelGGL(sg_shard_merge_kernel, dim3((uint32_t)blocks), dim3(kMergeThreads), 0, st, a);
  HIP_TRY(hipGetLastError());
  return SG_OK;
}

// The [shard][query][k] block of a slice of m queries over W shards: scores first (8-byte entries), then ids, then counts — no
// padding between them, W * m * row_bytes in all.
struct ShardBlock {
  size_t ids = 0, cnt = 0, bytes = 0;
  ShardBlock(uint32_t W, uint32_t m, uint32_t k, bool scores) {
    ids = scores ? (size_t)W * m * k * 8 : 0;
    cnt = ids + (size_t)W * m * k * 4;
    bytes = cnt + (size_t)W * m * 4;
  }
};
static inline size_t shard_row_bytes(uint32_t k, bool scores) { return (size_t)k * (scores ? 12 : 4) + 4; }
// queries per slice: as many as keep the block of all W shards within the budget (one at least)
static inline uint32_t shard_slice_queries(uint32_t W, uint32_t k, bool scores, uint32_t n_q) {
  const size_t per_q = (size_t)W * shard_row_bytes(k, scores);
  return (uint32_t)std::min<size_t>(n_q, std::max<size_t>(1, shard_slice_budget() / per_q));
}

}  // namespace sg

// The shards of one entry of the device list (sg_sharded_build) or of one device (sg_sharded_adopt).  Lane 0 holds shard 0: its
// device merges, and its shards run on the call's own stream into the call's own block — it keeps nothing.  Every other lane
// has, for the host-buffer calls of a handle with several lanes, a stream of its own and its shards' rows on its device, and
// on a device other than the merge device the queries.
struct ShardLane {
  int device = -1;
  uint32_t q_owner = 0;              // the first lane on the same device: the queries are copied there once, into its block
  std::vector<uint32_t> shards;      // ascending
  hipStream_t stream = nullptr;
  hipEvent_t ev_q = nullptr, ev_rows = nullptr;
  GrowBlock q;                       // [offsets | queries] (the owner's, on a device other than the merge device)
  GrowBlock rows;                    // [this lane's shards][m][k], copied from here into the call's [W][m][k] block
};

struct sg_sharded {
  std::atomic<int> refs{1};
  std::mutex mu;                     // held while a host-buffer call enqueues on lanes 1 ..: their streams, blocks and events
  std::vector<sg_index*> shard;      // retained
  std::vector<uint64_t> doc_lo;
  std::vector<int> device;           // of each shard's primary replica
  std::vector<ShardLane> lanes;
  bool one_device = true;            // every shard on the merge device: the device-resident call can run
  hipEvent_t ev_st = nullptr;        // recorded on a call's stream for lanes 1 .. to wait for (sharded_enqueue)
  ~sg_sharded() {
    int prev = -1;
    (void)hipGetDevice(&prev);
    for (auto& l : lanes) {
      if (!l.stream && !l.q.p && !l.rows.p) continue;
      if (hipSetDevice(l.device) != hipSuccess) continue;
      if (l.stream) { (void)hipStreamSynchronize(l.stream); (void)hipStreamDestroy(l.stream); }
      if (l.ev_q) (void)hipEventDestroy(l.ev_q);
      if (l.ev_rows) (void)hipEventDestroy(l.ev_rows);
      l.q.release(); l.rows.release();
    }
    if (ev_st && hipSetDevice(lanes[0].device) == hipSuccess) (void)hipEventDestroy(ev_st);
    if (prev >= 0) (void)hipSetDevice(prev);
    (void)hipGetLastError();
    for (sg_index* ix : shard) sg_index_release(ix);
  }
};

namespace {

bool same_description(const HostIndex& a, const HostIndex& b) {
  return a.q == b.q && a.wrap0_s == b.wrap0_s && a.wrap1_s == b.wrap1_s && a.pad_s == b.pad_s && a.alphabet_spec == b.alphabet_spec;
}

// The handle over shards that passed the checks; lane_of[s] = the lane of shard s (lane 0 = shard 0's).  Retains every shard.
int sharded_make(sg_index* const* shards, const uint64_t* doc_lo, uint32_t n, const std::vector<uint32_t>& lane_of,
                 const std::vector<int>& lane_device, sg_sharded** out) {
  std::unique_ptr<sg_sharded> h(new sg_sharded());
  for (uint32_t s = 0; s < n; s++) {
    sg_index_retain(shards[s]);
    h->shard.push_back(shards[s]);
    h->doc_lo.push_back(doc_lo[s]);
    h->device.push_back(shards[s]->device);
    if (shards[s]->device != shards[0]->device) h->one_device = false;
  }
  h->lanes.resize(lane_device.size());
  for (size_t j = 0; j < h->lanes.size(); j++) {
    h->lanes[j].device = lane_device[j];
    h->lanes[j].q_owner = (uint32_t)j;
    for (size_t i = 0; i < j; i++) if (lane_device[i] == lane_device[j]) { h->lanes[j].q_owner = (uint32_t)i; break; }
  }
  for (uint32_t s = 0; s < n; s++) h->lanes[lane_of[s]].shards.push_back(s);
  *out = h.release();
  return SG_OK;
}

// doc_lo ascends, no range reaches into the next or past 2^32 (host data only: checked before anything about a device)
int sharded_check_ranges(sg_index* const* shards, const uint64_t* doc_lo, uint32_t n) {
  for (uint32_t s = 0; s < n; s++) {
    if (!shards[s]) { set_error("sg_sharded_adopt: null shard"); return SG_E_INVALID; }
    if (s && doc_lo[s] < doc_lo[s - 1]) { set_error("sg_sharded_adopt: doc_lo does not ascend"); return SG_E_INVALID; }
  }
  for (uint32_t s = 0; s < n; s++) {
    const uint64_t end = doc_lo[s] + shards[s]->host.n_docs;
    if (doc_lo[s] > (1ull << 32) || end > (1ull << 32)) { set_error("sg_sharded_adopt: a shard's docIDs pass 2^32"); return SG_E_INVALID; }
    if (s + 1 < n && end > doc_lo[s + 1]) { set_error("sg_sharded_adopt: the docID ranges of two shards overlap"); return SG_E_INVALID; }
  }
  return SG_OK;
}

int sharded_check_shards(sg_index* const* shards, uint32_t n) {
  for (uint32_t s = 0; s < n; s++) {
    if (!shards[s]->uploaded.load(std::memory_order_acquire)) { set_error("sg_sharded_adopt: a shard is not uploaded"); return SG_E_INVALID; }
    if (shards[s]->host.n_segments != shards[0]->host.n_segments) {
      set_error("sg_sharded_adopt: the shards differ in n_segments (build them with the dictionary-wide min_segments)"); return SG_E_INVALID;
    }
    if (!same_description(shards[s]->host, shards[0]->host)) { set_error("sg_sharded_adopt: the shards' descriptions differ"); return SG_E_INVALID; }
  }
  return SG_OK;
}

int sharded_lane_init(ShardLane& l) {     // (the lane's device is current)
  if (l.stream) return SG_OK;
  HIP_TRY(hipStreamCreateWithFlags(&l.stream, hipStreamNonBlocking));
  HIP_TRY(hipEventCreateWithFlags(&l.ev_q, hipEventDisableTiming));
  HIP_TRY(hipEventCreateWithFlags(&l.ev_rows, hipEventDisableTiming));
  return SG_OK;
}

// one shard's search of the queries offs[0 .. m] into rows [slot][m][k] of a block
int sharded_search(sg_index* ix, const void* d_q, const uint64_t* d_offs, uint32_t m, const LaunchReq& base, char* blk, const ShardBlock& B,
                   uint32_t slot, hipStream_t st) {
  LaunchReq r = base;
  const size_t at = (size_t)slot * m;
  r.q = d_q; r.offs = d_offs; r.n_q = m; r.stream = st;
  r.ids = blk + B.ids + at * r.k * 4;
  r.scores = r.autocomplete ? nullptr : blk + at * r.k * 8;
  r.counts = blk + B.cnt + at * 4;
  return launch(ix, find_replica(ix, -1), r);
}

ShardMergeArgs sharded_merge_args(uint32_t W, const uint64_t* doc_lo, const char* blk, const ShardBlock& B, uint32_t m, uint32_t k, bool scores) {
  ShardMergeArgs a{};
  a.ids = (const uint32_t*)(blk + B.ids); a.scores = scores ? (const uint64_t*)blk : nullptr; a.counts = (const uint32_t*)(blk + B.cnt);
  a.W = W; a.n_q = m; a.k = k;
  for (uint32_t s = 0; s < W; s++) a.doc_lo[s] = doc_lo[s];
  return a;
}

int sharded_open(sg_sharded* h, const SearchKey& c, std::initializer_list<const void*> required) {
  if (!h) { set_error("null handle"); return SG_E_INVALID; }
  return open_search(h->shard[0], c, !c.autocomplete, required);
}

// The enqueue step of a sharded search: n_q > 0 queries, their offsets and the three arrays of merged rows on shard 0's device,
// everything enqueued slice by slice, nothing waited for; the device that was current is current again on return (a host-buffer
// call: shard 0's).
// with_lanes == false: every shard is searched on `st` into the calling thread's SCRATCH_SHARD block of (device, st) and merged
// on `st` into the caller's rows at the slice's offset.  Nothing of the handle is written: no lock.
// with_lanes == true (a host-buffer call on a handle with several lanes; d_q lies q_bytes long right behind the offsets, as in
// a search's block, host_call.inc): lane 0's shards as above; every other lane searches its shards on its own stream into its own rows, copies them
// into the SCRATCH_SHARD block behind each search and records ev_rows, which `st` waits for before the merge.  A lane on
// another device gets one peer copy of [offsets | queries], on its own stream.  h->mu is held while this enqueues, no longer:
// the lanes' streams order the calls of several threads, and each thread merges from a block of its own.
int sharded_enqueue(sg_sharded* h, const char* d_q, const uint64_t* d_offs, uint32_t n_q, size_t q_bytes, const LaunchReq& base, uint32_t* d_ids,
                    uint64_t* d_scores, uint32_t* d_counts, hipStream_t st, bool with_lanes) {
  const int dev = h->device[0];
  const uint32_t W = (uint32_t)h->shard.size(), k = base.k;
  const bool sc = !base.autocomplete;
  const uint32_t slice = shard_slice_queries(W, k, sc, n_q);
  const size_t off_bytes = ((size_t)n_q + 1) * 8;
  DeviceGuard dg;
  HIP_TRY(dg.set(dev));
  void* blk = nullptr;
  if (int rc = stream_scratch(dev, st, ShardBlock(W, slice, k, sc).bytes, &blk, SCRATCH_SHARD)) return rc;
  char* dst = (char*)blk;
  std::unique_lock<std::mutex> lock(h->mu, std::defer_lock);
  struct Drain {       // a call that fails half way waits for what it enqueued on the lanes: their blocks are the next call's
    sg_sharded* h; bool armed;
    ~Drain() { if (armed) for (auto& l : h->lanes) if (l.stream) (void)hipStreamSynchronize(l.stream); }
  } drain{h, with_lanes};
  struct Hold {        // the lanes' launches ask for scratch of their own streams: they must not recycle the block they copy into
    int dev; hipStream_t st; bool on;
    ~Hold() { if (on) scratch_hold(dev, st, SCRATCH_SHARD, false); }
  } hold{dev, st, with_lanes};
  if (with_lanes) {
    scratch_hold(dev, st, SCRATCH_SHARD, true);
    lock.lock();
    if (!h->ev_st) HIP_TRY(hipEventCreateWithFlags(&h->ev_st, hipEventDisableTiming));
    for (size_t j = 1; j < h->lanes.size(); j++) {
      ShardLane& l = h->lanes[j];
      HIP_TRY(dg.set(l.device));
      if (int rc = sharded_lane_init(l)) return rc;
      if (int rc = l.rows.grow(ShardBlock((uint32_t)l.shards.size(), slice, k, sc).bytes)) return rc;
      // (the owner's block is the next call's: the lanes that read it have to be through with this one's queries)
      if (l.device != dev && l.q_owner != j) HIP_TRY(hipStreamWaitEvent(h->lanes[l.q_owner].stream, l.ev_rows, 0));
    }
  }
  for (uint32_t lo = 0; lo < n_q; lo += slice) {
    const uint32_t m = std::min(slice, n_q - lo);
    const ShardBlock B(W, m, k, sc);
    // Two orders the lanes' streams do not give by themselves: no lane touches the inputs before `st` has copied them in, and no
    // lane copies rows of this slice into the block before the merge of the last slice has read it.
    if (with_lanes) { HIP_TRY(dg.set(dev)); HIP_TRY(hipEventRecord(h->ev_st, st)); }
    for (size_t j = 0; j < h->lanes.size(); j++) {
      ShardLane& l = h->lanes[j];
      const bool own = with_lanes && j > 0;         // on the lane's stream, else on `st`
      HIP_TRY(dg.set(l.device));
      const char* lq = d_q;
      const uint64_t* loffs = d_offs;
      if (own) {
        HIP_TRY(hipStreamWaitEvent(l.stream, h->ev_st, 0));
        if (l.device != dev) {
          ShardLane& owner = h->lanes[l.q_owner];
          if (lo == 0 && l.q_owner == j) {
            if (int rc = l.q.grow(off_bytes + q_bytes)) return rc;
            HIP_TRY(hipMemcpyPeerAsync(l.q.p, l.device, d_offs, dev, off_bytes + q_bytes, l.stream));
            HIP_TRY(hipEventRecord(l.ev_q, l.stream));
          } else if (lo == 0) HIP_TRY(hipStreamWaitEvent(l.stream, owner.ev_q, 0));
          loffs = (const uint64_t*)owner.q.p;
          lq = (const char*)owner.q.p + off_bytes;
        }
      }
      const ShardBlock Bj((uint32_t)l.shards.size(), m, k, sc);
      for (size_t i = 0; i < l.shards.size(); i++) {
        const uint32_t s = l.shards[i];
        if (!own) { if (int rc = sharded_search(h->shard[s], lq, loffs + lo, m, base, dst, B, s, st)) return rc; continue; }
        char* src = (char*)l.rows.p;
        if (int rc = sharded_search(h->shard[s], lq, loffs + lo, m, base, src, Bj, (uint32_t)i, l.stream)) return rc;
        // this shard's rows to their place in the call's block, behind the search on this lane's stream
        const size_t from = i * (size_t)m, to = (size_t)s * m;
        auto copy = [&](size_t d_off, size_t s_off, size_t bytes) -> hipError_t {
          if (l.device == dev) return hipMemcpyAsync(dst + d_off, src + s_off, bytes, hipMemcpyDeviceToDevice, l.stream);
          return hipMemcpyPeerAsync(dst + d_off, dev, src + s_off, l.device, bytes, l.stream);
        };
        if (sc) HIP_TRY(copy(to * k * 8, from * k * 8, (size_t)m * k * 8));
        HIP_TRY(copy(B.ids + to * k * 4, Bj.ids + from * k * 4, (size_t)m * k * 4));
        HIP_TRY(copy(B.cnt + to * 4, Bj.cnt + from * 4, (size_t)m * 4));
      }
      if (own) HIP_TRY(hipEventRecord(l.ev_rows, l.stream));
    }
    HIP_TRY(dg.set(dev));
    if (with_lanes) for (size_t j = 1; j < h->lanes.size(); j++) HIP_TRY(hipStreamWaitEvent(st, h->lanes[j].ev_rows, 0));
    ShardMergeArgs a = sharded_merge_args(W, h->doc_lo.data(), dst, B, m, k, sc);
    a.out_ids = d_ids + (size_t)lo * k;
    a.out_scores = sc ? d_scores + (size_t)lo * k : nullptr;
    a.out_counts = d_counts + lo;
    if (int rc = enqueue_shard_merge(a, st)) return rc;
  }
  drain.armed = false;
  return SG_OK;
}

// Host buffers: a synchronous host-buffer call (run_host_call) on the merge device around the enqueue step.
int sharded_host_call(sg_sharded* h, const uint8_t* q, const uint64_t* offs, uint32_t n_q, const LaunchReq& base, uint32_t* ids, double* scores,
                      uint32_t* counts) {
  if (n_q == 0) return SG_OK;
  // (the rows are not cleared: the merge kernel writes every slot of every row, flags included)
  return run_host_call(h->device[0], search_io(q, offs, n_q, (uint64_t)n_q * base.k, ids, base.autocomplete ? nullptr : scores, counts, nullptr, false), [&](const IoCall& io, hipStream_t st) {
    LaunchReq r = base;
    r.no_long_queries = no_long_queries(offs, n_q);
    return sharded_enqueue(h, io.at<char>(IO_Q), io.at<uint64_t>(IO_OFFS), n_q, io.r[IO_Q].bytes, r, io.at<uint32_t>(IO_IDS),
                           io.r[IO_SCORES].bytes ? io.at<uint64_t>(IO_SCORES) : nullptr, io.at<uint32_t>(IO_COUNTS), st, h->lanes.size() > 1);
  });
}

}  // namespace

extern "C" {

int sg_sharded_adopt(sg_index* const* shards, const uint64_t* doc_lo, uint32_t n_shards, sg_sharded** out) {
  SG_GUARD_BEGIN
  if (!shards || !doc_lo || !out) { set_error("null argument"); return SG_E_INVALID; }
  if (n_shards == 0 || n_shards > SG_MAX_SHARDS) { set_error("sg_sharded_adopt: n_shards outside 1 .. SG_MAX_SHARDS"); return SG_E_INVALID; }
  if (int rc = sharded_check_ranges(shards, doc_lo, n_shards)) return rc;
  if (int rc = sharded_check_shards(shards, n_shards)) return rc;
  std::vector<uint32_t> lane_of(n_shards);
  std::vector<int> lane_device;                 // a lane per device, in order of first appearance
  for (uint32_t s = 0; s < n_shards; s++) {
    size_t j = 0;
    while (j < lane_device.size() && lane_device[j] != shards[s]->device) j++;
    if (j == lane_device.size()) lane_device.push_back(shards[s]->device);
    lane_of[s] = (uint32_t)j;
  }
  return sharded_make(shards, doc_lo, n_shards, lane_of, lane_device, out);
  SG_GUARD_END(SG_RC)
}

int sg_sharded_build(const uint8_t* utf8, const uint64_t* offs, uint32_t n_docs, const sg_desc* desc, uint32_t n_shards, const int* devices,
                     uint32_t n_devices, int build_device, sg_sharded** out) {
  SG_GUARD_BEGIN
  if (!out || !offs || !desc || !devices || (!utf8 && n_docs && offs[n_docs] != offs[0])) { set_error("null argument"); return SG_E_INVALID; }
  if (n_shards == 0 || n_shards > SG_MAX_SHARDS) { set_error("sg_sharded_build: n_shards outside 1 .. SG_MAX_SHARDS"); return SG_E_INVALID; }
  if (n_devices == 0 || n_devices > SG_MAX_SHARDS) { set_error("sg_sharded_build: n_devices outside 1 .. SG_MAX_SHARDS"); return SG_E_INVALID; }
  for (uint32_t i = 0; i < n_devices; i++) if (devices[i] < 0) { set_error("sg_sharded_build: bad device"); return SG_E_INVALID; }
  struct Built {      // the shards of this call: released on every way out (the handle holds references of its own)
    std::vector<sg_index*> ix;
    ~Built() { for (sg_index* p : ix) sg_index_release(p); }
  } built;
  std::vector<uint64_t> lo_of;
  std::vector<uint32_t> lane_of;
  std::vector<std::vector<uint64_t>> shard_offs;
  const uint32_t base = n_docs / n_shards, rem = n_docs % n_shards;         // distributed.shard_bounds
  auto build_one = [&](size_t i, uint32_t min_segments, sg_index** ix) {
    const std::vector<uint64_t>& so = shard_offs[i];
    const int dev = devices[lane_of[i]];
    return build_any(utf8 ? utf8 + offs[lo_of[i]] : nullptr, so.data(), (uint32_t)(so.size() - 1), desc, min_segments, build_device >= 0 ? dev : -1, ix);
  };
  uint32_t segments = 0;
  for (uint32_t s = 0; s < n_shards; s++) {
    const uint32_t lo = s * base + std::min(s, rem), n = base + (s < rem ? 1u : 0u);
    if (n == 0 && s) continue;                  // an empty shard has no rows to add and no window to flag (shard 0 always stands)
    std::vector<uint64_t> so((size_t)n + 1);
    for (uint32_t i = 0; i <= n; i++) so[i] = offs[lo + i] - offs[lo];
    shard_offs.push_back(std::move(so));
    lo_of.push_back(lo);
    lane_of.push_back(s % n_devices);
    sg_index* ix = nullptr;
    if (int rc = build_one(built.ix.size(), 0, &ix)) return rc;
    built.ix.push_back(ix);
    segments = std::max(segments, ix->host.n_segments);
  }
  for (size_t i = 0; i < built.ix.size(); i++) {       // the shards short of the dictionary-wide number are built again with it
    if (built.ix[i]->host.n_segments == segments) continue;
    sg_index* ix = nullptr;
    if (int rc = build_one(i, segments, &ix)) return rc;
    sg_index_release(built.ix[i]);
    built.ix[i] = ix;
  }
  for (size_t i = 0; i < built.ix.size(); i++)
    if (int rc = sg_index_upload(built.ix[i], devices[lane_of[i]])) return rc;
  const uint32_t n = (uint32_t)built.ix.size();
  if (int rc = sharded_check_ranges(built.ix.data(), lo_of.data(), n)) return rc;
  if (int rc = sharded_check_shards(built.ix.data(), n)) return rc;
  std::vector<int> lane_device(devices, devices + std::min(n_devices, n));
  return sharded_make(built.ix.data(), lo_of.data(), n, lane_of, lane_device, out);
  SG_GUARD_END(SG_RC)
}

void sg_sharded_retain(sg_sharded* h) { if (h) h->refs.fetch_add(1); }
void sg_sharded_release(sg_sharded* h) {
  if (!h) return;
  if (h->refs.fetch_sub(1) != 1) return;
  delete h;
}

uint32_t sg_sharded_shards(const sg_sharded* h, uint64_t* out_doc_lo, int* out_devices, uint32_t cap) {
  if (!h) return 0;
  for (size_t s = 0; s < h->shard.size() && s < cap; s++) {
    if (out_doc_lo) out_doc_lo[s] = h->doc_lo[s];
    if (out_devices) out_devices[s] = h->device[s];
  }
  return (uint32_t)h->shard.size();
}

int sg_sharded_suggest_batch(sg_sharded* h, const uint8_t* q, const uint64_t* offs, uint32_t n_q, int metric, double similarity, uint32_t k,
                             uint32_t* ids, double* scores, uint32_t* counts) {
  SG_GUARD_BEGIN
  const SearchKey c = fuzzy_key(metric, similarity, k);
  if (int rc = sharded_open(h, c, {offs, ids, scores, counts})) return rc;
  return sharded_host_call(h, q, offs, n_q, search_req(c), ids, scores, counts);
  SG_GUARD_END(SG_RC)
}

int sg_sharded_autocomplete_batch(sg_sharded* h, const uint8_t* q, const uint64_t* offs, uint32_t n_q, uint32_t limit, uint32_t* ids,
                                  uint32_t* counts) {
  SG_GUARD_BEGIN
  const SearchKey c = prefix_key(limit);
  if (int rc = sharded_open(h, c, {offs, ids, counts})) return rc;
  return sharded_host_call(h, q, offs, n_q, search_req(c), ids, nullptr, counts);
  SG_GUARD_END(SG_RC)
}

int sg_sharded_suggest_batch_device(sg_sharded* h, const void* d_q, const void* d_offs, uint32_t n_q, int metric, double similarity, uint32_t k,
                                    void* d_ids, void* d_scores, void* d_counts, void* stream) {
  SG_GUARD_BEGIN
  const SearchKey c = fuzzy_key(metric, similarity, k);
  if (int rc = sharded_open(h, c, {})) return rc;                // (an empty batch needs no arrays: they are looked at below)
  if (n_q == 0) return SG_OK;
  if (!d_offs || !d_ids || !d_counts || !d_scores) { set_error("null argument"); return SG_E_INVALID; }
  hipPointerAttribute_t at;
  const bool there = h->one_device && hipPointerGetAttributes(&at, d_offs) == hipSuccess && at.type == hipMemoryTypeDevice && at.device == h->device[0];
  if (!there) {
    (void)hipGetLastError();
    set_error("sg_sharded_*_device: every shard has to be resident on the device that owns the buffers");
    return SG_E_UNSUPPORTED;
  }
  return sharded_enqueue(h, (const char*)d_q, (const uint64_t*)d_offs, n_q, 0, search_req(c), (uint32_t*)d_ids,
                         (uint64_t*)d_scores, (uint32_t*)d_counts, (hipStream_t)stream, false);
  SG_GUARD_END(SG_RC)
}

// Test hooks.  sg_debug_shard_slice_bytes, process-wide: the budget of the [shard][query][k] block, 0 = kShardSliceBytes.
int sg_debug_shard_slice_bytes(uint32_t bytes) {
  g_shard_slice_bytes.store(bytes, std::memory_order_relaxed);
  return SG_OK;
}

// sg_shard_merge_kernel alone, one launch over host arrays laid out as the block: ids / scores [n_shards][n_q][k], counts
// [n_shards][n_q]; autocomplete != 0: no scores (scores and out_scores may be null).
int sg_debug_shard_merge(int device, const uint32_t* ids, const double* scores, const uint32_t* counts, const uint64_t* doc_lo, uint32_t n_shards,
                         uint32_t n_q, uint32_t k, int autocomplete, uint32_t* out_ids, double* out_scores, uint32_t* out_counts) {
  SG_GUARD_BEGIN
  const bool sc = !autocomplete;
  if (!ids || !counts || !doc_lo || !out_ids || !out_counts || (sc && (!scores || !out_scores))) { set_error("null argument"); return SG_E_INVALID; }
  if (n_shards == 0 || n_shards > SG_MAX_SHARDS || k == 0 || k > SG_MAX_TOPK || device < 0) { set_error("sg_debug_shard_merge: bad argument"); return SG_E_INVALID; }
  if (n_q == 0) return SG_OK;
  const ShardBlock B(n_shards, n_q, k, sc);
  // the merged rows as a search lays them: [scores | ids | counts]
  Carve c;
  const size_t slots = (size_t)n_q * k, sc_bytes = sc ? slots * 8 : 0, o_sc = c.take(sc_bytes), o_ids = c.take(slots * 4, 4), o_cnt = c.take((size_t)n_q * 4, 4);
  DeviceGuard dg;
  HIP_TRY(dg.set(device));
  DeviceBlock mem;
  char *di = nullptr, *d_o = nullptr;
  int rc;
  if ((rc = mem.alloc(&di, block_capacity(B.bytes))) || (rc = mem.alloc(&d_o, block_capacity(c.off)))) return rc;   // (a search's GrowBlock sizes)
  if (sc) HIP_TRY(hipMemcpy(di, scores, B.ids, hipMemcpyHostToDevice));
  HIP_TRY(hipMemcpy(di + B.ids, ids, B.cnt - B.ids, hipMemcpyHostToDevice));
  HIP_TRY(hipMemcpy(di + B.cnt, counts, B.bytes - B.cnt, hipMemcpyHostToDevice));
  HIP_TRY(hipMemset(d_o, 0xA5, c.off));          // (the kernel writes every slot of every row)
  ShardMergeArgs a = sharded_merge_args(n_shards, doc_lo, di, B, n_q, k, sc);
  a.out_ids = (uint32_t*)(d_o + o_ids); a.out_scores = sc ? (uint64_t*)(d_o + o_sc) : nullptr; a.out_counts = (uint32_t*)(d_o + o_cnt);
  hipEvent_t ev[2] = {nullptr, nullptr};
  struct Events { hipEvent_t* e; ~Events() { for (int i = 0; i < 2; i++) if (e[i]) (void)hipEventDestroy(e[i]); } } events_{ev};
  HIP_TRY(hipEventCreate(&ev[0])); HIP_TRY(hipEventCreate(&ev[1]));
  HIP_TRY(hipEventRecord(ev[0], nullptr));
  if (int rc = enqueue_shard_merge(a, nullptr)) return rc;
  HIP_TRY(hipEventRecord(ev[1], nullptr));
  HIP_TRY(hipEventSynchronize(ev[1]));
  float ms = 0;
  HIP_TRY(hipEventElapsedTime(&ms, ev[0], ev[1]));
  t_shard_merge_ms = ms;
  if (sc) HIP_TRY(hipMemcpy(out_scores, d_o + o_sc, sc_bytes, hipMemcpyDeviceToHost));
  HIP_TRY(hipMemcpy(out_ids, d_o + o_ids, slots * 4, hipMemcpyDeviceToHost));
  HIP_TRY(hipMemcpy(out_counts, d_o + o_cnt, (size_t)n_q * 4, hipMemcpyDeviceToHost));
  return SG_OK;
  SG_GUARD_END(SG_RC)
}

// milliseconds between two events around the launch of the calling thread's last sg_debug_shard_merge (tools/shard_timing.py)
int sg_debug_shard_merge_time(double* out_ms) {
  if (!out_ms) { set_error("null argument"); return SG_E_INVALID; }
  *out_ms = t_shard_merge_ms;
  return SG_OK;
}

}  // extern "C"
