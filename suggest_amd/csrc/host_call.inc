// host_call.inc — one host-buffer call, whatever its kind: HostPool, the calling thread's HostCtx, the call's list of regions
// (IoRegion / IoCall, with the table of what every kind moves), the registry of pinned caller memory, and begin_host_call /
// finish_host_call / run_host_call, which loop over the list.  Uses host_base.inc and capi.inc (GrowBlock, Carve, the poison).

// A few worker threads for host steps that are worth spreading (Predict's word tokeniser and word ids, the copy of a big
// batch's rows out of the staging buffer): made on first use, kept — a call used to spawn and join up to 32 threads.  run() cuts [0, n) into one range per worker (at least `grain` items
// each), takes the first range itself and returns when all are done; concurrent callers take turns.
struct HostPool {
  std::mutex call_mu, mu;
  std::condition_variable cv_work, cv_done;
  std::vector<std::thread> workers;
  const std::function<void(uint32_t, uint32_t)>* body = nullptr;
  uint32_t n = 0, parts = 0, next = 0, pending = 0;
  uint64_t generation = 0;
  bool stop = false;
  HostPool() {
    const uint32_t n_thr = (uint32_t)env_int("SG_HOST_THREADS", 1, 64, (int32_t)std::min(std::max(std::thread::hardware_concurrency(), 2u), 16u));
    for (uint32_t t = 1; t < n_thr; t++) workers.emplace_back([this] { loop(); });
  }
  ~HostPool() {
    { std::lock_guard<std::mutex> lock(mu); stop = true; }
    cv_work.notify_all();
    for (auto& t : workers) t.join();
  }
  bool take(uint32_t* lo, uint32_t* hi) {                       // (under mu)
    if (next >= parts) return false;
    const uint32_t p = next++;
    *lo = (uint32_t)((uint64_t)n * p / parts); *hi = (uint32_t)((uint64_t)n * (p + 1) / parts);
    return true;
  }
  void loop() {
    uint64_t seen = 0;
    std::unique_lock<std::mutex> lock(mu);
    for (;;) {
      cv_work.wait(lock, [&] { return stop || (generation != seen && next < parts); });
      if (stop) return;
      seen = generation;
      uint32_t lo, hi;
      while (take(&lo, &hi)) {
        lock.unlock();
        (*body)(lo, hi);
        lock.lock();
        if (--pending == 0) cv_done.notify_all();
      }
    }
  }
  void run(uint32_t count, uint32_t grain, const std::function<void(uint32_t, uint32_t)>& f) {
    const uint32_t want = std::max(1u, std::min((uint32_t)workers.size() + 1u, count / std::max(grain, 1u)));
    if (want <= 1) { f(0, count); return; }
    std::lock_guard<std::mutex> turn(call_mu);
    std::unique_lock<std::mutex> lock(mu);
    body = &f; n = count; parts = want; next = 0; pending = want; generation++;
    cv_work.notify_all();
    uint32_t lo, hi;
    while (take(&lo, &hi)) {
      lock.unlock();
      f(lo, hi);
      lock.lock();
      --pending;
    }
    cv_done.wait(lock, [&] { return pending == 0; });
    body = nullptr;
  }
};
static HostPool& host_pool() { static HostPool pool; return pool; }

// Per-thread, per-device context of the synchronous host-buffer entry points (sg_*_batch, the coalescer, the workers of
// sg_*_batch_multi, sg_spell_predict_batch): a stream, a pinned staging buffer and a device block that are made once and
// reused (a request-per-call service pays ~60 us per call instead of ~450 us of hipMalloc / hipFree / stream creation).
// Contexts live as long as their thread.
struct HostCtx {
  int device = -1;
  hipStream_t stream = nullptr;
  GrowBlock pinned{true};          // staging of a call's inputs and results (kPinnedMax at most)
  GrowBlock dblock;                // the device side of a call: inputs + result rows
};
// The calling thread's contexts, one per device (a std::deque: push_back never moves a context, and a call keeps a pointer to
// its own from begin to finish).  A thread that ends (cgo / pthread pools, the coalescer's dispatchers, the multi workers)
// hands its streams, staging and device blocks back; the main thread's are left to process exit, when the HIP runtime may
// already be going down.
struct ThreadContexts {
  std::deque<HostCtx> ctx;
  void release();
  ~ThreadContexts() { if (!ctx.empty() && !on_main_thread()) release(); }
};
static thread_local ThreadContexts t_ctx_owner;
#define t_ctx (t_ctx_owner.ctx)
static const size_t kPinnedMax = (size_t)64 << 20;   // bigger synchronous calls copy straight from / to the caller's (pageable) buffers

static int host_ctx(int device, HostCtx** out) {
  for (auto& x : t_ctx) if (x.device == device) { *out = &x; return SG_OK; }
  hipStream_t st = nullptr;
  HIP_TRY(hipStreamCreateWithFlags(&st, hipStreamNonBlocking));
  t_ctx.push_back(HostCtx{});
  t_ctx.back().device = device;
  t_ctx.back().stream = st;
  *out = &t_ctx.back();
  return SG_OK;
}

// A thread that is about to end (the coalescer's dispatchers) hands its contexts and launch buffers back.
void ThreadContexts::release() {
  for (auto& c : ctx) {
    if (hipSetDevice(c.device) != hipSuccess) continue;
    if (c.stream) (void)hipStreamSynchronize(c.stream);
    c.dblock.release();
    c.pinned.release();
    if (c.stream) (void)hipStreamDestroy(c.stream);
  }
  ctx.clear();
}
static void thread_contexts_release() {
  t_ctx_owner.release();
  t_scratch_owner.release();
}

// ---- what a host-buffer call moves: a short list of regions, declared by the call.  A region is one array of the caller's and
// its place in the call's device block.  lay() orders the block [out | both ways | in], each class in the order of declaration, so
// that ONE range is copied back — [0, out_hi) — and ONE range is copied in — [in_lo, in_hi) — and a region that goes both ways lies
// where the two overlap; 16 bytes follow the last region.  The kinds (u32 unless marked; `?` = empty unless asked for):
//   kind                         out                                              both ways              in
//   search: fuzzy, prefix,       scores[slots] f64 · ids[slots] · counts[n_q] · aux[slots]   —           offs[n_q + 1] u64 · q
//   tables, _from, sharded; and: strings + text_offs[slots + 1] u64 · info[2] u64; mixed (slots = the sum of k) + sel[n_q] in;
//                                Predict: no scores, id rows of topK + 1; sg_suggest_batch_edit: aux = the distances, + info[2] u64
//   LM text (lm_api.inc)         scores[n] f64 · words[n]? · unknown[n]?          —                      offs[n + 1] u64 · text
//   LM word ids                  scores[n] f64                                    —                      offs[n + 1] u64 (in ids) · ids
//   dictionary rows              text_offs[slots + 1] u64 · info[2] u64           —                      row_offs[n_rows + 1]? u64 · ids · counts
//   edit rows / re-rank          dist[slots] · info[2] u64                        re-rank (else in):     q_offs u64 · q · row_offs? u64
//   (edit_rank.inc)                                                               scores? f64 · ids · counts
// Alignment in the block: 4 for u32 arrays, 8 for u64 / f64 arrays and a blob, 16 for the first region and for offsets.  It decides
// which copy-out route a ticket takes (16-byte pieces: host_store_kernel), so a kind's declaration is its layout. ----
enum IoDir : uint8_t { IO_IN = 1, IO_OUT = 2, IO_BOTH = 3 };
// host: the caller's array (null: the region lives in the block alone); off: its place (lay()); clear: an out region zeroed before the
// step; poison: the PoisonRegion it is filled and counted under while sg_debug_poison is on (-1: left alone); unit (0: no offsets):
// offsets select a window of the blob declared behind them and — rebase — go in minus their first, times `unit` bytes
struct IoRegion {
  void* host = nullptr; size_t bytes = 0, off = 0; uint32_t align = 16; IoDir dir = IO_IN; bool clear = false; int8_t poison = -1;
  uint32_t unit = 0; bool rebase = false;
};
struct IoCall {
  std::array<IoRegion, 10> r;    // (a declaration past it: std::out_of_range, an SG_E_* at the entry point)
  uint32_t n = 0;
  size_t out_hi = 0, in_lo = 0, in_hi = 0, total = 0;
  char* dev = nullptr;           // the block, from begin_host_call on
  bool stage_slices = false;     // a synchronous call rebases in the staging of ALL its inputs: a slice above kPinnedMax is refused
  IoCall& add(IoDir dir, const void* host, size_t bytes, uint32_t align, bool clear = false, int poison = -1) {
    r.at(n++) = IoRegion{const_cast<void*>(host), bytes, 0, align, dir, clear, (int8_t)poison};
    return *this;
  }
  // n_items + 1 offsets, counted in units of `unit` bytes, and the window of `base` they select: two in regions, the blob the next
  // index behind the offsets
  IoCall& add_window(const uint64_t* offs, uint32_t n_items, const void* base, uint32_t unit = 1, bool stage = true) {
    add(IO_IN, offs, ((size_t)n_items + 1) * 8, 16);
    r[n - 1].unit = unit; r[n - 1].rebase = unit != 1 || offs[0] != 0; stage_slices = stage;
    return add(IO_IN, base ? (const char*)base + offs[0] * unit : nullptr, (size_t)(offs[n_items] - offs[0]) * unit, 8);
  }
  template <class T> T* at(int i) const { return (T*)(dev + r[i].off); }
  void lay() {
    Carve c;
    in_lo = SIZE_MAX;
    for (IoDir pass : {IO_OUT, IO_BOTH, IO_IN})
      for (uint32_t i = 0; i < n; i++) if (r[i].dir == pass) {
        r[i].off = c.take(r[i].bytes, r[i].align);
        if (pass != IO_OUT) in_lo = std::min(in_lo, r[i].off);
        if (pass != IO_IN) out_hi = c.off;
      }
    in_hi = c.off; total = c.off + 16; in_lo = std::min(in_lo, in_hi);
  }
};

// The regions every search-shaped call declares, under these indices: result rows of `slots` slots in all, n_q counts, n_q queries;
// then a mixed call's config numbers, or a strings call's slots + 1 text offsets and the 16 bytes of its step's info (block only).
// clear: the rows are zeroed (sg_debug_poison: poisoned, the counts too) — a step that writes every slot itself passes false.
enum { IO_SCORES = 0, IO_IDS, IO_COUNTS, IO_AUX, IO_OFFS, IO_Q, IO_SEL, IO_TEXT_OFFS = IO_SEL, IO_INFO };
static IoCall search_io(const uint8_t* q, const uint64_t* offs, uint32_t n_q, uint64_t slots, uint32_t* ids, double* scores, uint32_t* counts,
                        uint32_t* aux, bool clear, uint64_t* text_offs = nullptr, const uint32_t* sel = nullptr) {
  if (text_offs && sel) throw std::logic_error("search_io: text offsets and config numbers share an index");
  IoCall io;
  io.add(IO_OUT, scores, scores ? (size_t)slots * 8 : 0, 16, clear, clear ? PZ_OUT_SCORES : -1);
  io.add(IO_OUT, ids, (size_t)slots * 4, 4, clear, clear ? PZ_OUT_IDS : -1);
  io.add(IO_OUT, counts, (size_t)n_q * 4, 4, false, clear ? PZ_OUT_COUNTS : -1);
  io.add(IO_OUT, aux, aux ? (size_t)slots * 4 : 0, 4, clear, clear ? PZ_OUT_IDS : -1);
  io.add_window(offs, n_q, q);
  if (text_offs) { io.add(IO_OUT, text_offs, ((size_t)slots + 1) * 8, 8); io.add(IO_OUT, nullptr, 16, 8); }
  if (sel) io.add(IO_IN, sel, (size_t)n_q * 4, 4);
  return io;
}

// Blocks handed out by sg_host_alloc: pinned by construction, looked up without a HIP call (hipPointerGetAttributes costs
// tens of microseconds per pointer, six pointers per submit).
static std::mutex g_pinned_mu;
static std::map<uintptr_t, size_t> g_pinned;       // start -> bytes
// Is [p, p + bytes) memory the device can read and write where it lies?  Only blocks handed out by sg_host_alloc qualify, and only
// when the WHOLE range lies inside one: the row store kernel dereferences the host pointer itself, so a range that runs past
// the block — or memory the caller pinned some other way (hipHostRegister: not necessarily mapped, its device alias may differ)
// — takes the staged path instead.
static bool is_pinned_host(const void* p, size_t bytes) {
  if (!p) return false;
  std::lock_guard<std::mutex> lock(g_pinned_mu);
  auto it = g_pinned.upper_bound((uintptr_t)p);
  if (it == g_pinned.begin()) return false;
  --it;
  return (uintptr_t)p >= it->first && (uintptr_t)p + bytes <= it->first + it->second;
}

// ---- one host-buffer call: begin_host_call stages the in regions, copies them in, enqueues the kind's work and the copy back,
// all asynchronous; finish_host_call waits and hands the out regions to the caller's arrays ----

// What a call runs on.  A synchronous call: the calling thread's HostCtx — one stream for everything, no events, one staging
// buffer both ways, staging up to kPinnedMax.  A ticket: its AsyncSlot — the copy-in, run and copy-out streams of the replica's
// pool tied by the slot's events, a staging buffer each way of any size, and caller memory from sg_host_alloc read and written
// where it lies.
struct IoCtx {
  hipStream_t in = nullptr, run = nullptr, out = nullptr;
  hipEvent_t ev_in = nullptr, ev_run = nullptr, ev_out = nullptr;
  GrowBlock *dev = nullptr, *pin_in = nullptr, *pin_out = nullptr;
  bool ticket = false;
};
// A call in flight, what finish_host_call needs: staged = the block's [0, out_hi) in pinned staging (null: the results went to the
// caller's arrays); finish waits for `done` if there is one, else for `out`
struct HostCall { IoCall io; const char* staged = nullptr; hipStream_t out = nullptr; hipEvent_t done = nullptr; };
// The kind's enqueue step (launch() for search, autocomplete and tables, predict_on_device for Predict, ...): the block's in
// regions -> its out regions, on stream `st`; io.at<T>(i) is region i on the device, i the index the call declared it under
using Enqueue = std::function<int(const IoCall& io, hipStream_t st)>;

static void host_copy(void* dst, const void* src, size_t n) {   // (8 MB of rows for 65 536 queries: one thread takes 0.5 ms)
  if (n < ((size_t)1 << 20)) { if (n) memcpy(dst, src, n); return; }
  const size_t piece = (size_t)256 << 10;
  host_pool().run((uint32_t)((n + piece - 1) / piece), 2, [&](uint32_t lo, uint32_t hi) {
    const size_t b = (size_t)lo * piece, e = std::min(n, (size_t)hi * piece);
    memcpy((char*)dst + b, (const char*)src + b, e - b);
  });
}

static int begin_host_call(const IoCall& call, const Enqueue& enqueue, const IoCtx& x, HostCall* c) {
  IoCall& io = c->io;
  io = call;
  bool in_pinned = true, out_pinned = true;       // (pinned: a ticket's caller memory, from sg_host_alloc)
  size_t rebase_bytes = 0;
  for (uint32_t i = 0; i < io.n; i++) {
    const IoRegion& R = io.r[i];
    if (R.unit && !io.r[i + 1].host && io.r[i + 1].bytes) { set_error("null query buffer"); return SG_E_INVALID; }
    if (R.rebase) rebase_bytes += R.bytes;
    if (!x.ticket || !R.bytes || !R.host || is_pinned_host(R.host, R.bytes)) continue;
    if (R.dir & IO_IN) in_pinned = false;
    if (R.dir & IO_OUT) out_pinned = false;
  }
  io.lay();
  const size_t in_bytes = io.in_hi - io.in_lo;
  // the routes.  A ticket: caller memory from sg_host_alloc where it lies, the rest staged.  A synchronous call: staged both ways
  // while it fits kPinnedMax, else straight from / to the caller's memory — but offsets that do not start at zero (a slice of a
  // larger batch) are rebased in the staging buffer: with the call's other inputs (stage_slices), else alone.
  const bool out_staged = x.ticket ? !out_pinned : std::max(in_bytes, io.out_hi) <= kPinnedMax;
  const bool in_staged = x.ticket ? rebase_bytes || !in_pinned : out_staged || (rebase_bytes && io.stage_slices);
  if (!x.ticket && in_staged && in_bytes > kPinnedMax) { set_error("batch slice too large to stage"); return SG_E_INVALID; }
  const size_t pin_in = in_staged ? in_bytes : rebase_bytes, pin_out = out_staged ? io.out_hi : 0;
  if (int rc = x.pin_in->grow(x.pin_in == x.pin_out ? std::max(pin_in, pin_out) : pin_in)) return rc;
  if (int rc = x.pin_out->grow(pin_out)) return rc;
  if (io.total > x.dev->cap && x.dev->p) HIP_TRY(hipStreamSynchronize(x.run));   // (hipFree would wait for the device anyway)
  if (int rc = x.dev->grow(io.total)) return rc;
  char* dev = io.dev = (char*)x.dev->p;
  // (a call that fails half way waits for what it enqueued: its buffers are reused by the next call)
  struct Drain {
    const IoCtx& x; bool armed = true;
    ~Drain() { if (armed) for (hipStream_t st : {x.in, x.run, x.out}) (void)hipStreamSynchronize(st); }
  } drain{x};
  // ---- copy in: one copy from staging, or a copy per region straight from the caller's memory ----
  char* pin = (char*)x.pin_in->p;
  for (const IoRegion& R : io.r) {
    if (!(R.dir & IO_IN) || !R.bytes) continue;
    char* to = in_staged ? pin + (R.off - io.in_lo) : pin;          // (unstaged: only rebased offsets pass through staging)
    const uint64_t* offs = (const uint64_t*)R.host;
    if (R.rebase) for (size_t j = 0; j < R.bytes / 8; j++) ((uint64_t*)to)[j] = (offs[j] - offs[0]) * R.unit;
    else if (in_staged) memcpy(to, R.host, R.bytes);
    if (in_staged) continue;
    HIP_TRY(hipMemcpyAsync(dev + R.off, R.rebase ? to : R.host, R.bytes, hipMemcpyHostToDevice, x.in));
    if (R.rebase) pin += R.bytes;
  }
  if (in_staged) HIP_TRY(hipMemcpyAsync(dev + io.in_lo, pin, in_bytes, hipMemcpyHostToDevice, x.in));
  // (rows of queries with fewer than k results stay zero; a ticket clears them on its copy-in stream, beside the previous
  //  ticket's search launch — on the run stream the 8 MB fill was 0.09 ms between two search launches.  Cleared regions that
  //  touch take one fill.)
  for (uint32_t i = 0; i < io.n; i++) {
    const IoRegion& R = io.r[i];
    if (poison_mode() ? R.poison < 0 : !R.clear || !R.bytes) continue;
    if (poison_mode()) { if (int rc = poison_fill(dev + R.off, R.bytes, (PoisonRegion)R.poison, x.in)) return rc; continue; }
    size_t end = R.off + R.bytes;
    while (i + 1 < io.n && io.r[i + 1].clear && io.r[i + 1].off == end) end += io.r[++i].bytes;
    HIP_TRY(hipMemsetAsync(dev + R.off, 0, end - R.off, x.in));
  }
  if (x.ev_in) { HIP_TRY(hipEventRecord(x.ev_in, x.in)); HIP_TRY(hipStreamWaitEvent(x.run, x.ev_in, 0)); }
  if (int rc = enqueue(io, x.run)) return rc;
  if (x.ev_run) { HIP_TRY(hipEventRecord(x.ev_run, x.run)); HIP_TRY(hipStreamWaitEvent(x.out, x.ev_run, 0)); }
  // ---- copy out: one copy to staging, or into the caller's arrays ----
  // (sg_host_alloc memory: a kernel's stores, not hipMemcpyAsync — see host_store_kernel; at most three regions of 16-byte pieces
  //  — the device block's regions are, the caller's pinned arrays usually are; anything else takes the runtime's copies)
  HostStoreArgs h{};
  uint32_t n_out = 0;
  bool store = x.ticket && out_pinned;
  for (uint32_t pass = 0; pass < 2 && !out_staged; pass++)          // first: may the store kernel take them all?  then: the copies, if not
    for (const IoRegion& R : io.r) {
      if (!(R.dir & IO_OUT) || !R.bytes || !R.host || (pass && store)) continue;
      if (pass) { HIP_TRY(hipMemcpyAsync(R.host, dev + R.off, R.bytes, hipMemcpyDeviceToHost, x.out)); continue; }
      if (n_out == 3 || ((uintptr_t)R.host | R.bytes | (uintptr_t)(dev + R.off)) % 16) { store = false; break; }
      h.src[n_out] = (const uint4*)(dev + R.off); h.dst[n_out] = (uint4*)R.host; h.n16[n_out++] = R.bytes / 16;
    }
  if (out_staged) HIP_TRY(hipMemcpyAsync(x.pin_out->p, dev, io.out_hi, hipMemcpyDeviceToHost, x.out));
  else if (store) { hipLaunchKernelGGL(host_store_kernel, dim3(128), dim3(256), 0, x.out, h); HIP_TRY(hipGetLastError()); }
  if (x.ev_out) HIP_TRY(hipEventRecord(x.ev_out, x.out));
  drain.armed = false;
  c->staged = out_staged ? (const char*)x.pin_out->p : nullptr; c->out = x.out; c->done = x.ev_out;
  return SG_OK;
}

static int finish_host_call(const HostCall& c) {
  if (c.done) HIP_TRY(hipEventSynchronize(c.done));
  else HIP_TRY(hipStreamSynchronize(c.out));
  for (const IoRegion& R : c.io.r) if (c.staged && (R.dir & IO_OUT) && R.host) host_copy(R.host, c.staged + R.off, R.bytes);
  return SG_OK;
}

// A synchronous host-buffer call: begin and finish on the calling thread's context for `device`, whose current device is the
// same afterwards.
static int run_host_call(int device, const IoCall& io, const Enqueue& enqueue) {
  DeviceGuard dg;
  HIP_TRY(dg.set(device));
  HostCtx* ctx;
  if (int rc = host_ctx(device, &ctx)) return rc;
  IoCtx x;
  x.in = x.run = x.out = ctx->stream;
  x.dev = &ctx->dblock; x.pin_in = x.pin_out = &ctx->pinned;
  HostCall c;
  if (int rc = begin_host_call(io, enqueue, x, &c)) return rc;
  return finish_host_call(c);
}
