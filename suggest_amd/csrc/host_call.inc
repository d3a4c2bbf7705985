// host_call.inc — one host-buffer call, whatever its kind: HostPool, the calling thread's HostCtx, IoLayout, the registry of
// pinned caller memory, and begin_host_call / finish_host_call / run_host_call.  Uses host_base.inc and capi.inc (GrowBlock,
// the poison).

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

// The device block of a host-buffer call: [scores | ids | counts | aux] — the results, one copy back — then, from the next 16
// bytes on, [offsets | queries] — the inputs, one copy in.  Offsets and sizes in bytes.  Predict: id rows of topK + 1, counts.
// A mixed call (mixed_batch.inc): ragged rows — `rows` slots in all in place of n_q * k — and, behind the queries, its [n_q] list
// of config numbers (sel); a fixed-k call has neither and lies exactly as it did.  A strings call (dict_rows.inc): behind the
// result rows, still inside the one copy back, the slots + 1 text offsets (toffs); the text itself is not part of this block.
struct IoLayout {
  size_t sc_bytes = 0, id_bytes = 0, cnt_bytes = 0, aux_bytes = 0, toffs_bytes = 0, off_bytes = 0, q_bytes = 0, sel_bytes = 0;
  size_t ids = 0, cnt = 0, aux = 0, toffs = 0, out_bytes = 0, offs = 0, q = 0, sel = 0, in_bytes = 0, total = 0;   // (the scores start the block)
};
constexpr uint64_t kRowsFixed = ~0ull;      // HostBufs::rows of a fixed-k call: n_q * row
static IoLayout io_layout(uint32_t n_q, uint32_t k, bool scores, bool aux, size_t q_bytes, uint64_t rows = kRowsFixed, bool sel = false,
                          bool text = false) {
  IoLayout L;
  const size_t slots = rows == kRowsFixed ? (size_t)n_q * k : (size_t)rows;
  L.sc_bytes = scores ? slots * 8 : 0; L.id_bytes = slots * 4; L.cnt_bytes = (size_t)n_q * 4;
  L.aux_bytes = aux ? slots * 4 : 0; L.off_bytes = (size_t)(n_q + 1) * 8; L.q_bytes = q_bytes;
  Carve c;
  c.take(L.sc_bytes);
  L.ids = c.take(L.id_bytes, 4); L.cnt = c.take(L.cnt_bytes, 4); L.aux = c.take(L.aux_bytes, 4);
  if (text) { L.toffs_bytes = (slots + 1) * 8; L.toffs = c.take(L.toffs_bytes + 16, 8); }   // (+ the step's two info words)
  L.out_bytes = c.off;
  L.offs = c.take(L.off_bytes); L.q = c.take(q_bytes, 8);
  if (sel) { L.sel_bytes = (size_t)n_q * 4; L.sel = c.take(L.sel_bytes, 4); }
  L.in_bytes = c.off - L.offs; L.total = c.off + 16;
  return L;
}

// sg_debug_poison: a host-buffer call's result rows — scores, ids, counts, aux — in place of the zeroed rows
static int poison_results(char* dev, const IoLayout& io, hipStream_t st) {
  int rc;
  if ((rc = poison_fill(dev, io.sc_bytes, PZ_OUT_SCORES, st))) return rc;
  if ((rc = poison_fill(dev + io.ids, io.id_bytes, PZ_OUT_IDS, st))) return rc;
  if ((rc = poison_fill(dev + io.cnt, io.cnt_bytes, PZ_OUT_COUNTS, st))) return rc;
  return poison_fill(dev + io.aux, io.aux_bytes, PZ_OUT_IDS, st);
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

// ---- one host-buffer call: begin_host_call stages the inputs, copies them in, enqueues the kind's work and the copy back,
// all asynchronous; finish_host_call waits and hands the rows to the caller's arrays ----

// The caller's side: n_q queries (blob + n_q + 1 offsets, which may start anywhere) and the result arrays — [n_q][row] ids,
// [n_q][row] scores (null: none), [n_q] counts, [n_q][row] aux (null: none).
struct HostBufs {
  const uint8_t* q = nullptr; const uint64_t* offs = nullptr; uint32_t n_q = 0, row = 0;
  uint32_t* ids = nullptr; double* scores = nullptr; uint32_t* counts = nullptr; uint32_t* aux = nullptr;
  uint64_t rows = kRowsFixed;          // a mixed call: the slots of its ragged ids / scores rows in all (`row` unused)
  const uint32_t* sel = nullptr;       // ... and its [n_q] config numbers, staged and copied in with the queries
  uint64_t* text_offs = nullptr;       // a strings call: the slots + 1 text offsets its enqueue step leaves at IoLayout::toffs
};
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
// A call in flight: what finish_host_call needs
struct HostCall {
  HostBufs b;
  IoLayout io;
  const char* staged = nullptr;      // the results in pinned staging (null: they went to the caller's arrays)
  hipStream_t out = nullptr;
  hipEvent_t done = nullptr;         // finish waits for this event if there is one, else for `out`
};
// The kind's enqueue step (launch() for search, autocomplete and tables, predict_on_device for Predict): the device block's
// inputs -> its result rows, on stream `st`
using Enqueue = std::function<int(char* dev, const IoLayout& io, hipStream_t st)>;

// b.n_q > 0.  clear_rows: the result rows are zeroed (sg_debug_poison: poisoned) before the enqueue step.
static int begin_host_call(const HostBufs& b, bool clear_rows, const Enqueue& enqueue, const IoCtx& x, HostCall* c) {
  const uint64_t q0 = b.offs[0];
  if (!b.q && b.offs[b.n_q] != q0) { set_error("null query buffer"); return SG_E_INVALID; }
  const IoLayout io = io_layout(b.n_q, b.row, b.scores != nullptr, b.aux != nullptr, (size_t)(b.offs[b.n_q] - q0), b.rows, b.sel != nullptr,
                                 b.text_offs != nullptr);
  // the routes.  A ticket: caller memory from sg_host_alloc where it lies, the rest staged.  A synchronous call: staged both ways
  // while it fits kPinnedMax, else straight from / to the caller's memory — but offsets that do not start at zero (a slice of a
  // larger batch) are rebased in the staging buffer.
  bool in_staged, out_staged, out_pinned = false;
  if (x.ticket) {
    in_staged = q0 != 0 || !is_pinned_host(b.offs, io.off_bytes) || (io.q_bytes && !is_pinned_host(b.q, io.q_bytes));
    out_pinned = is_pinned_host(b.ids, io.id_bytes) && is_pinned_host(b.counts, io.cnt_bytes) && (!b.scores || is_pinned_host(b.scores, io.sc_bytes));
    out_staged = !out_pinned;
  } else {
    out_staged = std::max(io.in_bytes, io.out_bytes) <= kPinnedMax;
    in_staged = out_staged || q0 != 0;
    if (in_staged && io.in_bytes > kPinnedMax) { set_error("batch slice too large to stage"); return SG_E_INVALID; }
  }
  const size_t pin_in = in_staged ? io.in_bytes : 0, pin_out = out_staged ? io.out_bytes : 0;
  if (int rc = x.pin_in->grow(x.pin_in == x.pin_out ? std::max(pin_in, pin_out) : pin_in)) return rc;
  if (int rc = x.pin_out->grow(pin_out)) return rc;
  if (io.total > x.dev->cap && x.dev->p) HIP_TRY(hipStreamSynchronize(x.run));   // (hipFree would wait for the device anyway)
  if (int rc = x.dev->grow(io.total)) return rc;
  char* dev = (char*)x.dev->p;
  // (a call that fails half way waits for what it enqueued: its buffers are reused by the next call)
  struct Drain {
    const IoCtx& x; bool armed = true;
    ~Drain() { if (armed) for (hipStream_t st : {x.in, x.run, x.out}) (void)hipStreamSynchronize(st); }
  } drain{x};
  // ---- copy in: one copy from staging, the offsets rebased to zero, or two straight from the caller's memory ----
  if (in_staged) {
    char* pin = (char*)x.pin_in->p;
    uint64_t* po = (uint64_t*)pin;
    if (q0) for (uint32_t i = 0; i <= b.n_q; i++) po[i] = b.offs[i] - q0; else memcpy(po, b.offs, io.off_bytes);
    if (io.q_bytes) memcpy(pin + io.off_bytes, b.q + q0, io.q_bytes);
    if (io.sel_bytes) memcpy(pin + (io.sel - io.offs), b.sel, io.sel_bytes);
    HIP_TRY(hipMemcpyAsync(dev + io.offs, pin, io.in_bytes, hipMemcpyHostToDevice, x.in));
  } else {
    HIP_TRY(hipMemcpyAsync(dev + io.offs, b.offs, io.off_bytes, hipMemcpyHostToDevice, x.in));
    if (io.q_bytes) HIP_TRY(hipMemcpyAsync(dev + io.q, b.q, io.q_bytes, hipMemcpyHostToDevice, x.in));
    if (io.sel_bytes) HIP_TRY(hipMemcpyAsync(dev + io.sel, b.sel, io.sel_bytes, hipMemcpyHostToDevice, x.in));
  }
  // (rows of queries with fewer than k results stay zero; a ticket clears them on its copy-in stream, beside the previous
  //  ticket's search launch — on the run stream the 8 MB fill was 0.09 ms between two search launches)
  if (clear_rows) {
    if (poison_mode()) { if (int rc = poison_results(dev, io, x.in)) return rc; }
    else {
      HIP_TRY(hipMemsetAsync(dev, 0, io.sc_bytes + io.id_bytes, x.in));
      if (io.aux_bytes) HIP_TRY(hipMemsetAsync(dev + io.aux, 0, io.aux_bytes, x.in));
    }
  }
  if (x.ev_in) { HIP_TRY(hipEventRecord(x.ev_in, x.in)); HIP_TRY(hipStreamWaitEvent(x.run, x.ev_in, 0)); }
  if (int rc = enqueue(dev, io, x.run)) return rc;
  if (x.ev_run) { HIP_TRY(hipEventRecord(x.ev_run, x.run)); HIP_TRY(hipStreamWaitEvent(x.out, x.ev_run, 0)); }
  // ---- copy out: one copy to staging, or into the caller's arrays ----
  const bool al16 = ((uintptr_t)b.scores | (uintptr_t)b.ids | (uintptr_t)b.counts | io.sc_bytes | io.id_bytes | io.cnt_bytes |
                     (uintptr_t)(dev + io.ids) | (uintptr_t)(dev + io.cnt)) % 16 == 0;
  if (out_staged) {
    HIP_TRY(hipMemcpyAsync(x.pin_out->p, dev, io.out_bytes, hipMemcpyDeviceToHost, x.out));
  } else if (out_pinned && al16 && !b.aux && !b.text_offs) {
    // (sg_host_alloc memory: a kernel's stores, not hipMemcpyAsync — see host_store_kernel; 16-byte pieces — the device block's
    //  regions are, the caller's pinned arrays usually are; anything else takes the runtime's copies)
    HostStoreArgs h{};
    h.src[0] = (const uint4*)dev; h.dst[0] = (uint4*)b.scores; h.n16[0] = io.sc_bytes / 16;
    h.src[1] = (const uint4*)(dev + io.ids); h.dst[1] = (uint4*)b.ids; h.n16[1] = io.id_bytes / 16;
    h.src[2] = (const uint4*)(dev + io.cnt); h.dst[2] = (uint4*)b.counts; h.n16[2] = io.cnt_bytes / 16;
    hipLaunchKernelGGL(host_store_kernel, dim3(128), dim3(256), 0, x.out, h);
    HIP_TRY(hipGetLastError());
  } else {
    if (io.sc_bytes) HIP_TRY(hipMemcpyAsync(b.scores, dev, io.sc_bytes, hipMemcpyDeviceToHost, x.out));
    HIP_TRY(hipMemcpyAsync(b.ids, dev + io.ids, io.id_bytes, hipMemcpyDeviceToHost, x.out));
    HIP_TRY(hipMemcpyAsync(b.counts, dev + io.cnt, io.cnt_bytes, hipMemcpyDeviceToHost, x.out));
    if (io.aux_bytes) HIP_TRY(hipMemcpyAsync(b.aux, dev + io.aux, io.aux_bytes, hipMemcpyDeviceToHost, x.out));
    if (io.toffs_bytes) HIP_TRY(hipMemcpyAsync(b.text_offs, dev + io.toffs, io.toffs_bytes, hipMemcpyDeviceToHost, x.out));
  }
  if (x.ev_out) HIP_TRY(hipEventRecord(x.ev_out, x.out));
  drain.armed = false;
  *c = HostCall{b, io, out_staged ? (const char*)x.pin_out->p : nullptr, x.out, x.ev_out};
  return SG_OK;
}

static int finish_host_call(const HostCall& c) {
  if (c.done) HIP_TRY(hipEventSynchronize(c.done));
  else HIP_TRY(hipStreamSynchronize(c.out));
  if (!c.staged) return SG_OK;
  auto copy_out = [](void* dst, const char* src, size_t n) {     // (8 MB of rows for 65 536 queries: one thread takes 0.5 ms)
    if (n < ((size_t)1 << 20)) { memcpy(dst, src, n); return; }
    const size_t piece = (size_t)256 << 10;
    host_pool().run((uint32_t)((n + piece - 1) / piece), 2, [&](uint32_t lo, uint32_t hi) {
      const size_t b = (size_t)lo * piece, e = std::min(n, (size_t)hi * piece);
      memcpy((char*)dst + b, src + b, e - b);
    });
  };
  const IoLayout& io = c.io;
  if (io.sc_bytes) copy_out(c.b.scores, c.staged, io.sc_bytes);
  copy_out(c.b.ids, c.staged + io.ids, io.id_bytes);
  memcpy(c.b.counts, c.staged + io.cnt, io.cnt_bytes);
  if (io.aux_bytes) copy_out(c.b.aux, c.staged + io.aux, io.aux_bytes);
  if (io.toffs_bytes) copy_out(c.b.text_offs, c.staged + io.toffs, io.toffs_bytes);
  return SG_OK;
}

// A synchronous host-buffer call: begin and finish on the calling thread's context for `device`, whose current device is the
// same afterwards.
static int run_host_call(int device, const HostBufs& b, bool clear_rows, const Enqueue& enqueue) {
  if (b.n_q == 0) return SG_OK;
  DeviceGuard dg;
  HIP_TRY(dg.set(device));
  HostCtx* ctx;
  if (int rc = host_ctx(device, &ctx)) return rc;
  IoCtx x;
  x.in = x.run = x.out = ctx->stream;
  x.dev = &ctx->dblock; x.pin_in = x.pin_out = &ctx->pinned;
  HostCall c;
  if (int rc = begin_host_call(b, clear_rows, enqueue, x, &c)) return rc;
  return finish_host_call(c);
}
