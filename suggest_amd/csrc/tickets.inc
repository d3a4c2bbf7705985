// tickets.inc — the asynchronous host-buffer calls: a replica's AsyncPool (three streams, a ring of slots), sg_ticket,
// async_submit, sg_host_alloc / sg_host_free, the three submit calls and sg_ticket_wait.  Uses host_call.inc and search_api.inc.

// ------------------------------------------------------------------------------------------
// Asynchronous host-buffer calls: sg_suggest_submit / sg_autocomplete_submit -> ticket, sg_ticket_wait.
// The synchronous entry points spend a third of a batch's time in staging copies on the calling thread while the GPU
// idles (headline: 25.9 M q/s against 38.6 M device-resident).  A Go host (north_star: "host code stays in Go") calls
// through host buffers, so it needs the copies of batch i + 1 to run beside the kernel of batch i:
//   * three streams per replica — copy-in, run, copy-out — tied by events, so that every search launch of the replica is
//     serialised on ONE stream (two search launches side by side undo the L2 sharing the query order sets up: DESIGN.md §5)
//     while the H2D of the next ticket and the D2H of the previous one overlap it;
//   * a ring of slots (device block + pinned staging + events) per replica; a ticket holds one until it is waited for;
//   * buffers the caller got from sg_host_alloc are pinned: they are read / written where they lie and nothing is staged;
//     other buffers are staged through the slot's pinned memory (one memcpy at submit, one at wait).
// Submit is begin_host_call on the slot, wait is finish_host_call: the routines of the synchronous calls.
// Tickets are plain heap objects: submit and wait may run on different OS threads (goroutines migrate).
// ------------------------------------------------------------------------------------------
#define SG_ASYNC_SLOTS 8
struct AsyncSlot {
  GrowBlock dev, pin_in{true}, pin_out{true};
  hipEvent_t ev_in = nullptr, ev_run = nullptr, ev_out = nullptr;
  bool busy = false;
};
struct AsyncPool {
  int device = -1;
  hipStream_t s_in = nullptr, s_run = nullptr, s_out = nullptr;
  AsyncSlot slot[SG_ASYNC_SLOTS];
  ~AsyncPool() {
    if (device < 0 || hipSetDevice(device) != hipSuccess) return;
    for (hipStream_t st : {s_in, s_run, s_out}) if (st) { (void)hipStreamSynchronize(st); (void)hipStreamDestroy(st); }
    for (auto& x : slot) {
      x.dev.release(); x.pin_in.release(); x.pin_out.release();
      for (hipEvent_t e : {x.ev_in, x.ev_run, x.ev_out}) if (e) (void)hipEventDestroy(e);
    }
  }
};
Replica::~Replica() {
  delete async_pool;
  mem.clear();
  if (h_fill) (void)hipHostFree(h_fill);
}

struct sg_ticket {
  sg_index* index = nullptr;
  Replica* rep = nullptr;
  int slot = -1;
  HostCall call;
};

static int async_submit(sg_index* index, const uint8_t* q, const uint64_t* offs, uint32_t n_q, const SearchKey& key, uint32_t* ids, double* scores,
                        uint32_t* counts, sg_ticket** out, uint32_t replica = 0) {
  if (!out) { set_error("null argument"); return SG_E_INVALID; }
  *out = nullptr;
  Replica* rep = nullptr;
  {
    std::lock_guard<std::mutex> lock(index->mu);
    if (replica < index->replicas.size()) rep = index->replicas[replica].get();
  }
  if (!rep) { set_error("no such replica"); return SG_E_INVALID; }
  std::unique_ptr<sg_ticket> t(new sg_ticket());
  t->index = index; t->rep = rep;
  if (n_q == 0) { sg_index_retain(index); *out = t.release(); return SG_OK; }
  DeviceGuard dg;
  HIP_TRY(dg.set(rep->device));
  // ---- a slot of the replica's ring ----
  AsyncPool* pool;
  AsyncSlot* sl = nullptr;
  {
    std::lock_guard<std::mutex> lock(rep->async_mu);
    if (!rep->async_pool) {
      std::unique_ptr<AsyncPool> np(new AsyncPool());
      np->device = rep->device;
      // The copy streams get the highest priority the device has: streams share a handful of hardware queues, and a copy
      // that lands on the run stream's queue waits behind (or holds up) a 1.7 ms search launch — measured before this:
      // 2.2 ms per headline batch with two or three tickets in flight, i.e. kernel + copies end to end.  Priorities map
      // to queues of their own.
      int prio_lo = 0, prio_hi = 0;
      (void)hipDeviceGetStreamPriorityRange(&prio_lo, &prio_hi);
      HIP_TRY(hipStreamCreateWithPriority(&np->s_in, hipStreamNonBlocking, prio_hi));
      HIP_TRY(hipStreamCreateWithPriority(&np->s_run, hipStreamNonBlocking, prio_lo));
      HIP_TRY(hipStreamCreateWithPriority(&np->s_out, hipStreamNonBlocking, prio_hi));
      rep->async_pool = np.release();
    }
    pool = rep->async_pool;
    for (int i = 0; i < SG_ASYNC_SLOTS && !sl; i++) if (!pool->slot[i].busy) { sl = &pool->slot[i]; t->slot = i; }
    if (!sl) { set_error("too many tickets in flight on this replica: wait for one first (SG_ASYNC_SLOTS = 8)"); return SG_E_INVALID; }
    sl->busy = true;
  }
  // (a submit that fails hands the slot back; begin_host_call has waited for whatever it enqueued)
  struct Unbusy {
    Replica* r; AsyncSlot* s; bool keep = false;
    ~Unbusy() { if (!keep) { std::lock_guard<std::mutex> lock(r->async_mu); s->busy = false; } }
  } unbusy{rep, sl};
  if (!sl->ev_in) {
    HIP_TRY(hipEventCreateWithFlags(&sl->ev_in, hipEventDisableTiming));
    HIP_TRY(hipEventCreateWithFlags(&sl->ev_run, hipEventDisableTiming));
    HIP_TRY(hipEventCreateWithFlags(&sl->ev_out, hipEventDisableTiming));
  }
  // copy in on s_in, every search launch of the replica's tickets on ONE stream (s_run), copy out on s_out
  IoCtx x;
  x.in = pool->s_in; x.run = pool->s_run; x.out = pool->s_out;
  x.ev_in = sl->ev_in; x.ev_run = sl->ev_run; x.ev_out = sl->ev_out;
  x.dev = &sl->dev; x.pin_in = &sl->pin_in; x.pin_out = &sl->pin_out;
  x.ticket = true;
  const LaunchReq r = search_req(key);
  if (int rc = begin_host_call(search_io(q, offs, n_q, (uint64_t)n_q * r.k, ids, r.autocomplete ? nullptr : scores, counts, nullptr, true), search_enqueue(index, rep, r, offs, n_q), x, &t->call)) return rc;
  unbusy.keep = true;
  sg_index_retain(index);
  *out = t.release();
  return SG_OK;
}

extern "C" {

// Pinned host memory for the buffers of sg_*_submit (queries, offsets, result rows): the DMA engine reads and writes it
// directly, nothing is staged.  Any thread may free it.
int sg_host_alloc(uint64_t bytes, void** out) {
  SG_GUARD_BEGIN
  if (!out) { set_error("null argument"); return SG_E_INVALID; }
  *out = nullptr;
  const size_t n = std::max<size_t>((size_t)bytes, 16);
  HIP_TRY(hipHostMalloc(out, n, hipHostMallocDefault));
  { std::lock_guard<std::mutex> lock(g_pinned_mu); g_pinned[(uintptr_t)*out] = n; }
  return SG_OK;
  SG_GUARD_END(SG_RC)
}
void sg_host_free(void* p) {
  if (!p) return;
  { std::lock_guard<std::mutex> lock(g_pinned_mu); g_pinned.erase((uintptr_t)p); }
  (void)hipHostFree(p);
}

// On replica number `replica` of the index (0 = the primary; sg_index_replicas lists them): ONE host thread keeps every GPU of
// the node busy by submitting a slice of its batch to each replica and waiting for the tickets.
int sg_suggest_submit_on(sg_index* index, uint32_t replica, const uint8_t* q, const uint64_t* offs, uint32_t n_q, int metric, double similarity,
                         uint32_t k, uint32_t* ids, double* scores, uint32_t* counts, sg_ticket** out) {
  SG_GUARD_BEGIN
  const SearchKey c = fuzzy_key(metric, similarity, k);
  if (int rc = open_search(index, c, true, {offs, ids, scores, counts})) return rc;
  return async_submit(index, q, offs, n_q, c, ids, scores, counts, out, replica);
  SG_GUARD_END(SG_RC)
}

int sg_suggest_submit(sg_index* index, const uint8_t* q, const uint64_t* offs, uint32_t n_q, int metric, double similarity, uint32_t k,
                      uint32_t* ids, double* scores, uint32_t* counts, sg_ticket** out) {
  return sg_suggest_submit_on(index, 0, q, offs, n_q, metric, similarity, k, ids, scores, counts, out);
}

int sg_autocomplete_submit(sg_index* index, const uint8_t* q, const uint64_t* offs, uint32_t n_q, uint32_t first_doc, uint32_t limit,
                           uint32_t* ids, uint32_t* counts, sg_ticket** out) {
  SG_GUARD_BEGIN
  const SearchKey c = prefix_key(limit, first_doc);
  if (int rc = open_search(index, c, false, {offs, ids, counts})) return rc;
  return async_submit(index, q, offs, n_q, c, ids, nullptr, counts, out);
  SG_GUARD_END(SG_RC)
}

// Blocks until the ticket's rows are in the caller's buffers, then frees the ticket (also on failure).  Any thread.
int sg_ticket_wait(sg_ticket* t) {
  SG_GUARD_BEGIN
  if (!t) { set_error("null ticket"); return SG_E_INVALID; }
  std::unique_ptr<sg_ticket> own(t);
  const Held<sg_index> release(t->index);                      // (the reference the submit took)
  if (t->slot < 0) return SG_OK;                               // an empty batch
  AsyncSlot* sl = &t->rep->async_pool->slot[t->slot];
  struct Unbusy { Replica* r; AsyncSlot* s; ~Unbusy() { std::lock_guard<std::mutex> lock(r->async_mu); s->busy = false; } } unbusy{t->rep, sl};
  return finish_host_call(t->call);
  SG_GUARD_END(SG_RC)
}
}  // extern "C"
