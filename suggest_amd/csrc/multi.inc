// multi.inc — the _multi calls: a worker thread per replica (MultiPool), run_multi, sg_suggest_batch_multi and
// sg_autocomplete_batch_multi.  Uses search_api.inc (run_host).

extern "C" {
// The batch cut into contiguous slices, one per replica (SURVEY.md §8e: queries are independent, the index is read-only —
// no data-path collective); rows land in caller order.  Every replica has a worker thread of its own (made on the first
// multi call, kept until the index goes): staging memcpy, H2D, launch, D2H and the copy out of the staging buffer of the
// slices all run side by side — issued from the one calling thread, 8 GPUs x 21 M q/s of host-buffer traffic is ~35 GB/s
// of memcpy on one core, and a slice was not begun before the previous one had been staged.  A worker owns its thread's
// context (stream, pinned staging, device block) like any other caller of the host-buffer entry points; concurrent multi
// calls queue on the workers in FIFO order.
struct MultiTask {
  std::function<int()> fn;
  int rc = SG_OK;
  std::string err;
  bool done = false;
};
struct MultiWorker {
  std::thread th;
  std::mutex mu;
  std::condition_variable cv, cv_done;
  std::deque<MultiTask*> queue;
  bool stop = false;
};
struct MultiPool {
  std::vector<std::unique_ptr<MultiWorker>> workers;      // [i] serves replica i
};

static void multi_worker_loop(MultiWorker* w) {
  struct AtExit { ~AtExit() { thread_contexts_release(); } } at_exit;
  std::unique_lock<std::mutex> lock(w->mu);
  for (;;) {
    w->cv.wait(lock, [&] { return w->stop || !w->queue.empty(); });
    if (w->queue.empty()) return;                          // stop, and nothing left to serve
    MultiTask* t = w->queue.front();
    w->queue.pop_front();
    lock.unlock();
    int rc;
    std::string err;
    try { rc = t->fn(); if (rc) err = g_err; }
    catch (const std::bad_alloc&) { rc = SG_E_NOMEM; err = "out of host memory"; }
    catch (const std::exception& e) { rc = SG_E_INVALID; err = std::string("internal error: ") + e.what(); }
    lock.lock();
    t->rc = rc; t->err = std::move(err); t->done = true;   // (t is the caller's: gone once it sees done)
    w->cv_done.notify_all();
  }
}

static MultiPool* multi_pool_of(sg_index* ix, size_t n_replicas) {
  std::lock_guard<std::mutex> lock(ix->mu);
  if (!ix->multi) ix->multi = new MultiPool();
  while (ix->multi->workers.size() < n_replicas) {           // (replicas are append-only: workers follow them)
    std::unique_ptr<MultiWorker> w(new MultiWorker());
    w->th = std::thread(multi_worker_loop, w.get());
    ix->multi->workers.push_back(std::move(w));
  }
  return ix->multi;
}

static void multi_pool_stop(MultiPool* p) {
  for (auto& w : p->workers) {
    { std::lock_guard<std::mutex> lock(w->mu); w->stop = true; }
    w->cv.notify_all();
    w->th.join();
  }
  delete p;
}

static int run_multi(sg_index* index, const uint8_t* q, const uint64_t* offs, uint32_t n_q, const SearchKey& key, uint32_t* ids, double* scores,
                     uint32_t* counts) {
  std::vector<Replica*> reps;
  { std::lock_guard<std::mutex> lock(index->mu); for (auto& r : index->replicas) reps.push_back(r.get()); }
  const uint32_t R = (uint32_t)reps.size();
  if (R <= 1 || n_q < 2 * R) return run_host(index, reps[0], q, offs, n_q, search_req(key), ids, scores, counts);
  MultiPool* pool = multi_pool_of(index, R);
  std::vector<MultiTask> tasks(R);
  for (uint32_t r = 0; r < R; r++) {
    const uint32_t lo = (uint32_t)((uint64_t)n_q * r / R), hi = (uint32_t)((uint64_t)n_q * (r + 1) / R);
    Replica* rep = reps[r];
    tasks[r].fn = [=]() {
      return run_host(index, rep, q, offs + lo, hi - lo, search_req(key), ids + (size_t)lo * key.k, scores ? scores + (size_t)lo * key.k : nullptr,
                      counts + lo);
    };
    MultiWorker* w = pool->workers[r].get();
    { std::lock_guard<std::mutex> lock(w->mu); w->queue.push_back(&tasks[r]); }
    w->cv.notify_one();
  }
  int rc = SG_OK;
  for (uint32_t r = 0; r < R; r++) {                          // every slice is awaited, also after a failure: the tasks live here
    MultiWorker* w = pool->workers[r].get();
    std::unique_lock<std::mutex> lock(w->mu);
    w->cv_done.wait(lock, [&] { return tasks[r].done; });
    if (tasks[r].rc && !rc) { rc = tasks[r].rc; set_error(tasks[r].err); }
  }
  return rc;
}

int sg_suggest_batch_multi(sg_index* index, const uint8_t* q, const uint64_t* offs, uint32_t n_q, int metric, double similarity,
                           uint32_t k, uint32_t* ids, double* scores, uint32_t* counts) {
  SG_GUARD_BEGIN
  const SearchKey c = fuzzy_key(metric, similarity, k);
  if (int rc = open_search(index, c, true, {offs, ids, scores, counts})) return rc;
  return run_multi(index, q, offs, n_q, c, ids, scores, counts);
  SG_GUARD_END(SG_RC)
}

int sg_autocomplete_batch_multi(sg_index* index, const uint8_t* q, const uint64_t* offs, uint32_t n_q, uint32_t limit,
                                uint32_t* ids, uint32_t* counts) {
  SG_GUARD_BEGIN
  const SearchKey c = prefix_key(limit);
  if (int rc = open_search(index, c, false, {offs, ids, counts})) return rc;
  return run_multi(index, q, offs, n_q, c, ids, nullptr, counts);
  SG_GUARD_END(SG_RC)
}

}  // extern "C"
