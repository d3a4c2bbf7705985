// coalescer.inc — the single-query calls, coalesced: OneReq, the Coalescer and its dispatcher lanes, answer_take, submit_one,
// sg_suggest_one and sg_autocomplete_one(_from).  Uses handles.inc (SearchKey), search_api.inc (run_host) and, for a take with
// several keys, mixed_batch.inc's mixed_host_call (declared here).

// ------------------------------------------------------------------------------------------
// Single-query callers, coalesced.  The reference's Suggest is called per query from many goroutines
// (pkg/suggest/suggester.go:46, service_test.go:36-79); a launch per query would cost ~40 us each.  sg_suggest_one /
// sg_autocomplete_one queue the request; dispatcher threads (SG_COALESCE_LANES per replica, default 1) take whatever is
// pending with the same search parameters and run it as ONE batch — no timer: an idle engine launches a lone request at
// once, a busy one finds the requests that arrived meanwhile.  Callers spin briefly on their request, then sleep.
// ------------------------------------------------------------------------------------------
struct OneWaiter {
  std::mutex mu; std::condition_variable cv;
  bool released = false;            // a sleeping caller leaves when its parent in the batch's wake-up tree (or the dispatcher) says so
  OneWaiter* child[2] = {nullptr, nullptr};   // ... and wakes these two first: the dispatcher pays ONE futex wake per batch
};
static void release_waiter(OneWaiter* w) {
  { std::lock_guard<std::mutex> lk(w->mu); w->released = true; }
  w->cv.notify_one();
}
struct OneReq {
  SearchKey key;                    // requests with equal keys share a launch
  const uint8_t* q; uint32_t len;
  uint32_t* ids; double* scores; uint32_t* count;
  int rc = SG_OK;
  std::string err;
  std::atomic<int> state{0};      // 0 pending, 1 done, 2 the caller sleeps on `waiter`
  OneWaiter* waiter = nullptr;
};
struct Coalescer {
  sg_index* index = nullptr;
  std::mutex mu;
  std::condition_variable cv;
  std::deque<OneReq*> pending;
  bool stop = false;
  std::vector<std::thread> lanes;
  uint32_t max_batch = 8192;
  std::atomic<uint32_t> batch_ns{100000};   // recent time from taking a batch to answering it (moving average): how long callers spin
  bool mixed = false;               // sg_coalesce_mixed: a take with several keys is ONE mixed call (mixed_batch.inc); under mu
  bool hold = false;                // sg_debug_coalesce_hold: the dispatchers take nothing (a stop overrides it); under mu
  std::atomic<uint64_t> n_batches{0}, n_mixed{0}, n_groups{0};   // sg_debug_coalesce_stats: takes, mixed ones, launches (a plain take is one)
};

// the mixed call over host buffers (mixed_batch.inc; the arguments of sg_suggest_batch_mixed, checked, on `rep`)
static int mixed_host_call(sg_index* index, Replica* rep, const uint8_t* q, const uint64_t* offs, uint32_t n_q, const sg_search_config* configs,
                           uint32_t n_configs, const uint32_t* config_of, uint64_t rows_cap, uint32_t* ids, double* scores, uint32_t* counts,
                           uint64_t* row_offs);

// The end of every take, plain or mixed: each caller gets its row (row i starts at row_offs[i]; at i * k where row_offs is null, a
// plain take, whose requests share one k), then the sleeping callers are woken.  ONE statement of the wake-up: OneWaiter::child is
// the caller thread's and outlives the request, so every take rewrites it for every sleeper.
static void answer_take(Coalescer* c, const std::vector<OneReq*>& batch, int rc, const std::string& err, const uint32_t* ids, const double* scores,
                        const uint32_t* counts, const uint64_t* row_offs, std::vector<OneWaiter*>& sleepers,
                        std::chrono::steady_clock::time_point t_batch) {
  sleepers.clear();
  for (size_t i = 0; i < batch.size(); i++) {
    OneReq* r = batch[i];
    r->rc = rc;
    if (rc) r->err = err;
    else {
      const uint32_t k = r->key.k, cnt = counts[i], m = cnt < k ? cnt : (cnt >= SG_COUNT_LM_ERROR ? 0u : k);
      const size_t at = row_offs ? (size_t)row_offs[i] : i * (size_t)k;
      *r->count = cnt;
#ifdef SG_PHASE_TIMING
      memcpy(r->ids, ids + at, (size_t)(row_offs ? m : k) * 4);   // (debug builds, a plain take: the whole row, it may carry debug words)
#else
      memcpy(r->ids, ids + at, (size_t)m * 4);
#endif
      if (!r->key.autocomplete) memcpy(r->scores, scores + at, (size_t)m * 8);
    }
    OneWaiter* w = r->waiter;                              // (r is the caller's: gone once it sees state 1)
    if (r->state.exchange(1, std::memory_order_acq_rel) == 2) sleepers.push_back(w);   // asleep: stays until released
  }
  // the sleeping callers are woken one by one; SG_COALESCE_TREE=1 lets them wake each other up as a binary tree instead
  // (one futex wake on the dispatcher per batch: better with spare cores, worse on a CPU quota)
  static const bool tree = env_int("SG_COALESCE_TREE", 0, 1, 0) != 0;
  for (size_t i = 0; i < sleepers.size(); i++) {
    sleepers[i]->child[0] = tree && 2 * i + 1 < sleepers.size() ? sleepers[2 * i + 1] : nullptr;
    sleepers[i]->child[1] = tree && 2 * i + 2 < sleepers.size() ? sleepers[2 * i + 2] : nullptr;
  }
  if (tree) { if (!sleepers.empty()) release_waiter(sleepers[0]); }
  else for (OneWaiter* w : sleepers) release_waiter(w);
  const uint32_t ns = (uint32_t)std::min<long long>(std::chrono::duration_cast<std::chrono::nanoseconds>(std::chrono::steady_clock::now() - t_batch).count(), 5000000);
  c->batch_ns.store((c->batch_ns.load(std::memory_order_relaxed) * 7u + ns) / 8u, std::memory_order_relaxed);
}

static void coalescer_lane(Coalescer* c, Replica* rep) {
  std::vector<OneReq*> batch, late;
  std::map<SearchKey, uint32_t> key_no;        // a mixed take: its keys, numbered as they first appear
  std::vector<uint8_t> blob;
  std::vector<uint64_t> offs;
  std::vector<uint32_t> ids, counts;
  std::vector<double> scores;
  std::vector<OneWaiter*> sleepers;
  std::vector<sg_search_config> cfgs;          // a mixed take: its distinct keys, the key of every request, the rows' starts
  std::vector<uint32_t> cfg_of;
  std::vector<uint64_t> row_offs;
  struct AtExit { ~AtExit() { thread_contexts_release(); } } at_exit;
  for (;;) {
    batch.clear(); late.clear();
    cfgs.clear(); cfg_of.clear(); key_no.clear();
    bool mixed_take;
    {
      std::unique_lock<std::mutex> lock(c->mu);
      c->cv.wait(lock, [&] { return c->stop || (!c->hold && !c->pending.empty()); });
      if (c->pending.empty()) return;                       // stop, and nothing left to serve
      OneReq* first = c->pending.front();
      c->pending.pop_front();
      batch.push_back(first);
      mixed_take = c->mixed;
      if (!mixed_take) {
        for (auto it = c->pending.begin(); it != c->pending.end() && batch.size() < c->max_batch;) {
          if ((*it)->key == first->key) { batch.push_back(*it); it = c->pending.erase(it); } else ++it;
        }
      } else {                                               // the oldest max_batch requests, whatever their keys: sorted out below, off the lock
        while (!c->pending.empty() && batch.size() < c->max_batch) { batch.push_back(c->pending.front()); c->pending.pop_front(); }
      }
    }
    if (mixed_take) {
      // the keys are numbered in order of first appearance, SG_MAX_MIXED_CONFIGS of them at the most: a request with one key more goes
      // back to the head of the queue, in its order, for the next take.
      size_t kept = 0;
      for (OneReq* r : batch) {
        auto it = key_no.find(r->key);
        if (it == key_no.end()) {
          if (key_no.size() == SG_MAX_MIXED_CONFIGS) { late.push_back(r); continue; }
          it = key_no.emplace(r->key, (uint32_t)key_no.size()).first;
          cfgs.push_back(r->key);
        }
        cfg_of.push_back(it->second);
        batch[kept++] = r;
      }
      batch.resize(kept);
      if (!late.empty()) {
        { std::lock_guard<std::mutex> lock(c->mu); c->pending.insert(c->pending.begin(), late.begin(), late.end()); }
        c->cv.notify_one();
      }
      if (cfgs.size() == 1) cfgs.clear();                    // a take with a single key goes exactly the old way
    }
    // the take's queries as one blob + offsets, and room for its rows: the sum of the requests' k slots (n x k in a plain take)
    auto pack_take = [&](bool with_scores) {
      blob.clear(); offs.assign(1, 0);
      uint64_t rows = 0;
      for (OneReq* r : batch) { blob.insert(blob.end(), r->q, r->q + r->len); offs.push_back(blob.size()); rows += r->key.k; }
      ids.resize(rows); counts.resize(batch.size());
      if (with_scores) scores.resize(rows);
      return rows;
    };
    if (!cfgs.empty()) {       // several keys: one mixed call, every caller's row cut out of the ragged rows
      const uint32_t n = (uint32_t)batch.size();
      const auto t_batch = std::chrono::steady_clock::now();
      int rc = SG_OK;
      std::string err;
      try {
        const uint64_t rows = pack_take(true);
        row_offs.resize((size_t)n + 1);
        rc = mixed_host_call(c->index, rep, blob.data(), offs.data(), n, cfgs.data(), (uint32_t)cfgs.size(), cfg_of.data(), rows, ids.data(),
                             scores.data(), counts.data(), row_offs.data());
        if (rc) err = g_err;
      } catch (const std::exception& e) { rc = SG_E_NOMEM; err = e.what(); }
      c->n_batches.fetch_add(1, std::memory_order_relaxed); c->n_mixed.fetch_add(1, std::memory_order_relaxed);
      c->n_groups.fetch_add(cfgs.size(), std::memory_order_relaxed);
      answer_take(c, batch, rc, err, ids.data(), scores.data(), counts.data(), row_offs.data(), sleepers, t_batch);
      continue;
    }
    c->n_batches.fetch_add(1, std::memory_order_relaxed); c->n_groups.fetch_add(1, std::memory_order_relaxed);
    // (copies: batch[0] lives on its caller's stack and is gone once that caller is answered)
    const SearchKey f = batch[0]->key;
    const uint32_t n = (uint32_t)batch.size();
    const auto t_batch = std::chrono::steady_clock::now();
    int rc = SG_OK;
    std::string err;
    try {
      pack_take(!f.autocomplete);
      rc = run_host(c->index, rep, blob.data(), offs.data(), n, search_req(f), ids.data(), f.autocomplete ? nullptr : scores.data(), counts.data());
      if (rc) err = g_err;
    } catch (const std::exception& e) { rc = SG_E_NOMEM; err = e.what(); }
    answer_take(c, batch, rc, err, ids.data(), scores.data(), counts.data(), nullptr, sleepers, t_batch);
  }
}

static Coalescer* coalescer_of(sg_index* ix) {
  std::lock_guard<std::mutex> lock(ix->mu);
  if (!ix->coalescer) {
    auto* c = new Coalescer();
    c->index = ix;
    const uint32_t lanes = (uint32_t)env_int("SG_COALESCE_LANES", 1, 16, 1);   // (one dispatcher per replica: larger batches beat overlap — 256 callers: 590 k q/s with 1, 215 k with 4)
    for (auto& r : ix->replicas) for (uint32_t l = 0; l < lanes; l++) c->lanes.emplace_back(coalescer_lane, c, r.get());
    ix->coalescer = c;
  }
  return ix->coalescer;
}

static void coalescer_stop(Coalescer* c) {
  { std::lock_guard<std::mutex> lock(c->mu); c->stop = true; }
  c->cv.notify_all();
  for (auto& t : c->lanes) t.join();
  delete c;
}

static int submit_one(sg_index* index, OneReq& r) {
  static thread_local OneWaiter waiter;
  r.waiter = &waiter;
  Coalescer* c = coalescer_of(index);
  { std::lock_guard<std::mutex> lock(c->mu); c->pending.push_back(&r); }
  c->cv.notify_one();
  // Callers sleep at once by default.  Spinning first (SG_COALESCE_SPIN_US) saves the futex round trip when every caller has
  // a core of its own — and is ruinous when they do not: 256 callers on the GPU box's 16-CPU quota reach 670 k q/s
  // sleeping, 137 k spinning 100 us, 59 k spinning 300 us (tests/cpp/single_query_load).
  static const uint32_t spin_ns = (uint32_t)env_int("SG_COALESCE_SPIN_US", 0, 100000, 0) * 1000u;
  const auto t_spin = std::chrono::steady_clock::now();
  for (uint32_t spin = 0; r.state.load(std::memory_order_acquire) != 1; spin++) {
    __builtin_ia32_pause();
    if ((spin & 63u) == 63u && (uint64_t)std::chrono::duration_cast<std::chrono::nanoseconds>(std::chrono::steady_clock::now() - t_spin).count() > spin_ns) break;
  }
  if (r.state.load(std::memory_order_acquire) != 1) {
    std::unique_lock<std::mutex> lk(waiter.mu);
    waiter.released = false;
    int expect = 0;
    if (r.state.compare_exchange_strong(expect, 2, std::memory_order_acq_rel)) {
      waiter.cv.wait(lk, [&] { return waiter.released; });
      OneWaiter* kids[2] = {waiter.child[0], waiter.child[1]};
      lk.unlock();
      for (OneWaiter* kid : kids) if (kid) release_waiter(kid);
    }
  }
  if (r.rc) set_error(r.err);
  return r.rc;
}

extern "C" {

int sg_suggest_one(sg_index* index, const uint8_t* q, uint32_t len, int metric, double similarity, uint32_t k, uint32_t* out_ids,
                   double* out_scores, uint32_t* out_count) {
  SG_GUARD_BEGIN
  OneReq r;
  r.key = fuzzy_key(metric, similarity, k);                 // (an empty query needs no bytes: "" stands for them in the pointer check)
  if (int rc = open_search(index, r.key, true, {len ? q : (const uint8_t*)"", out_ids, out_scores, out_count})) return rc;
  r.q = q; r.len = len;
  r.ids = out_ids; r.scores = out_scores; r.count = out_count;
  return submit_one(index, r);
  SG_GUARD_END(SG_RC)
}

int sg_autocomplete_one_from(sg_index* index, const uint8_t* q, uint32_t len, uint32_t first_doc, uint32_t limit, uint32_t* out_ids, uint32_t* out_count) {
  SG_GUARD_BEGIN
  OneReq r;
  r.key = prefix_key(limit, first_doc);
  if (int rc = open_search(index, r.key, false, {len ? q : (const uint8_t*)"", out_ids, out_count})) return rc;
  r.q = q; r.len = len;
  r.ids = out_ids; r.scores = nullptr; r.count = out_count;
  return submit_one(index, r);
  SG_GUARD_END(SG_RC)
}
int sg_autocomplete_one(sg_index* index, const uint8_t* q, uint32_t len, uint32_t limit, uint32_t* out_ids, uint32_t* out_count) {
  return sg_autocomplete_one_from(index, q, len, 0, limit, out_ids, out_count);
}

}  // extern "C"
