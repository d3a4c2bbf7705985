// search_api.inc — the host-buffer searches: search_req / search_enqueue / run_host, sg_suggest_batch and
// sg_autocomplete_batch with their _from forms, and the metric-table handle with its two searches.  Uses handles.inc
// (SearchKey, open_search), capi.inc and host_call.inc.

extern "C" {
// a host-buffer search: the key's five values in r (by_doc and mt are set by the caller)
static LaunchReq search_req(const SearchKey& c) {
  LaunchReq r;
  r.metric = c.metric; r.similarity = c.similarity; r.k = c.k; r.autocomplete = c.autocomplete; r.ac_first = c.first_doc;
  return r;
}

// LaunchReq::no_long_queries of a caller with host buffers, who knows its longest query: at most 112 bytes + the wrap runes stay
// within the wavefront kernel's 144 runes / 128 n-grams, and the long-query launch — a few microseconds of a single query's
// latency — is left out
static bool no_long_queries(const uint64_t* offs, uint32_t n_q) {
  uint64_t max_len = 0;
  for (uint32_t i = 0; i < n_q; i++) max_len = std::max<uint64_t>(max_len, offs[i + 1] - offs[i]);
  return max_len <= 112;
}

// the enqueue step of a search: launch() on the device block's regions (search_io's indices); aux: the call declared aux rows
static Enqueue search_enqueue(sg_index* index, Replica* rep, const LaunchReq& req, const uint64_t* offs, uint32_t n_q, bool aux = false) {
  return [=](const IoCall& io, hipStream_t st) {
    LaunchReq r = req;
    r.q = io.at<char>(IO_Q); r.offs = io.at<char>(IO_OFFS); r.n_q = n_q; r.stream = st; r.no_long_queries = no_long_queries(offs, n_q);
    r.ids = io.at<char>(IO_IDS); r.scores = r.autocomplete ? nullptr : io.at<char>(IO_SCORES); r.counts = io.at<char>(IO_COUNTS);
    r.out_aux = aux ? io.at<uint32_t>(IO_AUX) : nullptr;
    return launch(index, rep, r);
  };
}
static int run_host(sg_index* index, Replica* rep, const uint8_t* q, const uint64_t* offs, uint32_t n_q, const LaunchReq& r,
                    uint32_t* ids, double* scores, uint32_t* counts, uint32_t* aux = nullptr) {
  if (n_q == 0) return SG_OK;
  return run_host_call(rep->device, search_io(q, offs, n_q, (uint64_t)n_q * r.k, ids, r.autocomplete ? nullptr : scores, counts, aux, true), search_enqueue(index, rep, r, offs, n_q, aux != nullptr));
}

int sg_suggest_batch(sg_index* index, const uint8_t* q, const uint64_t* offs, uint32_t n_q, int metric, double similarity,
                     uint32_t k, uint32_t* ids, double* scores, uint32_t* counts) {
  SG_GUARD_BEGIN
  const SearchKey c = fuzzy_key(metric, similarity, k);
  if (int rc = open_search(index, c, true, {offs, ids, scores, counts})) return rc;
  return run_host(index, find_replica(index, -1), q, offs, n_q, search_req(c), ids, scores, counts);
  SG_GUARD_END(SG_RC)
}

// Autocomplete restricted to documents with docID >= first_doc: the `limit` smallest of those.  A caller that wants EVERY
// match (the reference streams them all to the caller's collector, pkg/suggest/autocomplete.go:40-77) pages through them:
// first_doc = 0, then last docID of the page + 1, until a page comes back short.
int sg_autocomplete_batch_from(sg_index* index, const uint8_t* q, const uint64_t* offs, uint32_t n_q, uint32_t first_doc, uint32_t limit,
                               uint32_t* ids, uint32_t* counts) {
  SG_GUARD_BEGIN
  const SearchKey c = prefix_key(limit, first_doc);
  if (int rc = open_search(index, c, false, {offs, ids, counts})) return rc;
  return run_host(index, find_replica(index, -1), q, offs, n_q, search_req(c), ids, nullptr, counts);
  SG_GUARD_END(SG_RC)
}
int sg_autocomplete_batch(sg_index* index, const uint8_t* q, const uint64_t* offs, uint32_t n_q, uint32_t limit, uint32_t* ids, uint32_t* counts) {
  return sg_autocomplete_batch_from(index, q, offs, n_q, 0, limit, ids, counts);
}

// ---- an opaque metric.Metric (pkg/metric/metric.go:7-16): tables built by the host, kept in HBM behind a handle ----
struct sg_metric_tables {
  sg_index* index = nullptr;           // (retained: the tables live in its primary replica's HBM)
  int device = -1;
  MetricTab tab{};
  DeviceBlock mem;                     // one block: tab's arrays are views into it
  std::atomic<int> refs{1};
};

// The segments the reference visits for a query of `a` n-grams under a metric whose MinY / MaxY are min_y / max_y, over an index
// of n_segments segments, as the pair the kernels take for [b_min, b_max].  suggester.go:113-121 does not walk [MinY, bMax]
// (bMax = min(MaxY, n_segments - 1)): it sends i = a, a - 1, ... >= MinY and j = a + 1, a + 2, ... <= bMax, so with a span above
// zero it visits [MinY, a] and [a + 1, bMax] — also a + 1 .. MinY - 1 where MinY > a + 1, and bMax + 1 .. a where bMax < a.  The
// five metrics of pkg/metric never leave that gap; a foreign one may.  A span of zero or below is handed back untouched, so that
// the kernels still flag it (SG_COUNT_REF_DEADLOCK / SG_COUNT_REF_PANIC).  Needs no GPU.
int sg_metric_window(int32_t min_y, int32_t max_y, uint32_t a, uint32_t n_segments, int32_t* out) {
  SG_GUARD_BEGIN
  if (!out) { set_error("null argument"); return SG_E_INVALID; }
  out[0] = min_y; out[1] = max_y;
  const int64_t b_max = std::min<int64_t>(max_y, (int64_t)n_segments - 1);
  if (b_max - (int64_t)min_y + 1 <= 0) return SG_OK;
  out[0] = (int32_t)std::min<int64_t>(min_y, (int64_t)a + 1);
  out[1] = (int32_t)std::min<int64_t>(std::max<int64_t>(b_max, a), INT32_MAX);
  return SG_OK;
  SG_GUARD_END(SG_RC)
}

// min_y[a], max_y[a] (a = 0 .. a_max) = Metric.MinY / MaxY(alpha, a); threshold[a * S + b] = Metric.Threshold(alpha, a, b);
// score[(a * S + b) * (a_max + 1) + o] = 1 - Metric.Distance(o, a, b) — the double metricScorer.Score returns
// (pkg/suggest/scorer.go:29-31) — for b = 0 .. S - 1 (S = the index's segment count, sg_index_stats), o = 0 .. a_max.  Every row of
// min_y / max_y goes through sg_metric_window before the upload: fill threshold and score over THAT range of b (an entry left 0
// is a segment that is not searched).  Entries above min(a, b) are never read for a query that repeats no term.
int sg_metric_tables_create(sg_index* index, uint32_t a_max, const int32_t* min_y, const int32_t* max_y, const int32_t* threshold,
                            const double* score, sg_metric_tables** out) {
  SG_GUARD_BEGIN
  if (!index || !min_y || !max_y || !threshold || !score || !out) { set_error("null argument"); return SG_E_INVALID; }
  if (!index->uploaded.load(std::memory_order_acquire)) { set_error("index not uploaded: call sg_index_upload first"); return SG_E_NOT_UPLOADED; }
  // (dense tables: (a_max + 1)^2 x S doubles — 34 MB at a_max 256 and 64 segments, gigabytes at 4096.  A binding caps a_max at what
  //  its queries need; a query with more n-grams than the tables hold comes back SG_COUNT_TOO_LONG.)
  if (a_max == 0 || a_max > 1024u) { set_error("a_max outside 1..1024"); return SG_E_INVALID; }
  const uint32_t S = index->host.n_segments;
  const size_t n_a = (size_t)a_max + 1, n_thr = n_a * S, n_sc = n_thr * n_a;
  if (n_sc * 8 > ((size_t)4 << 30)) { set_error("metric tables above 4 GiB"); return SG_E_INVALID; }
  Replica* rep = find_replica(index, -1);
  DeviceGuard dg;
  HIP_TRY(dg.set(rep->device));
  const size_t o_max = (n_a * 4 + 15) & ~(size_t)15, o_thr = 2 * o_max, o_sc = (o_thr + n_thr * 4 + 15) & ~(size_t)15, total = o_sc + n_sc * 8;
  std::unique_ptr<sg_metric_tables> t(new sg_metric_tables());   // (a step that fails below frees it, its block included)
  char* b = nullptr;
  if (int rc = t->mem.alloc(&b, total)) return rc;
  std::vector<int32_t> win_lo(n_a), win_hi(n_a);                 // the visited segments, not [MinY, MaxY] (sg_metric_window)
  for (size_t a = 0; a < n_a; a++) {
    int32_t w[2];
    if (int rc = sg_metric_window(min_y[a], max_y[a], (uint32_t)a, S, w)) return rc;
    win_lo[a] = w[0]; win_hi[a] = w[1];
  }
  HIP_TRY(hipMemcpy(b, win_lo.data(), n_a * 4, hipMemcpyHostToDevice));
  HIP_TRY(hipMemcpy(b + o_max, win_hi.data(), n_a * 4, hipMemcpyHostToDevice));
  if (n_thr) HIP_TRY(hipMemcpy(b + o_thr, threshold, n_thr * 4, hipMemcpyHostToDevice));
  if (n_sc) HIP_TRY(hipMemcpy(b + o_sc, score, n_sc * 8, hipMemcpyHostToDevice));
  t->tab.min_y = (const int32_t*)b; t->tab.max_y = (const int32_t*)(b + o_max); t->tab.thr = (const int32_t*)(b + o_thr);
  t->tab.score = (const double*)(b + o_sc); t->tab.a_max = a_max; t->tab.S = S;
  t->device = rep->device;
  sg_index_retain(index);
  t->index = index;
  *out = t.release();
  return SG_OK;
  SG_GUARD_END(SG_RC)
}

// One more reference: a caller that shares a table set between threads (a binding's cache and the calls in flight on it) takes
// one per user; the HBM goes with the last release.
void sg_metric_tables_retain(sg_metric_tables* t) { if (t) t->refs.fetch_add(1); }
void sg_metric_tables_release(sg_metric_tables* t) {
  if (!t || t->refs.fetch_sub(1) != 1) return;
  sg_index* index = t->index;
  delete t;                            // (the block goes before the index that holds its device's replica)
  sg_index_release(index);
}

static int check_tables(sg_index* index, const sg_metric_tables* tables) {
  if (tables && tables->index != index) { set_error("metric tables belong to another index"); return SG_E_INVALID; }
  return SG_OK;
}

// sg_suggest_batch with the metric given as tables (similarity is folded into them): same rows, same order.
int sg_suggest_batch_tables(sg_index* index, const uint8_t* q, const uint64_t* offs, uint32_t n_q, const sg_metric_tables* tables, uint32_t k,
                            uint32_t* ids, double* scores, uint32_t* counts) {
  SG_GUARD_BEGIN
  const SearchKey c = fuzzy_key(SG_JACCARD, 0.5, k);           // (the launch reads the tables, not these two)
  if (int rc = open_search(index, c, false, {offs, ids, scores, counts, tables})) return rc;
  if (int rc = check_tables(index, tables)) return rc;
  LaunchReq r = search_req(c);
  r.mt = &tables->tab;
  return run_host(index, find_replica(index, -1), q, offs, n_q, r, ids, scores, counts);
  SG_GUARD_END(SG_RC)
}

// The fuzzy search for ANY collector (pkg/suggest/suggester.go:78-99 hands every document with overlap >= Threshold to the
// caller's collector): row i = the `limit` smallest docIDs >= first_doc among query i's candidates over every admissible
// segment, ascending; out_scores their scores, out_aux (may be null) segment << 16 | overlap of each — what a binding needs to
// rebuild merger.MergeCandidate{Position, Overlap} and the segment's scorer.  A caller pages: first_doc = 0, then the last
// docID of a full page + 1 (a document that repeats a term can appear more than once: see INTEGRATION.md).  `tables` non-null
// replaces (metric, similarity).
int sg_suggest_batch_from(sg_index* index, const uint8_t* q, const uint64_t* offs, uint32_t n_q, int metric, double similarity,
                          const sg_metric_tables* tables, uint32_t first_doc, uint32_t limit, uint32_t* ids, double* scores, uint32_t* aux,
                          uint32_t* counts) {
  SG_GUARD_BEGIN
  const SearchKey c = tables ? fuzzy_key(SG_JACCARD, 0.5, limit, first_doc) : fuzzy_key(metric, similarity, limit, first_doc);
  if (int rc = open_search(index, c, tables == nullptr, {offs, ids, scores, counts})) return rc;
  if (int rc = check_tables(index, tables)) return rc;
  LaunchReq r = search_req(c);
  r.by_doc = true;
  if (tables) r.mt = &tables->tab;
  return run_host(index, find_replica(index, -1), q, offs, n_q, r, ids, scores, counts, aux);
  SG_GUARD_END(SG_RC)
}

}  // extern "C"
