// debug_api.inc — test hooks, statistics and introspection: sg_debug_*, the launch / pipeline counters, sg_index_stats, the knob
// table's rows, the algorithmic-bytes models.  Uses handles.inc, capi.inc, tune.inc and knobs.inc.

extern "C" {
// Test hook: the permutation the device's Go-1.14 sort.Sort restatement (PairSort, engine.hip) gives `n` <= 128 keys
// (out[i] = original index of the element that ends at position i).
int sg_debug_pairsort(int device, const uint32_t* keys, uint32_t n, uint32_t* out) {
  SG_GUARD_BEGIN
  if (!keys || !out || n > SG_MAX_A) { set_error("bad argument"); return SG_E_INVALID; }
  DeviceGuard dg;
  HIP_TRY(dg.set(device));
  DeviceBlock mem;
  uint32_t *dk = nullptr, *dv = nullptr;
  int rc;
  if ((rc = mem.alloc(&dk, SG_MAX_A)) || (rc = mem.alloc(&dv, SG_MAX_A))) return rc;
  HIP_TRY(hipMemcpy(dk, keys, (size_t)n * 4, hipMemcpyHostToDevice));
  hipLaunchKernelGGL(pairsort_test_kernel, dim3(1), dim3(64), 0, 0, dk, n, dv);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipMemcpy(out, dv, (size_t)n * 4, hipMemcpyDeviceToHost));
  return SG_OK;
  SG_GUARD_END(SG_RC)
}

#ifdef SG_PHASE_TIMING
void sg_debug_set_prof(void* device_u64x8) { g_prof_buf = device_u64x8; }
#endif

// The sampled launch counters of the primary replica (cumulative, wrapping at 2^32): out[0] sampled fuzzy queries whose top-k
// ended full, [1] sampled fuzzy queries (one in 32 of a batch above 1 024 queries, else every one), [2] their results, [3] the
// 16-byte chunks of the packed posting store they streamed.  Synchronises the device.  For bench.py's roofline.model_bytes.
int sg_index_launch_stats(sg_index* index, uint64_t out[4]) {
  SG_GUARD_BEGIN
  if (!index || !out) { set_error("null argument"); return SG_E_INVALID; }
  Replica* rep = find_replica(index, -1);
  if (!rep || !rep->d_fill) { set_error("index not uploaded"); return SG_E_NOT_UPLOADED; }
  DeviceGuard dg;
  HIP_TRY(dg.set(rep->device));
  uint32_t w[SG_STAT_WORDS] = {0};
  HIP_TRY(hipDeviceSynchronize());
  HIP_TRY(hipMemcpy(w, rep->d_fill, sizeof w, hipMemcpyDeviceToHost));
  out[0] = w[SG_STAT_FULL]; out[1] = w[SG_STAT_SAMPLED]; out[2] = w[SG_STAT_RESULTS];
  out[3] = (uint64_t)w[SG_STAT_CHUNKS] | ((uint64_t)w[SG_STAT_CHUNKS + 1] << 32);               // (the chunk counter is 64 bits wide: a long-list batch streams 10^8 chunks per launch over its sampled queries)
  return SG_OK;
  SG_GUARD_END(SG_RC)
}

// [r5] What the three-launch pipeline (pipeline.inc) left to the fused kernel, cumulative over the fuzzy launches of the primary
// replica (wrapping at 2^32): out[0] queries the plan could not express, [1] queries whose candidates overflowed their slots, [2]
// queries with a matching document that repeats a term, [3] the queries of all launches that took the pipeline (not wrapping).
// [r6] The counters are the pipeline's own (PipeArgs::stat): on whatever SG_TIGHTEN says.  Synchronises the device.
int sg_index_pipe_stats(sg_index* index, uint64_t out[4]) {
  SG_GUARD_BEGIN
  if (!index || !out) { set_error("null argument"); return SG_E_INVALID; }
  Replica* rep = find_replica(index, -1);
  if (!rep || !rep->d_fill) { set_error("index not uploaded"); return SG_E_NOT_UPLOADED; }
  DeviceGuard dg;
  HIP_TRY(dg.set(rep->device));
  uint32_t w[SG_STAT_WORDS] = {0};
  HIP_TRY(hipDeviceSynchronize());
  HIP_TRY(hipMemcpy(w, rep->d_fill, sizeof w, hipMemcpyDeviceToHost));
  out[0] = w[SG_STAT_UNPLANNED]; out[1] = w[SG_STAT_OVERFLOW]; out[2] = w[SG_STAT_REPEATS]; out[3] = rep->pipe_queries.load(std::memory_order_relaxed);
  return SG_OK;
  SG_GUARD_END(SG_RC)
}

// [r6] The pipeline's sampled volumes, cumulative (wrapping at 2^32): out[0] sampled queries the plan expressed (one in 256 of a
// batch above 1 024 queries, else every one), [1] their groups (plan items), [2] streamed lists, [3] rows of 64 lanes, [4] the
// candidates the stream launch pushed for the sampled queries that reached the verify launch; [5] the 16-byte chunks of the packed
// posting store, [6] 1 when the stream launch takes 8-byte sub-row descriptors (2^26 chunks and more, or SG_PIPE_WIDE), [7] 0.
// Synchronises the device.
int sg_index_pipe_volumes(sg_index* index, uint64_t out[8]) {
  SG_GUARD_BEGIN
  if (!index || !out) { set_error("null argument"); return SG_E_INVALID; }
  Replica* rep = find_replica(index, -1);
  if (!rep || !rep->d_fill) { set_error("index not uploaded"); return SG_E_NOT_UPLOADED; }
  DeviceGuard dg;
  HIP_TRY(dg.set(rep->device));
  uint32_t w[SG_STAT_WORDS] = {0};
  HIP_TRY(hipDeviceSynchronize());
  HIP_TRY(hipMemcpy(w, rep->d_fill, sizeof w, hipMemcpyDeviceToHost));
  for (int i = 0; i < 5; i++) out[i] = w[SG_STAT_PLANNED + i];
  out[5] = rep->packed_chunks; out[6] = pipe_wide(index, rep) ? 1u : 0u;
  out[7] = !index->knobs.pipe_shape_auto ? 3u : rep->shape_floor.last.load(std::memory_order_relaxed);   // the stream workgroup of the latest launch: 0 / 1 / 2 = 2 / 4 / 8 wavefronts, 3 = the knobs' own
  return SG_OK;
  SG_GUARD_END(SG_RC)
}

// Test hooks of the auto-tuner (no GPU needed): the choices for given statistics, and the statistics + choices of a built index.
// out: {log2 counter words, filter level, pipeline pays, wavefronts / log2 counters / descriptor bytes of a stream workgroup}.
int sg_debug_tune_choice(double est_query_chunks, double max_term_chunks, int32_t out[6]) {
  if (!out) { set_error("null argument"); return SG_E_INVALID; }
  const TuneChoice c = tune_choice(est_query_chunks, max_term_chunks);
  out[0] = (int32_t)c.log2_cnt; out[1] = (int32_t)c.filter_level; out[2] = c.pipe_pays;
  out[3] = (int32_t)c.pipe_nw; out[4] = (int32_t)c.pipe_log2_cnt; out[5] = (int32_t)c.pipe_dt_bytes;
  return SG_OK;
}
int sg_debug_pipe_shape(double est_query_chunks, double terms_per_doc, int32_t t_floor, int32_t metric, double similarity, int32_t* out_shape) {
  SG_GUARD_BEGIN
  if (!out_shape || metric < SG_JACCARD || metric > SG_OVERLAP || !(similarity > 0 && similarity <= 1)) { set_error("bad argument"); return SG_E_INVALID; }
  *out_shape = (int32_t)pipe_shape_model(est_query_chunks, terms_per_doc, t_floor, metric, similarity);
  return SG_OK;
  SG_GUARD_END(SG_RC)
}
int sg_debug_poison(uint32_t on) {
  SG_GUARD_BEGIN
  if (on > 2u) { set_error("poison: 0 off, 1 or 2 a pattern family"); return SG_E_INVALID; }
  g_poison.store(on, std::memory_order_relaxed);
  return SG_OK;
  SG_GUARD_END(SG_RC)
}
int sg_debug_poison_stats(uint64_t out[8]) {
  SG_GUARD_BEGIN
  if (!out) { set_error("null argument"); return SG_E_INVALID; }
  for (int i = 0; i < 8; i++) { out[i] = t_poisoned[i]; t_poisoned[i] = 0; }
  return SG_OK;
  SG_GUARD_END(SG_RC)
}
int sg_debug_rows_layout(uint32_t n_q, uint32_t k, int32_t split, int32_t reorder, uint64_t out[16]) {
  SG_GUARD_BEGIN
  if (!out || n_q == 0 || k == 0 || reorder < 0 || reorder > 2) { set_error("bad argument"); return SG_E_INVALID; }
  LaunchPlan p;
  if (split && k <= SG_K_LDS) { p.split_min = 1; split_caps(p, n_q, k); }
  p.reorder = reorder != 0; p.ord_blocks = (n_q + 1023u) / 1024u; p.ord_direct = reorder == 2;
  const RowsLayout L = rows_layout(p, n_q, k);
  const uint64_t v[16] = {L.s, L.id, L.split, L.items, L.slot, L.part_n, L.part_s, L.part_id, L.ord, L.ord_ctl, L.bytes,
                          p.slot_cap, p.item_cap, p.ord_blocks, SG_MAX_PARTS, SG_ORDER_CTL_WORDS};
  for (int i = 0; i < 16; i++) out[i] = v[i];
  return SG_OK;
  SG_GUARD_END(SG_RC)
}
int sg_debug_pipe_layout(uint32_t n_q, uint32_t cand_cap, uint64_t out[12]) {
  SG_GUARD_BEGIN
  if (!out || n_q == 0 || cand_cap == 0) { set_error("bad argument"); return SG_E_INVALID; }
  const PipeLayout L = pipe_layout(n_q, cand_cap);
  const uint64_t v[12] = {L.rec, L.vrec, L.ovf, L.cand_n, L.fb_list, L.bytes, L.piece, L.vrec_words, L.ovf_cap,
                          SG_PIPE_REC_STRIDE, SG_PIPE_OVF_WORDS, SG_PIPE_PIECE};
  for (int i = 0; i < 12; i++) out[i] = v[i];
  return SG_OK;
  SG_GUARD_END(SG_RC)
}
int sg_debug_tune_index(sg_index* ix, double out_stats[2], int32_t out[6]) {
  SG_GUARD_BEGIN
  if (!ix || !out_stats || !out) { set_error("null argument"); return SG_E_INVALID; }
  {
    std::lock_guard<std::mutex> lock(ix->mu);
    if (const int rc = tune_index(ix)) return rc;
  }
  out_stats[0] = ix->est_query_chunks; out_stats[1] = ix->max_term_chunks;
  out[0] = ix->knobs.log2_cnt; out[1] = ix->knobs.filter_level; out[2] = ix->pipe_pays ? 1 : 0;
  out[3] = ix->knobs.pipe_nw; out[4] = ix->knobs.pipe_log2_cnt; out[5] = ix->knobs.pipe_dt_bytes;
  return SG_OK;
  SG_GUARD_END(SG_RC)
}
int sg_debug_knob(const sg_index* ix, uint32_t i, char name[32], int32_t out[6]) {   // (nothing in it throws)
  if (!name || !out || i >= kNumKnobs) { set_error("null argument / no such row of the knob table"); return SG_E_INVALID; }
  const KnobRow& row = kKnobs[i];
  snprintf(name, 32, "%s", row.name);
  out[0] = row.lo; out[1] = row.hi; out[2] = row.def; out[3] = (int32_t)row.flags;
  out[4] = ix ? ix->knobs.*row.field : row.def; out[5] = ix ? (int32_t)((ix->knobs.explicit_set >> i) & 1u) : 0;
  return SG_OK;
}

int sg_index_stats(const sg_index* ix, sg_stats* out) {
  if (!ix || !out) { set_error("null argument"); return SG_E_INVALID; }
  const HostIndex& h = ix->host;
  out->n_docs = h.n_docs; out->n_segments = h.n_segments; out->n_terms = h.term_key.size();
  out->n_lists = h.n_lists; out->n_postings = h.n_postings; out->n_postings_raw = h.n_postings_raw;
  out->posting_bytes = h.postings.size() * 4;
  out->table_bytes = h.seg_off.size() * 4 + h.slots.size() * sizeof(TermSlot);
  out->device_bytes = 0;
  { std::lock_guard<std::mutex> lock(const_cast<sg_index*>(ix)->mu); for (auto& r : ix->replicas) out->device_bytes += r->mem.total(); }
  return SG_OK;
}

int sg_tokenize(const sg_index* ix, const uint8_t* text, uint32_t len, int autocomplete, uint64_t* out_keys, uint32_t cap) {
  if (!ix) { set_error("null index"); return SG_E_INVALID; }
  std::vector<uint64_t> keys;
  if (!tokenize_keys(ix->host, text, len, autocomplete != 0, keys)) { set_error("term exceeds the 8-symbol key"); return SG_E_UNSUPPORTED; }
  for (size_t i = 0; i < keys.size() && i < cap; i++) out_keys[i] = keys[i];
  return (int)keys.size();
}

int sg_term_string(const sg_index* ix, uint64_t key, char* out, uint32_t cap) {
  if (!ix) { set_error("null index"); return SG_E_INVALID; }
  std::string s;
  for (int i = 0; i < 8; i++) {
    uint32_t id = (key >> (8 * i)) & 0xFF;
    if (!id) break;
    if (id >= ix->host.sym.sym_rune.size()) { set_error("bad symbol id in key"); return SG_E_INVALID; }
    uint32_t r = ix->host.sym.sym_rune[id];
    if (r < 0x80) s.push_back((char)r);
    else if (r < 0x800) { s.push_back((char)(0xC0 | (r >> 6))); s.push_back((char)(0x80 | (r & 0x3F))); }
    else if (r < 0x10000) { s.push_back((char)(0xE0 | (r >> 12))); s.push_back((char)(0x80 | ((r >> 6) & 0x3F))); s.push_back((char)(0x80 | (r & 0x3F))); }
    else { s.push_back((char)(0xF0 | (r >> 18))); s.push_back((char)(0x80 | ((r >> 12) & 0x3F))); s.push_back((char)(0x80 | ((r >> 6) & 0x3F))); s.push_back((char)(0x80 | (r & 0x3F))); }
  }
  if (s.size() <= cap) memcpy(out, s.data(), s.size());
  return (int)s.size();
}

int64_t sg_index_list(const sg_index* ix, uint32_t segment, uint64_t key, uint32_t* out, uint64_t cap, uint64_t* raw_len) {
  if (!ix) return -1;
  const HostIndex& h = ix->host;
  auto it = h.term_of.find(key);
  if (it == h.term_of.end() || segment >= h.n_segments) return -1;
  const size_t t = it->second, S = h.n_segments;
  const uint32_t len = h.list_len[t * S + segment];
  if (!len) return -1;
  const uint32_t* p = h.postings.data() + (size_t)h.seg_off[t * (S + 1) + segment] * 4;
  for (uint32_t i = 0; i < len && i < cap; i++) out[i] = p[i];
  if (raw_len) {
    uint64_t raw = len;
    DupEntry probe{(uint32_t)t, segment, 0, 0};
    auto lo = std::lower_bound(h.dups.begin(), h.dups.end(), probe, [](const DupEntry& x, const DupEntry& y) {
      return x.term != y.term ? x.term < y.term : x.segment < y.segment;
    });
    for (; lo != h.dups.end() && lo->term == t && lo->segment == segment; ++lo) raw += lo->mult - 1;
    *raw_len = raw;
  }
  return len;
}

uint64_t sg_index_lists(const sg_index* ix, uint32_t* out_segments, uint64_t* out_keys, uint64_t cap) {
  if (!ix) return 0;
  const HostIndex& h = ix->host;
  const size_t S = h.n_segments;
  uint64_t n = 0;
  for (size_t t = 0; t < h.term_key.size(); t++)
    for (size_t b = 0; b < S; b++)
      if (h.list_len[t * S + b]) {
        if (n < cap) { out_segments[n] = (uint32_t)b; out_keys[n] = h.term_key[t]; }
        n++;
      }
  return n;
}

// Autocomplete's share of the same accounting: every segment from |terms| up whose lists hold all the terms is intersected
// (autocomplete.go:47-66, list_intersector.go:23-81): 4 bytes per posting of every term there + the query + 4 * limit out.
int sg_autocomplete_algorithmic_bytes(const sg_index* ix, const uint8_t* q, const uint64_t* offs, uint32_t n_q, uint32_t limit, uint64_t* out_total) {
  if (!ix || !offs || !out_total) { set_error("null argument"); return SG_E_INVALID; }
  const HostIndex& h = ix->host;
  const int S = (int)h.n_segments;
  uint64_t total = 0;
  std::vector<uint64_t> keys;
  std::vector<uint32_t> terms;
  for (uint32_t i = 0; i < n_q; i++) {
    const size_t len = (size_t)(offs[i + 1] - offs[i]);
    total += len + 4ull * limit;
    if (!tokenize_keys(h, q + offs[i], len, true, keys) || keys.empty()) continue;
    terms.clear();
    bool all = true;
    for (uint64_t key : keys) { auto it = h.term_of.find(key); if (it == h.term_of.end()) { all = false; break; } terms.push_back(it->second); }
    if (!all) continue;
    for (int b = (int)keys.size(); b < S; b++) {
      uint64_t vol = 0;
      bool present = true;
      for (uint32_t t : terms) { const uint32_t l = h.list_len[(size_t)t * S + b]; if (!l) { present = false; break; } vol += l; }
      if (present) total += 4ull * vol;
    }
  }
  *out_total = total;
  return SG_OK;
}

int sg_suggest_algorithmic_bytes(const sg_index* ix, const uint8_t* q, const uint64_t* offs, uint32_t n_q, int metric,
                                 double similarity, uint32_t k, uint64_t* out_total) {
  if (!ix || !offs || !out_total) { set_error("null argument"); return SG_E_INVALID; }
  const HostIndex& h = ix->host;
  const int S = (int)h.n_segments;
  uint64_t total = 0;
  std::vector<uint64_t> keys;
  for (uint32_t i = 0; i < n_q; i++) {
    const size_t len = (size_t)(offs[i + 1] - offs[i]);
    total += len + 12ull * k;
    if (!tokenize_keys(h, q + offs[i], len, false, keys) || keys.empty()) continue;
    const int A = (int)keys.size();
    int b_min = metric_min_y(metric, similarity, A), b_max = metric_max_y(metric, similarity, A);
    if (b_max >= S) b_max = S - 1;
    for (int b = std::max(b_min, 0); b <= b_max; b++) {
      const int T = metric_threshold(metric, similarity, A, b);
      if (T == 0 || T > b || T > A) continue;
      for (uint64_t key : keys) {
        auto it = h.term_of.find(key);
        if (it != h.term_of.end()) total += 4ull * h.list_len[(size_t)it->second * S + b];
      }
    }
  }
  *out_total = total;
  return SG_OK;
}

}  // extern "C"
