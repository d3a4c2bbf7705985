// index_api.inc — the index's C entry points (include/suggest_hip.h): sg_last_error, build, load, upload, replicate, tune,
// forward, retain / release, and the two searches on device pointers.  Uses handles.inc (open_search), capi.inc and tune.inc.

// ------------------------------------------------------------------------------------------
// C ABI (include/suggest_hip.h)
// ------------------------------------------------------------------------------------------
extern "C" {

const char* sg_last_error(void) { return g_err.c_str(); }

static int build_any(const uint8_t* utf8, const uint64_t* offs, uint32_t n_docs, const sg_desc* desc, uint32_t min_segments, int device,
                     sg_index** out) {
  if (!out || !offs || (!utf8 && n_docs && offs[n_docs])) { set_error("null argument"); return SG_E_INVALID; }   // (all-empty documents need no bytes)
  std::unique_ptr<sg_index> ix(new (std::nothrow) sg_index());
  if (!ix) return SG_E_NOMEM;
  ix->host.min_segments = min_segments;
  std::string err;
  int rc;
  if (device < 0) {
    rc = build_host_index(utf8, offs, n_docs, desc, ix->host, err);
    if (rc) set_error(err);
  } else {
    rc = init_description(desc, ix->host, err);
    if (rc) set_error(err);
    else rc = build_on_device(ix.get(), utf8, offs, n_docs, device);
  }
  if (!rc && (ix->host.wrap0.size() > SG_WRAP_MAX || ix->host.wrap1.size() > SG_WRAP_MAX)) {
    set_error("wrap strings longer than 8 runes"); rc = SG_E_UNSUPPORTED;
  }
  if (rc) return rc;
  *out = ix.release();
  return SG_OK;
}

int sg_index_build(const uint8_t* utf8, const uint64_t* offs, uint32_t n_docs, const sg_desc* desc, sg_index** out) {
  SG_GUARD_BEGIN
  return build_any(utf8, offs, n_docs, desc, 0, -1, out);
  SG_GUARD_END(SG_RC)
}

int sg_index_build_device(const uint8_t* utf8, const uint64_t* offs, uint32_t n_docs, const sg_desc* desc, int device, sg_index** out) {
  SG_GUARD_BEGIN
  if (device < 0) { set_error("bad device"); return SG_E_INVALID; }
  return build_any(utf8, offs, n_docs, desc, 0, device, out);
  SG_GUARD_END(SG_RC)
}

int sg_index_build_ex(const uint8_t* utf8, const uint64_t* offs, uint32_t n_docs, const sg_desc* desc, uint32_t min_segments, int device,
                      sg_index** out) {
  SG_GUARD_BEGIN
  return build_any(utf8, offs, n_docs, desc, min_segments, device, out);
  SG_GUARD_END(SG_RC)
}

int sg_debug_index_build_table_bits(uint32_t bits) {
  if (bits && (bits < 4u || bits > 20u)) { set_error("table bits: 0 (the default, 20) or 4 .. 20"); return SG_E_INVALID; }
  g_index_build_table_bits.store(bits, std::memory_order_relaxed);
  return SG_OK;
}

int sg_debug_index_build_report(uint32_t out[4]) {
  if (!out) { set_error("null argument"); return SG_E_INVALID; }
  for (int i = 0; i < 4; i++) out[i] = t_index_build_report[i];
  return SG_OK;
}

int sg_index_digest(const sg_index* ix, uint64_t out[4]) {
  if (!ix || !out) { set_error("null argument"); return SG_E_INVALID; }
  const HostIndex& h = ix->host;
  auto fold = [](const void* p, size_t bytes) {
    uint64_t acc = 0x9E3779B97F4A7C15ull ^ bytes;
    const uint8_t* b = (const uint8_t*)p;
    size_t i = 0;
    for (; i + 8 <= bytes; i += 8) { uint64_t w; memcpy(&w, b + i, 8); acc = mix64(acc ^ w); }
    for (; i < bytes; i++) acc = mix64(acc ^ b[i]);
    return acc;
  };
  out[0] = fold(h.postings.data(), h.postings.size() * 4);
  out[1] = fold(h.seg_off.data(), h.seg_off.size() * 4);
  out[2] = fold(h.list_len.data(), h.list_len.size() * 4);
  out[3] = fold(h.term_key.data(), h.term_key.size() * 8) ^ mix64(h.dups.size() * 4 + h.n_segments) ^
           fold(h.dups.data(), h.dups.size() * sizeof(DupEntry));
  return SG_OK;
}

int sg_index_load_reference(const char* hd_path, const char* dl_path, const sg_desc* desc, sg_index** out) {
  SG_GUARD_BEGIN
  if (!out || !hd_path || !dl_path) { set_error("null argument"); return SG_E_INVALID; }
  std::unique_ptr<sg_index> ix(new (std::nothrow) sg_index());
  if (!ix) return SG_E_NOMEM;
  std::string err;
  const int rc = load_reference_index(hd_path, dl_path, desc, ix->host, err);
  if (rc) { set_error(err); return rc; }
  if (ix->host.wrap0.size() > SG_WRAP_MAX || ix->host.wrap1.size() > SG_WRAP_MAX) {
    set_error("wrap strings longer than 8 runes"); return SG_E_UNSUPPORTED;
  }
  *out = ix.release();
  return SG_OK;
  SG_GUARD_END(SG_RC)
}

int sg_index_upload(sg_index* ix, int device) {
  SG_GUARD_BEGIN
  if (!ix) { set_error("null index"); return SG_E_INVALID; }
  if (find_replica(ix, device)) return SG_OK;              // already resident there
  return add_replica(ix, device);
  SG_GUARD_END(SG_RC)
}

int sg_index_replicate(sg_index* ix, const int* devices, uint32_t n_devices) {
  SG_GUARD_BEGIN
  if (!ix || (!devices && n_devices)) { set_error("null argument"); return SG_E_INVALID; }
  for (uint32_t i = 0; i < n_devices; i++) {
    uint32_t nth = 0;                                       // a device named j times ends up with j replicas
    for (uint32_t j = 0; j < i; j++) nth += devices[j] == devices[i];
    if (find_replica(ix, devices[i], nth)) continue;
    const int rc = add_replica(ix, devices[i]);
    if (rc) return rc;
  }
  return SG_OK;
  SG_GUARD_END(SG_RC)
}

uint32_t sg_index_replicas(sg_index* ix, int* out_devices, uint32_t cap) {
  if (!ix) return 0;
  std::lock_guard<std::mutex> lock(ix->mu);
  for (size_t i = 0; i < ix->replicas.size() && i < cap; i++) out_devices[i] = ix->replicas[i]->device;
  return (uint32_t)ix->replicas.size();
}

// [r6] Test hook: where replica number `replica` of the index lives, array by array — out[0] the replica's device ordinal, then the
// device hipPointerGetAttributes reports for its posting store, seg_off, orig_of, forward-index records and terms, term table and
// counter block (-1: null / not device memory).  Every array of a replica must sit on the replica's own device: a launch that
// took another replica's pointer would run on the wrong GPU's memory over xGMI — or fault — without any row telling.
int sg_debug_replica_devices(sg_index* ix, uint32_t replica, int32_t out[8]) {
  SG_GUARD_BEGIN
  if (!ix || !out) { set_error("null argument"); return SG_E_INVALID; }
  Replica* r = nullptr;
  { std::lock_guard<std::mutex> lock(ix->mu); if (replica < ix->replicas.size()) r = ix->replicas[replica].get(); }
  if (!r) { set_error("no such replica"); return SG_E_INVALID; }
  const void* ptrs[7] = {r->dix.postings, r->dix.seg_off, r->dix.orig_of, r->dix.fwd_rec, r->dix.fwd_terms, r->dix.slots, r->d_fill};
  out[0] = r->device;
  for (int i = 0; i < 7; i++) {
    out[1 + i] = -1;
    if (!ptrs[i]) continue;
    hipPointerAttribute_t at;
    if (hipPointerGetAttributes(&at, ptrs[i]) == hipSuccess && at.type == hipMemoryTypeDevice) out[1 + i] = at.device;
    else (void)hipGetLastError();
  }
  return SG_OK;
  SG_GUARD_END(SG_RC)
}

// Test hook: one array of replica number `replica` as it lies in HBM, undecoded (tests/packed_ref.py holds the second statement of
// the formats and compares), or one of the two host CSR arrays everything on the device is derived from.  `which`: 0 the packed
// chunks + the slack row, 1 the packed seg_off (bit-31 flags as stored), 2 orig_of, 3 x_of, 4 seg_base (S + 1), 5 cut_sample,
// 6 fwd_rec, 7 fwd_terms, 8 fx_base (0 bytes when null), 9 / 10 the host CSR's postings / seg_off (no replica, no GPU needed).
// *out_bytes = the array's size; it is copied when `out` is not null (cap_bytes below the size: SG_E_INVALID).  Reads only.
int sg_debug_index_array(sg_index* ix, uint32_t replica, uint32_t which, void* out, uint64_t cap_bytes, uint64_t* out_bytes) {
  SG_GUARD_BEGIN
  if (!ix || !out_bytes) { set_error("null argument"); return SG_E_INVALID; }
  const HostIndex& h = ix->host;
  const void* src = nullptr;
  uint64_t bytes = 0;
  Replica* r = nullptr;
  if (which == 9u) { src = h.postings.data(); bytes = (uint64_t)h.postings.size() * 4; }
  else if (which == 10u) { src = h.seg_off.data(); bytes = (uint64_t)h.seg_off.size() * 4; }
  else if (which > 10u) { set_error("sg_debug_index_array: unknown array"); return SG_E_INVALID; }
  else {
    { std::lock_guard<std::mutex> lock(ix->mu); if (replica < ix->replicas.size()) r = ix->replicas[replica].get(); }
    if (!r) { set_error("sg_debug_index_array: index not uploaded / no such replica"); return SG_E_INVALID; }
    const DeviceIndex& d = r->dix;
    const uint64_t n_docs = d.n_docs, S = d.S;
    switch (which) {
      case 0: src = d.postings; bytes = (r->packed_chunks + 64) * 16; break;
      case 1: src = d.seg_off; bytes = (uint64_t)d.n_terms * (S + 1) * 4; break;
      case 2: src = d.orig_of; bytes = n_docs * 4; break;
      case 3: src = r->x_of; bytes = n_docs * 4; break;
      case 4: src = d.seg_base; bytes = (S + 1) * 4; break;
      case 5: src = d.cut_sample; bytes = ~0ull; break;          // (as long as it was allocated)
      case 6: src = d.fwd_rec; bytes = n_docs * 8; break;
      case 7: src = d.fwd_terms; bytes = ~0ull; break;           // (the same: a whole number of 16-byte chunks)
      default: src = d.fx_base; bytes = src ? (S + 1) * 4 : 0; break;
    }
    if (bytes) {    // every array is one block of the replica: never read past what it was allocated with
      const uint64_t have = r->mem.bytes_of(src);
      if (bytes == ~0ull) bytes = have;
      if (!src || bytes > have) { set_error("sg_debug_index_array: the array is not an allocation of the replica"); return SG_E_INVALID; }
    }
  }
  *out_bytes = bytes;
  if (!out || !bytes) return SG_OK;
  if (cap_bytes < bytes) { set_error("sg_debug_index_array: buffer too small"); return SG_E_INVALID; }
  if (!r) { memcpy(out, src, (size_t)bytes); return SG_OK; }
  DeviceGuard dg;
  HIP_TRY(dg.set(r->device));
  HIP_TRY(hipMemcpy(out, src, (size_t)bytes, hipMemcpyDeviceToHost));
  return SG_OK;
  SG_GUARD_END(SG_RC)
}

// Sets a knob of the table (knobs.inc), before or after the first upload.  Results never depend on the knobs; not synchronised with
// launches in flight (a tool for sweeps, tools/sweep_knobs.py).
int sg_index_tune(sg_index* ix, const char* knob, int value) {
  SG_GUARD_BEGIN
  if (!ix || !knob) { set_error("null argument"); return SG_E_INVALID; }
  for (const KnobRow& row : kKnobs) if (!strcmp(row.name, knob)) return set_knob(ix->knobs, row, value, KNOB_TUNE);
  set_error(std::string("unknown knob: ") + knob); return SG_E_INVALID;
  SG_GUARD_END(SG_RC)
}

// The forward index of the primary replica, copied back for `n` documents starting at `first` (tests): out_card[i] = the
// document's cardinality, out_n[i] = its distinct terms, out_keys[i * cap ..] = their packed term keys (any order).
int sg_index_forward(sg_index* ix, uint32_t first, uint32_t n, uint32_t cap, uint32_t* out_card, uint32_t* out_n, uint64_t* out_keys) {
  SG_GUARD_BEGIN
  Replica* r = ix ? find_replica(ix, -1) : nullptr;
  if (!r || !out_card || !out_n || !out_keys) { set_error("index not uploaded / null argument"); return SG_E_INVALID; }
  if ((uint64_t)first + n > ix->host.n_docs) { set_error("document range outside the dictionary"); return SG_E_INVALID; }
  HIP_TRY(hipSetDevice(r->device));
  std::vector<uint2> rec(n);                                    // (the records are kept in the packed store's numbering)
  std::vector<uint32_t> xs(n);
  if (n) HIP_TRY(hipMemcpy(xs.data(), r->x_of + first, (size_t)n * 4, hipMemcpyDeviceToHost));
  for (uint32_t i = 0; i < n; i++) HIP_TRY(hipMemcpy(&rec[i], r->dix.fwd_rec + xs[i], 8, hipMemcpyDeviceToHost));
  std::vector<uint32_t> terms;
  for (uint32_t i = 0; i < n; i++) {
    const uint32_t nd = rec[i].y >> 16;
    out_card[i] = rec[i].y & 0xFFFFu; out_n[i] = nd;
    terms.resize(nd);
    if (nd) HIP_TRY(hipMemcpy(terms.data(), r->dix.fwd_terms + (uint64_t)rec[i].x * 4, (size_t)nd * 4, hipMemcpyDeviceToHost));
    for (uint32_t j = 0; j < nd && j < cap; j++) out_keys[(size_t)i * cap + j] = terms[j] < ix->host.term_key.size() ? ix->host.term_key[terms[j]] : ~0ull;
  }
  return SG_OK;
  SG_GUARD_END(SG_RC)
}

void sg_index_retain(sg_index* ix) { if (ix) ix->refs.fetch_add(1); }
void sg_index_release(sg_index* ix) {
  if (!ix) return;
  if (ix->refs.fetch_sub(1) != 1) return;
  if (ix->coalescer) coalescer_stop(ix->coalescer);
  if (ix->multi) multi_pool_stop(ix->multi);
  delete ix;                                               // the replicas free their HBM
}

// the replica a device-pointer call runs on: the one on the device that owns the caller's buffers
static Replica* replica_of_pointer(sg_index* index, const void* d_ptr) {
  { std::lock_guard<std::mutex> lock(index->mu); if (index->replicas.size() == 1) return index->replicas[0].get(); }
  hipPointerAttribute_t at;
  if (d_ptr && hipPointerGetAttributes(&at, d_ptr) == hipSuccess) {
    Replica* r = find_replica(index, at.device);
    if (r) return r;
  } else (void)hipGetLastError();
  return find_replica(index, -1);
}

int sg_suggest_batch_device(sg_index* index, const void* d_q, const void* d_offs, uint32_t n_q, int metric,
                            double similarity, uint32_t k, void* d_ids, void* d_scores, void* d_counts, void* stream) {
  SG_GUARD_BEGIN
  if (int rc = open_search(index, fuzzy_key(metric, similarity, k), true, {})) return rc;
  LaunchReq r;
  r.q = d_q; r.offs = d_offs; r.n_q = n_q; r.metric = metric; r.similarity = similarity; r.k = k;
  r.ids = d_ids; r.scores = d_scores; r.counts = d_counts; r.stream = (hipStream_t)stream;
  return launch(index, replica_of_pointer(index, d_offs), r);
  SG_GUARD_END(SG_RC)
}

int sg_autocomplete_batch_device(sg_index* index, const void* d_q, const void* d_offs, uint32_t n_q, uint32_t limit,
                                 void* d_ids, void* d_counts, void* stream) {
  SG_GUARD_BEGIN
  if (int rc = open_search(index, prefix_key(limit), false, {})) return rc;
  LaunchReq r;
  r.q = d_q; r.offs = d_offs; r.n_q = n_q; r.k = limit; r.autocomplete = 1;
  r.ids = d_ids; r.counts = d_counts; r.stream = (hipStream_t)stream;
  return launch(index, replica_of_pointer(index, d_offs), r);
  SG_GUARD_END(SG_RC)
}
}  // extern "C"
