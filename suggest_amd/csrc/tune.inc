// tune.inc — the tuner: tune_choice, the stream workgroup's shape model, tune_index, and add_replica (the upload of one replica,
// which tunes first).  Uses handles.inc, knobs.inc, and the builders of index_build.inc, forward_index.inc and packed_store.inc.

namespace {

// The choices tune_index() derives from an index's two statistics — the expected posting volume of a query (16-byte chunks of
// u32 postings: size-biased mean term length x terms per document) and the longest term — in one place, so that a test can
// hold them against the dictionaries they were measured on (tests/test_capi_cpu.py::test_tuner_choices_are_pinned;
// sg_debug_tune_choice).  Rounds 2-3 shipped the wrong filter table for three regimes without anybody noticing.
struct TuneChoice { uint32_t log2_cnt, filter_level; int pipe_pays; uint32_t pipe_nw, pipe_log2_cnt, pipe_dt_bytes; };
TuneChoice tune_choice(double est_query_chunks, double max_term_chunks) {
  TuneChoice c{11u, 4u, 0, 8u, 13u, 8192u};
  // [r4] The counter array.  Long-list indexes (megabytes of postings per query) run mostly docID-range passes, and 2^12
  // words halve the passes — but cost the wavefronts: 7 per CU instead of 12.  Swept on the final round-3 kernel
  // (profiles/r04o_sweep_*, r04p_sweep_*): a uniform bigram index (q = 2, 10 M strings: every term about as long as any
  // other) does best at 2^11 — 20.0 ms per 16 384 queries against 24.3 at 2^12 and 33.8 at 2^13; an index whose longest
  // terms are as heavy as a typical query's whole volume (Zipf symbols: a few lists of millions of postings, met by a
  // minority of the queries, which then set the launch's tail) does best at 2^12 ... 2^13 (28.4 / 27.0 ms against 34.8 at
  // 2^11).  So: 2^12 where the longest term holds more than a quarter of the expected query volume, else 2^11.
  // (Rounds 2-3 took 2^12 for every index above 2 MiB per query: cfg 4 paid 30 % for it.)
  if (est_query_chunks > 131072.0 && max_term_chunks > 0.25 * est_query_chunks) c.log2_cnt = 12;
  // [r4] The filter level.  The loose per-posting table (level 4) is right for every index above a few thousand chunks
  // per query — long-list ones included: since verification is one forward-index read (round 2) and the queue takes
  // whatever comes (round 3), q = 2 on 10 M strings runs 20.0 ms at level 4 against 22.7 at level 2 (same counter array),
  // the Zipf dictionary 28.4 against 39.2.  (The strict table was chosen for them in round 2, when a false candidate
  // cost a binary search per query term: level 2 0.41 M q/s, level 4 0.39 then.)
  // Small dictionaries of real words (the reference's cars / words: a few thousand chunks per query, and n-gram lists as
  // uneven as a language's — the longest term holds a third to two thirds of a query's volume) merge their few postings
  // into large groups either way; with the loose table they also skip deeper and flag every matching document — they
  // have many per query — in more of its lists: words Jaccard k=10 56.8 M q/s at level 2, 31.8 at level 4
  // (profiles/r04q_small_dictionaries_levels.txt).  A small dictionary of UNIFORM strings (1 M synthetic strings: the
  // longest term a tenth of a query's volume, 0.9 results per query) is the headline in small and takes the loose table
  // like it: cfg 2 0.585 ms per 65 536 queries at level 4, 0.648 at level 2 (profiles/r04q_sweep_cfg2.txt).
  const bool small_uneven = est_query_chunks < 8192.0 && max_term_chunks > 0.25 * est_query_chunks;
  if (small_uneven) c.filter_level = 2;
  // [r5] plan -> stream -> verify pays wherever its stream workgroup has the size of the queries' streams: for 10 M strings
  // (21 500 chunks a query) eight wavefronts on 2^13 counters, four workgroups a CU (+15 % over the fused kernel); a query of a
  // 1 M dictionary streams 15 rows — less than two per wavefront of such a workgroup, whose launch then is a chain of memory
  // round trips (slot record, descriptors, first row) that four workgroups a CU cannot hide (parity with the fused kernel).  Two
  // wavefronts on 2^11 counters and 2 KB of descriptors are 10 KB of LDS: sixteen workgroups a CU, 145 M q/s against 108
  // (60 k ... 2 M strings: +95 % ... +43 %; profiles/r05zj_*).  In between (4 M strings), four wavefronts on 2^12.
  // Not where the queries are split / streamed in docID-range passes anyway (long-list indexes, above 131 072: the plan hands
  // those back), nor for the small dictionaries of real words (the reference's word lists, Predict's vocabulary: many results
  // per query, their candidates overflow the slots).
  c.pipe_pays = est_query_chunks <= 131072.0 && !small_uneven;
  if (est_query_chunks < 6000.0) { c.pipe_nw = 2u; c.pipe_log2_cnt = 11u; c.pipe_dt_bytes = 2048u; }
  else if (est_query_chunks < 14000.0) { c.pipe_nw = 4u; c.pipe_log2_cnt = 12u; c.pipe_dt_bytes = 4096u; }
  return c;
}

// The statistics the tuner and the launch plans go by: a query term is a dictionary term drawn by occurrence, so the expected list
// length is size-biased — E[list length] = sum len^2 / sum len.
void index_statistics(sg_index* ix) {
  const HostIndex& h = ix->host;
  const size_t S = h.n_segments, nt = h.term_key.size();
  double s1 = 0, s2 = 0;
  for (size_t t = 0; t < nt; t++) {
    const double len = (double)(h.seg_off[t * (S + 1) + S] - h.seg_off[t * (S + 1)]);
    s1 += len; s2 += len * len;
    ix->max_term_chunks = std::max(ix->max_term_chunks, len);
  }
  ix->terms_per_doc = h.n_docs ? (double)h.n_postings_raw / (double)h.n_docs : 0.0;
  ix->est_query_chunks = s1 > 0 ? ix->terms_per_doc * s2 / s1 : 0.0;
}

// Once per index, at its first upload (caller holds ix->mu): the statistics, the environment's knobs, then the tuner's choice for
// every knob it may choose that nobody set explicitly.  A value the table refuses fails the upload and leaves the index untuned.
int tune_index(sg_index* ix) {
  if (ix->tuned) return SG_OK;
  index_statistics(ix);
  Knobs k = ix->knobs;                       // (a copy: nothing half-set reaches the index when a value is refused)
  for (const KnobRow& row : kKnobs) {
    int32_t v = 0;
    const char* e = getenv(row.name);
    if (!e || !*e) continue;                 // (an empty variable counts as not set)
    if ((row.flags & KNOB_ENV) && !parse_int32(e, &v)) return knob_refused(row, std::string("=") + e + ": not an integer");
    if (const int rc = set_knob(k, row, v, KNOB_ENV)) return rc;
  }
  const TuneChoice c = tune_choice(ix->est_query_chunks, ix->max_term_chunks);
  Knobs t = k;   // (the choice as knobs: taken where the row lets the tuner choose and nobody chose before it)
  t.log2_cnt = c.log2_cnt; t.filter_level = c.filter_level; t.pipe_nw = c.pipe_nw; t.pipe_log2_cnt = c.pipe_log2_cnt; t.pipe_dt_bytes = c.pipe_dt_bytes;
  for (uint32_t i = 0; i < kNumKnobs; i++)
    if ((kKnobs[i].flags & KNOB_TUNER) && !((k.explicit_set >> i) & 1u)) k.*kKnobs[i].field = t.*kKnobs[i].field;
  ix->knobs = k; ix->pipe_pays = c.pipe_pays != 0; ix->tuned = true;
  if (env_int("SG_VERBOSE", 0, 1, 0)) fprintf(stderr, "[suggest_hip] terms/doc %.2f, expected query volume %.0f chunks, longest term %.0f chunks\n", ix->terms_per_doc, ix->est_query_chunks, ix->max_term_chunks);
  return SG_OK;
}

// Fills a replica on `device` (caller holds ix->mu).  `r` may already own the u32 posting store and seg_off (device build).
int fill_replica(sg_index* ix, Replica* r, int device) {
  HIP_TRY(hipSetDevice(device));
  r->device = device;
  { int cus = 0; if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, device) == hipSuccess && cus > 0) r->n_cus = cus; }
  const HostIndex& h = ix->host;
  DeviceIndex& d = r->dix;
  int rc;
  // the u32 CSR goes up (or is already there), the forward index is derived from it, then the store is packed and the u32
  // arrays are freed (packed_store.inc): what stays resident is ~0.57x the u32 store + the forward index
  if (!d.postings && (rc = r->mem.upload(h.postings, &d.postings))) return rc;
  if (!d.seg_off && (rc = r->mem.upload(h.seg_off, &d.seg_off))) return rc;
  if ((rc = build_forward_index(h, r))) return rc;
  if ((rc = pack_store(h, r, ix->knobs.g8))) return rc;
  {  // long-query working memory: sized by the largest cardinality segment (one counter per document of a segment)
    std::vector<uint32_t> sb((size_t)h.n_segments + 1, 0);
    HIP_TRY(hipMemcpy(sb.data(), d.seg_base, sb.size() * 4, hipMemcpyDeviceToHost));
    uint32_t max_seg = 0;
    for (size_t b = 0; b + 1 < sb.size(); b++) max_seg = std::max(max_seg, sb[b + 1] - sb[b]);
    r->long_max_seg = max_seg;
    r->long_slot_bytes = LongSlot::bytes(max_seg);
    if (!env_int("SG_NO_LONG_QUERIES", 0, 1, 0)) {
      if ((rc = r->mem.alloc(&r->long_scratch, (size_t)(r->long_slot_bytes * SG_LONG_SLOTS)))) return rc;
      if ((rc = r->mem.alloc(&r->long_lock, (size_t)SG_LONG_SLOTS + 4))) return rc;
      HIP_TRY(hipMemset(r->long_lock, 0, (SG_LONG_SLOTS + 4) * 4));
    }
  }
  if ((rc = r->mem.upload(h.slots, &d.slots))) return rc;
  if ((rc = upload_description(h, r->mem, d))) return rc;
  if ((rc = r->mem.alloc(&r->d_fill, (size_t)SG_STAT_WORDS))) return rc;     // the statistics block (StatWord: the 64-bit chunk counter 8-byte aligned)
  HIP_TRY(hipMemset(r->d_fill, 0, SG_STAT_WORDS * 4));
  HIP_TRY(hipHostMalloc((void**)&r->h_fill, SG_STAT_WORDS * 4, hipHostMallocMapped));
  for (int i = 0; i < SG_STAT_WORDS; i++) r->h_fill[i] = 0;
  HIP_TRY(hipHostGetDevicePointer((void**)&r->h_fill_dev, r->h_fill, 0));
  if (!h.dups.empty()) {   // documents that repeat a term: side tables for the secondary-entry path
    const uint32_t S32 = h.n_segments;
    std::vector<uint32_t> dts, ddoc, dmult, ddocs, ets, ecnt;
    for (const auto& e : h.dups) {
      const uint32_t ts = e.term * S32 + e.segment;
      // doc == 0xFFFFFFFF: a roaring list of a reference-built index that dropped its repeats (ref_index_reader.cpp) —
      // only the raw-length surplus is known, no document: it feeds extra_ts / extra_cnt alone
      if (e.doc != 0xFFFFFFFFu) { dts.push_back(ts); ddoc.push_back(e.doc); dmult.push_back(e.mult); ddocs.push_back(e.doc); }
      if (!ets.empty() && ets.back() == ts) ecnt.back() += e.mult - 1; else { ets.push_back(ts); ecnt.push_back(e.mult - 1); }
    }
    std::sort(ddocs.begin(), ddocs.end());
    ddocs.erase(std::unique(ddocs.begin(), ddocs.end()), ddocs.end());
    if ((rc = r->mem.upload(dts, &d.dup_ts))) return rc;
    if ((rc = r->mem.upload(ddoc, &d.dup_doc))) return rc;
    if ((rc = r->mem.upload(dmult, &d.dup_mult))) return rc;
    if ((rc = r->mem.upload(ddocs, &d.dup_docs))) return rc;
    std::vector<uint32_t> dbits((size_t)(h.n_docs + 31) / 32 + 1, 0u);
    for (uint32_t dd : ddocs) if ((size_t)(dd >> 5) < dbits.size()) dbits[dd >> 5] |= 1u << (dd & 31u);
    if ((rc = r->mem.upload(dbits, &d.dup_bits))) return rc;
    if ((rc = r->mem.upload(ets, &d.extra_ts))) return rc;
    if ((rc = r->mem.upload(ecnt, &d.extra_cnt))) return rc;
    if ((rc = r->mem.upload(h.list_len, &d.list_len))) return rc;
    d.n_dups = (uint32_t)dts.size(); d.n_dup_docs = (uint32_t)ddocs.size(); d.n_extra = (uint32_t)ets.size();
  }
  d.slot_mask = (uint32_t)h.slots.size() - 1;
  d.S = h.n_segments;
  d.n_docs = (uint32_t)h.n_docs;
  d.n_terms = (uint32_t)h.term_key.size();
  // (the attribute belongs to the function, not to the index: always the largest size any index may ask for)
  HIP_TRY(hipFuncSetAttribute((const void*)sg_parts_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_bytes(14, SG_K_LDS, true)));
  HIP_TRY(hipFuncSetAttribute((const void*)sg_lm_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_bytes(14, SG_K_LDS, true)));
  HIP_TRY(hipFuncSetAttribute((const void*)sg_search_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_bytes(14, SG_K_LDS, true)));
  HIP_TRY(hipFuncSetAttribute((const void*)sg_search_kernel_loop, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_bytes(14, SG_K_LDS, true)));
  HIP_TRY(hipFuncSetAttribute((const void*)sg_search_kernel_tight, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_bytes(14, SG_K_LDS, true)));
  HIP_TRY(hipFuncSetAttribute((const void*)sg_search_kernel_slim, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_bytes(14, SG_K_LDS, true)));
  HIP_TRY(hipFuncSetAttribute((const void*)sg_lm_kernel_slim, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_bytes(14, SG_K_LDS, true)));
  HIP_TRY(hipFuncSetAttribute((const void*)sg_parts_kernel_tight, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_bytes(14, SG_K_LDS, true)));
  HIP_TRY(hipFuncSetAttribute((const void*)sg_search_kernel_g8, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_bytes(14, SG_K_LDS, true)));
  HIP_TRY(hipFuncSetAttribute((const void*)sg_search_kernel_tight_g8, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_bytes(14, SG_K_LDS, true)));
  HIP_TRY(hipFuncSetAttribute((const void*)sg_parts_kernel_g8, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_bytes(14, SG_K_LDS, true)));
  HIP_TRY(hipFuncSetAttribute((const void*)sg_parts_kernel_tight_g8, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_bytes(14, SG_K_LDS, true)));
  HIP_TRY(hipFuncSetAttribute((const void*)sg_lm_kernel_g8, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_bytes(14, SG_K_LDS, true)));
  HIP_TRY(hipDeviceSynchronize());
  return SG_OK;
}

// One more replica on `device` (any number per device: a second one on the same GPU is only useful for exercising the
// multi-replica paths on a one-GPU box).
int add_replica(sg_index* ix, int device) {
  int n_dev = 0;
  HIP_TRY(hipGetDeviceCount(&n_dev));
  if (device < 0 || device >= n_dev) { set_error("no such device"); return SG_E_INVALID; }
  int prev = -1;
  (void)hipGetDevice(&prev);
  std::lock_guard<std::mutex> lock(ix->mu);
  if (const int rc = tune_index(ix)) return rc;   // (a knob the environment sets out of range: before anything is allocated)
  std::unique_ptr<Replica> r;
  if (ix->prebuilt && ix->prebuilt->device == device) r = std::move(ix->prebuilt);
  else r.reset(new Replica());
  ix->prebuilt.reset();                                  // a device build's arrays serve the first upload only
  const int rc = fill_replica(ix, r.get(), device);       // on failure `r` frees what it had allocated
  if (prev >= 0) (void)hipSetDevice(prev);
  if (rc) return rc;
  if (ix->replicas.empty()) ix->device = device;
  ix->replicas.push_back(std::move(r));
  ix->uploaded.store(true, std::memory_order_release);
  return SG_OK;
}

}  // namespace
