// lm_api.inc — the language model's C API: load, build, store and query entry points, the model's upload, SpellChecker.Predict
// (predict_on_device and its two calls) and batch sentence scoring.  Uses handles.inc (sg_lm), capi.inc, host_call.inc,
// lm_build.inc and lm_score.inc.

extern "C" {
// ------------------------------------------------------------------------------------------
// language model + SpellChecker.Predict (SURVEY.md §8f-3)
// ------------------------------------------------------------------------------------------
static int lm_load_any(const char* a, const char* b, uint32_t order, const char* start_symbol, const char* end_symbol, const char* const* alphabet,
                       uint32_t n_alphabet, int mode, sg_lm** out) {
  SG_GUARD_BEGIN
  if (!a || !out || (mode == 2 && !b)) { set_error("null argument"); return SG_E_INVALID; }
  std::unique_ptr<sg_lm> lm(new (std::nothrow) sg_lm());
  if (!lm) return SG_E_NOMEM;
  std::vector<std::string> alpha;
  for (uint32_t i = 0; i < n_alphabet; i++) alpha.emplace_back(alphabet[i]);
  std::string err;
  const int rc = mode == 2 ? lm_load_binary(a, b, start_symbol, end_symbol, alpha, lm->host, err)
                           : lm_load_google(a, order, start_symbol, end_symbol, alpha, mode, lm->host, err);
  if (rc) { set_error(err); return rc; }
  *out = lm.release();
  return SG_OK;
  SG_GUARD_END(SG_RC)
}

int sg_lm_load_google(const char* dir, uint32_t order, const char* start_symbol, const char* end_symbol, const char* const* alphabet,
                      uint32_t n_alphabet, sg_lm** out) {
  return lm_load_any(dir, nullptr, order, start_symbol, end_symbol, alphabet, n_alphabet, 0, out);
}

int sg_lm_load_google_ex(const char* dir, uint32_t order, const char* start_symbol, const char* end_symbol, const char* const* alphabet,
                         uint32_t n_alphabet, int id_order, sg_lm** out) {
  if (id_order != 0 && id_order != 1) { set_error("id_order is 0 (1-gm line order) or 1 (count desc, word asc)"); return SG_E_INVALID; }
  return lm_load_any(dir, nullptr, order, start_symbol, end_symbol, alphabet, n_alphabet, id_order, out);
}

int sg_lm_load_binary(const char* lm_path, const char* cdb_path, const char* start_symbol, const char* end_symbol, const char* const* alphabet,
                      uint32_t n_alphabet, sg_lm** out) {
  return lm_load_any(lm_path, cdb_path, 0, start_symbol, end_symbol, alphabet, n_alphabet, 2, out);
}

int sg_lm_level(const sg_lm* lm, uint32_t level, uint64_t* containers, uint32_t cap_containers, uint32_t* n_containers, uint64_t* values,
                uint32_t cap_values, uint32_t* n_values, uint32_t* total) {
  SG_GUARD_BEGIN
  if (!lm || level >= lm->host.level.size() || !n_containers || !n_values || !total) { set_error("bad argument"); return SG_E_INVALID; }
  std::vector<uint64_t> c, v;
  lm_level_packed(lm->host, level, c, v, total);
  *n_containers = (uint32_t)c.size(); *n_values = (uint32_t)v.size();
  if (containers) memcpy(containers, c.data(), std::min<size_t>(c.size(), cap_containers) * 8);
  if (values) memcpy(values, v.data(), std::min<size_t>(v.size(), cap_values) * 8);
  return SG_OK;
  SG_GUARD_END(SG_RC)
}

uint32_t sg_lm_order(const sg_lm* lm) { return lm ? lm->host.order : 0u; }

int sg_lm_build_google(const uint8_t* text, uint64_t len, uint32_t order, const char* start_symbol, const char* end_symbol,
                       const char* const* alphabet, uint32_t n_alphabet, const char* const* separators, uint32_t n_separators,
                       const char* out_dir) {
  if ((!text && len) || !start_symbol || !end_symbol || !out_dir) { set_error("null argument"); return SG_E_INVALID; }
  std::vector<std::string> alpha, seps;
  for (uint32_t i = 0; i < n_alphabet; i++) alpha.emplace_back(alphabet[i]);
  for (uint32_t i = 0; i < n_separators; i++) seps.emplace_back(separators[i]);
  std::string err;
  const int rc = lm_build_google_files(text, (size_t)len, order, start_symbol, end_symbol, alpha, seps, out_dir, err);
  if (rc) set_error(err);
  return rc;
}

int sg_lm_build_device(const uint8_t* text, uint64_t len, uint32_t order, const char* start_symbol, const char* end_symbol,
                       const char* const* alphabet, uint32_t n_alphabet, const char* const* separators, uint32_t n_separators,
                       int id_order, int device, sg_lm** out) {
  SG_GUARD_BEGIN
  if ((!text && len) || !start_symbol || !end_symbol || !out || (n_alphabet && !alphabet) || (n_separators && !separators)) { set_error("null argument"); return SG_E_INVALID; }
  if (order < 1 || order > 8) { set_error("nGramOrder should be 1 .. 8"); return SG_E_INVALID; }
  if (id_order != 0 && id_order != 1) { set_error("id_order is 0 (first appearance) or 1 (count desc, word asc)"); return SG_E_INVALID; }
  for (const char* sym : {start_symbol, end_symbol}) {           // (what the Google files between builder and loader could not carry either)
    if (!*sym) { set_error("the start and end symbols must not be empty"); return SG_E_INVALID; }
    if (strpbrk(sym, " \t\n")) { set_error("the start and end symbols must not contain a space, tab or newline"); return SG_E_INVALID; }
  }
  if (len > ((uint64_t)1 << 30)) { set_error("corpus above 1 GiB: beyond the device builder"); return SG_E_UNSUPPORTED; }
  std::unique_ptr<sg_lm> lm(new (std::nothrow) sg_lm());
  if (!lm) { set_error("out of host memory"); return SG_E_NOMEM; }
  HostLM& h = lm->host;
  std::vector<std::string> seps;
  for (uint32_t i = 0; i < n_alphabet; i++) h.alphabet.emplace_back(alphabet[i]);
  for (uint32_t i = 0; i < n_separators; i++) seps.emplace_back(separators[i]);
  if (host_alphabet_has(h.alphabet, ' ')) { set_error("an alphabet with U+0020 is beyond the device builder (the tokeniser trims it)"); return SG_E_UNSUPPORTED; }
  h.order = order;
  if (len == 0) lm_build_empty(h, order);
  else if (int rc = lm_build_on_device(text, len, order, start_symbol, end_symbol, seps, id_order, device, h)) return rc;
  h.start_symbol = lm_word_id(h, start_symbol);
  h.end_symbol = lm_word_id(h, end_symbol);
  *out = lm.release();
  return SG_OK;
  SG_GUARD_END(SG_RC)
}

int sg_lm_store_binary_ex(const sg_lm* lm, const char* lm_path, const char* cdb_path, uint32_t flags) {
  SG_GUARD_BEGIN
  if (!lm || !lm_path || !cdb_path) { set_error("null argument"); return SG_E_INVALID; }
  if (flags & ~(uint32_t)SG_LM_STORE_MPH) { set_error("unknown flag: SG_LM_STORE_MPH is the only one"); return SG_E_INVALID; }
  std::string err;
  const int rc = lm_store_binary(lm->host, lm_path, cdb_path, flags, err);
  if (rc) set_error(err);
  return rc;
  SG_GUARD_END(SG_RC)
}

int sg_lm_store_binary(const sg_lm* lm, const char* lm_path, const char* cdb_path) { return sg_lm_store_binary_ex(lm, lm_path, cdb_path, 0); }

int sg_debug_lm_build_hash_bits(uint32_t bits) {
  if (bits > 64u) { set_error("hash bits: 0 (all 64) .. 64"); return SG_E_INVALID; }
  g_lm_build_hash_bits.store(bits, std::memory_order_relaxed);
  return SG_OK;
}

void sg_lm_retain(sg_lm* lm) { if (lm) lm->refs.fetch_add(1); }
void sg_lm_release(sg_lm* lm) {
  if (!lm || lm->refs.fetch_sub(1) != 1) return;
  delete lm;
}
uint32_t sg_lm_num_words(const sg_lm* lm) { return lm ? (uint32_t)lm->host.words.size() : 0u; }
int sg_lm_word(const sg_lm* lm, uint32_t id, char* out, uint32_t cap) {
  if (!lm || id >= lm->host.words.size()) { set_error("no such word id"); return SG_E_INVALID; }
  const std::string& w = lm->host.words[id];
  if (w.size() <= cap) memcpy(out, w.data(), w.size());
  return (int)w.size();
}
uint32_t sg_lm_word_id(const sg_lm* lm, const uint8_t* word, uint32_t len) {
  return lm ? lm_word_id(lm->host, std::string((const char*)word, len)) : kUnknownWord;
}
double sg_lm_score(const sg_lm* lm, const uint32_t* ids, uint32_t n) { return lm_model_score(lm->host, ids, n); }
double sg_lm_score_word_ids(const sg_lm* lm, const uint32_t* ids, uint32_t n) { return lm_score_word_ids(lm->host, ids, n); }
int sg_lm_next_score(const sg_lm* lm, const uint32_t* context, uint32_t n, uint32_t word, int model_level, double* score) {
  const LmNext nx = model_level ? lm_model_next(lm->host, context, n) : lm_next(lm->host, context, n);
  if (score) *score = nx.status ? 0.0 : lm_next_score(lm->host, nx, word);
  return nx.status;
}
int sg_lm_tokenize(const sg_lm* lm, const uint8_t* text, uint32_t len, char* out, uint32_t cap) {
  std::vector<std::string> toks;
  lm_tokenize(lm->host, text, len, toks);
  std::string joined;
  for (size_t i = 0; i < toks.size(); i++) { if (i) joined.push_back('\n'); joined += toks[i]; }
  if (joined.size() < cap) { memcpy(out, joined.data(), joined.size()); out[joined.size()] = 0; }
  return (int)toks.size();
}

int sg_spell_index_build(const sg_lm* lm, const sg_desc* desc, int device, sg_index** out) {
  if (!lm || !out) { set_error("null argument"); return SG_E_INVALID; }
  std::string blob;
  std::vector<uint64_t> offs(1, 0);
  for (const auto& w : lm->host.words) { blob += w; offs.push_back(blob.size()); }   // docID = word id
  int rc = sg_index_build((const uint8_t*)blob.data(), offs.data(), (uint32_t)lm->host.words.size(), desc, out);
  if (rc) return rc;
  rc = sg_index_upload(*out, device);
  if (rc) { sg_index_release(*out); *out = nullptr; return rc; }
  // A vocabulary is short documents (3 .. 12 n-grams) searched at low thresholds (T = 3 .. 5): with the strict bucket table
  // the fuzzy top-up ran 6.7 groups per query, each a chain of dependent round trips; the looser table halves them
  // (BASELINE config 5: 1.88 -> 1.70 ms per Predict step, profiles/r04c_spell_sweep.txt).  SG_FILTER_LEVEL still overrides.
  if (!knob_is_explicit((*out)->knobs, &Knobs::filter_level)) (*out)->knobs.filter_level = 4;
  return rc;
}

static int lm_upload(sg_lm* lm, int device) {
  std::lock_guard<std::mutex> lock(lm->mu);
  if (lm->d_values) {
    if (lm->device != device) { set_error("language model already resident on another device"); return SG_E_INVALID; }
    return SG_OK;
  }
  // (built into locals and a local DeviceBlock, committed to the handle only when every step has succeeded: a failed
  //  upload leaks nothing and a retry starts from a clean handle; the caller's current device is restored)
  std::vector<uint64_t> flat;
  std::vector<uint32_t> cb, level_base, cb_base;
  for (const LmLevel& lv : lm->host.level) {
    level_base.push_back((uint32_t)flat.size());
    cb_base.push_back((uint32_t)cb.size());
    for (size_t i = 0; i < lv.word.size(); i++) flat.push_back(((uint64_t)lv.word[i] << 32) | lv.count[i]);
    cb.insert(cb.end(), lv.child_begin.begin(), lv.child_begin.end());
  }
  if (flat.size() >= 0xFFFFFFF0ull) { set_error("language model too large"); return SG_E_UNSUPPORTED; }
  DeviceGuard dg;
  HIP_TRY(dg.set(device));
  DeviceBlock mem;                                   // the device blocks of an upload in progress
  int rc;
  const uint64_t* p = nullptr;
  const uint32_t* q = nullptr;
  if ((rc = mem.upload(flat, &p)) || (rc = mem.upload(cb, &q))) return rc;
  {  // the word tokeniser's tables: alphabet membership (bitmap below 128, inclusive ranges above) ...
    const HostLM& h = lm->host;
    std::vector<uint2> ranges;
    uint64_t alpha_ascii[2] = {0, 0};
    lm_alphabet_tables(h.alphabet, alpha_ascii, ranges);
    const uint2* ar = nullptr;
    if ((rc = mem.upload(ranges, &ar))) return rc;
    // ... and the vocabulary: open addressing on a 64-bit hash of the word bytes (FNV-1a, then the splitmix finaliser —
    // d_word_id in engine.hip computes the same), load <= 0.5; a hit is confirmed on the bytes, so the ids are exact.
    // Words that occur twice keep their first id, like the host's id_of.emplace.
    const size_t nw = h.words.size();
    size_t cap = 16;
    while (cap < nw * 2) cap <<= 1;
    std::vector<uint4> table(cap, make_uint4(0u, 0u, 0xFFFFFFFFu, 0u));
    std::vector<uint32_t> off(nw + 1, 0);
    std::string bytes;
    for (size_t i = 0; i < nw; i++) { off[i] = (uint32_t)bytes.size(); bytes += h.words[i]; }
    off[nw] = (uint32_t)bytes.size();
    if (bytes.size() >= 0xFFFFFFF0ull) { set_error("vocabulary too large"); return SG_E_UNSUPPORTED; }
    for (size_t i = 0; i < nw; i++) {
      uint64_t hh = 0xCBF29CE484222325ull;
      for (unsigned char c : h.words[i]) hh = (hh ^ c) * 0x100000001B3ull;
      hh = mix64(hh);
      bool dup = false;
      size_t sidx = (size_t)((uint32_t)hh & (uint32_t)(cap - 1));
      for (;; sidx = (sidx + 1) & (cap - 1)) {
        const uint4& e = table[sidx];
        if (e.z == 0xFFFFFFFFu) break;
        if (e.x == (uint32_t)hh && e.y == (uint32_t)(hh >> 32) && h.words[e.z] == h.words[i]) { dup = true; break; }
      }
      if (!dup) table[sidx] = make_uint4((uint32_t)hh, (uint32_t)(hh >> 32), (uint32_t)i, 0u);
    }
    const uint4* vt = nullptr;
    const uint8_t* vb = nullptr;
    const uint32_t *vo = nullptr, *lfd = nullptr, *ltd = nullptr;
    if ((rc = mem.upload(table, &vt)) || (rc = mem.upload((const uint8_t*)bytes.data(), bytes.size(), &vb)) || (rc = mem.upload(off, &vo))) return rc;
    // ... and, for sentence scoring, the simple lower-case pairs (Predict takes the index replica's)
    std::vector<uint32_t> lf, lt;
    for (const auto& pr : kLowerPairs) { lf.push_back(pr.from); lt.push_back(pr.to); }
    if ((rc = mem.upload(lf, &lfd)) || (rc = mem.upload(lt, &ltd))) return rc;
    // ---- every step succeeded: commit ----
    lm->mem = std::move(mem);
    lm->n_alpha_ranges = (uint32_t)ranges.size();
    lm->d_alpha_ranges = (uint2*)ar;
    lm->alpha_ascii[0] = alpha_ascii[0]; lm->alpha_ascii[1] = alpha_ascii[1];
    lm->d_vocab = (uint4*)vt; lm->vocab_mask = (uint32_t)(cap - 1);
    lm->d_vocab_bytes = (uint8_t*)vb; lm->d_vocab_off = (uint32_t*)vo;
    lm->d_lower_from = (uint32_t*)lfd; lm->d_lower_to = (uint32_t*)ltd; lm->n_lower = (uint32_t)lf.size();
    // (a token of invalid bytes lengthens 1 -> 3 bytes when U+FFFD is in the alphabet; a lower-case mapping 2 -> 3 at most)
    lm->slot_mul = host_alphabet_has(h.alphabet, kRuneError) ? 3u : 2u;
  }
  {  // the unigram level as a direct index: one bucket (the orphans') holding word i at entry i, every i
    const LmLevel& u = lm->host.level[0];
    bool dense = u.child_begin.size() == 2 && u.child_begin[0] == 0 && u.child_begin[1] == u.word.size();
    for (size_t i = 0; dense && i < u.word.size(); i++) dense = u.word[i] == (uint32_t)i;
    lm->uni_dense = dense;
  }
  lm->level_base = std::move(level_base); lm->cb_base = std::move(cb_base);
  lm->d_child_begin = (uint32_t*)q;
  lm->d_values = (uint64_t*)p;
  lm->device = device;
  return SG_OK;
}

// What Predict and sentence scoring pass to their kernels alike: the model's levels, the alphabet and the vocabulary.
static SpellArgs lm_spell_args(const sg_lm* lm) {
  const HostLM& h = lm->host;
  SpellArgs p{};
  p.values = lm->d_values; p.child_begin = lm->d_child_begin;
  for (size_t l = 0; l < h.level.size(); l++) {
    p.level_base[l] = lm->level_base[l]; p.cb_base[l] = lm->cb_base[l];
    p.n_parents[l] = l ? (uint32_t)h.level[l - 1].word.size() : 0u;
  }
  p.order = h.order;
  p.alpha_ranges = lm->d_alpha_ranges; p.n_alpha_ranges = lm->n_alpha_ranges; p.alpha_ascii[0] = lm->alpha_ascii[0]; p.alpha_ascii[1] = lm->alpha_ascii[1];
  p.vocab = lm->d_vocab; p.vocab_mask = lm->vocab_mask; p.vocab_bytes = lm->d_vocab_bytes; p.vocab_off = lm->d_vocab_off;
  p.start_symbol = h.start_symbol;
  return p;
}

// SpellChecker.Predict (pkg/spellchecker/spellchecker.go:40-92) for a batch, on the device end to end: six launches on the
// caller's stream —
//   spell_tokenize_kernel   the word tokeniser, the word ids (vocabulary hash) and the wrap / trim rules of
//                           LanguageModel.Next (language_model.go:100-112); the last word goes to a slot of its own
//   spell_next_kernel       NGramModel.Next (binary searches down the levels)
//   sg_search_kernel_t<LM>  Autocomplete with the LM collector (top-k by ScoreNext = by the continuation count)
//   spell_select_kernel     the queries whose list is short
//   sg_search_kernel_t      the Cosine fuzzy search for those
//   spell_merge_kernel      merge + stable re-rank by ScoreNext + candidates[:topK+1] (sic)
// Everything it needs in between lives in one block of the calling thread's per-stream scratch.
static int predict_on_device(sg_index* index, sg_lm* lm, Replica* rep, const uint8_t* d_q, const uint64_t* d_offs, uint32_t n_q, uint64_t q_bytes,
                             uint32_t top_k, double similarity, uint32_t* d_out_ids, uint32_t* d_out_counts, hipStream_t st) {
  Carve c;
  const size_t o_aids = c.take((size_t)n_q * top_k * 4), o_acnt = c.take((size_t)n_q * 4), o_fids = c.take((size_t)n_q * top_k * 4), o_fcnt = c.take((size_t)n_q * 4),
               o_zero_end = c.size(),
               o_from = c.take((size_t)n_q * 4), o_to = c.take((size_t)n_q * 4), o_sel = c.take((size_t)n_q * 4), o_stat = c.take(n_q),
               o_ctx = c.take((size_t)n_q * 32), o_clen = c.take(n_q), o_hasw = c.take(n_q), o_wlen = c.take((size_t)n_q * 4),
               o_woff = c.take((size_t)(n_q + 1) * 8), o_words = c.take((size_t)q_bytes * lm->slot_mul + 16);
  void* blk = nullptr;
  if (int rc = stream_scratch(rep->device, st, c.size(), &blk, SCRATCH_PREDICT)) return rc;
  char* dev = (char*)blk;
  HIP_TRY(hipMemsetAsync(dev, 0, o_zero_end, st));                 // autocomplete / fuzzy rows and counts, the selection counter
  if (poison_mode()) {   // (sg_debug_poison: the two launches' id rows — the merge reads a row up to its count and compares the ids)
    if (int rc = poison_fill(dev + o_aids, (size_t)n_q * top_k * 4, PZ_PREDICT, st)) return rc;
    if (int rc = poison_fill(dev + o_fids, (size_t)n_q * top_k * 4, PZ_PREDICT, st)) return rc;
  }
  SpellArgs p = lm_spell_args(lm);
  p.n_q = n_q; p.top_k = top_k;
  p.q_blob = d_q; p.q_offs = d_offs;
  p.ctx_w = (uint32_t*)(dev + o_ctx); p.ctx_len_w = (uint8_t*)(dev + o_clen); p.has_word_w = (uint8_t*)(dev + o_hasw);
  p.ctx = p.ctx_w; p.ctx_len = p.ctx_len_w; p.has_word = p.has_word_w;
  p.w_blob = (uint8_t*)(dev + o_words); p.w_off = (uint64_t*)(dev + o_woff); p.w_len = (uint32_t*)(dev + o_wlen);
  p.lower_from = rep->dix.lower_from; p.lower_to = rep->dix.lower_to; p.n_lower = rep->dix.n_lower;   // (the index replica's table)
  p.slot_mul = lm->slot_mul;
  p.lm_from = (uint32_t*)(dev + o_from); p.lm_to = (uint32_t*)(dev + o_to); p.status = (uint8_t*)(dev + o_stat);
  p.a_ids = (const uint32_t*)(dev + o_aids); p.a_cnt = (const uint32_t*)(dev + o_acnt);
  p.f_ids = (const uint32_t*)(dev + o_fids); p.f_cnt = (const uint32_t*)(dev + o_fcnt);
  p.sel_flag = (uint8_t*)(dev + o_sel);
  p.out_ids = d_out_ids; p.out_counts = d_out_counts;
  HIP_TRY(hipMemsetAsync(d_out_ids, 0, (size_t)n_q * (top_k + 1) * 4, st));   // rows of queries with fewer predictions stay zero
  const unsigned gb = (n_q + 255) / 256;
  hipLaunchKernelGGL(spell_tokenize_kernel, dim3(gb), dim3(256), 0, st, p);
  hipLaunchKernelGGL(spell_next_kernel, dim3(gb), dim3(256), 0, st, p);
  HIP_TRY(hipGetLastError());
  const LmRanges ranges{lm->d_values, p.lm_from, p.lm_to};
  // (the launch orders its queries itself — shortest last words first: they match the most — from the lengths in w_len)
  LaunchReq r;
  r.q = p.w_blob; r.offs = p.w_off; r.n_q = n_q; r.k = top_k; r.autocomplete = 1;
  r.ids = dev + o_aids; r.counts = dev + o_acnt; r.stream = st; r.lm = &ranges; r.len = p.w_len;
  int rc = launch(index, rep, r);
  if (rc) return rc;
  hipLaunchKernelGGL(spell_select_kernel, dim3(gb), dim3(256), 0, st, p);
  HIP_TRY(hipGetLastError());
  r.metric = SG_COSINE; r.similarity = similarity; r.autocomplete = 0;     // (the same queries: the Cosine search of those the selection flagged)
  r.ids = dev + o_fids; r.counts = dev + o_fcnt; r.lm = nullptr; r.flag = p.sel_flag;
  rc = launch(index, rep, r);
  if (rc) return rc;
  hipLaunchKernelGGL(spell_merge_kernel, dim3(n_q), dim3(64), (size_t)top_k * 24, st, p);
  HIP_TRY(hipGetLastError());
  return SG_OK;
}

static int predict_check(sg_index* index, sg_lm* lm, const void* offs, const void* ids, const void* counts, uint32_t top_k, double similarity) {
  if (int rc = open_search(index, fuzzy_key(SG_COSINE, similarity, top_k), true, {lm, offs, ids, counts})) return rc;
  if (top_k + 1 > 1024u) { set_error("topK above 1023"); return SG_E_INVALID; }                 // (the merge step keeps 2 x topK candidates in LDS)
  if (lm->host.order > 8) { set_error("nGramOrder above 8"); return SG_E_UNSUPPORTED; }
  return SG_OK;
}

// Device-resident Predict: queries (blob of q_bytes bytes + n_q + 1 offsets) and result rows ([n_q][top_k + 1] ids, [n_q]
// counts) in the HBM of the GPU that holds the index's primary replica; asynchronous on `stream`.
int sg_spell_predict_batch_device(sg_index* index, sg_lm* lm, const void* d_q, const void* d_offs, uint32_t n_q, uint64_t q_bytes, uint32_t top_k,
                                  double similarity, void* d_out_ids, void* d_out_counts, void* stream) {
  SG_GUARD_BEGIN
  int rc = predict_check(index, lm, d_offs, d_out_ids, d_out_counts, top_k, similarity);
  if (rc) return rc;
  if (n_q == 0) return SG_OK;
  const auto held_index = hold(index);
  const auto held_lm = hold(lm);
  Replica* rep = find_replica(index, -1);
  if ((rc = lm_upload(lm, rep->device))) return rc;
  DeviceGuard dg;
  HIP_TRY(dg.set(rep->device));
  return predict_on_device(index, lm, rep, (const uint8_t*)d_q, (const uint64_t*)d_offs, n_q, q_bytes, top_k, similarity, (uint32_t*)d_out_ids,
                           (uint32_t*)d_out_counts, (hipStream_t)stream);
  SG_GUARD_END(SG_RC)
}

// Host buffers: a synchronous host-buffer call (run_host_call) around the device pipeline.
int sg_spell_predict_batch(sg_index* index, sg_lm* lm, const uint8_t* q_utf8, const uint64_t* q_offs, uint32_t n_q, uint32_t top_k,
                           double similarity, uint32_t* out_ids, uint32_t* out_counts) {
  SG_GUARD_BEGIN
  int rc = predict_check(index, lm, q_offs, out_ids, out_counts, top_k, similarity);
  if (rc) return rc;
  if (n_q == 0) return SG_OK;
  const auto held_index = hold(index);
  const auto held_lm = hold(lm);
  Replica* rep = find_replica(index, -1);
  if ((rc = lm_upload(lm, rep->device))) return rc;
  // a search's regions without scores, id rows of topK + 1, not cleared (the pipeline writes every row it counts)
  const IoCall call = search_io(q_utf8, q_offs, n_q, (uint64_t)n_q * (top_k + 1), out_ids, nullptr, out_counts, nullptr, false);
  return run_host_call(rep->device, call, [&](const IoCall& io, hipStream_t st) {
    return predict_on_device(index, lm, rep, io.at<uint8_t>(IO_Q), io.at<uint64_t>(IO_OFFS), n_q, io.r[IO_Q].bytes, top_k, similarity,
                             io.at<uint32_t>(IO_IDS), io.at<uint32_t>(IO_COUNTS), st);
  });
  SG_GUARD_END(SG_RC)
}

// ---- LanguageModel.ScoreSentence / ScoreWordIDs for a batch (lm_score.inc) ----
static const uint64_t kLmTextMax = (uint64_t)1 << 30;    // bytes of a text batch: a line's slot (3 bytes per byte at most) has 32-bit offsets

// The launches of one batch on `st`, every pointer on the device.  is_text: lines (text_bytes bytes, n + 1 byte offsets)
// through the tokeniser first; else ids with n + 1 BYTE offsets into them.  words / unknown may be null.
static int lm_score_on_device(sg_lm* lm, int device, bool is_text, const uint8_t* text, uint64_t text_bytes, const uint32_t* ids, const uint64_t* offs,
                              uint32_t n, uint64_t n_ids, double* scores, uint32_t* words, uint32_t* unknown, hipStream_t st) {
  const HostLM& h = lm->host;
  LmScoreArgs a{};
  SpellArgs& p = a.sp;
  p = lm_spell_args(lm);
  p.n_q = n;
  p.lower_from = lm->d_lower_from; p.lower_to = lm->d_lower_to; p.n_lower = lm->n_lower;   // (the model's own table)
  p.q_blob = text;
  a.n = n; a.end_symbol = h.end_symbol; a.total0 = (uint32_t)h.level[0].total; a.n_uni = (uint32_t)h.level[0].word.size();
  a.uni_dense = lm->uni_dense ? 1u : 0u; a.text = is_text ? 1u : 0u; a.slot_mul = lm->slot_mul; a.text_bytes = text_bytes;
  a.offs = offs; a.ids = ids; a.out_scores = scores; a.out_words = words; a.out_unknown = unknown;
  // sentences per workgroup: about two rounds of SG_LM_GROUP windows (a text line: a word per ~6 bytes, a guess)
  const double per = is_text ? (double)text_bytes / n / 6.0 + 1.0 : (double)n_ids / n;
  const double win = std::max(1.0, per + 3.0 - (double)h.order);
  a.per_group = (uint32_t)std::min<double>(SG_LM_GROUP, std::max(4.0, 2.0 * SG_LM_GROUP / win));
  if (is_text) {
    Carve c;
    const size_t o_blob = c.take((size_t)text_bytes * lm->slot_mul + 16), o_tok = c.take(((size_t)(text_bytes >> 1) + n + 1) * 4),
                 o_ntok = c.take((size_t)n * 4), o_wlen = c.take((size_t)n * 4);
    void* blk = nullptr;
    if (int rc = stream_scratch(device, st, c.size(), &blk, SCRATCH_LM_SCORE)) return rc;
    char* dev = (char*)blk;
    a.w_blob = (uint8_t*)(dev + o_blob); a.tok = (uint32_t*)(dev + o_tok); a.n_tok = (uint32_t*)(dev + o_ntok); a.w_len = (uint32_t*)(dev + o_wlen);
    hipLaunchKernelGGL(lm_text_tokenize_kernel, dim3((n + 255) / 256), dim3(256), 0, st, a);
  }
  hipLaunchKernelGGL(lm_score_kernel, dim3((n + a.per_group - 1) / a.per_group), dim3(SG_LM_GROUP), 0, st, a);
  HIP_TRY(hipGetLastError());
  return SG_OK;
}

// the arguments every scoring entry point checks before any HIP call
static int lm_score_check(sg_lm* lm, int device, const void* offs, const void* scores) {
  if (!lm || !offs || !scores) { set_error("null argument"); return SG_E_INVALID; }
  if (device < 0) { set_error("negative device"); return SG_E_INVALID; }
  if (lm->host.order < 1 || lm->host.order > 8) { set_error("nGramOrder outside 1 .. 8"); return SG_E_UNSUPPORTED; }
  return SG_OK;
}

// The regions of a host-buffer scoring call: a score per sentence (cleared), the word and unknown-word counts where the caller
// wants them (null: an empty region), and the sentences — n + 1 offsets counted in units of `unit` bytes (1: text, 4: word ids; they
// go in as the byte offsets the kernels read) into `blob`
enum { LM_SCORES = 0, LM_WORDS, LM_UNKNOWN, LM_OFFS, LM_BLOB };
static IoCall lm_score_io(const void* blob, uint32_t unit, const uint64_t* offs, uint32_t n, double* scores, uint32_t* words, uint32_t* unknown) {
  return IoCall().add(IO_OUT, scores, (size_t)n * 8, 16, true, PZ_OUT_SCORES).add(IO_OUT, words, words ? (size_t)n * 4 : 0, 4, true, PZ_OUT_IDS)
      .add(IO_OUT, unknown, unknown ? (size_t)n * 4 : 0, 4, false, PZ_OUT_COUNTS)
      .add_window(offs, n, blob, unit, unit == 1);   // (a slice of a text batch above 64 MiB is refused, as a search's is; of ids, served)
}

// host offsets: ascending, the buffer they index present, at most max_span units of it
static int lm_check_offsets(const void* buf, const uint64_t* offs, uint32_t n, uint64_t max_span) {
  for (uint32_t i = 0; i < n; i++)
    if (offs[i + 1] < offs[i]) { set_error("offsets are not ascending"); return SG_E_INVALID; }
  if (!buf && offs[n] != offs[0]) { set_error("null input buffer"); return SG_E_INVALID; }
  if (offs[n] - offs[0] > max_span) { set_error("batch too large"); return SG_E_INVALID; }
  return SG_OK;
}

int sg_lm_score_text_batch(sg_lm* lm, int device, const uint8_t* text, const uint64_t* offs, uint32_t n, double* out_scores, uint32_t* out_words,
                           uint32_t* out_unknown) {
  SG_GUARD_BEGIN
  int rc = lm_score_check(lm, device, offs, out_scores);
  if (rc) return rc;
  if (n == 0) return SG_OK;
  if ((rc = lm_check_offsets(text, offs, n, kLmTextMax))) return rc;
  const auto held_lm = hold(lm);
  if ((rc = lm_upload(lm, device))) return rc;
  return run_host_call(device, lm_score_io(text, 1, offs, n, out_scores, out_words, out_unknown), [&](const IoCall& io, hipStream_t st) {
    return lm_score_on_device(lm, device, true, io.at<uint8_t>(LM_BLOB), io.r[LM_BLOB].bytes, nullptr, io.at<uint64_t>(LM_OFFS), n, 0, io.at<double>(LM_SCORES),
                              out_words ? io.at<uint32_t>(LM_WORDS) : nullptr, out_unknown ? io.at<uint32_t>(LM_UNKNOWN) : nullptr, st);
  });
  SG_GUARD_END(SG_RC)
}

int sg_lm_score_text_batch_device(sg_lm* lm, int device, const void* d_text, const void* d_offs, uint32_t n, uint64_t text_bytes, void* d_out_scores,
                                  void* d_out_words, void* d_out_unknown, void* stream) {
  SG_GUARD_BEGIN
  int rc = lm_score_check(lm, device, d_offs, d_out_scores);
  if (rc) return rc;
  if (n == 0) return SG_OK;
  if (!d_text && text_bytes) { set_error("null text"); return SG_E_INVALID; }
  if (text_bytes > kLmTextMax) { set_error("text batch above 1 GiB"); return SG_E_INVALID; }
  const auto held_lm = hold(lm);
  if ((rc = lm_upload(lm, device))) return rc;
  DeviceGuard dg;
  HIP_TRY(dg.set(device));
  return lm_score_on_device(lm, device, true, (const uint8_t*)d_text, text_bytes, nullptr, (const uint64_t*)d_offs, n, 0,
                            (double*)d_out_scores, (uint32_t*)d_out_words, (uint32_t*)d_out_unknown, (hipStream_t)stream);
  SG_GUARD_END(SG_RC)
}

int sg_lm_score_word_ids_batch(sg_lm* lm, int device, const uint32_t* ids, const uint64_t* offs, uint32_t n, double* out_scores) {
  SG_GUARD_BEGIN
  int rc = lm_score_check(lm, device, offs, out_scores);
  if (rc) return rc;
  if (n == 0) return SG_OK;
  if ((rc = lm_check_offsets(ids, offs, n, (uint64_t)1 << 30))) return rc;
  const auto held_lm = hold(lm);
  if ((rc = lm_upload(lm, device))) return rc;
  return run_host_call(device, lm_score_io(ids, 4, offs, n, out_scores, nullptr, nullptr), [&](const IoCall& io, hipStream_t st) {
    return lm_score_on_device(lm, device, false, nullptr, 0, io.at<uint32_t>(LM_BLOB), io.at<uint64_t>(LM_OFFS), n, offs[n] - offs[0], io.at<double>(LM_SCORES), nullptr, nullptr, st);
  });
  SG_GUARD_END(SG_RC)
}
}  // extern "C"
