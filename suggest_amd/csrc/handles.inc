// handles.inc — the handles and what hangs on them: the three launch controllers, Replica, sg_index (its knobs: knobs.inc), sg_lm,
// Held, the lower-case pairs, find_replica, and the one statement of a search request (SearchKey) with its checks and the opening
// of a search entry point.  Uses host_base.inc.

// ---- the launch controllers (plan_launch): each reads the words of the replica's statistics block it needs from the host's copy,
// and keeps what it saw last ----

// [SG_TIGHTEN=2] The tightening instantiation for fuzzy launches: on while more than 30 % of the queries sampled since the last look
// (32 at least) ended with a full top-k, off again below 15 %.  Before the first statistics, on for a similarity below 0.3: it admits
// most of the window — over a dictionary of near-duplicates a million candidates per query unless the thresholds follow the top-k;
// the wrong guess costs a few per cent.
struct TightenCtl {
  std::atomic<uint32_t> seen_full{0}, seen_total{0};
  std::atomic<bool> on{false};
  bool now(const volatile uint32_t* h, double similarity) const {   // the decision as it stands (h may be null)
    return on.load(std::memory_order_relaxed) || (similarity < 0.3 && h && h[SG_STAT_SAMPLED] == 0u);
  }
  bool step(const volatile uint32_t* h, double similarity) {
    const uint32_t full = h[SG_STAT_FULL], total = h[SG_STAT_SAMPLED];
    const uint32_t d_total = total - seen_total.load(std::memory_order_relaxed), d_full = full - seen_full.load(std::memory_order_relaxed);
    if (d_total >= 32u && d_full <= d_total) {
      seen_total.store(total, std::memory_order_relaxed); seen_full.store(full, std::memory_order_relaxed);
      if (d_full * 100u > d_total * 30u) on.store(true, std::memory_order_relaxed);
      else if (d_full * 100u < d_total * 15u) on.store(false, std::memory_order_relaxed);
    }
    return on.load(std::memory_order_relaxed) || (total == 0u && similarity < 0.3);
  }
};

// [r5, SG_PIPE=2] The pipeline's run-time guard: a replica that saw more than a fifth of its recent pipeline queries (4 096 at least
// since the last look) come back to the fused kernel — dictionaries of near-duplicates: hundreds of flagged postings per query;
// documents that repeat terms — keeps its next 64 launches off the pipeline, then tries again.
struct PipeGuard {
  std::atomic<uint64_t> seen_queries{0};
  std::atomic<uint32_t> seen_fb{0}, off_launches{0};
  bool holding() const { return off_launches.load(std::memory_order_relaxed) != 0u; }
  // q_now: the queries sent through the pipeline so far; true: this launch stays off it
  bool step(const volatile uint32_t* h, uint64_t q_now) {
    const uint32_t fb = h[SG_STAT_UNPLANNED] + h[SG_STAT_OVERFLOW] + h[SG_STAT_REPEATS];
    const uint64_t q_seen = seen_queries.load(std::memory_order_relaxed);
    const uint32_t d_fb = fb - seen_fb.load(std::memory_order_relaxed);
    if (d_fb && q_now - q_seen >= 4096u) {
      seen_fb.store(fb, std::memory_order_relaxed); seen_queries.store(q_now, std::memory_order_relaxed);
      if ((uint64_t)d_fb * 5u > q_now - q_seen) off_launches.store(64u, std::memory_order_relaxed);
    }
    const uint32_t off = off_launches.load(std::memory_order_relaxed);
    if (off) off_launches.store(off - 1u, std::memory_order_relaxed);
    return off != 0u;
  }
};

// [r6] The lightest stream-workgroup shape this replica's pipeline launches may take: raised past the latest launch's shape when
// more than a hundredth of a window's queries (4 096 at least) came back unplanned.  `last`: the latest launch's shape (0 .. 2, 3 =
// the knobs' own; sg_index_pipe_volumes).
struct ShapeFloor {
  std::atomic<uint32_t> floor{0}, last{2}, seen_unplanned{0};
  std::atomic<uint64_t> seen_queries{0};
  // shape: the model's; returns the one this launch takes.  h may be null: no new statistics
  uint32_t step(const volatile uint32_t* h, uint64_t q_now, uint32_t shape) {
    if (h) {
      const uint32_t unplanned = h[SG_STAT_UNPLANNED];
      const uint64_t q_seen = seen_queries.load(std::memory_order_relaxed);
      if (q_now - q_seen >= 4096u) {
        const uint32_t d_un = unplanned - seen_unplanned.load(std::memory_order_relaxed), l = last.load(std::memory_order_relaxed);
        seen_unplanned.store(unplanned, std::memory_order_relaxed); seen_queries.store(q_now, std::memory_order_relaxed);
        if ((uint64_t)d_un * 100u > q_now - q_seen && l < 2u && l >= floor.load(std::memory_order_relaxed)) floor.store(l + 1u, std::memory_order_relaxed);
      }
    }
    shape = std::max(shape, floor.load(std::memory_order_relaxed));
    last.store(shape, std::memory_order_relaxed);
    return shape;
  }
};

// One copy of the index in the HBM of one GPU.  Immutable once published in sg_index::replicas.
struct Replica {
  int device = -1;
  DeviceIndex dix{};
  DeviceBlock mem;                     // every array of dix and the working memory below: mem.total() is the replica's device_bytes
  // working memory of sg_long_kernel (queries with more than SG_MAX_A n-grams): SG_LONG_SLOTS slots + a lock word each
  uint8_t* long_scratch = nullptr; uint32_t* long_lock = nullptr; uint64_t long_slot_bytes = 0; uint32_t long_max_seg = 0;
  const uint32_t* x_of = nullptr;      // [n_docs] docID -> the packed store's number (packed_store.inc; introspection only)
  uint64_t packed_chunks = 0;          // 16-byte chunks of the packed store
  int n_cus = 256;                     // compute units of the device (the persistent launches' grids)
  // the statistics block (StatWord, engine.hip): the kernels count into it, and every few launches a one-thread kernel copies it to
  // pinned memory behind them, where the next launches' controllers read what has arrived (no synchronisation: a decision that
  // lags a launch or two only costs a few per cent)
  uint32_t* d_fill = nullptr;
  uint32_t* h_fill = nullptr;          // pinned + mapped (h_fill_dev = its device address)
  uint32_t* h_fill_dev = nullptr;
  std::atomic<uint32_t> launches{0};   // launches that fed the block (every fourth copies it)
  std::atomic<uint64_t> pipe_queries{0};   // queries sent through the pipeline
  TightenCtl tighten;
  PipeGuard pipe_guard;
  ShapeFloor shape_floor;
  // sg_*_batch_multi and the single-query coalescer drive a replica from threads of their own: a stream and a pinned
  // staging buffer per lane, made on first use
  struct AsyncPool* async_pool = nullptr;   // sg_suggest_submit / sg_ticket_wait: three streams + a ring of slots (made on first use)
  std::mutex async_mu;
  ~Replica();
};

#include "knobs.inc"
struct Coalescer;
static void coalescer_stop(Coalescer* c);
struct MultiPool;
static void multi_pool_stop(MultiPool* p);

struct sg_index {
  HostIndex host;
  std::atomic<int> refs{1};
  std::mutex mu;                                        // guards `replicas` (append-only), `prebuilt`, `coalescer` and the one-time tuning
  std::vector<std::unique_ptr<Replica>> replicas;       // [0] = the primary (first upload)
  std::unique_ptr<Replica> prebuilt;                    // posting store + seg_off a device build left in HBM: adopted by the
                                                        // first upload to that device instead of a D2H + H2D round trip
  std::atomic<bool> uploaded{false};
  int device = -1;                                      // the primary replica's
  bool tuned = false;
  Knobs knobs;                     // knobs.inc: environment at the first upload, sg_index_tune; below: what tune_index() derives
  double terms_per_doc = 0;
  double max_term_chunks = 0;      // chunks of the longest term (all segments)
  double est_query_chunks = 0;     // expected 16-byte chunks of postings a query's terms hold (size-biased mean list x terms per doc)
  uint32_t parts_grid = 3072;      // wavefronts of the second launch (three per SIMD are resident)
  bool pipe_pays = false;          // [r5] plan -> stream -> verify pays for this index (tune_choice; SG_PIPE=2 asks)
  Coalescer* coalescer = nullptr;  // sg_suggest_one / sg_autocomplete_one (made on first use)
  MultiPool* multi = nullptr;      // sg_*_batch_multi: one worker thread per replica (made on first use)
};

struct sg_lm {
  HostLM host;
  std::atomic<int> refs{1};
  std::mutex mu;                       // guards the lazy upload
  int device = -1;
  DeviceBlock mem;                     // owns every d_* array below (they are views into it)
  uint64_t* d_values = nullptr;        // every level's (word << 32 | count), level after level
  uint32_t* d_child_begin = nullptr;   // every level's bucket offsets, level after level
  std::vector<uint32_t> level_base;    // first entry of level l in d_values
  std::vector<uint32_t> cb_base;       // first entry of level l in d_child_begin
  // what the device word tokeniser reads (spell_tokenize_kernel): the alphabet, the vocabulary as a hash of the word bytes
  uint2* d_alpha_ranges = nullptr; uint32_t n_alpha_ranges = 0; uint64_t alpha_ascii[2] = {0, 0};
  uint4* d_vocab = nullptr; uint32_t vocab_mask = 0;
  uint8_t* d_vocab_bytes = nullptr; uint32_t* d_vocab_off = nullptr;
  // sentence scoring (lm_score.inc): its own copy of the simple lower-case pairs (there is no index replica to take them from),
  // whether the unigram level is every word in id order (a direct index instead of a search), a line's slot per byte
  uint32_t* d_lower_from = nullptr; uint32_t* d_lower_to = nullptr; uint32_t n_lower = 0;
  bool uni_dense = false;
  uint32_t slot_mul = 2;
};

// A reference on an index or a language model that goes at the end of the scope: hold(h) takes one for the duration of a call,
// Held<H>(h) adopts one the caller already has.
struct HandleRelease {
  void operator()(sg_index* i) const { sg_index_release(i); }
  void operator()(sg_lm* l) const { sg_lm_release(l); }
};
template <class H> using Held = std::unique_ptr<H, HandleRelease>;
inline Held<sg_index> hold(sg_index* i) { sg_index_retain(i); return Held<sg_index>(i); }
inline Held<sg_lm> hold(sg_lm* l) { sg_lm_retain(l); return Held<sg_lm>(l); }

// What a search is asked for besides its queries and arrays — metric, prefix or fuzzy, similarity, k, first document — is one
// sg_search_config wherever it travels: an entry point makes it, search_req() turns it into a launch, the coalescer batches by it,
// and a mixed call's table is an array of them.  Equality and order over the five values: -0.0 and +0.0 are one key, no NaN gets this far.
using SearchKey = sg_search_config;
inline SearchKey fuzzy_key(int metric, double similarity, uint32_t k, uint32_t first_doc = 0) { return SearchKey{metric, 0, similarity, k, first_doc}; }
inline SearchKey prefix_key(uint32_t limit, uint32_t first_doc = 0) { return SearchKey{0, 1, 0.0, limit, first_doc}; }
inline auto key_values(const SearchKey& c) { return std::tie(c.metric, c.autocomplete, c.similarity, c.k, c.first_doc); }
inline bool operator==(const SearchKey& a, const SearchKey& b) { return key_values(a) == key_values(b); }
inline bool operator<(const SearchKey& a, const SearchKey& b) { return key_values(a) < key_values(b); }

static void* g_prof_buf = nullptr;   // SG_PHASE_TIMING builds only (sg_debug_set_prof)

namespace {

struct LowerPair { uint32_t from, to; };
const LowerPair kLowerPairs[] = {
#include "unicode_lower.inc"
};

// alphabet.CreateAlphabet(spec).Has as the device word tokeniser reads it (d_lm_alpha_has): a bitmap below 128, inclusive ranges
// above — from the runes the specification lists, not from a probe of every code point.  lm_upload and lm_build.inc use it.
void lm_alphabet_tables(const std::vector<std::string>& spec, uint64_t ascii[2], std::vector<uint2>& ranges) {
  ascii[0] = ascii[1] = 0;
  ranges.clear();
  std::vector<uint32_t> runes;
  host_alphabet_runes(spec, runes);
  for (uint32_t r : runes) {
    if (r < 128u) ascii[r >> 6] |= 1ull << (r & 63u);
    else if (!ranges.empty() && ranges.back().y + 1u == r) ranges.back().y = r;
    else ranges.push_back(make_uint2(r, r));
  }
}

// symbol tables, lower-case table, wrap and pad of the description: what the device tokeniser reads
int upload_description(const HostIndex& h, DeviceBlock& mem, DeviceIndex& d) {
  int rc;
  if ((rc = mem.upload(h.sym.ascii_sym, 128, &d.ascii_sym))) return rc;
  if ((rc = mem.upload(h.sym.ascii_alpha, 128, &d.ascii_alpha))) return rc;
  if ((rc = mem.upload(h.sym.na_rune, &d.na_rune))) return rc;
  if ((rc = mem.upload(h.sym.na_sym, &d.na_sym))) return rc;
  if ((rc = mem.upload(h.sym.na_alpha, &d.na_alpha))) return rc;
  std::vector<uint32_t> lf, lt;
  for (const auto& p : kLowerPairs) { lf.push_back(p.from); lt.push_back(p.to); }
  if ((rc = mem.upload(lf, &d.lower_from))) return rc;
  if ((rc = mem.upload(lt, &d.lower_to))) return rc;
  d.n_na = (uint32_t)h.sym.na_rune.size();
  d.n_lower = (uint32_t)lf.size();
  d.q = h.q;
  d.n_wrap0 = (uint32_t)h.wrap0.size();
  d.n_wrap1 = (uint32_t)h.wrap1.size();
  for (size_t i = 0; i < h.wrap0.size(); i++) d.wrap0[i] = h.wrap0[i];
  for (size_t i = 0; i < h.wrap1.size(); i++) d.wrap1[i] = h.wrap1[i];
  d.n_pad = h.sym.n_pad;
  memcpy(d.pad_sym, h.sym.pad_sym, 8);
  return SG_OK;
}

size_t lds_bytes(uint32_t log2_cnt, uint32_t k, bool roomy = false, bool slim = false) {   // the kernel's LDS layout (engine.hip)
  const size_t words = ((size_t)1 << log2_cnt) + (slim ? Lds<true>::fixed_words : Lds<false>::fixed_words) +
                       2 * (size_t)sg_queue_cap(log2_cnt, k, roomy, slim) + sg_topk_words(k);
  return words * 4;
}

// the n-th (0-based) replica on `device`; device < 0: the primary
Replica* find_replica(sg_index* ix, int device, uint32_t nth = 0) {
  std::lock_guard<std::mutex> lock(ix->mu);
  if (device < 0) return ix->replicas.empty() ? nullptr : ix->replicas[0].get();
  for (auto& r : ix->replicas)
    if (r->device == device) { if (nth == 0) return r.get(); nth--; }
  return nullptr;
}

// the checks of a search's values alone (a mixed call makes them for every entry of its table before it looks at the index)
int check_search_values(uint32_t k, bool need_alpha, double similarity, int metric) {
  if (k == 0) { set_error("topK should be greater or equal to 1"); return SG_E_INVALID; }       // search.go:20-22
  if (k > SG_MAX_TOPK) { set_error("topK above SG_MAX_TOPK"); return SG_E_INVALID; }
  if (need_alpha) {
    if (!(similarity > 0 && similarity <= 1)) { set_error("similarity shouble be in (0.0, 1.0]"); return SG_E_INVALID; }  // search.go:24-26
    if (metric < SG_JACCARD || metric > SG_OVERLAP) { set_error("unknown metric"); return SG_E_INVALID; }
  }
  return SG_OK;
}
// The opening of every search entry point, in the one order they all keep: null index, not uploaded, k, the similarity and metric
// where the call takes them from its arguments (need_alpha), then the pointers it cannot do without.
int open_search(sg_index* index, const SearchKey& c, bool need_alpha, std::initializer_list<const void*> required) {
  if (!index) { set_error("null index"); return SG_E_INVALID; }
  if (!index->uploaded.load(std::memory_order_acquire)) { set_error("index not uploaded: call sg_index_upload first"); return SG_E_NOT_UPLOADED; }
  if (int rc = check_search_values(c.k, need_alpha, c.similarity, c.metric)) return rc;
  for (const void* p : required) if (!p) { set_error("null argument"); return SG_E_INVALID; }
  return SG_OK;
}
}  // namespace
