// capi.inc — host side of libsuggest_hip, included by engine.hip (it launches the kernels defined there):
// the index handle and its per-GPU replicas, launches, the C ABI of include/suggest_hip.h.

#include <hipcub/hipcub.hpp>

// ------------------------------------------------------------------------------------------
// host side: handle, replicas, launches
// ------------------------------------------------------------------------------------------
namespace sg {
static thread_local std::string g_err;
void set_error(const std::string& m) { g_err = m; }
}  // namespace sg

using namespace sg;

#define HIP_TRY(expr)                                                                   \
  do {                                                                                  \
    hipError_t e_ = (expr);                                                             \
    if (e_ != hipSuccess) {                                                             \
      set_error(std::string(#expr) + ": " + hipGetErrorString(e_));                     \
      return SG_E_HIP;                                                                  \
    }                                                                                   \
  } while (0)

// Every extern "C" body runs inside this pair: no C++ exception crosses the C boundary (a cgo caller would abort).
#define SG_GUARD_BEGIN try {
#define SG_GUARD_END(on_fail)                                                           \
  } catch (const std::bad_alloc&) { set_error("out of host memory"); return on_fail(SG_E_NOMEM); } \
  catch (const std::exception& e_) { set_error(std::string("internal error: ") + e_.what()); return on_fail(SG_E_INVALID); }
#define SG_RC(x) (x)

// Makes a device the calling thread's current one for the rest of a scope and puts the previous one back at its end:
// `DeviceGuard dg; HIP_TRY(dg.set(device));`
struct DeviceGuard {
  int prev = -1, cur = -1;
  hipError_t set(int device) {
    if (prev < 0) {
      const hipError_t e = hipGetDevice(&prev);
      if (e != hipSuccess) { prev = -1; return e; }
      cur = prev;
    }
    if (device == cur) return hipSuccess;
    const hipError_t e = hipSetDevice(device);
    if (e == hipSuccess) cur = device;
    return e;
  }
  ~DeviceGuard() { if (prev >= 0 && cur != prev) (void)hipSetDevice(prev); }
};

// The one owner of device memory that is held, not reused (reuse buffers are GrowBlocks, below): a replica's arrays, a language
// model's tables, metric tables, the working memory of a build / store / load call.  Its blocks live on the device that was current
// at the first alloc(); the destructor frees them with that device current and puts the caller's back.  Movable: "commit on
// success" is to build in a local DeviceBlock and move it into the handle as the last step.  A failed hipMalloc is SG_E_NOMEM.
struct DeviceBlock {
  struct Block { void* p; size_t bytes; };
  std::vector<Block> blocks;
  int device = -1;
  uint64_t sum = 0;
  DeviceBlock() = default;
  DeviceBlock(DeviceBlock&& o) noexcept { swap(o); }
  DeviceBlock& operator=(DeviceBlock&& o) noexcept { clear(); swap(o); return *this; }
  ~DeviceBlock() { clear(); }
  void swap(DeviceBlock& o) { blocks.swap(o.blocks); std::swap(device, o.device); std::swap(sum, o.sum); }
  void clear() {
    if (blocks.empty()) return;
    DeviceGuard dg;
    if (dg.set(device) == hipSuccess) for (const Block& b : blocks) (void)hipFree(b.p);
    blocks.clear(); sum = 0;
  }
  template <class T> int alloc(T** out, size_t n) {   // n elements, 16 bytes at least
    if (device < 0) HIP_TRY(hipGetDevice(&device));
    void* p = nullptr;
    const size_t bytes = std::max<size_t>(n * sizeof(T), 16);
    const hipError_t e = hipMalloc(&p, bytes);
    if (e != hipSuccess) { set_error(std::string("hipMalloc: ") + hipGetErrorString(e)); return SG_E_NOMEM; }
    blocks.push_back(Block{p, bytes});
    sum += bytes;
    *out = (T*)p;
    return SG_OK;
  }
  // a block holding src[0 .. n): copied before the call returns, or on `st` when one is given (the caller synchronises it)
  template <class T> int upload(const T* src, size_t n, const T** out, hipStream_t st = nullptr) {
    T* p = nullptr;
    if (int rc = alloc(&p, n)) return rc;
    if (n && st) HIP_TRY(hipMemcpyAsync(p, src, n * sizeof(T), hipMemcpyHostToDevice, st));
    else if (n) HIP_TRY(hipMemcpy(p, src, n * sizeof(T), hipMemcpyHostToDevice));
    *out = p;
    return SG_OK;
  }
  template <class T> int upload(const std::vector<T>& src, const T** out, hipStream_t st = nullptr) { return upload(src.data(), src.size(), out, st); }
  const Block* find(const void* p) const { for (const Block& b : blocks) if (b.p == p) return &b; return nullptr; }
  size_t bytes_of(const void* p) const { const Block* b = find(p); return b ? b->bytes : 0; }   // 0: not a block of this owner
  uint64_t total() const { return sum; }
  void release(const void* p) {   // frees one block (null or unknown: nothing)
    const Block* b = p ? find(p) : nullptr;
    if (!b) return;
    DeviceGuard dg;
    if (dg.set(device) == hipSuccess) (void)hipFree(b->p);
    sum -= b->bytes;
    blocks.erase(blocks.begin() + (b - blocks.data()));
  }
};

// hipcub's two-call idiom, once: ask for the working memory's size, take it from `mem` (it goes when `mem` goes), run.  A loop that
// runs one sort or scan many times over one working block (lm_build.inc, lm_store.inc) calls hipcub itself.
template <class T>
int device_exclusive_sum(DeviceBlock& mem, const T* in, T* out, size_t n, hipStream_t st = nullptr) {
  size_t tb = 0;
  HIP_TRY(hipcub::DeviceScan::ExclusiveSum(nullptr, tb, in, out, (int)n, st));
  uint8_t* tmp;
  if (int rc = mem.alloc(&tmp, tb)) return rc;
  HIP_TRY(hipcub::DeviceScan::ExclusiveSum(tmp, tb, in, out, (int)n, st));
  return SG_OK;
}
// ... over working memory the caller holds already (a call on a caller's stream takes it from its scratch block: nothing is
// allocated or freed while the stream runs): exclusive_sum_bytes says how much a scan of n elements needs
template <class T>
int exclusive_sum_bytes(size_t n, size_t* bytes) {
  *bytes = 0;
  HIP_TRY(hipcub::DeviceScan::ExclusiveSum(nullptr, *bytes, (const T*)nullptr, (T*)nullptr, (int)n, (hipStream_t) nullptr));
  return SG_OK;
}
template <class T>
int device_exclusive_sum(void* tmp, size_t tmp_bytes, const T* in, T* out, size_t n, hipStream_t st) {
  HIP_TRY(hipcub::DeviceScan::ExclusiveSum(tmp, tmp_bytes, in, out, (int)n, st));
  return SG_OK;
}
template <class K, class V>   // stable, ascending by bits [begin_bit, end_bit) of the keys
int device_sort_pairs(DeviceBlock& mem, const K* keys_in, K* keys_out, const V* vals_in, V* vals_out, size_t n, int begin_bit = 0,
                      int end_bit = 8 * (int)sizeof(K), hipStream_t st = nullptr) {
  size_t tb = 0;
  HIP_TRY(hipcub::DeviceRadixSort::SortPairs(nullptr, tb, keys_in, keys_out, vals_in, vals_out, (int)n, begin_bit, end_bit, st));
  uint8_t* tmp;
  if (int rc = mem.alloc(&tmp, tb)) return rc;
  HIP_TRY(hipcub::DeviceRadixSort::SortPairs(tmp, tb, keys_in, keys_out, vals_in, vals_out, (int)n, begin_bit, end_bit, st));
  return SG_OK;
}
// the sum of val[0 .. n) from its exclusive prefix sums: last prefix + last value (n >= 1)
template <class Out>
int device_total(const uint32_t* val, const uint32_t* pre, size_t n, Out* out) {
  uint32_t a = 0, b = 0;
  HIP_TRY(hipMemcpy(&a, val + n - 1, 4, hipMemcpyDeviceToHost));
  HIP_TRY(hipMemcpy(&b, pre + n - 1, 4, hipMemcpyDeviceToHost));
  *out = (Out)a + b;
  return SG_OK;
}

using clk = std::chrono::steady_clock;   // the stopwatch of the store / load codecs' phase times
inline double since(clk::time_point t) { return std::chrono::duration<double>(clk::now() - t).count(); }

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
int check_search_args(sg_index* index, uint32_t k, bool need_alpha, double similarity, int metric) {
  if (!index) { set_error("null index"); return SG_E_INVALID; }
  if (!index->uploaded.load(std::memory_order_acquire)) { set_error("index not uploaded: call sg_index_upload first"); return SG_E_NOT_UPLOADED; }
  return check_search_values(k, need_alpha, similarity, metric);
}

struct LmRanges { const uint64_t* values; const uint32_t *from, *to; };   // device pointers (spellchecker mode)

// One launch as its caller asks for it: device pointers, on `stream`.
struct LaunchReq {
  const void* q = nullptr; const void* offs = nullptr; uint32_t n_q = 0;   // query blob and n_q + 1 u64 offsets
  int metric = 0; double similarity = 0; uint32_t k = 0;
  int autocomplete = 0;               // 1: prefix search (BatchArgs::autocomplete)
  bool by_doc = false;                // sg_suggest_batch_from: fuzzy window and thresholds, rows ordered by docID from ac_first on
  uint32_t ac_first = 0;
  void* ids = nullptr; void* scores = nullptr; void* counts = nullptr;      // [n_q][k] u32, [n_q][k] f64 (may be null), [n_q] u32
  hipStream_t stream = nullptr;
  const LmRanges* lm = nullptr;       // the spellchecker's LM collector (Predict)
  const uint32_t* sel = nullptr; const uint32_t* sel_n = nullptr;   // the queries to answer (BatchArgs::q_sel / q_sel_n)
  const uint32_t* len = nullptr;      // query lengths (BatchArgs::q_len)
  bool no_long_queries = false;       // the caller knows no query passes the wavefront kernel's tables: no long-query launch
  uint32_t* out_aux = nullptr;        // by_doc: [n_q][k] segment << 16 | overlap (may be null)
  const MetricTab* mt = nullptr;      // a tabulated metric in place of (metric, similarity)
  const uint8_t* flag = nullptr;      // only the queries this [n_q] array marks (Predict's fuzzy launch)
};

size_t block_capacity(size_t bytes) {
  if (bytes > ((size_t)64 << 20)) return (bytes + ((size_t)64 << 20) - 1) & ~(((size_t)64 << 20) - 1);
  size_t cap = (size_t)1 << 16;
  while (cap < bytes) cap <<= 1;
  return cap;
}
// A grow-only block of device memory (hipMalloc) or pinned host memory (hipHostMalloc) of block_capacity bytes — a power of two
// from 64 KiB on, a multiple of 64 MiB above that: growing frees the old block (its contents are lost) and allocates a larger one
struct GrowBlock {
  bool host = false;
  void* p = nullptr;
  size_t cap = 0;
  void release() {
    if (p) (void)(host ? hipHostFree(p) : hipFree(p));
    p = nullptr; cap = 0;
  }
  int grow(size_t bytes) {
    if (bytes <= cap) return SG_OK;
    release();
    const size_t c = block_capacity(bytes);
    if (host) HIP_TRY(hipHostMalloc(&p, c, hipHostMallocDefault)); else HIP_TRY(hipMalloc(&p, c));
    cap = c;
    return SG_OK;
  }
};

// Working memory of a launch (top-k rows above SG_K_LDS, the split-query queue): one grow-only buffer per calling thread
// and (device, stream), reused by that thread's next launch on the stream — which is ordered behind this one.  No
// stream-ordered pool: its blocks were seen handed to a second stream while the first still used them (callers on
// several streams during an index swap, tests/cpp/service_test.cpp).  hipFree waits for the device, so growing or
// dropping a buffer never pulls it from under a running kernel.
// A block per tag: one launch holds SCRATCH_ROWS, SCRATCH_LONG_LIST and one of SCRATCH_PRETOK / SCRATCH_PIPE of its stream at
// once, and Predict's block besides when Predict is the caller — four at most.  Sentence scoring (lm_score.inc) holds its own
// block alone.  A sharded search (shard_merge.inc) holds SCRATCH_SHARD, the shards' rows, around its launches.
// A mixed call (mixed_batch.inc) holds SCRATCH_MIXED, its lists and offsets, and SCRATCH_MIXED_ROWS, the grouped queries and the
// groups' rows, around its launches.  The materialise step (dict_rows.inc) holds SCRATCH_DICT, its lengths and the scan's working
// memory, until its gather launch is enqueued.
enum ScratchTag { SCRATCH_ROWS = 0, SCRATCH_PREDICT = 1, SCRATCH_LONG_LIST = 2, SCRATCH_PRETOK = 3, SCRATCH_PIPE = 4, SCRATCH_LM_SCORE = 5, SCRATCH_SHARD = 6,
                  SCRATCH_MIXED = 7, SCRATCH_MIXED_ROWS = 8, SCRATCH_DICT = 9 };
struct ScratchSlot { int device; hipStream_t stream; int tag; GrowBlock blk; bool held = false; };
inline bool on_main_thread() { return (long)getpid() == (long)syscall(SYS_gettid); }
// (a thread that ends hands its buffers back; the main thread's are left to process exit, when the HIP runtime may already
//  be going down)
struct ThreadScratch {
  std::vector<ScratchSlot> slots;
  void release() {
    for (auto& x : slots) if (x.blk.p && hipSetDevice(x.device) == hipSuccess) x.blk.release();
    slots.clear();
  }
  ~ThreadScratch() { if (!slots.empty() && !on_main_thread()) release(); }
};
thread_local ThreadScratch t_scratch_owner;
#define t_scratch (t_scratch_owner.slots)
int stream_scratch(int device, hipStream_t stream, size_t bytes, void** out, ScratchTag tag) {
  ScratchSlot* sl = nullptr;
  for (auto& x : t_scratch) if (x.device == device && x.stream == stream && x.tag == tag) sl = &x;
  if (!sl) {
    // a block of the requesting (device, stream) is never the one to go: the oldest block of ANOTHER stream is (hipFree waits
    // for the device, so nothing running loses its memory)
    if (t_scratch.size() >= 16) {
      for (size_t i = 0; i < t_scratch.size(); i++) {
        if ((t_scratch[i].device == device && t_scratch[i].stream == stream) || t_scratch[i].held) continue;
        if (t_scratch[i].blk.p) { (void)hipSetDevice(t_scratch[i].device); t_scratch[i].blk.release(); (void)hipSetDevice(device); }
        t_scratch.erase(t_scratch.begin() + (long)i);
        break;
      }
    }
    t_scratch.push_back(ScratchSlot{device, stream, tag, GrowBlock{}});
    sl = &t_scratch.back();
  }
  if (int rc = sl->blk.grow(bytes)) return rc;
  *out = sl->blk.p;
  return SG_OK;
}

// A block its holder keeps across this thread's launches on OTHER streams (a sharded call with lanes, shard_merge.inc): not
// recycled while held
void scratch_hold(int device, hipStream_t stream, ScratchTag tag, bool on) {
  for (auto& x : t_scratch) if (x.device == device && x.stream == stream && x.tag == tag) x.held = on;
}

// A block cut into regions, in order: take() places the next one at the first multiple of `align` bytes behind the last;
// size() is the block's size (a multiple of 16 bytes).
struct Carve {
  size_t off = 0;
  size_t take(size_t bytes, size_t align = 16) { const size_t at = (off + align - 1) & ~(align - 1); off = at + bytes; return at; }
  size_t size() const { return (off + 15) & ~(size_t)15; }
};

// [r6] Whether the three-launch pipeline can run on this replica at all (one predicate for every place that asks): a dictionary
// above the one-counter-per-document size, a chunk index of 32 bits.  Stores of 2^26 chunks (1 GiB) and more take the stream
// launch's 8-byte sub-row descriptors (pipe_wide); top-k rows above SG_K_LDS entries live in HBM as the fused kernel's.
bool pipe_capable(const sg_index* index, const Replica* rep) {
  return index->knobs.pipe != 0 && rep->dix.n_docs > (4u << index->knobs.log2_cnt) && rep->packed_chunks < (1ull << 32);
}
// the tokeniser as a launch of its own (512 B of scratch per query: a batch of more than 2 M queries — 1 GiB of it — lets the
// search kernel tokenise itself)
bool pretok_launch(const sg_index* index, uint32_t n_q) { return index->knobs.pretok && n_q >= (uint32_t)index->knobs.pretok && n_q <= (1u << 21); }
// [r5] Whether a launch may go through plan -> stream -> verify (pipeline.inc: the plan launch tokenises; the fused kernel runs
// behind them over the queries they hand back): an ordinary fuzzy batch — top-k by score, no LM collector, no 8-bit gaps, no
// tightening — large enough for a tokeniser launch of its own, on a replica that can run the pipeline, always (SG_PIPE=1) or
// where it pays (tune_choice; profiles/r05r_*) while the run-time guard does not hold it off.  launch() adds: no split queries.
bool pipe_eligible(const sg_index* index, const Replica* rep, const LaunchReq& r, bool tight, bool guard_off) {
  return pipe_capable(index, rep) && !r.lm && !r.autocomplete && !r.by_doc && !rep->dix.has_g8 && !tight && pretok_launch(index, r.n_q) &&
         (index->knobs.pipe == 1 || (index->pipe_pays && !guard_off));
}
// [r6] The stream workgroup a launch starts from (plan_launch): 0 / 1 / 2 = 2 / 4 / 8 wavefronts on 2^11 / 2^12 /
// 2^13 counters, by the index's expected query volume x the square of the share of a typical query's lists that skipping leaves
// under the metric and similarity.  One place, so that a test can hold it against the launches it was measured on
// (tests/test_capi_cpu.py::test_stream_shapes_are_pinned; sg_debug_pipe_shape).
uint32_t pipe_shape_model(double est_query_chunks, double terms_per_doc, int t_floor, int metric, double similarity) {
  const int A_t = std::max(1, (int)(terms_per_doc + 0.5));
  const int T_t = metric_threshold(metric, similarity, A_t, A_t);
  const double kept = std::min(1.0, std::max(1.0, (double)(A_t - std::max(T_t - t_floor, 0))) / (double)A_t);
  const double vol = est_query_chunks * kept * kept;
  return vol < 3200.0 ? 0u : vol < 12000.0 ? 1u : 2u;
}
// [r6] sg_plan2_kernel (two queries per wavefront) tokenises ASCII text with q <= 3 and one pad symbol, under a wrap of ASCII runes,
// and computes the five metrics of pkg/metric itself: any other description or a tabulated metric keeps sg_plan_kernel
bool plan2_usable(const sg_index* index, const Replica* rep, int metric) {
  const DeviceIndex& d = rep->dix;
  if (!index->knobs.plan2 || metric == SG_TABLE || d.q > 3u || d.q == 0u || d.n_pad != 1u || !d.slots || d.n_wrap0 > SG_WRAP_MAX || d.n_wrap1 > SG_WRAP_MAX) return false;
  for (uint32_t i = 0; i < d.n_wrap0; i++) if (d.wrap0[i] >= 128u) return false;
  for (uint32_t i = 0; i < d.n_wrap1; i++) if (d.wrap1[i] >= 128u) return false;
  return true;
}
bool pipe_wide(const sg_index* index, const Replica* rep) { return index->knobs.pipe_wide || rep->packed_chunks >= (1ull << 26); }

// What a launch does, decided before it allocates or enqueues anything.  One thing may change it afterwards: a pipeline launch
// whose block of records the device cannot give takes the fused kernel with the tokeniser launch instead (launch()).
struct LaunchPlan {
  int mode = 0, metric = 0;            // BatchArgs::autocomplete (2: by_doc) and ::metric (SG_TABLE: tabulated)
  bool long_list = false;              // a list of the queries beyond the wavefront kernel's tables, for sg_long_kernel
  bool reorder = false, ord_direct = false;   // heaviest queries first (query_order_*); per-block histograms instead of atomics
  uint32_t ord_blocks = 0;
  uint32_t split_min = 0, split_chunks = 0, slot_cap = 0, item_cap = 0;      // split queries (BatchArgs); split_min 0: none
  bool sample = false;                 // the kernels sample the statistics block for the tightening controller
  bool tight = false, roomy = false, slim = false, g8 = false;               // the fused kernel's instantiation and queue
  bool pretok = false;                 // the tokeniser as a launch of its own (on the pipeline: the plan launch's job)
  bool pipe = false;                   // plan -> stream -> verify, the fused kernel behind them
  uint32_t nw = 0, log2_cnt = 0, dt_bytes = 0;   // the stream workgroup: wavefronts, log2 of its counters, LDS of its descriptors
  bool wide = false;                   // 8-byte sub-row descriptors
  bool two = false; Plan2Args p2{};    // sg_plan2_kernel (two queries per wavefront) and its LDS
};

// the split-query queue's sizes: a slot per query (the parts' rows of all slots below 1 GiB), four items per query
void split_caps(LaunchPlan& p, uint32_t n_q, uint32_t k) {
  p.slot_cap = (uint32_t)std::min<size_t>(n_q, ((size_t)1 << 30) / ((size_t)SG_MAX_PARTS * k * 12));
  p.item_cap = std::min<uint32_t>(std::max<uint32_t>(n_q * 4u, 4096u), 262144u);
}

LaunchPlan plan_launch(sg_index* index, Replica* rep, const LaunchReq& r) {
  const uint32_t n_q = r.n_q, k = r.k;
  const volatile uint32_t* h = rep->h_fill;
  const Knobs& kn = index->knobs;
  LaunchPlan p;
  p.mode = r.by_doc ? 2 : r.autocomplete; p.metric = r.mt ? SG_TABLE : r.metric;
  p.long_list = rep->long_scratch && !r.no_long_queries;
  // heaviest queries first (query_order_kernel): a batch that fills the machine many times over, no order given by the caller
  // (flag: a launch over the queries a flag array marks — the order kernels make the list, heaviest first like any other)
  p.reorder = r.flag || (!r.sel && kn.order && n_q >= (kn.order == 1 ? 8192u : (uint32_t)kn.order));
  p.ord_blocks = (n_q + 1023u) / 1024u; p.ord_direct = p.ord_blocks <= SG_ORDER_DIRECT_BLOCKS;
  p.pretok = pretok_launch(index, n_q);
  p.g8 = rep->dix.has_g8 != 0u;             // dense terms with 8-bit gaps: the kG8 instantiations (full LDS layout)
  // [r6] Split queries, unless the launch will take the pipeline — judged on the controllers as they stand before this launch steps
  // them: a stream workgroup per query is the balance there.  (Round 5 had the two exclude each other the other way round, and an
  // index whose queries pass the splitting threshold — 25 M strings — dropped to the fused kernel without a word.)
  const bool tight_before = kn.tighten == 1 || (kn.tighten == 2 && rep->tighten.now(h, r.similarity));
  if (k <= SG_K_LDS && kn.split_chunks && !r.lm && !r.by_doc && !pipe_eligible(index, rep, r, tight_before, rep->pipe_guard.holding())) {
    // Splitting pays (1) when the batch cannot fill the machine by itself: every query above 2 MiB of postings is cut
    // into 1 MiB parts; (2) for the outliers of a big batch, which would otherwise be its tail: one wavefront streams
    // ~1/3000 of the machine's rate, so a query holding more than 2x the expected volume and more than ~1/30000 of the
    // batch's is cut into parts of a quarter of that.  A big batch of equally heavy queries is left alone.
    const double batch_chunks = (double)n_q * index->est_query_chunks;
    double smin = 2.0 * kn.split_chunks;
    if (n_q > 4096u) smin = std::max(smin, std::max(2.0 * index->est_query_chunks, batch_chunks / 30000.0));
    // (the figures above are in chunks of the u32 CSR — 4 postings; the kernel counts chunks of the packed store — SG_PPC)
    const double pk = 4.0 / SG_PPC;
    p.split_min = (uint32_t)std::min(smin * pk, 4.0e9);
    p.split_chunks = std::max<uint32_t>((uint32_t)(kn.split_chunks * pk), p.split_min / 4u);
    // an index whose queries do not come near the threshold (4x the expected volume) pays nothing for the machinery
    if (4.0 * index->est_query_chunks * pk < (double)p.split_min) p.split_min = 0;
  }
  if (p.split_min) split_caps(p, n_q, k);
  if (!r.lm && p.mode == 0) {
    p.tight = kn.tighten == 1;
    if (kn.tighten == 2 && h) { p.tight = rep->tighten.step(h, r.similarity); p.sample = true; }
  }
  // [r4] The large queue (11 wavefronts per CU instead of 12) only for the tightening instantiation (the full layout anyway)
  // and the docID-ordered mode (every candidate is a result).  Rounds 2-3 also gave it to launches whose recent queries had
  // more than ~1.25 results each; on the round-4 kernel the small one is as good or better for every such workload (same box,
  // small / large: words Jaccard 58.9 / 56.7 M q/s, families 33.4 / 32.5, cfg 5 39.5 / 37.1 M predictions/s —
  // profiles/r04t_*, r04s_spell_sweep.txt): a queue that fills is emptied by the overflow walk, a wavefront that is missing is missing
  // all the time.
  p.roomy = kn.roomy == 2 ? (p.tight || r.by_doc) : kn.roomy == 1;
  // the slim table sizes where they buy a wavefront per CU (engine.hip, Lds<>); the tightening instantiation has the full ones
  p.slim = !p.tight && !p.g8 && sg_lds_waves(kn.log2_cnt, k, p.roomy, true) > sg_lds_waves(kn.log2_cnt, k, p.roomy, false);
  // the pipeline on the controllers' state after this launch's step; the guard looks only at launches that could take it
  p.pipe = !p.split_min && pipe_eligible(index, rep, r, p.tight, false) &&
           !(kn.pipe == 2 && h && rep->pipe_guard.step(h, rep->pipe_queries.load(std::memory_order_relaxed)));
  if (!p.pipe) return p;
  // [r6] The stream workgroup's shape, per launch.  Which of the three measured shapes is fastest follows what a query of THIS
  // launch streams, not the index alone: 10 M strings want four wavefronts on 2^12 counters at Jaccard >= 0.5 (1.324 against
  // 1.346 ms; 8 M: 1.10 against 1.15) and eight on 2^13 at Cosine >= 0.4 (2.45 against 4.44 ms: the lighter shape leaves 40 % of
  // the queries unplanned).  The estimate: the index's expected query volume (tune_index) x the square of the share of a typical
  // query's lists that list skipping leaves under this metric and similarity (the lists left are the short ones); the cuts, 3 200
  // and 12 000 chunks, put all sixteen measured launches — 1 M ... 16 M strings under both — on their fastest shape
  // (profiles/r06final_shape_by_size.txt, r06final_shape_auto_by_size.txt).  Where the model is wrong, ShapeFloor corrects it.
  p.nw = kn.pipe_nw; p.log2_cnt = kn.pipe_log2_cnt; p.dt_bytes = kn.pipe_dt_bytes;
  if (kn.pipe_shape_auto && p.metric >= SG_JACCARD && p.metric <= SG_OVERLAP) {
    uint32_t shape = pipe_shape_model(index->est_query_chunks, index->terms_per_doc, kn.t_floor, p.metric, r.similarity);
    shape = (uint32_t)std::max(0, (int)shape + kn.pipe_shape_bias);
    shape = rep->shape_floor.step(h, rep->pipe_queries.load(std::memory_order_relaxed), shape);
    static const uint32_t kShape[3][3] = {{2u, 11u, 2048u}, {4u, 12u, 4096u}, {8u, 13u, 8192u}};
    p.nw = kShape[shape][0]; p.log2_cnt = kShape[shape][1]; p.dt_bytes = kShape[shape][2];
  } else rep->shape_floor.last.store(3u, std::memory_order_relaxed);   // (the knobs' / the index's own: its unplanned queries say nothing about the three)
  p.wide = pipe_wide(index, rep);                                         // sub-row descriptors of 8 bytes: a store of 2^26 chunks and more
  // [r6] two queries per plan wavefront (plan2.inc) where the description allows.  Its LDS — hence its wavefronts per SIMD — follows
  // the largest table of chunk offsets a query of <= 32 n-grams can need under this metric and similarity: n-grams x (segments of
  // the window + 1); queries beyond are planned one per wavefront inside the same launch.
  p.two = plan2_usable(index, rep, p.metric);
  if (p.two) {
    uint32_t need = 0;
    const int S_i = (int)rep->dix.S;
    for (int A_i = 1; A_i <= 32; A_i++) {
      const int lo = std::max(metric_min_y(p.metric, r.similarity, A_i), 0), hi = std::min(metric_max_y(p.metric, r.similarity, A_i), S_i - 1), W_i = hi - lo + 1;
      if (W_i >= 1 && W_i <= 32) need = std::max<uint32_t>(need, (uint32_t)A_i * (uint32_t)(W_i + 1));
    }
    p.p2.rows_cap = std::min<uint32_t>(std::max<uint32_t>(need, 64u), SG_PLAN2_ROWS_MAX);
    p.p2.half_words = std::max<uint32_t>(p.p2.rows_cap + 32u, SG_PIPE_ROWS_WORDS / 2u);
    p.p2.half_words = std::max<uint32_t>(p.p2.half_words, SG_PLAN2_RUNES + 96u);
  }
  return p;
}

// The SCRATCH_ROWS block: the top-k rows in HBM (k > SG_K_LDS) or the split-query queue (a 64-byte control head, then items, slot
// words, the parts' counts, rows and ids), then the ordered list of the queries, its control words and block histograms.
struct RowsLayout { size_t s = 0, id = 0, split = 0, items = 0, slot = 0, part_n = 0, part_s = 0, part_id = 0, ord = 0, ord_ctl = 0, bytes = 0; };
RowsLayout rows_layout(const LaunchPlan& p, uint32_t n_q, uint32_t k) {
  RowsLayout L;
  Carve c;
  if (k > SG_K_LDS) {
    L.s = c.take((size_t)n_q * k * 8); L.id = c.take((size_t)n_q * k * 4, 4);
  } else if (p.split_min) {
    L.split = c.take(64); L.items = c.take((size_t)p.item_cap * 16); L.slot = c.take((size_t)p.slot_cap * 8);
    L.part_n = c.take((size_t)p.slot_cap * SG_MAX_PARTS * 4, 4);
    L.part_s = c.take((size_t)p.slot_cap * SG_MAX_PARTS * k * 8); L.part_id = c.take((size_t)p.slot_cap * SG_MAX_PARTS * k * 4);
  }
  if (p.reorder) {   // (the block histograms follow the control words)
    L.ord = c.take((size_t)n_q * 4); L.ord_ctl = c.take(SG_ORDER_CTL_WORDS * 4); c.take(p.ord_direct ? (size_t)p.ord_blocks * 1024 : 0);
  }
  L.bytes = c.size();
  return L;
}

// The SCRATCH_PIPE block: its two counters, then a piece's records (SG_PIPE_PIECE queries at most), verify records, overflow
// blocks and candidate counts, then the batch's list of the queries handed back to the fused kernel.  ~5.2 KB per query of a piece
// (4 KB + 0.64 KB + an eighth of a 4 KB overflow block), so the block stays below ~345 MB whatever the batch (round 5: 8.5 KB per
// query of the batch, 17 GB for 2 M queries).
struct PipeLayout { uint32_t piece, vrec_words, ovf_cap; size_t rec, vrec, ovf, cand_n, fb_list, bytes; };
PipeLayout pipe_layout(uint32_t n_q, uint32_t cand_cap) {
  PipeLayout L;
  L.piece = std::min<uint32_t>(n_q, SG_PIPE_PIECE); L.vrec_words = sg_pipe_vrec_words(cand_cap); L.ovf_cap = std::max<uint32_t>(L.piece / 8u, 64u);
  Carve c;
  c.take(8);                                                    // fb_n, ovf_n (unless the ordering launch keeps them)
  L.rec = c.take((size_t)L.piece * SG_PIPE_REC_STRIDE * 4, 256); L.vrec = c.take((size_t)L.piece * L.vrec_words * 4);
  L.ovf = c.take((size_t)L.ovf_cap * SG_PIPE_OVF_WORDS * 4); L.cand_n = c.take(((size_t)L.piece * 4 + 255) & ~(size_t)255);
  L.fb_list = c.take(((size_t)n_q + 1) * 4);
  L.bytes = c.size();
  return L;
}

// ---- Test-only poison (sg_debug_poison; off by default).  While it is on, every region a call is meant to write before it reads —
// its share of the per-stream scratch blocks and the result rows of a host-buffer call — is filled first, on the call's stream, so that
// a read of a word this call did not write returns a pattern instead of an earlier call's leftover.  Regions launch() zeroes stay
// zeroed.  A value is chosen region by region so that a stale read can only make a row wrong, never send a kernel out of its arrays:
//   docIDs, score bits, slot words, aux words: the family's byte pattern (0xA5... / 0x5A...) — ids are copied and compared, never
//     indexed with; a slot's part total of 0xA5A5A5A5 never equals the finished count (<= SG_MAX_PARTS): no merge, the count shows it;
//   queue items: 0xFFFFFFFF, the hole marker (the parts launch skips it);
//   part_n: k, the largest count a part's row has: a stale count reads k entries of that part's poisoned row, inside the block;
//   lists of query numbers (the ordered list, the pipeline's fb_list, the long-query list's entries): 0, a query of every batch;
//   the tokeniser launch's n-gram counts: 0 (an empty query), its term ids: kNoTerm, which every reader skips.
// Left alone: the pipeline's records, verify records, overflow blocks and candidate counts (offsets and loop bounds of the stream /
// verify launches, with no value that is safe whatever a stale word meets), the ordering launch's control words and histograms.
// Cost when off: one load of the switch and a few untaken branches per call; nothing more is enqueued. ----
std::atomic<uint32_t> g_poison{0};             // 0 off, 1 the 0xA5 family, 2 the 0x5A family
enum PoisonRegion { PZ_ROWS = 0, PZ_PIPE = 1, PZ_PRETOK = 2, PZ_LONG_LIST = 3, PZ_PREDICT = 4, PZ_OUT_IDS = 5, PZ_OUT_SCORES = 6, PZ_OUT_COUNTS = 7 };
thread_local uint64_t t_poisoned[8];           // bytes poisoned per region by this thread's calls since sg_debug_poison_stats
inline uint32_t poison_mode() { return g_poison.load(std::memory_order_relaxed); }
inline uint32_t poison_word() { return poison_mode() == 2 ? 0x5A5A5A5Au : 0xA5A5A5A5u; }
int poison_fill(void* p, size_t bytes, PoisonRegion r, hipStream_t st) {       // the family's byte pattern
  if (!bytes) return SG_OK;
  HIP_TRY(hipMemsetAsync(p, (int)(poison_word() & 0xFFu), bytes, st));
  t_poisoned[r] += bytes;
  return SG_OK;
}
int poison_words(void* p, size_t n, uint32_t v, PoisonRegion r, hipStream_t st) {   // n 32-bit words of v
  if (!n) return SG_OK;
  HIP_TRY(hipMemsetD32Async((hipDeviceptr_t)p, (int)v, n, st));
  t_poisoned[r] += n * 4;
  return SG_OK;
}

BatchArgs batch_args(const sg_index* index, const Replica* rep, const LaunchReq& r, const LaunchPlan& p) {
  BatchArgs a{};
  a.ix = rep->dix;
  a.q_sel = r.sel; a.q_sel_n = r.sel_n;
  a.long_scratch = rep->long_scratch; a.long_lock = rep->long_lock; a.long_slot_bytes = rep->long_slot_bytes; a.long_max_seg = rep->long_max_seg;
  a.q_len = r.len; a.ac_first = r.ac_first; a.out_aux = r.out_aux;
  if (r.mt) a.mt = *r.mt;
  if (r.lm) { a.lm_values = r.lm->values; a.lm_from = r.lm->from; a.lm_to = r.lm->to; }
  a.q_blob = (const uint8_t*)r.q; a.q_offs = (const uint64_t*)r.offs;
  a.out_ids = (uint32_t*)r.ids; a.out_scores = (double*)r.scores; a.out_counts = (uint32_t*)r.counts;
  a.alpha = r.similarity; a.n_q = r.n_q; a.k = r.k; a.metric = p.metric; a.autocomplete = p.mode;
  a.log2_cnt = index->knobs.log2_cnt; a.t_floor = index->knobs.t_floor; a.filter_level = index->knobs.filter_level;
  a.prof = (unsigned long long*)g_prof_buf;
#ifdef SG_PHASE_TIMING
  a.dbg_skip = (uint32_t)env_int("SG_DEBUG_SKIP", 0, INT32_MAX, 0);
#endif
  a.split_min = p.split_min; a.split_chunks = p.split_chunks; a.slot_cap = p.slot_cap; a.item_cap = p.item_cap;
  if (p.sample) { a.fill_stat = rep->d_fill; a.fill_mask = r.n_q <= 1024u ? 0u : 31u; }
  a.cq_cap = sg_queue_cap(a.log2_cnt, r.k, p.roomy, p.slim);
  return a;
}

// ---- the kernel instantiations a plan takes (defined in the order the launch ladders named them: the device code's function
// order follows the host's first references) ----
using BatchKernel = void (*)(BatchArgs);
using PipeKernel = void (*)(BatchArgs, PipeArgs);
PipeKernel stream_kernel(uint32_t nw, bool wide) {   // nw: 2, 4 or 8 wavefronts of a workgroup
  static const PipeKernel kByShape[2][3] = {{sg_stream_kernel<8, true>, sg_stream_kernel<4, true>, sg_stream_kernel<2, true>},
                                            {sg_stream_kernel<8, false>, sg_stream_kernel<4, false>, sg_stream_kernel<2, false>}};
  return kByShape[wide ? 0 : 1][nw == 8 ? 0 : nw == 4 ? 1 : 2];
}

// plan -> stream -> verify over pieces of at most SG_PIPE_PIECE queries (positions of the ordered list, or of the batch), then the
// fused kernel over the queries they handed back, in its full LDS layout
int enqueue_pipeline(const sg_index* index, const Replica* rep, const BatchArgs& a, const LaunchPlan& p, const PipeLayout& L, char* blk,
                     uint32_t* order_ctl, hipStream_t stream) {
  const uint32_t n_q = a.n_q, k = a.k;
  PipeArgs pa{};
  pa.sub_log2 = index->knobs.pipe_sub;
  pa.stat = rep->d_fill; pa.stat_mask = n_q <= 1024u ? 0u : 255u;      // (one query in 256: a few hundred atomics on one line per launch)
  pa.log2_cnt = p.log2_cnt; pa.cand_cap = index->knobs.pipe_cand_cap; pa.vrec_words = L.vrec_words;
  // a stream workgroup's LDS (pipeline.inc): counters | sub-row descriptors of the query's groups + a dead one
  const size_t cnt_bytes = 4 * std::max<size_t>((size_t)1 << pa.log2_cnt, SG_PIPE_REC_WORDS);
  const size_t lds = std::min<size_t>((cnt_bytes + p.dt_bytes + 1279) / 1280 * 1280, 65536);   // (whole allocation granules: 40 960 B = four workgroups per CU with the defaults; a workgroup's limit is 64 KB)
  pa.dt_rows = (uint32_t)((lds - cnt_bytes - 16) / (p.wide ? 8 : 4) / (64u >> pa.sub_log2));     // (behind the table: a dead descriptor)
  pa.ovf_cap = L.ovf_cap; pa.rec = (uint32_t*)(blk + L.rec); pa.vrec = (uint32_t*)(blk + L.vrec); pa.ovf = (uint32_t*)(blk + L.ovf); pa.cand_n = (uint32_t*)(blk + L.cand_n);
  pa.fb_list = (uint32_t*)(blk + L.fb_list);
  if (order_ctl) { pa.fb_n = order_ctl + 1; pa.ovf_n = order_ctl + 2; }     // (zeroed by the ordering launch)
  else { pa.fb_n = (uint32_t*)blk; pa.ovf_n = (uint32_t*)blk + 1; HIP_TRY(hipMemsetAsync(blk, 0, 8, stream)); }
  const PipeKernel stream_k = stream_kernel(p.nw, p.wide), verify_k = k > SG_K_LDS ? sg_verify_kernel_bigk : sg_verify_kernel;
  for (uint32_t b0 = 0; b0 < n_q; b0 += L.piece) {
    pa.b0 = b0; pa.n = std::min(L.piece, n_q - b0);
    if (p.two) hipLaunchKernelGGL(sg_plan2_kernel, dim3((pa.n + 1u) / 2u), dim3(64), (size_t)p.p2.half_words * 8, stream, a, pa, p.p2);
    else hipLaunchKernelGGL(sg_plan_kernel, dim3(pa.n), dim3(64), 0, stream, a, pa);
    hipLaunchKernelGGL(stream_k, dim3(pa.n), dim3(64 * p.nw), lds, stream, a, pa);
    hipLaunchKernelGGL(verify_k, dim3(pa.n), dim3(64), 0, stream, a, pa);
    if (b0 + L.piece < n_q) HIP_TRY(hipMemsetAsync(pa.ovf_n, 0, 4, stream));       // (the next piece's overflow blocks)
  }
  BatchArgs fa = a;
  fa.q_sel = pa.fb_list; fa.q_sel_n = pa.fb_n; fa.cq_cap = sg_queue_cap(a.log2_cnt, k, p.roomy, false);
  hipLaunchKernelGGL(sg_search_kernel_loop, dim3(std::min<uint32_t>(n_q, 3072u)), dim3(64), lds_bytes(a.log2_cnt, k, p.roomy, false), stream, fa);
  return SG_OK;
}

BatchKernel fused_kernel(bool lm, bool tight, bool slim, bool g8) {
  if (g8 && lm) return sg_lm_kernel_g8;                 // (8-bit gaps: the full LDS layout)
  if (g8) return tight ? sg_search_kernel_tight_g8 : sg_search_kernel_g8;
  if (lm) return slim ? sg_lm_kernel_slim : sg_lm_kernel;
  if (tight) return sg_search_kernel_tight;
  return slim ? sg_search_kernel_slim : sg_search_kernel;
}
BatchKernel parts_kernel(bool tight, bool g8) {
  return g8 ? (tight ? sg_parts_kernel_tight_g8 : sg_parts_kernel_g8) : (tight ? sg_parts_kernel_tight : sg_parts_kernel);
}

// sg_debug_poison: the SCRATCH_ROWS block's regions (see poison_fill) — HBM top-k rows, the split-query queue but its zeroed control
// head, the ordered list of the queries but its control words.  by_doc_tables: a docID-ordered launch under a tabulated metric
// turns a row's score bits into table positions, so its HBM score rows are left alone.
int poison_rows(const LaunchPlan& p, const RowsLayout& R, char* b, uint32_t n_q, uint32_t k, bool by_doc_tables, hipStream_t st) {
  int rc = SG_OK;
  if (k > SG_K_LDS) {
    if (!by_doc_tables && (rc = poison_fill(b + R.s, (size_t)n_q * k * 8, PZ_ROWS, st))) return rc;
    if ((rc = poison_fill(b + R.id, (size_t)n_q * k * 4, PZ_ROWS, st))) return rc;
  } else if (p.split_min) {
    const size_t parts = (size_t)p.slot_cap * SG_MAX_PARTS;
    HIP_TRY(hipMemsetAsync(b + R.items, 0xFF, (size_t)p.item_cap * 16, st));
    t_poisoned[PZ_ROWS] += (size_t)p.item_cap * 16;
    if ((rc = poison_fill(b + R.slot, (size_t)p.slot_cap * 8, PZ_ROWS, st))) return rc;
    if ((rc = poison_words(b + R.part_n, parts, k, PZ_ROWS, st))) return rc;
    if ((rc = poison_fill(b + R.part_s, parts * k * 8, PZ_ROWS, st))) return rc;
    if ((rc = poison_fill(b + R.part_id, parts * k * 4, PZ_ROWS, st))) return rc;
  }
  if (p.reorder && (rc = poison_words(b + R.ord, n_q, 0u, PZ_ROWS, st))) return rc;
  return SG_OK;
}

// Every batch goes through here: plan, allocate, enqueue.
int launch(sg_index* index, Replica* rep, const LaunchReq& r) {
  const uint32_t n_q = r.n_q, k = r.k;
  const hipStream_t stream = r.stream;
  if (n_q == 0) return SG_OK;
  // top-k rows above SG_K_LDS entries live in HBM, k x 12 bytes per query: a batch whose rows would pass 1 GiB goes
  // through in pieces (the queries are independent)
  if (k > SG_K_LDS && !r.sel && (size_t)n_q * k * 12 > ((size_t)1 << 30)) {
    const uint32_t piece = (uint32_t)std::max<size_t>(1, ((size_t)1 << 30) / ((size_t)k * 12));
    for (uint32_t lo = 0; lo < n_q; lo += piece) {
      LaunchReq s = r;
      LmRanges lm{};
      s.offs = (const uint64_t*)r.offs + lo; s.n_q = std::min(piece, n_q - lo); s.sel_n = nullptr;
      s.ids = (uint32_t*)r.ids + (size_t)lo * k; s.counts = (uint32_t*)r.counts + lo;
      if (r.scores) s.scores = (double*)r.scores + (size_t)lo * k;
      if (r.lm) { lm = LmRanges{r.lm->values, r.lm->from + lo, r.lm->to + lo}; s.lm = &lm; }
      if (r.len) s.len = r.len + lo;
      if (r.out_aux) s.out_aux = r.out_aux + (size_t)lo * k;
      if (r.flag) s.flag = r.flag + lo;
      if (int rc = launch(index, rep, s)) return rc;
    }
    return SG_OK;
  }
  LaunchPlan p = plan_launch(index, rep, r);
  BatchArgs a = batch_args(index, rep, r, p);
  DeviceGuard dg;   // the launch goes to the replica's device whatever the calling thread's current device is
  HIP_TRY(dg.set(rep->device));
  void* blk = nullptr;
  if (p.long_list) {   // the list of queries beyond the wavefront kernel's tables (its count is zeroed below: by the ordering launch when there is one)
    if (int rc = stream_scratch(rep->device, stream, ((size_t)n_q + 1) * 4, &blk, SCRATCH_LONG_LIST)) return rc;
    a.long_list = (uint32_t*)blk;
  }
  const bool poison = poison_mode() != 0;
  if (poison && a.long_list) if (int rc = poison_words(a.long_list + 1, n_q, 0u, PZ_LONG_LIST, stream)) return rc;   // (not the count)
  const RowsLayout R = rows_layout(p, n_q, k);
  uint32_t* order_ctl = nullptr;            // (ctl[1], ctl[2]: the pipeline's counts of queries handed back and overflow blocks — zeroed with it)
  if (R.bytes) {
    if (int rc = stream_scratch(rep->device, stream, R.bytes, &blk, SCRATCH_ROWS)) return rc;
    char* b = (char*)blk;
    if (poison) if (int rc = poison_rows(p, R, b, n_q, k, r.mt != nullptr && p.mode == 2, stream)) return rc;
    if (k > SG_K_LDS) { a.scratch_s = (uint64_t*)(b + R.s); a.scratch_id = (uint32_t*)(b + R.id); }
    if (p.split_min) {
      HIP_TRY(hipMemsetAsync(b + R.split, 0, 64, stream));    // queue control words
      a.split_ctl = (uint32_t*)(b + R.split); a.items = (uint32_t*)(b + R.items); a.slot_ctl = (uint32_t*)(b + R.slot);
      a.part_n = (uint32_t*)(b + R.part_n); a.part_s = (uint64_t*)(b + R.part_s); a.part_id = (uint32_t*)(b + R.part_id);
    }
    if (p.reorder) {
      uint32_t* ord = (uint32_t*)(b + R.ord);
      order_ctl = (uint32_t*)(b + R.ord_ctl);
      uint32_t* blk_hist = p.ord_direct ? order_ctl + SG_ORDER_CTL_WORDS : nullptr;
      if (!p.ord_direct) HIP_TRY(hipMemsetAsync(order_ctl, 0, SG_ORDER_CTL_WORDS * 4, stream));   // (the direct path keeps no batch-wide histogram there)
      hipLaunchKernelGGL(query_order_count_kernel, dim3(p.ord_blocks), dim3(1024), 0, stream, (const uint64_t*)r.offs, r.len, n_q, p.mode == 1, order_ctl, r.flag,
                         blk_hist, a.long_list, nullptr);
      hipLaunchKernelGGL(query_order_scatter_kernel, dim3(p.ord_blocks), dim3(1024), 0, stream, (const uint64_t*)r.offs, r.len, n_q, p.mode == 1, ord, order_ctl,
                         r.flag, blk_hist);
      HIP_TRY(hipGetLastError());
      a.q_sel = ord; a.q_sel_n = order_ctl;
    }
  }
  if (a.long_list && !order_ctl) HIP_TRY(hipMemsetAsync(a.long_list, 0, 4, stream));
  // the pipeline's records; if the device cannot give them the launch takes the fused kernel with the tokeniser launch — less memory
  // — instead of failing (the one change to a plan after it is made)
  const PipeLayout P = pipe_layout(n_q, index->knobs.pipe_cand_cap);
  void* pipe_blk = nullptr;
  if (p.pipe && stream_scratch(rep->device, stream, P.bytes, &pipe_blk, SCRATCH_PIPE) != SG_OK) { p.pipe = false; (void)hipGetLastError(); }
  if (p.pipe && poison) if (int rc = poison_words((char*)pipe_blk + P.fb_list, (size_t)n_q + 1, 0u, PZ_PIPE, stream)) return rc;
  if (p.pipe) rep->pipe_queries.fetch_add(n_q, std::memory_order_relaxed);
  else if (p.pretok) {   // every query of the batch in the caller's numbering (the search launch may run them in another order), or the caller's subset
    Carve c;
    const size_t o_A = c.take((size_t)n_q * 4), o_terms = c.take((size_t)n_q * SG_MAX_A * 4, 256);
    void* pt = nullptr;
    if (int rc = stream_scratch(rep->device, stream, c.size(), &pt, SCRATCH_PRETOK)) return rc;
    a.pre_A = (int32_t*)((char*)pt + o_A); a.pre_terms = (uint32_t*)((char*)pt + o_terms);
    if (poison) {
      if (int rc = poison_words(a.pre_A, n_q, 0u, PZ_PRETOK, stream)) return rc;
      if (int rc = poison_words(a.pre_terms, (size_t)n_q * SG_MAX_A, kNoTerm, PZ_PRETOK, stream)) return rc;
    }
    BatchArgs ta = a;
    if (!r.flag) { ta.q_sel = r.sel; ta.q_sel_n = r.sel_n; }      // (the caller's subset; a flagged subset: the list just made)
    hipLaunchKernelGGL(sg_terms_kernel, dim3(n_q), dim3(64), 0, stream, ta);
    HIP_TRY(hipGetLastError());
  }
  if (p.pipe) {
    if (int rc = enqueue_pipeline(index, rep, a, p, P, (char*)pipe_blk, order_ctl, stream)) return rc;
  } else hipLaunchKernelGGL(fused_kernel(r.lm != nullptr, p.tight, p.slim, p.g8), dim3(n_q), dim3(64), lds_bytes(a.log2_cnt, k, p.roomy, p.slim), stream, a);
  HIP_TRY(hipGetLastError());
  if (a.split_ctl) {     // the queued parts of split queries: persistent wavefronts, which leave at once if there are none
    // the parts of a small batch are long streams on a machine they cannot fill anyway: they get 4x the counters (fewer
    // docID-range passes; the launch has its own LDS size).  q=2: one query 0.57 -> 0.43 ms, 256 queries +30 %.
    a.log2_cnt = std::min<uint32_t>(index->knobs.log2_cnt + (n_q <= 4096u ? index->knobs.parts_cnt_bonus : 0), 14u);
    a.cq_cap = sg_queue_cap(a.log2_cnt, k, p.roomy, false);
    hipLaunchKernelGGL(parts_kernel(p.tight, p.g8), dim3(index->parts_grid), dim3(64), lds_bytes(a.log2_cnt, k, p.roomy), stream, a);
    HIP_TRY(hipGetLastError());
  }
  if (a.long_list) {   // queries the wavefront kernel listed as beyond its tables: a few workgroups answer them (none listed: they leave at once)
    hipLaunchKernelGGL(sg_long_kernel, dim3(std::min<uint32_t>(n_q, 8u)), dim3(64), 0, stream, a);
    HIP_TRY(hipGetLastError());
  }
  // every fourth launch that fed the statistics block copies it to the host for the controllers (not hipMemcpyAsync: a 16-byte
  // device-to-host copy blocks the calling thread until the stream has drained — every fourth submit of a pipelined host stalled
  // for three batches, 5 ms, and the GPU idled behind it; a store from a kernel into mapped host memory is just another launch)
  if ((a.fill_stat || p.pipe) && (rep->launches.fetch_add(1, std::memory_order_relaxed) % 4u) == 0u) {
    hipLaunchKernelGGL(fill_stat_copy_kernel, dim3(1), dim3(64), 0, stream, (const uint32_t*)rep->d_fill, rep->h_fill_dev);
    HIP_TRY(hipGetLastError());
  }
  return SG_OK;
}

}  // namespace

#include "index_build.inc"
#include "lm_build.inc"
#include "forward_index.inc"
#include "packed_store.inc"

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
  int rc = check_search_args(index, k, true, similarity, metric);
  if (rc) return rc;
  LaunchReq r;
  r.q = d_q; r.offs = d_offs; r.n_q = n_q; r.metric = metric; r.similarity = similarity; r.k = k;
  r.ids = d_ids; r.scores = d_scores; r.counts = d_counts; r.stream = (hipStream_t)stream;
  return launch(index, replica_of_pointer(index, d_offs), r);
  SG_GUARD_END(SG_RC)
}

int sg_autocomplete_batch_device(sg_index* index, const void* d_q, const void* d_offs, uint32_t n_q, uint32_t limit,
                                 void* d_ids, void* d_counts, void* stream) {
  SG_GUARD_BEGIN
  int rc = check_search_args(index, limit, false, 0, 0);
  if (rc) return rc;
  LaunchReq r;
  r.q = d_q; r.offs = d_offs; r.n_q = n_q; r.k = limit; r.autocomplete = 1;
  r.ids = d_ids; r.counts = d_counts; r.stream = (hipStream_t)stream;
  return launch(index, replica_of_pointer(index, d_offs), r);
  SG_GUARD_END(SG_RC)
}

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

// a host-buffer search: metric, similarity, k, autocomplete, ac_first of r (by_doc and mt are set by the caller)
static LaunchReq search_req(int metric, double sim, uint32_t k, int autocomplete, uint32_t ac_first = 0) {
  LaunchReq r;
  r.metric = metric; r.similarity = sim; r.k = k; r.autocomplete = autocomplete; r.ac_first = ac_first;
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

// the enqueue step of a search: launch() on the device block, with what the caller's buffers say
static Enqueue search_enqueue(sg_index* index, Replica* rep, const LaunchReq& req, const HostBufs& b) {
  return [=](char* dev, const IoLayout& io, hipStream_t st) {
    LaunchReq r = req;
    r.q = dev + io.q; r.offs = dev + io.offs; r.n_q = b.n_q; r.stream = st; r.no_long_queries = no_long_queries(b.offs, b.n_q);
    r.ids = dev + io.ids; r.scores = r.autocomplete ? nullptr : dev; r.counts = dev + io.cnt;
    r.out_aux = b.aux ? (uint32_t*)(dev + io.aux) : nullptr;
    return launch(index, rep, r);
  };
}
static HostBufs search_bufs(const uint8_t* q, const uint64_t* offs, uint32_t n_q, const LaunchReq& r, uint32_t* ids, double* scores,
                            uint32_t* counts, uint32_t* aux) {
  return HostBufs{q, offs, n_q, r.k, ids, r.autocomplete ? nullptr : scores, counts, aux};
}

static int run_host(sg_index* index, Replica* rep, const uint8_t* q, const uint64_t* offs, uint32_t n_q, const LaunchReq& r,
                    uint32_t* ids, double* scores, uint32_t* counts, uint32_t* aux = nullptr) {
  const HostBufs b = search_bufs(q, offs, n_q, r, ids, scores, counts, aux);
  return run_host_call(rep->device, b, true, search_enqueue(index, rep, r, b));
}

int sg_suggest_batch(sg_index* index, const uint8_t* q, const uint64_t* offs, uint32_t n_q, int metric, double similarity,
                     uint32_t k, uint32_t* ids, double* scores, uint32_t* counts) {
  SG_GUARD_BEGIN
  int rc = check_search_args(index, k, true, similarity, metric);
  if (rc) return rc;
  if (!offs || !ids || !scores || !counts) { set_error("null argument"); return SG_E_INVALID; }
  return run_host(index, find_replica(index, -1), q, offs, n_q, search_req(metric, similarity, k, 0), ids, scores, counts);
  SG_GUARD_END(SG_RC)
}

int sg_autocomplete_batch(sg_index* index, const uint8_t* q, const uint64_t* offs, uint32_t n_q, uint32_t limit,
                          uint32_t* ids, uint32_t* counts) {
  SG_GUARD_BEGIN
  int rc = check_search_args(index, limit, false, 0, 0);
  if (rc) return rc;
  if (!offs || !ids || !counts) { set_error("null argument"); return SG_E_INVALID; }
  return run_host(index, find_replica(index, -1), q, offs, n_q, search_req(0, 0, limit, 1), ids, nullptr, counts);
  SG_GUARD_END(SG_RC)
}

// Autocomplete restricted to documents with docID >= first_doc: the `limit` smallest of those.  A caller that wants EVERY
// match (the reference streams them all to the caller's collector, pkg/suggest/autocomplete.go:40-77) pages through them:
// first_doc = 0, then last docID of the page + 1, until a page comes back short.
int sg_autocomplete_batch_from(sg_index* index, const uint8_t* q, const uint64_t* offs, uint32_t n_q, uint32_t first_doc, uint32_t limit,
                               uint32_t* ids, uint32_t* counts) {
  SG_GUARD_BEGIN
  int rc = check_search_args(index, limit, false, 0, 0);
  if (rc) return rc;
  if (!offs || !ids || !counts) { set_error("null argument"); return SG_E_INVALID; }
  return run_host(index, find_replica(index, -1), q, offs, n_q, search_req(0, 0, limit, 1, first_doc), ids, nullptr, counts);
  SG_GUARD_END(SG_RC)
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
  int rc = check_search_args(index, k, false, 0, 0);
  if (rc) return rc;
  if (!offs || !ids || !scores || !counts || !tables) { set_error("null argument"); return SG_E_INVALID; }
  if ((rc = check_tables(index, tables))) return rc;
  LaunchReq r = search_req(SG_JACCARD, 0.5, k, 0);
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
  int rc = check_search_args(index, limit, tables == nullptr, similarity, metric);
  if (rc) return rc;
  if (!offs || !ids || !scores || !counts) { set_error("null argument"); return SG_E_INVALID; }
  if ((rc = check_tables(index, tables))) return rc;
  LaunchReq r = tables ? search_req(SG_JACCARD, 0.5, limit, 0, first_doc) : search_req(metric, similarity, limit, 0, first_doc);
  r.by_doc = true;
  if (tables) r.mt = &tables->tab;
  return run_host(index, find_replica(index, -1), q, offs, n_q, r, ids, scores, counts, aux);
  SG_GUARD_END(SG_RC)
}

}  // extern "C"

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

static int async_submit(sg_index* index, const uint8_t* q, const uint64_t* offs, uint32_t n_q, int metric, double sim, uint32_t k,
                        int autocomplete, uint32_t* ids, double* scores, uint32_t* counts, uint32_t ac_first, sg_ticket** out, uint32_t replica = 0) {
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
  const LaunchReq r = search_req(metric, sim, k, autocomplete, ac_first);
  const HostBufs b = search_bufs(q, offs, n_q, r, ids, scores, counts, nullptr);
  if (int rc = begin_host_call(b, true, search_enqueue(index, rep, r, b), x, &t->call)) return rc;
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

int sg_suggest_submit(sg_index* index, const uint8_t* q, const uint64_t* offs, uint32_t n_q, int metric, double similarity, uint32_t k,
                      uint32_t* ids, double* scores, uint32_t* counts, sg_ticket** out) {
  SG_GUARD_BEGIN
  int rc = check_search_args(index, k, true, similarity, metric);
  if (rc) return rc;
  if (!offs || !ids || !scores || !counts) { set_error("null argument"); return SG_E_INVALID; }
  return async_submit(index, q, offs, n_q, metric, similarity, k, 0, ids, scores, counts, 0, out);
  SG_GUARD_END(SG_RC)
}

// The same on replica number `replica` of the index (0 = the primary; sg_index_replicas lists them): ONE host thread
// keeps every GPU of the node busy by submitting a slice of its batch to each replica and waiting for the tickets.
int sg_suggest_submit_on(sg_index* index, uint32_t replica, const uint8_t* q, const uint64_t* offs, uint32_t n_q, int metric, double similarity,
                         uint32_t k, uint32_t* ids, double* scores, uint32_t* counts, sg_ticket** out) {
  SG_GUARD_BEGIN
  int rc = check_search_args(index, k, true, similarity, metric);
  if (rc) return rc;
  if (!offs || !ids || !scores || !counts) { set_error("null argument"); return SG_E_INVALID; }
  return async_submit(index, q, offs, n_q, metric, similarity, k, 0, ids, scores, counts, 0, out, replica);
  SG_GUARD_END(SG_RC)
}

int sg_autocomplete_submit(sg_index* index, const uint8_t* q, const uint64_t* offs, uint32_t n_q, uint32_t first_doc, uint32_t limit,
                           uint32_t* ids, uint32_t* counts, sg_ticket** out) {
  SG_GUARD_BEGIN
  int rc = check_search_args(index, limit, false, 0, 0);
  if (rc) return rc;
  if (!offs || !ids || !counts) { set_error("null argument"); return SG_E_INVALID; }
  return async_submit(index, q, offs, n_q, 0, 0, limit, 1, ids, nullptr, counts, first_doc, out);
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

static int run_multi(sg_index* index, const uint8_t* q, const uint64_t* offs, uint32_t n_q, int metric, double sim, uint32_t k,
                     int autocomplete, uint32_t* ids, double* scores, uint32_t* counts) {
  std::vector<Replica*> reps;
  { std::lock_guard<std::mutex> lock(index->mu); for (auto& r : index->replicas) reps.push_back(r.get()); }
  const uint32_t R = (uint32_t)reps.size();
  if (R <= 1 || n_q < 2 * R) return run_host(index, reps[0], q, offs, n_q, search_req(metric, sim, k, autocomplete), ids, scores, counts);
  MultiPool* pool = multi_pool_of(index, R);
  std::vector<MultiTask> tasks(R);
  for (uint32_t r = 0; r < R; r++) {
    const uint32_t lo = (uint32_t)((uint64_t)n_q * r / R), hi = (uint32_t)((uint64_t)n_q * (r + 1) / R);
    Replica* rep = reps[r];
    tasks[r].fn = [=]() {
      return run_host(index, rep, q, offs + lo, hi - lo, search_req(metric, sim, k, autocomplete), ids + (size_t)lo * k,
                      scores ? scores + (size_t)lo * k : nullptr, counts + lo);
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
  int rc = check_search_args(index, k, true, similarity, metric);
  if (rc) return rc;
  if (!offs || !ids || !scores || !counts) { set_error("null argument"); return SG_E_INVALID; }
  return run_multi(index, q, offs, n_q, metric, similarity, k, 0, ids, scores, counts);
  SG_GUARD_END(SG_RC)
}

int sg_autocomplete_batch_multi(sg_index* index, const uint8_t* q, const uint64_t* offs, uint32_t n_q, uint32_t limit,
                                uint32_t* ids, uint32_t* counts) {
  SG_GUARD_BEGIN
  int rc = check_search_args(index, limit, false, 0, 0);
  if (rc) return rc;
  if (!offs || !ids || !counts) { set_error("null argument"); return SG_E_INVALID; }
  return run_multi(index, q, offs, n_q, 0, 0, limit, 1, ids, nullptr, counts);
  SG_GUARD_END(SG_RC)
}

}  // extern "C"

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
  const uint8_t* q; uint32_t len;
  int metric; double sim; uint32_t k; int autocomplete;
  uint32_t ac_first = 0;
  uint32_t* ids; double* scores; uint32_t* count;
  int rc = SG_OK;
  std::string err;
  std::atomic<int> state{0};      // 0 pending, 1 done, 2 the caller sleeps on `waiter`
  OneWaiter* waiter = nullptr;
  bool same_key(const OneReq& o) const { return metric == o.metric && sim == o.sim && k == o.k && autocomplete == o.autocomplete && ac_first == o.ac_first; }
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
      const uint32_t k = r->k, cnt = counts[i], m = cnt < k ? cnt : (cnt >= SG_COUNT_LM_ERROR ? 0u : k);
      const size_t at = row_offs ? (size_t)row_offs[i] : i * (size_t)k;
      *r->count = cnt;
#ifdef SG_PHASE_TIMING
      memcpy(r->ids, ids + at, (size_t)(row_offs ? m : k) * 4);   // (debug builds, a plain take: the whole row, it may carry debug words)
#else
      memcpy(r->ids, ids + at, (size_t)m * 4);
#endif
      if (!r->autocomplete) memcpy(r->scores, scores + at, (size_t)m * 8);
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
  std::map<std::tuple<int, uint64_t, uint32_t, int, uint32_t>, uint32_t> key_no;   // a mixed take: its keys, numbered as they first appear
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
          if ((*it)->same_key(*first)) { batch.push_back(*it); it = c->pending.erase(it); } else ++it;
        }
      } else {                                               // the oldest max_batch requests, whatever their keys: sorted out below, off the lock
        while (!c->pending.empty() && batch.size() < c->max_batch) { batch.push_back(c->pending.front()); c->pending.pop_front(); }
      }
    }
    if (mixed_take) {
      // the keys are numbered in order of first appearance, SG_MAX_MIXED_CONFIGS of them at the most: a request with one key more goes
      // back to the head of the queue, in its order, for the next take.  (The key holds the similarity's bits, -0 as +0: what
      // same_key calls equal.)
      size_t kept = 0;
      for (OneReq* r : batch) {
        const double sim = r->sim + 0.0;
        uint64_t sim_bits;
        memcpy(&sim_bits, &sim, 8);
        const auto key = std::make_tuple(r->metric, sim_bits, r->k, r->autocomplete, r->ac_first);
        auto it = key_no.find(key);
        if (it == key_no.end()) {
          if (key_no.size() == SG_MAX_MIXED_CONFIGS) { late.push_back(r); continue; }
          it = key_no.emplace(key, (uint32_t)key_no.size()).first;
          cfgs.push_back(sg_search_config{r->metric, r->autocomplete, r->sim, r->k, r->ac_first});
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
    if (!cfgs.empty()) {       // several keys: one mixed call, every caller's row cut out of the ragged rows
      const uint32_t n = (uint32_t)batch.size();
      const auto t_batch = std::chrono::steady_clock::now();
      int rc = SG_OK;
      std::string err;
      try {
        blob.clear(); offs.assign(1, 0);
        uint64_t rows = 0;
        for (OneReq* r : batch) { blob.insert(blob.end(), r->q, r->q + r->len); offs.push_back(blob.size()); rows += r->k; }
        ids.resize(rows); scores.resize(rows); counts.resize(n); row_offs.resize((size_t)n + 1);
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
    const struct { int metric; double sim; uint32_t k; int autocomplete; uint32_t ac_first; } f = {batch[0]->metric, batch[0]->sim, batch[0]->k, batch[0]->autocomplete, batch[0]->ac_first};
    const uint32_t n = (uint32_t)batch.size(), k = f.k;
    const auto t_batch = std::chrono::steady_clock::now();
    int rc = SG_OK;
    std::string err;
    try {
      blob.clear(); offs.assign(1, 0);
      for (OneReq* r : batch) { blob.insert(blob.end(), r->q, r->q + r->len); offs.push_back(blob.size()); }
      ids.resize((size_t)n * k); counts.resize(n);
      if (!f.autocomplete) scores.resize((size_t)n * k);
      rc = run_host(c->index, rep, blob.data(), offs.data(), n, search_req(f.metric, f.sim, k, f.autocomplete, f.ac_first), ids.data(),
                    f.autocomplete ? nullptr : scores.data(), counts.data());
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
  int rc = check_search_args(index, k, true, similarity, metric);
  if (rc) return rc;
  if ((!q && len) || !out_ids || !out_scores || !out_count) { set_error("null argument"); return SG_E_INVALID; }
  OneReq r;
  r.q = q; r.len = len; r.metric = metric; r.sim = similarity; r.k = k; r.autocomplete = 0;
  r.ids = out_ids; r.scores = out_scores; r.count = out_count;
  return submit_one(index, r);
  SG_GUARD_END(SG_RC)
}

static int autocomplete_one_from(sg_index* index, const uint8_t* q, uint32_t len, uint32_t first_doc, uint32_t limit, uint32_t* out_ids, uint32_t* out_count) {
  int rc = check_search_args(index, limit, false, 0, 0);
  if (rc) return rc;
  if ((!q && len) || !out_ids || !out_count) { set_error("null argument"); return SG_E_INVALID; }
  OneReq r;
  r.q = q; r.len = len; r.metric = 0; r.sim = 0; r.k = limit; r.autocomplete = 1; r.ac_first = first_doc;
  r.ids = out_ids; r.scores = nullptr; r.count = out_count;
  return submit_one(index, r);
}
int sg_autocomplete_one(sg_index* index, const uint8_t* q, uint32_t len, uint32_t limit, uint32_t* out_ids, uint32_t* out_count) {
  SG_GUARD_BEGIN
  return autocomplete_one_from(index, q, len, 0, limit, out_ids, out_count);
  SG_GUARD_END(SG_RC)
}
int sg_autocomplete_one_from(sg_index* index, const uint8_t* q, uint32_t len, uint32_t first_doc, uint32_t limit, uint32_t* out_ids, uint32_t* out_count) {
  SG_GUARD_BEGIN
  return autocomplete_one_from(index, q, len, first_doc, limit, out_ids, out_count);
  SG_GUARD_END(SG_RC)
}

}  // extern "C"

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
  int rc = check_search_args(index, top_k, true, similarity, SG_COSINE);
  if (rc) return rc;
  if (!lm || !offs || !ids || !counts) { set_error("null argument"); return SG_E_INVALID; }
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
  const HostBufs b{q_utf8, q_offs, n_q, top_k + 1, out_ids, nullptr, out_counts, nullptr};
  return run_host_call(rep->device, b, false, [&](char* dev, const IoLayout& io, hipStream_t st) {
    return predict_on_device(index, lm, rep, (const uint8_t*)(dev + io.q), (const uint64_t*)(dev + io.offs), n_q, io.q_bytes, top_k, similarity,
                             (uint32_t*)(dev + io.ids), (uint32_t*)(dev + io.cnt), st);
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
  std::vector<uint32_t> words_tmp, unknown_tmp;                  // (the host-buffer path copies both rows back)
  if (!out_words) { words_tmp.resize(n); out_words = words_tmp.data(); }
  if (!out_unknown) { unknown_tmp.resize(n); out_unknown = unknown_tmp.data(); }
  const HostBufs b{text, offs, n, 1, out_words, out_scores, out_unknown, nullptr};
  return run_host_call(device, b, true, [&](char* dev, const IoLayout& io, hipStream_t st) {
    return lm_score_on_device(lm, device, true, (const uint8_t*)(dev + io.q), io.q_bytes, nullptr, (const uint64_t*)(dev + io.offs), n, 0, (double*)dev,
                              (uint32_t*)(dev + io.ids), (uint32_t*)(dev + io.cnt), st);
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
  // the host-buffer path moves bytes: the ids as a blob, offsets in bytes from the first sentence's ids on
  std::vector<uint64_t> boffs((size_t)n + 1);
  for (uint32_t i = 0; i <= n; i++) boffs[i] = (offs[i] - offs[0]) * 4;
  std::vector<uint32_t> rows_a(n), rows_b(n);                    // (the two u32 rows of the host-buffer block: unused here)
  const HostBufs b{(const uint8_t*)(ids ? ids + offs[0] : nullptr), boffs.data(), n, 1, rows_a.data(), out_scores, rows_b.data(), nullptr};
  const uint64_t n_ids = offs[n] - offs[0];
  return run_host_call(device, b, true, [&](char* dev, const IoLayout& io, hipStream_t st) {
    return lm_score_on_device(lm, device, false, nullptr, 0, (const uint32_t*)(dev + io.q), (const uint64_t*)(dev + io.offs), n, n_ids, (double*)dev,
                              nullptr, nullptr, st);
  });
  SG_GUARD_END(SG_RC)
}

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
