// capi.inc — host side of libsuggest_hip, included by engine.hip: the list of the host files, one per concern, in the order the text
// always had (the device code's function order follows the host's first mention of each kernel: see the note above stream_kernel()),
// and in place between them the launch section — LaunchReq, scratch, plan_launch, layouts, the poison, batch_args, launch().

#include "host_base.inc"
#include "handles.inc"
namespace {
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
// memory, until its gather launch is enqueued.  An edit-distance call (edit_rank.inc) holds SCRATCH_EDIT — the list of long rows, the
// long kernel's regions, a sort's arrays, sg_suggest_batch_edit's candidate rows — around the search launch it may contain.
// An edit search (edit_search.inc) holds SCRATCH_EDIT_SEARCH alone: a chunk's rows and, where the caller wants none, the histograms.
enum ScratchTag { SCRATCH_ROWS = 0, SCRATCH_PREDICT = 1, SCRATCH_LONG_LIST = 2, SCRATCH_PRETOK = 3, SCRATCH_PIPE = 4, SCRATCH_LM_SCORE = 5, SCRATCH_SHARD = 6,
                  SCRATCH_MIXED = 7, SCRATCH_MIXED_ROWS = 8, SCRATCH_DICT = 9, SCRATCH_EDIT = 10, SCRATCH_EDIT_SEARCH = 11 };
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

#include "tune.inc"
#include "index_api.inc"
#include "host_call.inc"
#include "search_api.inc"
#include "tickets.inc"
#include "multi.inc"
#include "coalescer.inc"
#include "lm_api.inc"
#include "debug_api.inc"
