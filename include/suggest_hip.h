/* suggest_hip.h — C ABI of libsuggest_hip.so, the MI355X (gfx950) engine behind suggest-go's
 * n-gram fuzzy-search path.
 *
 * The reference has no FFI; its extension seam is the pair of Go interfaces
 *   suggest.Builder{Build() (NGramIndex, error)}          pkg/suggest/ngram_index_builder.go:14-17
 *   suggest.NGramIndex = Suggester + Autocomplete          pkg/suggest/ngram_index.go:7-10
 * consumed by Service.AddIndex / Suggest / Autocomplete    pkg/suggest/service.go:78-173.
 * A cgo shim implementing those two interfaces binds exactly the entry points below
 * (see INTEGRATION.md for the shim).  Every function cites the reference code it replaces.
 *
 * Conventions: return 0 on success, a negative SG_E_* code on failure (sg_last_error() gives a
 * thread-local message); the caller owns every host buffer; the library owns device memory;
 * no callbacks; every entry point may be called concurrently from any thread on the same handle
 * (the handle is immutable after sg_index_upload and reference counted).
 */
#ifndef SUGGEST_HIP_H
#define SUGGEST_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct sg_index sg_index;

/* IndexDescription — pkg/suggest/config.go:25-35 (the fields the tokenizer and index use) */
typedef struct sg_desc {
  uint32_t ngram_size;          /* NGramSize, 1..8 (pkg/analysis/ngram_tokenizer.go:3) */
  const char* wrap_start;       /* Wrap[0], UTF-8, NUL terminated */
  const char* wrap_end;         /* Wrap[1] */
  const char* pad;              /* Pad */
  const char* const* alphabet;  /* Alphabet: "english" | "russian" | "numbers" | literal rune set
                                   (pkg/alphabet/alphabet.go:23-36) */
  uint32_t n_alphabet;
} sg_desc;

/* metric.Metric implementations — pkg/metric/{jaccard,cosine,dice,exact,overlap}.go */
enum sg_metric { SG_JACCARD = 0, SG_COSINE = 1, SG_DICE = 2, SG_EXACT = 3, SG_OVERLAP = 4 };

enum sg_error {
  SG_OK = 0,
  SG_E_INVALID = -1,      /* bad argument (k == 0, similarity outside (0,1], q outside 1..8 ...) —
                             the checks of NewSearchConfig, pkg/suggest/search.go:18-35 */
  SG_E_UNSUPPORTED = -2,  /* description outside what the packed 64-bit term key can hold */
  SG_E_NOT_UPLOADED = -3,
  SG_E_HIP = -4,          /* HIP runtime error; message has the hipError string */
  SG_E_NOMEM = -5         /* out of memory: host (message "out of host memory") or device — every failed hipMalloc of an
                             upload, build, store, load, language model or metric table ("hipMalloc: <hipError string>");
                             upload, the language model's upload and sg_metric_tables_create returned SG_E_HIP for it once */
};

/* Values stored in out_counts[i] instead of a count, for queries the reference itself does not
 * answer (pkg/suggest/suggester.go:62: the clipped window [bMin,bMax] is empty) and for queries
 * beyond the device path's limits.  Rows of such queries are left zeroed. */
#define SG_COUNT_REF_PANIC 0xFFFFFFFFu     /* reference: make(chan, negative) panics */
#define SG_COUNT_REF_DEADLOCK 0xFFFFFFFEu  /* reference: capacity-0 channel, send blocks forever */
#define SG_COUNT_TOO_LONG 0xFFFFFFFDu      /* more than SG_MAX_QUERY_TERMS n-grams (queries above 128 n-grams take a slower kernel) */
#define SG_COUNT_LM_ERROR 0xFFFFFFFCu       /* LanguageModel.Next returned an error (sg_spell_predict_batch) */
#define SG_MAX_QUERY_TERMS 65536u
#define SG_MAX_TOPK 65536u

/* suggest.Index + Writer.AddDocument/Commit + Reader.Read
 * (pkg/suggest/indexer.go:14-45, pkg/index/indexer_writer.go:66-145, index_reader.go:29-120):
 * tokenises docs[i] = utf8[offs[i]..offs[i+1]) (docID = i, dictionary order) and builds the
 * cardinality-segmented inverted index as term-major CSR in host memory. */
int sg_index_build(const uint8_t* utf8, const uint64_t* offs, uint32_t n_docs, const sg_desc* desc, sg_index** out);

/* Same index, built on the GPU `device`: documents are tokenised by the kernel-side tokenizer, terms
 * interned in a device hash table, postings radix-sorted and laid out as the same CSR — array for array identical to
 * sg_index_build's (sg_index_digest).  Fails with SG_E_UNSUPPORTED when a document has more than 65 536 bytes or the
 * dictionary 2^26 documents or more (use sg_index_build).  The index still has to be uploaded with sg_index_upload. */
int sg_index_build_device(const uint8_t* utf8, const uint64_t* offs, uint32_t n_docs, const sg_desc* desc, int device,
                          sg_index** out);

/* Either builder (device < 0: host) with at least `min_segments` cardinality segments: the shards of a dictionary split by
 * docID range (suggest_amd/distributed.py) agree on the global number, so that every shard clips the
 * window [MinY, MaxY] at the same segment (suggester.go:57-59) as the unsharded index would.  This builds ONE shard:
 * sg_sharded_build builds, uploads and searches all of them behind one handle; sg_sharded_adopt takes shards built here. */
int sg_index_build_ex(const uint8_t* utf8, const uint64_t* offs, uint32_t n_docs, const sg_desc* desc, uint32_t min_segments,
                      int device, sg_index** out);
/* Test hooks like the other sg_debug_* entries (bindings need not mirror them).  sg_debug_index_build_table_bits, process-wide
 * (like sg_debug_lm_build_hash_bits): the device builder starts its term table at exactly 2^bits slots — bits 4 .. 20 — instead of
 * 2^20 or a sixteenth of the dictionary's rune capacity, whichever is larger; 0 restores that default.  Either way the table grows
 * fourfold, with the tokenise pass repeated, once more than half of it is taken.  sg_debug_index_build_report: the calling thread's last
 * device build (sg_index_build_device, sg_index_build_ex with device >= 0; all zero if it tokenised nothing), failed ones
 * included — out = {tokenise passes; log2 of the slots of the final table; terms interned by the last pass; documents the long
 * tokeniser took in the last pass (those above 128 n-grams)}.  No reference counterpart. */
int sg_debug_index_build_table_bits(uint32_t bits);
int sg_debug_index_build_report(uint32_t out[4]);

/* NewFSBuilder + Reader.Read (pkg/suggest/ngram_index_builder.go:44-83, pkg/index/index_reader.go:29-120): loads an
 * index the reference itself built — <name>.hd (gob header) and <name>.dl (VB / skip-VB / roaring posting lists,
 * pkg/index/codec.go:39-51) — into the same CSR.  `desc` must be the IndexDescription the files were built with. */
int sg_index_load_reference(const char* hd_path, const char* dl_path, const sg_desc* desc, sg_index** out);
/* The same load with the posting lists decoded on a GPU.  device < 0 is sg_index_load_reference itself: the host
 * reader, no GPU initialised.  device >= 0 uploads the .dl and decodes its VB / skip-VB / roaring lists there in two passes (count,
 * then write) with the positions scanned on the host between them; the handle's CSR — postings, offsets, lengths, terms, the
 * repeats table, the counters — is word for word the host reader's for every file it accepts, and every file it refuses is refused
 * with the same code and message (SG_E_INVALID names the term of the first malformed list).  The header parse, the term interning,
 * the position scan and the term table stay on the host.  Needs no sg_index_upload and makes no replica: it works in memory of its
 * own on a stream of its own and frees it before it returns.  A header that gives one (term, segment) pair two lists, and a
 * roaring list whose values do not strictly ascend, are decoded by the host's decoders: no writer emits either. */
int sg_index_load_reference_ex(const char* hd_path, const char* dl_path, const sg_desc* desc, int device, sg_index** out);
/* Test hook like the other sg_debug_* entries (tools/index_load_timing.py reads it; bindings need not mirror it): milliseconds the
 * calling thread's last successful sg_index_load_reference_ex spent — out_ms[0 .. min(cap, 7)) = {reading the files; parsing the
 * header and interning the terms; host-to-device copies with the kernels' input tables; the kernels (device < 0: the host
 * decoders); device-to-host copies; assembly on the host: positions, repeats, the term table; the whole call}.  No reference
 * counterpart. */
int sg_debug_index_load_times(double* out_ms, uint32_t cap);

/* Writer.Commit (pkg/index/indexer_writer.go:88-167) + index.NewEncoder (pkg/index/codec.go:17-51): saves the index as the
 * <name>.hd / <name>.dl pair sg_index_load_reference and the reference's NewFSBuilder open — what the reference's `indexer`
 * command leaves behind.  device >= 0 encodes the posting lists on that GPU (VB, skip blocks of 64, roaring after RunOptimize;
 * DESIGN.md §4f), device < 0 with the host encoder; both write the same bytes.  Works on any handle — host-built, device-built,
 * loaded from reference files — and needs no sg_index_upload: the device path stages the host CSR into memory of its own, on a
 * stream of its own, frees it before it returns and touches no replica.  The terms are written segment ascending, then in the
 * order of sg_index_lists (the reference's order is Go-map random).  SG_E_INVALID: a file cannot be written (the .dl is written
 * first; a failed store may leave it behind); SG_E_UNSUPPORTED: the .dl would reach 4 GiB (PostingListPosition is a uint32: the
 * reference would wrap it silently). */
int sg_index_store_reference(sg_index* index, const char* hd_path, const char* dl_path, int device);
/* dictionary.BuildCDBDictionary (pkg/dictionary/helpers.go:52-95): key = docID as 4 LE bytes, value = the line — the <name>.cdb
 * the reference's services open beside the index.  docs[i] = utf8[offs[i]..offs[i+1]), records in docID order. */
int sg_dictionary_store_cdb(const uint8_t* utf8, const uint64_t* offs, uint32_t n_docs, const char* cdb_path);
/* Test hook like the other sg_debug_* entries (tools/index_store_timing.py reads it; bindings need not mirror it): seconds the
 * calling thread's last sg_index_store_reference spent — out = {encoding: the kernels, or the host encoder, each with the position
 * scan and without the list table both modes build first; staging: the kernels' input tables and the copies to and from the
 * device, 0 on the host; building and writing the header; the whole call}.  No reference counterpart. */
int sg_debug_index_store_times(double out[4]);

/* Copies the CSR index into the HBM of `device` (one replica per GPU; per-process).  The first upload makes the primary
 * replica (the one sg_suggest_batch / sg_autocomplete_batch run on); uploading to a device that already holds a replica is
 * a no-op.  A device-built index (sg_index_build_device) whose first upload goes to the building device keeps the posting
 * store where the build left it (no D2H + H2D round trip).  Safe to call concurrently.  SG_E_UNSUPPORTED: the packed
 * posting store numbers documents below 2^29 (a larger dictionary is sharded by docID range behind one handle:
 * sg_sharded_build, below). */
int sg_index_upload(sg_index* index, int device);

/* Multi-GPU (BASELINE north_star: "query batches shard naturally across the 8 GPUs of one node"): ONE host
 * build, one replica per listed device.  A device listed j times ends up with j replicas (only useful to exercise the
 * multi-replica paths on a one-GPU box).  Replicas already present are kept. */
int sg_index_replicate(sg_index* index, const int* devices, uint32_t n_devices);
/* Devices of the replicas in upload order (primary first): fills up to cap entries, returns their number. */
uint32_t sg_index_replicas(sg_index* index, int* out_devices, uint32_t cap);

/* nGramSuggester.Suggest for a batch of queries — pkg/suggest/suggester.go:46-131 with
 * newFuzzyCollectorManager(k) (collector.go:143-149): tokenise, window [MinY,MaxY], per segment
 * T-occurrence merge (pkg/index/searcher.go:28-78, pkg/merger/cp_merge.go:19-120 result set),
 * score 1-Distance (scorer.go:29-31), top-k by (score desc, docID asc) (collector.go:20-26,
 * topk.go:82-147).  Row i of out_ids/out_scores (k entries each) holds the candidates of query i
 * best first; out_counts[i] = how many (or an SG_COUNT_* flag).  Host buffers; synchronous. */
int sg_suggest_batch(sg_index* index, const uint8_t* q_utf8, const uint64_t* q_offs, uint32_t n_q, int metric,
                     double similarity, uint32_t k, uint32_t* out_ids, double* out_scores, uint32_t* out_counts);

/* Same, on buffers already resident in HBM; enqueued on `stream` (a hipStream_t of that device, NULL = the legacy default
 * stream) and asynchronous w.r.t. the host.  With several replicas the one on the device that owns d_q_offs runs it. */
int sg_suggest_batch_device(sg_index* index, const void* d_q_utf8, const void* d_q_offs, uint32_t n_q, int metric,
                            double similarity, uint32_t k, void* d_out_ids, void* d_out_scores, void* d_out_counts,
                            void* stream);

/* nGramAutocomplete.Autocomplete with newFirstKCollectorManager(limit) —
 * pkg/suggest/autocomplete.go:40-77, collector.go:48-115: the `limit` smallest docIDs whose
 * n-gram set contains every n-gram of the (tail-unwrapped) query. */
int sg_autocomplete_batch(sg_index* index, const uint8_t* q_utf8, const uint64_t* q_offs, uint32_t n_q,
                          uint32_t limit, uint32_t* out_ids, uint32_t* out_counts);
int sg_autocomplete_batch_device(sg_index* index, const void* d_q_utf8, const void* d_q_offs, uint32_t n_q,
                                 uint32_t limit, void* d_out_ids, void* d_out_counts, void* stream);

/* sg_suggest_batch / sg_autocomplete_batch over every replica of the index: the batch is cut into contiguous slices, one per
 * replica, every slice is in flight (copy in, launch, copy out on that device's stream) before the first is awaited, and
 * rows land in caller order.  No collective: queries are independent and the index is read-only.  With
 * one replica these are the plain calls. */
int sg_suggest_batch_multi(sg_index* index, const uint8_t* q_utf8, const uint64_t* q_offs, uint32_t n_q, int metric,
                           double similarity, uint32_t k, uint32_t* out_ids, double* out_scores, uint32_t* out_counts);
int sg_autocomplete_batch_multi(sg_index* index, const uint8_t* q_utf8, const uint64_t* q_offs, uint32_t n_q,
                                uint32_t limit, uint32_t* out_ids, uint32_t* out_counts);

/* ---- a dictionary sharded by docID range behind one handle ---------------------------
 * For dictionaries past one index's limits — 2^29 documents per upload, 2^26 per device build, one GPU's HBM per replica: W
 * shards, each an sg_index over the documents [doc_lo, doc_lo + n) under local docIDs, on one GPU or several.  One call searches
 * the whole batch on every shard and a merge launch (sg_shard_merge_kernel) combines the per-shard top-k rows on the device of
 * shard 0 under the reference's total order (score desc, docID asc; collector.go:20-26); rows come back with dictionary-wide
 * docIDs, which may use all of uint32 while every shard stays below 2^29 documents.  A query that any shard flags (SG_COUNT_*)
 * stays flagged, its row zeroed; slots past a row's count are zero.
 * That order is total, so the rows equal the unsharded index's for dictionaries without documents that repeat a term.  With such
 * documents the primary entries are the same, but the reference's SECONDARY duplicate rows depend on the relative
 * lengths of posting lists, which differ inside a shard: those rows can differ from the unsharded index's (they always equal the
 * merge of the shards' own rows).
 * Concurrency: any number of threads may call one handle at once.  A host-buffer call stages, copies and waits on the calling
 * thread's own stream and buffers, as sg_suggest_batch does; on a handle with several lanes it holds a mutex in the handle while
 * it enqueues on the lanes' streams, no longer.  A handle with one lane takes no lock, and neither does the device-resident call,
 * which writes nothing of the handle.
 * A host-buffer call goes the way of every other one, so a batch whose inputs or merged rows pass 64 MiB is copied straight from
 * and to the caller's memory instead of through pinned staging, and a batch whose offsets do not start at zero AND whose inputs
 * pass 64 MiB is refused: SG_E_INVALID, "batch slice too large to stage". */
typedef struct sg_sharded sg_sharded;
#define SG_MAX_SHARDS 64u        /* a design limit: 8 GPUs with 8 shards each */

/* Cuts docs [0, n_docs) into n_shards (1 .. SG_MAX_SHARDS) contiguous docID ranges, builds every non-empty one with the global
 * number of cardinality segments (the shards short of it are built again with min_segments, as sg_index_build_ex does), and
 * uploads shard s to devices[s % n_devices].  Ranges differ in size by at most one, by the rule of distributed.shard_bounds: the
 * first n_docs % n_shards ranges hold one more.  A range without documents (n_shards > n_docs) is not built: it adds no rows and
 * no flag (range 0 always is, so that an empty dictionary answers like an empty index).  build_device >= 0: the path of
 * sg_index_build_device on the shard's own device; < 0: the host builder.  An entry of `devices` is a lane: the shards of one
 * lane are searched one after the other on one stream, lanes side by side; a device listed twice makes two lanes (only
 * useful to exercise the path for rows from another device on a one-GPU box). */
int sg_sharded_build(const uint8_t* utf8, const uint64_t* offs, uint32_t n_docs, const sg_desc* desc, uint32_t n_shards,
                     const int* devices, uint32_t n_devices, int build_device, sg_sharded** out);

/* Adopts handles that are already built and uploaded, and retains each: doc_lo[s] = the dictionary docID of shard s's document
 * 0.  For shards loaded with sg_index_load_reference, or built elsewhere.  A lane per device.  SG_E_INVALID: n_shards outside
 * 1 .. SG_MAX_SHARDS, doc_lo that does not ascend, a range doc_lo[s] + n_docs_s that reaches into the next shard's or passes
 * 2^32, a handle that is not uploaded, shards whose n_segments or descriptions differ. */
int sg_sharded_adopt(sg_index* const* shards, const uint64_t* doc_lo, uint32_t n_shards, sg_sharded** out);

void sg_sharded_retain(sg_sharded* sharded);
void sg_sharded_release(sg_sharded* sharded);
/* The shards that stand, in docID order: fills up to cap entries of out_doc_lo / out_devices (either may be NULL), returns their number. */
uint32_t sg_sharded_shards(const sg_sharded* sharded, uint64_t* out_doc_lo, int* out_devices, uint32_t cap);

/* sg_suggest_batch over every shard, merged: host buffers, synchronous.  The queries are uploaded once, to shard 0's device,
 * and copied from there once to every other device that holds a lane; the batch goes through in slices of queries whose
 * [shard][query][k] block of ids, scores and counts stays within 256 MiB, and the merged rows of the whole batch come back in
 * one copy; rows of a lane other than shard 0's are copied to its block asynchronously behind their searches and ordered by
 * events. */
int sg_sharded_suggest_batch(sg_sharded* sharded, const uint8_t* q_utf8, const uint64_t* q_offs, uint32_t n_q, int metric,
                             double similarity, uint32_t k, uint32_t* out_ids, double* out_scores, uint32_t* out_counts);
/* The same on buffers resident in HBM, asynchronous on `stream` — searches and merge are enqueued there, the shards' rows stay
 * in HBM.  Needs every shard on the device that owns the buffers: SG_E_UNSUPPORTED otherwise. */
int sg_sharded_suggest_batch_device(sg_sharded* sharded, const void* d_q_utf8, const void* d_q_offs, uint32_t n_q, int metric,
                                    double similarity, uint32_t k, void* d_out_ids, void* d_out_scores, void* d_out_counts,
                                    void* stream);
/* sg_autocomplete_batch over every shard: the shards own ascending docID ranges, so the merged row is their rows one after the
 * other, cut at `limit`. */
int sg_sharded_autocomplete_batch(sg_sharded* sharded, const uint8_t* q_utf8, const uint64_t* q_offs, uint32_t n_q,
                                  uint32_t limit, uint32_t* out_ids, uint32_t* out_counts);
/* Test hooks (bindings need not mirror them).  sg_debug_shard_slice_bytes, process-wide: lowers the 256 MiB budget of the
 * [shard][query][k] block — a slice holds max(1, budget / (shards * (k * 12 + 4))) queries, k * 4 + 4 for autocomplete —
 * 0 restores it.  sg_debug_shard_merge: the merge launch alone over host arrays laid out as that block — ids, scores
 * [n_shards][n_q][k] with local docIDs, counts [n_shards][n_q], doc_lo [n_shards]; autocomplete != 0: no scores (scores and
 * out_scores may be NULL); sg_debug_shard_merge_time: the milliseconds between two events around the launch of the calling
 * thread's last sg_debug_shard_merge (tools/shard_timing.py reads it). */
int sg_debug_shard_slice_bytes(uint32_t bytes);
int sg_debug_shard_merge(int device, const uint32_t* ids, const double* scores, const uint32_t* counts, const uint64_t* doc_lo,
                         uint32_t n_shards, uint32_t n_q, uint32_t k, int autocomplete, uint32_t* out_ids, double* out_scores,
                         uint32_t* out_counts);
int sg_debug_shard_merge_time(double* out_ms);

/* Suggester.Suggest / Autocomplete.Autocomplete as the reference calls them: ONE query per call, from many goroutines at
 * once (pkg/suggest/suggester.go:46, autocomplete.go:40, service_test.go:36-79).  Blocking; concurrent callers are
 * coalesced: the request is queued and dispatcher threads (SG_COALESCE_LANES per replica, default 1) run whatever is
 * pending with the same (metric, similarity, k) as one launch — no timer, an idle engine serves a lone request at once.
 * out_ids / out_scores hold k entries, *out_count the number written (or an SG_COUNT_* flag, nothing written). */
int sg_suggest_one(sg_index* index, const uint8_t* q_utf8, uint32_t len, int metric, double similarity, uint32_t k,
                   uint32_t* out_ids, double* out_scores, uint32_t* out_count);
int sg_autocomplete_one(sg_index* index, const uint8_t* q_utf8, uint32_t len, uint32_t limit, uint32_t* out_ids,
                        uint32_t* out_count);
/* Autocomplete restricted to documents with docID >= first_doc (the `limit` smallest of those).  The reference hands EVERY
 * match to the caller's collector (pkg/suggest/autocomplete.go:40-77; pkg/spellchecker/collector.go:61-79 ranks them all):
 * a binding that must do the same pages through them — first_doc = 0, then the last docID of a page + 1, until a page comes
 * back with fewer than `limit` entries. */
int sg_autocomplete_one_from(sg_index* index, const uint8_t* q_utf8, uint32_t len, uint32_t first_doc, uint32_t limit,
                             uint32_t* out_ids, uint32_t* out_count);
int sg_autocomplete_batch_from(sg_index* index, const uint8_t* q_utf8, const uint64_t* q_offs, uint32_t n_q, uint32_t first_doc,
                               uint32_t limit, uint32_t* out_ids, uint32_t* out_counts);

/* ---- the Suggester seam for ANY Metric and ANY collector (pkg/suggest/suggester.go:17-20) -------------------------
 * metric.Metric is an interface (pkg/metric/metric.go:7-16: MinY, MaxY, Threshold, Distance); the five implementations
 * above have device twins, any other one reaches the engine as tables its binding fills by calling the four methods:
 *   min_y[a], max_y[a]                      a = 0 .. a_max          Metric.MinY / MaxY(alpha, a)
 *   threshold[a * S + b]                    b = 0 .. S - 1          Metric.Threshold(alpha, a, b)
 *   score[(a * S + b) * (a_max + 1) + o]    o = 0 .. a_max          1 - Metric.Distance(o, a, b)   (scorer.go:29-31)
 * S = sg_stats.n_segments of `index`.  A query with more than a_max n-grams comes back SG_COUNT_TOO_LONG.  The tables are
 * copied to the HBM of the index's primary replica and live until released (they retain the index).
 * Which b a query of a n-grams visits: NOT [MinY, min(MaxY, S - 1)] but what suggester.go:113-121 sends — a, a - 1, ... down to
 * MinY and a + 1, a + 2, ... up to min(MaxY, S - 1).  sg_metric_window gives that range as one pair (out[0] .. out[1]; the raw
 * pair where the span is zero or below: such a query stays flagged); sg_metric_tables_create passes every row of min_y / max_y
 * through it, and a binding fills threshold and score over out[0] .. min(out[1], S - 1).  It needs no GPU. */
int sg_metric_window(int32_t min_y, int32_t max_y, uint32_t a, uint32_t n_segments, int32_t* out);
typedef struct sg_metric_tables sg_metric_tables;
int sg_metric_tables_create(sg_index* index, uint32_t a_max, const int32_t* min_y, const int32_t* max_y,
                            const int32_t* threshold, const double* score, sg_metric_tables** out);
void sg_metric_tables_retain(sg_metric_tables* tables);   /* one reference per user: a cache entry, a call in flight ([r5]) */
void sg_metric_tables_release(sg_metric_tables* tables);
/* sg_suggest_batch under a tabulated metric: same rows, same order. */
int sg_suggest_batch_tables(sg_index* index, const uint8_t* q_utf8, const uint64_t* q_offs, uint32_t n_q,
                            const sg_metric_tables* tables, uint32_t k, uint32_t* out_ids, double* out_scores,
                            uint32_t* out_counts);
/* nGramSuggester.Suggest hands EVERY document whose overlap reaches the segment's threshold to the caller's collector
 * (suggester.go:78-99; the fuzzy top-k manager is only the usual one).  For a binding that must serve another collector:
 * row i = the `limit` smallest docIDs >= first_doc among query i's candidates over all admissible segments, ascending,
 * with their scores and (out_aux, may be NULL) segment << 16 | overlap — enough to rebuild
 * merger.MergeCandidate{Position, Overlap} and the segment's scorer.
 * Paging: a document that repeats a term has SEVERAL entries (same docID, one per secondary candidate), and a full page may
 * end inside such a run.  Resume with first_doc = the LAST docID of the full page (not + 1) and drop, from the head of the next
 * page, as many entries of that docID as the pages so far have already delivered; if a whole page consists of one docID, ask
 * again with twice the limit.  (first_doc = last docID + 1 loses the rest of the run.)  A page that comes back short is the last.
 * `tables` non-NULL replaces (metric, similarity). */
int sg_suggest_batch_from(sg_index* index, const uint8_t* q_utf8, const uint64_t* q_offs, uint32_t n_q, int metric,
                          double similarity, const sg_metric_tables* tables, uint32_t first_doc, uint32_t limit,
                          uint32_t* out_ids, double* out_scores, uint32_t* out_aux, uint32_t* out_counts);

/* ---- asynchronous host-buffer calls -----------------------------------------------------------------
 * Service.Suggest (pkg/suggest/service.go:105-139) is called with host strings and returns host rows; a Go host behind
 * this ABI therefore lives on host buffers.  The synchronous calls above copy in, run and copy out one after the other;
 * these let the copies of one batch run beside the kernel of another: submit returns once everything is enqueued (copy
 * in -> search launch -> copy out, on three streams of the primary replica tied by events; all search launches of the
 * replica stay serialised on one stream), sg_ticket_wait blocks until the rows are in the caller's buffers and frees the
 * ticket.  Up to 8 tickets may be in flight per replica; two are enough to hide PCIe behind the kernel.  Buffers from
 * sg_host_alloc (pinned) are read / written by the DMA engine directly; other buffers are staged through pinned memory
 * (a memcpy at submit, one at wait).  ONLY sg_host_alloc blocks count as pinned, and only when the whole range lies inside one:
 * memory the caller pinned itself (hipHostMalloc, torch pin_memory) is correct but staged like pageable memory — the library
 * keeps a registry of its own blocks instead of asking the driver about every pointer (tens of microseconds per call).  The caller's buffers must stay valid and untouched until the wait returns.  Submit
 * and wait may be called from different threads. */
typedef struct sg_ticket sg_ticket;
int sg_host_alloc(uint64_t bytes, void** out);
void sg_host_free(void* p);
int sg_suggest_submit(sg_index* index, const uint8_t* q_utf8, const uint64_t* q_offs, uint32_t n_q, int metric,
                      double similarity, uint32_t k, uint32_t* out_ids, double* out_scores, uint32_t* out_counts,
                      sg_ticket** out_ticket);
/* ... on replica number `replica` of the index (0 = the primary, in the order of sg_index_replicas): a slice of a batch per GPU
 * from ONE host thread, no staging copy when the buffers are pinned (the north star's "query batches shard naturally across
 * the 8 GPUs of one node"; sg_suggest_batch_multi is the synchronous form over pageable buffers). */
int sg_suggest_submit_on(sg_index* index, uint32_t replica, const uint8_t* q_utf8, const uint64_t* q_offs, uint32_t n_q,
                         int metric, double similarity, uint32_t k, uint32_t* out_ids, double* out_scores,
                         uint32_t* out_counts, sg_ticket** out_ticket);
int sg_autocomplete_submit(sg_index* index, const uint8_t* q_utf8, const uint64_t* q_offs, uint32_t n_q, uint32_t first_doc,
                           uint32_t limit, uint32_t* out_ids, uint32_t* out_counts, sg_ticket** out_ticket);
int sg_ticket_wait(sg_ticket* ticket);

/* Reference counting: the Go shim retains while a query is in flight and releases from a
 * finalizer, mirroring the reference's mmap release (pkg/index/index_reader.go:49-51). */
void sg_index_retain(sg_index* index);
void sg_index_release(sg_index* index);

const char* sg_last_error(void);

/* ---- the spellchecker caller of the path --------------------------------------
 * pkg/lm: n-gram language model with stupid backoff; pkg/spellchecker: SpellChecker.Predict. */
typedef struct sg_lm sg_lm;

/* NewGoogleNGramReader(order, indexer, dir).Read + NewLanguageModel (pkg/lm/ngram_reader.go:38-98, indexer.go:86-114,
 * language_model.go:24-49): <dir>/1-gm .. <dir>/<order>-gm hold "w1 .. wk\tcount" lines; word ids are the line numbers
 * of 1-gm; `alphabet` is the words alphabet of the lm config (pkg/lm/config.go:25-27) used by the query tokenizer. */
int sg_lm_load_google(const char* dir, uint32_t order, const char* start_symbol, const char* end_symbol,
                      const char* const* alphabet, uint32_t n_alphabet, sg_lm** out);
/* The same files with the word ids the production path gives them: id_order 1 = buildDictionary (pkg/lm/binary.go:101-199),
 * words ordered by (count desc, word asc) — what `lm build-lm` stores and RetrieveLMFromBinary serves; id_order 0 = the line
 * order of 1-gm (buildIndexerWithInMemoryDictionary, indexer.go:88-114, used by the reference's tests).  The ids matter:
 * SpellChecker.Predict breaks ties by docID = word id. */
int sg_lm_load_google_ex(const char* dir, uint32_t order, const char* start_symbol, const char* end_symbol,
                         const char* const* alphabet, uint32_t n_alphabet, int id_order, sg_lm** out);
/* RetrieveLMFromBinary (pkg/lm/binary.go:59-98) — what BuildSpellChecker loads (internal/spellchecker/dep/spellchecker.go:13-53):
 * <name>.lm (nGramModel.Load ngram_model.go:123-160: "0.0.2", order, per level packedArray.Load packed_array.go:118-160)
 * and the dictionary <name>.cdb (word of every id; pkg/dictionary/cdb_dictionary.go).  The MPH table behind the model in the
 * file is not read: lookups here are exact. */
int sg_lm_load_binary(const char* lm_path, const char* cdb_path, const char* start_symbol, const char* end_symbol,
                      const char* const* alphabet, uint32_t n_alphabet, sg_lm** out);
/* One level of the model in the reference's packed form (packed_array.go:12-16: containers context<<32|from, values
 * word<<32|count, total) — what packedArray.Store writes.  Introspection (tests compare with the bytes of a .lm file). */
int sg_lm_level(const sg_lm* lm, uint32_t level, uint64_t* containers, uint32_t cap_containers, uint32_t* n_containers,
                uint64_t* values, uint32_t cap_values, uint32_t* n_values, uint32_t* total);
uint32_t sg_lm_order(const sg_lm* lm);
/* NGramBuilder.Build over NewSentenceRetriever + googleNGramFormatWriter.Write (pkg/lm/ngram_builder.go:16-64,
 * sentence_retriever.go:17-81, ngram_writer.go:32-76) — what `lm build-lm` does to a corpus: sentences are cut at the
 * runes of `separators`, tokenised, wrapped in start/end symbols and their k-grams (k = 1..order) counted into
 * <out_dir>/<k>-gm.  Lines come in order of first appearance (the reference's order is Go-map random). */
int sg_lm_build_google(const uint8_t* text, uint64_t len, uint32_t order, const char* start_symbol, const char* end_symbol,
                       const char* const* alphabet, uint32_t n_alphabet, const char* const* separators, uint32_t n_separators,
                       const char* out_dir);
/* The same corpus straight to a ready model, on the GPU `device`, with no files in between: sg_lm_build_google followed by
 * sg_lm_load_google_ex on what it wrote (NGramBuilder.Build over NewSentenceRetriever, pkg/lm/ngram_builder.go:19-64,
 * sentence_retriever.go:54-81; lm.NewTokenizer; buildDictionary's numbering, binary.go:140-198; the vector builder,
 * ngram_vector_builder.go).  id_order 1 numbers the words by (count desc, bytes asc), id_order 0 by first appearance in the
 * wrapped token stream — the line order sg_lm_build_google writes.  Decoding, lower-casing, classifying, hashing, counting and the
 * sort and reduce of every level run on the device; the host numbers the distinct words and receives the finished levels, which
 * are uploaded on first use like a loaded model's.  order is 1 .. 8; at most 1 GiB of text (SG_E_UNSUPPORTED above);
 * an empty start or end symbol, or one with a space, tab or newline, is SG_E_INVALID; an alphabet that holds U+0020 is
 * SG_E_UNSUPPORTED.  len == 0 or a text without a token gives the empty model the file path gives; len == 0 touches no
 * device.  On failure *out is untouched. */
int sg_lm_build_device(const uint8_t* text, uint64_t len, uint32_t order, const char* start_symbol, const char* end_symbol,
                       const char* const* alphabet, uint32_t n_alphabet, const char* const* separators, uint32_t n_separators,
                       int id_order, int device, sg_lm** out);
/* Any model in the production format that sg_lm_load_binary reads: lm_path = nGramModel.Store (ngram_model.go:100-121,
 * packed_array.go:96-116) — "0.0.2", the order byte, per level "container-bytes value-bytes total\n" and the little-endian
 * containers and values of sg_lm_level; cdb_path = BuildCDBDictionary (pkg/dictionary/helpers.go:52-100) — key = word id as 4
 * bytes little endian, value = the word.  sg_lm_store_binary writes the model section alone, which reloads here; the minimal
 * perfect hash the reference appends to the .lm (buildMPH, binary.go:200-210) and Go's RetrieveLMFromBinary reads straight after
 * the model (table.Load, binary.go:59-98) is written by sg_lm_store_binary_ex with SG_LM_STORE_MPH: mph.Build + mph.Store
 * (pkg/mph/mph.go:40-145,159-192) restated on the host, bucket order of Go 1.14's sort.Slice included — u32 n, n values, u32 n,
 * n auxiliary i32, little endian; an empty dictionary gives the two zero lengths.  A dictionary that lists a word twice, or a
 * bucket no seed below 2^31 places, is SG_E_UNSUPPORTED before a file is touched.  flags == 0 is sg_lm_store_binary; an unknown
 * flag is SG_E_INVALID.  A file that cannot be written is SG_E_INVALID with its path in the message; the .lm is written first,
 * so a failed store may leave it (or a partial file) behind. */
#define SG_LM_STORE_MPH 1u
int sg_lm_store_binary(const sg_lm* lm, const char* lm_path, const char* cdb_path);
int sg_lm_store_binary_ex(const sg_lm* lm, const char* lm_path, const char* cdb_path, uint32_t flags);
/* googleNGramFormatWriter.Write (pkg/lm/ngram_writer.go:12,32-76) for a model that is already counted: <out_dir>/<k>-gm for
 * k = 1 .. order, lines "w1 .. wk\tcount\n" — what the reference's ngram-count step writes and its build-lm step reads.  1-gm has
 * a line per word in id order, k-gm is in level entry order (by context entry, then by word id); the reference's order is Go-map
 * random, so any order is a valid file, and this one makes sg_lm_load_google_ex(out_dir, id_order = 0) give the model back array
 * for array.  device >= 0 formats the lines on that GPU (a size pass, a 64-bit prefix sum, a write pass; a stream and memory of
 * the call's own, nothing of scoring or Predict touched, a model resident on another device no obstacle); device < 0 runs the
 * plain host writer; both write identical files.  Refused with SG_E_UNSUPPORTED and the level in the message, before a file is
 * created: a level with entries whose context is missing from the level below (their leading words are not recoverable), an
 * entry that ends in the unknown word, a level 1 that is not one entry per word in id order.  A model from sg_lm_build_device
 * has none of these.  A file that cannot be created or written is SG_E_INVALID with its path. */
int sg_lm_store_google(const sg_lm* lm, const char* out_dir, int device);
/* Test hooks.  sg_debug_lm_store_slice_bytes, process-wide (like sg_debug_lm_build_hash_bits): the device writer formats a level
 * in slices of entries whose text fits 256 MiB; this lowers the budget, 0 restores it.  sg_debug_lm_store_times: seconds of the
 * calling thread's last sg_lm_store_google — staging, kernels (host writer: formatting), copy-back, file writes. */
int sg_debug_lm_store_slice_bytes(uint32_t bytes);
int sg_debug_lm_store_times(double out[4]);
/* Test hook, process-wide (like sg_debug_poison): sg_lm_build_device keeps only the low `bits` bits of a word's hash, 0 = all 64 —
 * words then collide in its vocabulary table and are told apart by their bytes alone. */
int sg_debug_lm_build_hash_bits(uint32_t bits);
void sg_lm_retain(sg_lm* lm);
void sg_lm_release(sg_lm* lm);
uint32_t sg_lm_num_words(const sg_lm* lm);
int sg_lm_word(const sg_lm* lm, uint32_t id, char* out, uint32_t cap);             /* Indexer.Find; returns the length */
uint32_t sg_lm_word_id(const sg_lm* lm, const uint8_t* word, uint32_t len);          /* Indexer.Get; 0xFFFFFFFF = unknown */
double sg_lm_score(const sg_lm* lm, const uint32_t* ids, uint32_t n);                /* NGramModel.Score, ngram_model.go:44-62 */
double sg_lm_score_word_ids(const sg_lm* lm, const uint32_t* ids, uint32_t n);       /* LanguageModel.ScoreWordIDs, language_model.go:78-86 */
/* Next(context).ScoreNext(word): returns 0 (score written), 1 (nil scorer) or 2 (error); model_level != 0 calls
 * NGramModel.Next (ngram_model.go:64-98) instead of LanguageModel.Next (language_model.go:100-112). */
int sg_lm_next_score(const sg_lm* lm, const uint32_t* context, uint32_t n, uint32_t word, int model_level, double* score);
/* lm.NewTokenizer(alphabet).Tokenize (pkg/lm/tokenizer.go:26-31): tokens joined by '\n' into out; returns their number */
int sg_lm_tokenize(const sg_lm* lm, const uint8_t* text, uint32_t len, char* out, uint32_t cap);

/* LanguageModel.ScoreSentence / ScoreWordIDs for a batch, on the GPU `device` (pkg/lm/language_model.go:55-92, ngram_model.go:44-62,
 * 163-175; generator.go:9-24).  The first call uploads the model to `device` (the lazy upload Predict uses); a model already
 * resident on another device fails with SG_E_INVALID.  A sentence with fewer than order - 2 words has no window and scores 0.0.
 * The device evaluates log() with its own math library: scores agree with sg_lm_score_word_ids to about an ulp of the log, not
 * necessarily to the bit.  n == 0 returns SG_OK without touching a device. */
/* lm eval / ScoreSentence(Tokenize(line)) for a batch of lines (cmd/language-model/cmd/eval.go:41-61): line i is
 * text[offs[i] .. offs[i+1]), at most 1 GiB of text in all.  out_scores[i] gets its score, out_words[i] the tokens of
 * Tokenize(line), out_unknown[i] how many of them have no id (indexer.go:57-71: UnknownWordID, no error); out_words /
 * out_unknown may be null. */
int sg_lm_score_text_batch(sg_lm* lm, int device, const uint8_t* text, const uint64_t* offs, uint32_t n,
                           double* out_scores, uint32_t* out_words, uint32_t* out_unknown);
/* The same with every buffer in the HBM of `device`, asynchronous on `stream`: d_text = text_bytes bytes, d_offs = n + 1 uint64
 * offsets starting at 0, d_out_scores = [n] double, d_out_words / d_out_unknown = [n] uint32 or null. */
int sg_lm_score_text_batch_device(sg_lm* lm, int device, const void* d_text, const void* d_offs, uint32_t n,
                                  uint64_t text_bytes, void* d_out_scores, void* d_out_words, void* d_out_unknown,
                                  void* stream);
/* ScoreWordIDs (language_model.go:83-92) for a batch: sentence i = ids[offs[i] .. offs[i+1]) (offsets in ids, at most 2^30
 * ids in all); any id is allowed (an id outside the vocabulary scores as an unknown word). */
int sg_lm_score_word_ids_batch(sg_lm* lm, int device, const uint32_t* ids, const uint64_t* offs, uint32_t n,
                               double* out_scores);

/* The fuzzy index of the spellchecker: built over the model's vocabulary (docID = word id) and uploaded —
 * internal/spellchecker/dep/spellchecker.go:33-45 (NewRAMBuilder over the LM dictionary). */
int sg_spell_index_build(const sg_lm* lm, const sg_desc* desc, int device, sg_index** out);

/* SpellChecker.Predict (pkg/spellchecker/spellchecker.go:40-92) for a batch of queries: the last word of a query is
 * completed (Autocomplete with the LM collector, collector.go / scorer.go: top_k by ScoreNext of the preceding words),
 * topped up by the Cosine fuzzy search when fewer than top_k complete it, re-ranked by ScoreNext (stable) and cut to
 * top_k + 1 entries (sic, :87-89).  Row i of out_ids (top_k + 1 word ids) holds the prediction of query i,
 * out_counts[i] how many (or SG_COUNT_REF_PANIC / _DEADLOCK / _TOO_LONG / _LM_ERROR).  `index` must come from
 * sg_spell_index_build (or be any uploaded index over the model's vocabulary in id order). */
int sg_spell_predict_batch(sg_index* index, sg_lm* lm, const uint8_t* q_utf8, const uint64_t* q_offs, uint32_t n_q,
                           uint32_t top_k, double similarity, uint32_t* out_ids, uint32_t* out_counts);
/* The same with every buffer in the HBM of the GPU that holds `index`'s primary replica, asynchronous on `stream`: d_q =
 * the queries (q_bytes bytes), d_offs = n_q + 1 uint64 offsets starting at 0, d_out_ids = [n_q][top_k + 1] uint32,
 * d_out_counts = [n_q] uint32.  The word tokeniser, the word ids and LanguageModel.Next's wrap / trim rules run on the
 * device too (spellchecker.go:40-64,94-107; language_model.go:100-112): nothing of a query touches the host. */
int sg_spell_predict_batch_device(sg_index* index, sg_lm* lm, const void* d_q, const void* d_offs, uint32_t n_q, uint64_t q_bytes,
                                  uint32_t top_k, double similarity, void* d_out_ids, void* d_out_counts, void* stream);

/* ---- introspection (tests, bench.py) ---------------------------------------------------- */
typedef struct sg_stats {
  uint64_t n_docs, n_segments, n_terms, n_lists, n_postings /* (term,doc) pairs stored */,
      n_postings_raw /* incl. repeated terms of a doc, as the reference stores them */, posting_bytes /* padded */,
      table_bytes, device_bytes;
} sg_stats;
int sg_index_stats(const sg_index* index, sg_stats* out);

/* Sampled counters the fuzzy launches of the primary replica leave (cumulative; [0..2] wrap at 2^32, [3] is 64 bits wide): out[0] sampled queries
 * whose top-k ended full, [1] sampled queries, [2] their results, [3] the 16-byte chunks of the packed posting store they
 * streamed — what bench.py's roofline.model_bytes is made of.  Synchronises the device. */
int sg_index_launch_stats(sg_index* index, uint64_t out[4]);

/* [r5] Queries the three-launch pipeline of ordinary fuzzy batches (plan -> stream -> verify) handed to the fused
 * kernel, cumulative (wrapping at 2^32): out[0] the plan could not express them (more than 64 n-grams, a window of more than 63
 * segments, a segment that needs docID-range passes, more groups / lists than a slot record holds), [1] their candidates
 * overflowed the slots, [2] a matching document repeats a term (the secondary entries of SURVEY.md §A.3); [3] the queries
 * of all launches that took the pipeline so far (not wrapping).
 * Results never depend on which path answered.  Synchronises the device. */
int sg_index_pipe_stats(sg_index* index, uint64_t out[4]);

/* [r6] The pipeline's sampled volumes, cumulative (wrapping at 2^32): out[0] sampled queries the plan expressed (one in 256 of a batch
 * above 1 024 queries, else every one), [1] their groups of cardinality segments, [2] streamed lists, [3] rows of 64 lanes,
 * [4] candidates pushed for the sampled queries that reached the verify launch, [5] 16-byte chunks of the packed posting store,
 * [6] 1 when the stream launch uses 8-byte sub-row descriptors (stores of 2^26 chunks and more), [7] the stream workgroup of the replica's latest
 * launch: 0 / 1 / 2 = 2 / 4 / 8 wavefronts on 2^11 / 2^12 / 2^13 counters (chosen per launch from the index's expected query volume
 * and the metric's threshold), 3 = fixed by SG_PIPE_NW / SG_PIPE_LOG2_CNT / SG_PIPE_DT_BYTES.  Introspection for bench.py and the
 * tests; no reference counterpart.  Synchronises the device. */
int sg_index_pipe_volumes(sg_index* index, uint64_t out[8]);

/* The forward index (doc -> distinct terms) of the primary replica, copied back for documents
 * first .. first+n-1: out_card[i] = cardinality, out_n[i] = number of distinct terms, out_keys[i*cap ..] their term keys. */
int sg_index_forward(sg_index* index, uint32_t first, uint32_t n, uint32_t cap, uint32_t* out_card, uint32_t* out_n,
                     uint64_t* out_keys);

/* Test hook: the permutation the device's restatement of Go 1.14 sort.Sort (it orders equal-length posting lists in
 * cpMerge.Merge, cp_merge.go:24) gives n <= 128 keys; out[i] = original index of the element that ends at position i. */
int sg_debug_pairsort(int device, const uint32_t* keys, uint32_t n, uint32_t* out);
/* [r5] The auto-tuner's choices (no GPU needed): out = {log2 of the LDS counter words, filter level, 1 if the plan -> stream ->
 * verify pipeline pays} for an index whose queries are expected to stream est_query_chunks 16-byte chunks of u32 postings and
 * whose longest term holds max_term_chunks; and the same for a built index together with its two statistics. */
int sg_debug_tune_choice(double est_query_chunks, double max_term_chunks, int32_t out[6]);
/* [r6] Test hook: the stream workgroup a launch under `metric` / `similarity` starts from on an index with these statistics
 * (expected query volume in 16-byte chunks, n-grams per document, SG_T_FLOOR): *out_shape = 0 / 1 / 2 for 2 / 4 / 8 wavefronts on
 * 2^11 / 2^12 / 2^13 counters.  No GPU needed; no reference counterpart. */
int sg_debug_pipe_shape(double est_query_chunks, double terms_per_doc, int32_t t_floor, int32_t metric, double similarity, int32_t* out_shape);
int sg_debug_tune_index(sg_index* index, double out_stats[2], int32_t out[6]);
/* Test hook (no GPU needed): row i of the knob table (i = 0 .. n-1; SG_E_INVALID past the end): its name, out = {lowest, highest,
 * default, flags: 1 environment, 2 sg_index_tune, 4 pins the stream shape, 8 the auto-tuner may choose it, 16 powers of two only},
 * and, when index is not null, out[4] = its current value and out[5] = 1 if it was set explicitly (else the default and 0). */
int sg_debug_knob(const sg_index* index, uint32_t i, char name[32], int32_t out[6]);
/* Test hook, off by default: with on = 1 or 2 every call of the process first fills the working memory and result rows it is meant to
 * write before it reads with a pattern (1: 0xA5 bytes, 2: 0x5A bytes; item queue, part counts, query lists and term ids take values a
 * kernel can read safely — capi.inc, "Test-only poison"), so that a read of a word the call did not write shows as a wrong row.
 * Rows past a query's count then hold the pattern instead of zeros.  on = 0: off (the default).  sg_debug_poison_stats: bytes poisoned
 * by the calling thread since its last call, per region — out = {split queue / HBM top-k rows / ordered list (SCRATCH_ROWS),
 * pipeline fb_list, tokeniser launch, long-query list, Predict rows, result ids + aux (and the other u32 / u64 result rows of a
 * host-buffer call: edit distances, sg_dictionary_rows' text offsets, sentence word counts), result scores, result counts}; clears them. */
int sg_debug_poison(uint32_t on);
int sg_debug_poison_stats(uint64_t out[8]);
/* Test hooks (no GPU needed): the carving of a launch's SCRATCH_ROWS block for n_q queries, top-k k, split queries on / off and the
 * query order off (0), with atomics (1) or with per-block histograms (2): out = {s, id, split, items, slot, part_n, part_s, part_id, ord,
 * ord_ctl, bytes, slot_cap, item_cap, ord_blocks, SG_MAX_PARTS, SG_ORDER_CTL_WORDS}; and of its SCRATCH_PIPE block: out = {rec, vrec,
 * ovf, cand_n, fb_list, bytes, piece, vrec_words, ovf_cap, SG_PIPE_REC_STRIDE, SG_PIPE_OVF_WORDS, SG_PIPE_PIECE}.  Offsets in bytes. */
int sg_debug_rows_layout(uint32_t n_q, uint32_t k, int32_t split, int32_t reorder, uint64_t out[16]);
int sg_debug_pipe_layout(uint32_t n_q, uint32_t cand_cap, uint64_t out[12]);
/* Test hook (no GPU needed): the regions a host-buffer call declares and the device block made of them.  kind: 0 a search of n queries
 * and rows of k (flags bit 0: scores, bit 1: aux), 1 the same with the text offsets of a _strings call, 2 a mixed call (`rows` slots in
 * all), 3 Predict (k = topK), 4 sg_dictionary_rows (n rows, `rows` slots; bit 2: ragged), 5 sg_edit_rows and 6 sg_edit_rerank (bit 0:
 * scores, bit 2: ragged), 7 sg_lm_score_text_batch (bit 0: words, bit 1: unknown), 8 sg_lm_score_word_ids_batch; blob_bytes: the bytes
 * of the queries / text / ids.  out[0] = the number of regions, [0, out[1]) the one range copied back, [out[2], out[3]) the one range
 * copied in, out[4] the block's bytes; then four words per region in the order of declaration: offset, bytes, alignment, direction
 * (1 in, 2 out, 3 both ways). */
int sg_debug_io_layout(uint32_t kind, uint32_t n, uint32_t k, uint32_t flags, uint64_t blob_bytes, uint64_t rows, uint64_t out[45]);
/* [r6] Test hook: out[0] = the device ordinal of replica number `replica`, out[1..7] = the device its posting store, seg_off, orig_of,
 * forward-index records and terms, term table and counter block are resident on (-1: null).  All must equal out[0]. */
int sg_debug_replica_devices(sg_index* index, uint32_t replica, int32_t out[8]);
/* Test hook: one array of replica number `replica` copied back as it lies in HBM, undecoded (tests/packed_ref.py restates the formats
 * and compares; tests/test_gpu_store.py).  which = 0 the packed posting chunks and the 64-chunk slack row behind them, 1 the packed
 * seg_off (bit 31 = the term's 8-bit format, as stored), 2 orig_of, 3 x_of, 4 seg_base (segments + 1 entries), 5 cut_sample, 6 the
 * forward-index records, 7 the forward-index term ids, 8 fx_base (0 bytes where the index has none); 9 / 10 the postings / seg_off of
 * the host CSR they are all derived from (`replica` ignored; no GPU needed).  *out_bytes = the array's size; with out != NULL it is
 * copied (SG_E_INVALID if cap_bytes is smaller).  SG_E_INVALID: not uploaded, no such replica, unknown array.  Reads only. */
int sg_debug_index_array(sg_index* index, uint32_t replica, uint32_t which, void* out, uint64_t cap_bytes, uint64_t* out_bytes);

/* A batch whose queries differ in metric, similarity and k.  The reference takes a SearchConfig per call
 * (pkg/suggest/service.go:105) and its HTTP handler reads metric | similarity | topK per request
 * (internal/suggest/api/suggest_handler.go:79-101); here the caller passes a table of DISTINCT configs and, per query, an index
 * into it.  The device groups the queries by config (a stable permutation: within a group they keep the caller's order), gathers
 * each group's queries into one contiguous blob, runs every non-empty group as the ordinary launch of its config and scatters the
 * groups' rows back in caller order.  A row is bit for bit the row the plain call with that config gives the query.
 *
 * Output, ragged: row i starts at out_row_offs[i] = k_0 + ... + k_(i-1) (k_j: the k of query j's config) and has k_i slots of
 * out_ids and out_scores; out_row_offs has n_q + 1 entries.  Slots past a row's count are zero; an autocomplete row's score slots
 * are zero.  out_counts[i] is the plain call's, SG_COUNT_* values included.  rows_cap: the slots out_ids and out_scores have room
 * for; a batch that needs more is refused.
 *
 * 1 <= n_configs <= SG_MAX_MIXED_CONFIGS.  Every entry is checked as the plain call checks its arguments; a config no query names
 * is legal (an empty group, no launch), two equal entries are two groups.  config_of[i] >= n_configs is refused (invalid argument)
 * on either route with no access outside any array — the device route finds it on the device.  n_q == 0 succeeds.  Not offered:
 * docID-ordered configs, tabulated metrics, Predict, sharded handles, tickets, several replicas.
 *
 * The device route takes device pointers (d_out_row_offs: n_q + 1 u64, computed on the device), `configs` in host memory, and
 * enqueues on `stream` — but it is the one device call that is NOT asynchronous: the group sizes come back through pinned memory
 * with ONE wait on `stream` after the counting launch, before the groups are launched.  It returns with the groups' launches and
 * the scatter enqueued. */
#define SG_MAX_MIXED_CONFIGS 256u
typedef struct sg_search_config {      /* 24 bytes */
  int32_t metric;        /* enum sg_metric; ignored when autocomplete */
  int32_t autocomplete;  /* 0: Suggest, 1: Autocomplete (k = limit, first_doc as in sg_autocomplete_batch_from) */
  double similarity;     /* ignored when autocomplete */
  uint32_t k, first_doc; /* first_doc must be 0 when autocomplete == 0 */
} sg_search_config;
int sg_suggest_batch_mixed(sg_index* index, const uint8_t* q_utf8, const uint64_t* q_offs, uint32_t n_q,
                           const sg_search_config* configs, uint32_t n_configs, const uint32_t* config_of, uint64_t rows_cap,
                           uint32_t* out_ids, double* out_scores, uint32_t* out_counts, uint64_t* out_row_offs);
int sg_suggest_batch_mixed_device(sg_index* index, const void* d_q_utf8, const void* d_q_offs, uint32_t n_q,
                                  const sg_search_config* configs, uint32_t n_configs, const void* d_config_of, uint64_t rows_cap,
                                  void* d_out_ids, void* d_out_scores, void* d_out_counts, void* d_out_row_offs, void* stream);
/* The single-query coalescer (sg_suggest_one, sg_autocomplete_one): on != 0 lets a dispatcher whose pending queue holds more than
 * one key take everything pending — up to its batch limit and SG_MAX_MIXED_CONFIGS distinct keys, the rest waits for the next
 * take — and answer it with ONE mixed call; a take with a single key goes as before.  Off by default: the dispatcher then takes
 * only the requests that share the first one's key.  Results do not depend on it. */
int sg_coalesce_mixed(sg_index* index, int on);
/* Test hooks like the other sg_debug_* entries (bindings need not mirror them).  sg_debug_mixed_last: the calling thread's last
 * successful mixed call with n_q > 0 — perm[j] (cap entries at least n_q) = the caller's number of the query at grouped position
 * j, group_start[g] (n_configs + 1 entries) = the first grouped position of config g.  Fails when there was none, when n_configs is
 * not that call's or cap is too small.  sg_debug_coalesce_hold: while on, the dispatchers take nothing (requests queue up); off
 * releases them.  Release before the index goes.  sg_debug_coalesce_stats: out = {requests pending now; batches taken; of them
 * mixed; launches — a mixed batch counts its configs, a plain one 1}.  No reference counterpart. */
int sg_debug_mixed_last(uint32_t* perm, uint32_t cap, uint32_t* group_start, uint32_t n_configs);
int sg_debug_coalesce_hold(sg_index* index, int on);
int sg_debug_coalesce_stats(sg_index* index, uint64_t out[4]);
/* Milliseconds of the calling thread's last device-route mixed call, between events on its stream, taken only while on != 0 was
 * set by the first function (process-wide; it makes the call wait for its own end): out = {count; permute; gather; the groups'
 * launches; scatter}.  tools/mixed_timing.py reads it.  A measuring hook only: while it is on, EVERY thread's device-route mixed
 * call blocks until its own work has ended, so it must not stay on in a service. */
int sg_debug_mixed_timing(int on);
int sg_debug_mixed_times(double out_ms[5]);

/* Result rows as strings.  sg_dictionary is the reference's dictionary.Dictionary — docID -> string, docID = line
 * number — as an immutable, reference-counted handle.  With device >= 0 it lives in the HBM of that GPU as doc_offs[n_docs + 1]
 * (u64) and the blob, and the rows of any search are turned into strings there; with device < 0 it is host-resident, needs no GPU,
 * and sg_dictionary_rows is the plain host loop (the reference's Service.Suggest, pkg/suggest/service.go:129-136).
 *
 * sg_dictionary_upload takes the (blob, n_docs + 1 u64 offsets) pair of sg_index_build; the offsets may start anywhere and must
 * not decrease.  sg_dictionary_open_cdb reads the <name>.cdb that BuildCDBDictionary / sg_dictionary_store_cdb writes (key =
 * docID as 4 bytes little endian); a truncated or corrupted file or a hole in the ids is refused (invalid argument).
 * Limits: n_docs <= 2^32 - 1; one string is shorter than 4 GiB; every offset and every sum of lengths is 64-bit; the CDB route
 * inherits the format's 4 GiB.  sg_dictionary_bytes: the bytes of all strings; sg_dictionary_max_len: the longest string, so a
 * caller can bound a text buffer by slots * max_len.
 *
 * The materialise step.  In: id rows, counts[n_rows] and a row geometry — a fixed stride `row` (row_offs null; row i holds slots
 * i * row .. i * row + row) or ragged row_offs[n_rows + 1] as sg_suggest_batch_mixed returns it (`row` unused).  `slots`: the
 * slots of `ids` in all (fixed stride: at least n_rows * row).  Out: text_offs[slots + 1] (u64) and text; the string of slot s is
 * text[text_offs[s] .. text_offs[s + 1]), slots laid out exactly as the id rows are — the form of a query batch or a dictionary.
 * Row i has min(counts[i], its length) entries; counts[i] >= 0xFFFFFFF0 is a SG_COUNT_* flag: no entries.  Every other slot —
 * past the count, in a flagged row, in no ragged row — has length 0 and its id is never read.  An entry whose id is >= n_docs has
 * length 0 and is counted.  A string that would end past text_cap is not written; text_offs is complete whatever text_cap is, so
 * a caller can size a retry.
 *
 * sg_dictionary_rows_device: device pointers, asynchronous on `stream`, writes nothing of the handle, callable from any number of
 * threads.  d_info: two u64 — [0] the bytes the text needs, [1] the entries with an id outside the dictionary.  A host-resident
 * handle is refused (unsupported).
 * sg_dictionary_rows: host buffers; uploads ids and counts, returns the strings.  *needed (may be null) = the bytes the text
 * needs.  Invalid argument: an id outside the dictionary ("docID outside the dictionary" — the reference's dict.Get fails there
 * too), needed > text_cap ("text buffer too small": *needed and text_offs are set), null pointers.
 * sg_suggest_batch_strings / sg_autocomplete_batch_strings: sg_suggest_batch / sg_autocomplete_batch whose rows go from the search
 * to the gather without visiting the host; text_offs has n_q * k + 1 entries.  ids, scores and counts are bit for bit the plain
 * call's and are delivered also when the text is refused.  The call waits for the device twice (the total, then rows and text)
 * and holds no more device memory for text than text_cap.  The dictionary must be on the device of the index's primary replica,
 * else unsupported. */
typedef struct sg_dictionary sg_dictionary;
int sg_dictionary_upload(const uint8_t* utf8, const uint64_t* offs, uint32_t n_docs, int device, sg_dictionary** out);
int sg_dictionary_open_cdb(const char* cdb_path, int device, sg_dictionary** out);
void sg_dictionary_retain(sg_dictionary* dict);
void sg_dictionary_release(sg_dictionary* dict);
uint32_t sg_dictionary_size(const sg_dictionary* dict);
uint64_t sg_dictionary_bytes(const sg_dictionary* dict);
uint32_t sg_dictionary_max_len(const sg_dictionary* dict);
int sg_dictionary_device(const sg_dictionary* dict);       /* -1: host-resident */
int sg_dictionary_rows_device(sg_dictionary* dict, const void* d_ids, const void* d_counts, const void* d_row_offs_or_null,
                              uint32_t n_rows, uint32_t row, uint64_t slots, void* d_text, uint64_t text_cap, void* d_text_offs,
                              void* d_info, void* stream);
int sg_dictionary_rows(sg_dictionary* dict, const uint32_t* ids, const uint32_t* counts, const uint64_t* row_offs_or_null,
                       uint32_t n_rows, uint32_t row, uint64_t slots, uint8_t* text, uint64_t text_cap, uint64_t* text_offs,
                       uint64_t* needed);
int sg_suggest_batch_strings(sg_index* index, const uint8_t* q_utf8, const uint64_t* q_offs, uint32_t n_q, int metric,
                             double similarity, uint32_t k, uint32_t* out_ids, double* out_scores, uint32_t* out_counts,
                             sg_dictionary* dict, uint8_t* text, uint64_t text_cap, uint64_t* text_offs, uint64_t* needed);
int sg_autocomplete_batch_strings(sg_index* index, const uint8_t* q_utf8, const uint64_t* q_offs, uint32_t n_q, uint32_t limit,
                                  uint32_t* out_ids, uint32_t* out_counts, sg_dictionary* dict, uint8_t* text, uint64_t text_cap,
                                  uint64_t* text_offs, uint64_t* needed);

/* Result rows ranked by edit distance: the second stage of the q-gram count filter.  The rows of a search are
 * verified against the strings of an sg_dictionary and ranked by the distance between row i's query and each of its entries.
 * THE RESULT IS THE EXACT TOP-K BY EDIT DISTANCE AMONG THE CANDIDATES THE Q-GRAM SEARCH RETURNED — not over the whole dictionary: a
 * string the search did not return is never looked at, so fetch more candidates than you keep.
 *
 * Distances are over runes: both strings are decoded as Go's `range` does (an invalid byte is one U+FFFD of width 1); nothing is
 * trimmed, wrapped or mapped through an index alphabet.  fold_case != 0: every rune of both strings first goes through the simple
 * lower-case pairs of the tokenisers (the handle keeps its own copy of the table; a host-resident handle uses the host's function).
 * SG_EDIT_LEVENSHTEIN: unit insert, delete, substitute.  SG_EDIT_OSA: the same plus the transposition of two adjacent runes at cost 1
 * — optimal string alignment: "ca" -> "abc" is 3, not unrestricted Damerau's 2.  Both are symmetric.
 *
 * Geometry exactly as sg_dictionary_rows (a fixed `row`, or ragged row_offs); row i belongs to query i = q[q_offs[i] ..
 * q_offs[i + 1]), 65 536 bytes at most.  dist[slots] (u32): the distance of every entry; 0xFFFFFFFF for a slot that holds none (past
 * the count, a flagged row, no row) and for an entry whose id is outside the dictionary, which is counted in info[1] (d_info: two
 * u64, [0] = 0); the host-buffer routes answer invalid argument for such an id after delivering the rest.
 *
 * Re-rank: a row's entries are reordered by (distance ascending, then the order they had) — a stable sort: a fuzzy row keeps (score
 * descending, docID ascending) among equal distances, an autocomplete row (scores null) docID ascending.  Entries with a distance
 * above max_distance are removed (0xFFFFFFFF: no bound); the count becomes the number kept, at most k_out; slots from the count on are
 * zeroed in ids, scores and distances.  Flagged rows (SG_COUNT_*) pass through untouched, their distances 0xFFFFFFFF.
 *
 * The _device calls take device pointers, are asynchronous on `stream`, write nothing of any handle and may be called from any number
 * of threads; a host-resident handle is refused (unsupported).  On that route a query of more than 65 536 bytes gets no distances:
 * its entries stay 0xFFFFFFFF and are counted in info[1].  sg_edit_rows / sg_edit_rerank take host buffers; with a host-resident
 * handle they are a plain host loop and need no GPU; with a device handle they are host-buffer calls like sg_suggest_batch (q_offs
 * may start anywhere; a call whose rows pass 64 MiB copies straight from and to the caller's arrays).
 * sg_suggest_batch_edit: search and rank in one call — k_candidates per query by the q-gram metric, of those the k nearest by edit
 * distance; rows of k; one staging in, one copy out, one wait.  Invalid argument: null pointers, an unknown mode, k == 0,
 * k > k_candidates, k_candidates above SG_MAX_TOPK; unsupported: a dictionary that is host-resident or not on the device of the
 * index's primary replica.
 * Queries of up to 64 runes take the hot path (a lane per candidate, one 64-bit word of bit vectors); longer ones a slower kernel
 * whose working memory is bounded by a byte budget — sg_debug_edit_slice_bytes lowers it for tests (0: the default, 64 MiB). */
enum sg_edit_mode { SG_EDIT_LEVENSHTEIN = 0, SG_EDIT_OSA = 1 };
typedef struct sg_edit_config { int32_t mode; int32_t fold_case; uint32_t max_distance; uint32_t reserved; } sg_edit_config;
int sg_edit_rows_device(sg_dictionary* dict, const sg_edit_config* config, const void* d_q_blob, const void* d_q_offs, const void* d_ids,
                        const void* d_counts, const void* d_row_offs_or_null, uint32_t n_rows, uint32_t row, uint64_t slots, void* d_dist,
                        void* d_info, void* stream);
int sg_edit_rows(sg_dictionary* dict, const sg_edit_config* config, const uint8_t* q_utf8, const uint64_t* q_offs, const uint32_t* ids,
                 const uint32_t* counts, const uint64_t* row_offs_or_null, uint32_t n_rows, uint32_t row, uint64_t slots, uint32_t* dist);
int sg_edit_rerank_device(sg_dictionary* dict, const sg_edit_config* config, const void* d_q_blob, const void* d_q_offs, void* d_ids,
                          void* d_scores_or_null, void* d_counts, const void* d_row_offs_or_null, uint32_t n_rows, uint32_t row, uint64_t slots,
                          uint32_t k_out, void* d_dist, void* d_info, void* stream);
int sg_edit_rerank(sg_dictionary* dict, const sg_edit_config* config, const uint8_t* q_utf8, const uint64_t* q_offs, uint32_t* ids,
                   double* scores_or_null, uint32_t* counts, const uint64_t* row_offs_or_null, uint32_t n_rows, uint32_t row, uint64_t slots,
                   uint32_t k_out, uint32_t* dist);
int sg_suggest_batch_edit(sg_index* index, const uint8_t* q_utf8, const uint64_t* q_offs, uint32_t n_q, int metric, double similarity,
                          uint32_t k_candidates, sg_dictionary* dict, const sg_edit_config* config, uint32_t k, uint32_t* out_ids,
                          double* out_scores, uint32_t* out_dist, uint32_t* out_counts);
int sg_debug_edit_slice_bytes(uint64_t bytes);
/* Test hook (no GPU needed): the kernels' own statement of the bit-vector recurrence, run on the host over two rune strings — the
 * one-word form with its Peq table for n_a <= 64, the blocked form over sorted (rune, position) pairs above. */
int sg_debug_edit_bitvector(int mode, const uint32_t* a, uint32_t n_a, const uint32_t* b, uint32_t n_b, uint32_t* out);

/* A complete search of a dictionary by edit distance: every string of the sg_dictionary within max_distance edits
 * of the query, the k nearest returned — over the WHOLE dictionary, with no q-gram index and no candidates: nothing is missed.
 * Distance semantics are exactly those above (runes, folding, both modes; nothing trimmed, wrapped or mapped through an alphabet).
 *
 * sg_edit_index is the search structure over one dictionary: immutable, reference-counted, it retains `dict`.  It holds two arrays
 * of n_docs entries — in HBM, built by a kernel, for a device-resident dictionary; host vectors for a host-resident one:
 * runes[d] (u32) the rune count of string d, and sig[d] (u64) the OR over its runes (folded, if fold_case) of bit
 * (rune * 0x9E3779B1) >> 26 (a 32-bit product).  One insert, delete or substitute removes at most one rune and adds at most one, a
 * transposition neither, so distance >= max(popcount(sigQ & ~sigD), popcount(sigD & ~sigQ)) and distance >= |runesQ - runesD|: a
 * document that breaks either bound for max_distance is rejected without being decoded, and no other is.
 *
 * config: mode as above; fold_case must equal the index's; max_distance is a true bound here, 0 .. SG_EDIT_SEARCH_MAX_DISTANCE
 * (0xFFFFFFFF and anything else above is an invalid argument).  k: 1 .. 1 024.  Queries as (blob, n_q + 1 u64 offsets).
 * Out: ids[n_q * k], dist[n_q * k], counts[n_q] (all u32) and, unless null, hist[n_q * (max_distance + 1)] (u32): hist[i][t] = the
 * number of dictionary strings at distance exactly t from query i — their sum is the number of matches.  Row i holds the
 * min(k, that sum) nearest strings by (distance ascending, docID ascending); slots from the count on are zeroed.  A query of more
 * than 64 runes comes back with counts[i] = SG_COUNT_TOO_LONG, its row and histogram zeroed (a limit of this version;
 * sg_suggest_batch_edit remains the route for such queries); a query of 64 runes, of one, of none is answered — for the empty query
 * the distance is the document's rune count.
 * sg_edit_search_device: device pointers, asynchronous on `stream`, writes nothing of any handle, callable from any number of
 * threads; its working memory is a block of the calling thread's per-stream scratch, bounded whatever the number of matches; a
 * host-resident index is refused (unsupported).  sg_edit_search: host buffers; over a device index a host-buffer call like
 * sg_suggest_batch (offsets may start anywhere), over a host-resident index a plain host loop that needs no GPU.
 * Test hooks: sg_debug_edit_index_array reads one of the two arrays back raw (which 0: runes, 1: sig; out null: *out_bytes alone);
 * sg_debug_edit_search_slices forces the number of docID slices the scan cuts the dictionary into (slice s = documents
 * [s * ceil(n_docs / n), (s + 1) * ceil(n_docs / n)); 0: automatic); sg_debug_edit_search_bytes lowers the byte budget of the rows
 * one chunk of queries may take (0: the default, 256 MiB), so that a batch is enqueued in several chunks. */
#define SG_EDIT_SEARCH_MAX_DISTANCE 32u
typedef struct sg_edit_index sg_edit_index;
int sg_edit_index_create(sg_dictionary* dict, int fold_case, sg_edit_index** out);
void sg_edit_index_retain(sg_edit_index* index);
void sg_edit_index_release(sg_edit_index* index);
int sg_edit_search_device(sg_edit_index* index, const sg_edit_config* config, const void* d_q_blob, const void* d_q_offs, uint32_t n_q, uint32_t k,
                          void* d_ids, void* d_dist, void* d_counts, void* d_hist_or_null, void* stream);
int sg_edit_search(sg_edit_index* index, const sg_edit_config* config, const uint8_t* q_utf8, const uint64_t* q_offs, uint32_t n_q, uint32_t k,
                   uint32_t* ids, uint32_t* dist, uint32_t* counts, uint32_t* hist_or_null);
int sg_debug_edit_index_array(sg_edit_index* index, uint32_t which, void* out, uint64_t cap_bytes, uint64_t* out_bytes);
int sg_debug_edit_search_slices(uint32_t n);
int sg_debug_edit_search_bytes(uint64_t bytes);

/* Sets a tuning knob of the index, before or after its first upload: SG_LOG2_CNT, SG_T_FLOOR, SG_FILTER_LEVEL, SG_TIGHTEN, SG_ROOMY,
 * SG_ORDER, SG_PRETOK, SG_SPLIT_CHUNKS, SG_PARTS_CNT_BONUS; the pipeline's SG_PIPE, SG_PIPE_SUB, SG_PIPE_CAND_CAP, SG_PIPE_WIDE,
 * SG_PLAN2.  SG_PIPE_NW, SG_PIPE_LOG2_CNT and SG_PIPE_DT_BYTES freeze the stream workgroup's shape for every launch;
 * SG_PIPE_SHAPE_AUTO = 1 hands it back to the per-launch choice, SG_PIPE_SHAPE_BIAS is a test hook (these two: this call only).
 * The others are also read from the environment at the first upload, and SG_G8 only there.  Ranges, defaults and meanings: the
 * table of DESIGN.md §4c.  An unknown name or a value outside its range is refused (invalid argument) on either route — from the
 * environment, by the first upload.  A knob set explicitly is not chosen by the auto-tuner.  Results never depend on the knobs;
 * for parameter sweeps; not synchronised with launches in flight. */
int sg_index_tune(sg_index* index, const char* knob, int value);

/* Tokens of `text` as the index sees them, one packed 64-bit term key each (DESIGN.md §Term keys);
 * returns the token count (may exceed cap; only cap are written).  NewSuggestTokenizer /
 * NewAutocompleteTokenizer, pkg/suggest/tokenizer.go:9-34. */
int sg_tokenize(const sg_index* index, const uint8_t* text, uint32_t len, int autocomplete, uint64_t* out_keys,
                uint32_t cap);
/* Renders a term key back to the reference's term string (UTF-8); returns its byte length. */
int sg_term_string(const sg_index* index, uint64_t key, char* out, uint32_t cap);
/* Posting list of (segment, term key) from the host CSR: returns the stored (de-duplicated)
 * length, writes up to cap docIDs; *raw_len = length incl. a doc's repeated terms. -1 if absent. */
int64_t sg_index_list(const sg_index* index, uint32_t segment, uint64_t key, uint32_t* out, uint64_t cap,
                      uint64_t* raw_len);
/* Enumerates the non-empty (segment, term) lists: fills up to cap entries, returns the total. */
uint64_t sg_index_lists(const sg_index* index, uint32_t* out_segments, uint64_t* out_keys, uint64_t cap);

/* 64-bit digests of the host CSR: postings, seg_off, list lengths, term keys (+ repeated-term table). */
int sg_index_digest(const sg_index* index, uint64_t out[4]);

/* Algorithmic bytes of a suggest batch: per query 4*sum of |postings| over every
 * admissible segment and present term + len(query) + 12*k.  Host-side accounting for bench.py. */
int sg_suggest_algorithmic_bytes(const sg_index* index, const uint8_t* q_utf8, const uint64_t* q_offs, uint32_t n_q,
                                 int metric, double similarity, uint32_t k, uint64_t* out_total);

/* Same accounting for sg_autocomplete_batch: 4 * |postings| of every query term in every segment >= |terms| that holds them all. */
int sg_autocomplete_algorithmic_bytes(const sg_index* index, const uint8_t* q_utf8, const uint64_t* q_offs, uint32_t n_q,
                                      uint32_t limit, uint64_t* out_total);

#ifdef __cplusplus
}
#endif
#endif /* SUGGEST_HIP_H */
