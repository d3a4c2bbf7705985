// index_build.inc — device-side index build (SURVEY.md §8f-4), included by engine.hip (it shares the device tokeniser).
//
// Replaces the host loop of suggest.Index + Writer.AddDocument/Commit (pkg/suggest/indexer.go:14-45,
// pkg/index/indexer_writer.go:66-145) for large dictionaries: tokenise every document on the GPU, intern the terms in
// a device hash table, radix-sort the (term, segment, docID) postings and lay them out as the same term-major CSR the
// host builder produces — bit-identical arrays (term ids are numbered by first appearance in dictionary order, like the
// host's), so everything downstream (upload, search, introspection) is unchanged.
//
//   K1 build_tokenize    one wavefront per document: d_tokenize -> keys to HBM, keys interned (CAS on the 64-bit key),
//                        first appearance (doc << 20 | min(position, 0xFFFFF)) kept with atomicMin, cardinality -> doc_cnt
//   K2 build_collect     occupied slots -> (stamp, key) pairs; hipcub radix sort by stamp = term numbering;
//      build_assign      term id written back into the slot
//   K3 build_emit        one wavefront per document: keys -> term ids, repeated terms of a document folded (side list
//                        for the reference's duplicate quirk), sort key term*S + cardinality, list_len histogram
//   K4 device_sort_pairs (hipcub radix sort; stable: docIDs stay ascending inside a list)
//   K5 two exclusive scans: chunk offsets (lists padded to 16 bytes) and offsets in the sorted stream
//   K6 build_scatter     sorted stream -> padded posting store; build_seg_off -> seg_off rows

namespace sg {

struct BuildSlot { unsigned long long key, stamp; };   // stamp: first appearance, later the term id

struct BuildArgs {
  DeviceIndex ix;                 // description tables only
  const uint8_t* docs;
  const uint64_t* offs;           // [n_docs + 1]
  const uint64_t* cap_off;        // [n_docs + 1] where a document's keys / postings go (capacity = runes it can have)
  uint32_t n_docs;
  uint64_t* doc_keys;             // [cap_total]
  uint32_t* doc_cnt;              // [n_docs] cardinality (tokens incl. repeats); 0xFFFFFFFF: beyond the device tokeniser
  BuildSlot* table;
  uint32_t table_mask;
  unsigned long long* zero_term;  // [1] the empty term (key 0: every rune replaced by an empty pad) cannot live in the table,
                                  //     whose empty slots are key 0: its first appearance, later its term id
  uint32_t* stats;                // [0] max cardinality [1] docs for the long tokeniser [2] terms [3] table overflow [4] dups [5] dup overflow
                                  // [6] docs beyond the long tokeniser too
  uint32_t* long_docs;            // [n_docs] the documents build_tokenize left to build_tokenize_long (stats[1] of them)
  uint8_t* long_slots;            // working memory of build_tokenize_long: one LongSlot per workgroup
  uint64_t long_slot_bytes;
  // emit
  uint32_t S;
  uint32_t* sort_key;             // [cap_total] term * S + cardinality, 0xFFFFFFFF = no posting
  uint32_t* sort_doc;             // [cap_total]
  uint32_t* list_len;             // [n_terms * S]
  uint32_t* dups;                 // [dup_cap][3] doc, term, multiplicity
  uint32_t dup_cap;
};

// keys of document d -> HBM, interned (CAS on the 64-bit key), first appearance (doc << 20 | position) kept with atomicMin
__device__ __forceinline__ void build_intern(const BuildArgs& b, uint32_t d, uint32_t i, unsigned long long key, uint64_t base) {
  b.doc_keys[base + i] = key;
  const unsigned long long stamp = ((unsigned long long)d << 20) | (unsigned long long)min(i, 0xFFFFFu);
  if (key == 0ull) {
    if (atomicMin(b.zero_term, stamp) == ~0ull) atomicAdd(b.stats + 2, 1u);
    return;
  }
  uint32_t h = (uint32_t)d_mix64(key) & b.table_mask;
  for (uint32_t probes = 0;; probes++) {
    if (probes > b.table_mask) { atomicExch(b.stats + 3, 1u); break; }
    unsigned long long cur = b.table[h].key;
    if (cur == 0ull) {
      cur = atomicCAS(&b.table[h].key, 0ull, key);
      if (cur == 0ull) {                                      // this lane interned the term
        if (atomicAdd(b.stats + 2, 1u) > (b.table_mask >> 1)) atomicExch(b.stats + 3, 1u);
        cur = key;
      }
    }
    if (cur == key) {                                         // (the plain read spares the atomic once the term is old)
      if (stamp < __hip_atomic_load(&b.table[h].stamp, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicMin(&b.table[h].stamp, stamp);
      break;
    }
    h = (h + 1) & b.table_mask;
  }
}

__global__ __launch_bounds__(64) void build_tokenize(const BuildArgs b) {
  __shared__ uint32_t runes[SG_MAX_RUNES];
  __shared__ uint64_t keys[SG_MAX_A];
  __shared__ uint32_t term[SG_MAX_A];
  const int lane = threadIdx.x;
  const uint32_t d = blockIdx.x;
  BatchArgs a{};
  a.ix = b.ix;
  const uint64_t o0 = b.offs[d], o1 = b.offs[d + 1];
  const int A = d_tokenize(a, b.docs + o0, (uint32_t)(o1 - o0), runes, keys, term, lane);
  if (A < 0) {                                                  // beyond the LDS tokeniser: build_tokenize_long's
    if (lane == 0) { b.doc_cnt[d] = 0xFFFFFFFFu; b.long_docs[atomicAdd(b.stats + 1, 1u)] = d; }
    return;
  }
  if (lane == 0) { b.doc_cnt[d] = (uint32_t)A; atomicMax(b.stats + 0, (uint32_t)A); }
  const uint64_t base = b.cap_off[d];
  for (int i = lane; i < A; i += 64) build_intern(b, d, (uint32_t)i, keys[i], base);
}

// documents with more than SG_MAX_A n-grams (the reference's Writer.AddDocument has no limit, indexer_writer.go:66-86):
// the long tokeniser (engine.hip), a workgroup per slot of working memory
__global__ __launch_bounds__(64) void build_tokenize_long(const BuildArgs b, uint32_t n_long) {
  const int lane = threadIdx.x;
  uint8_t* slot = b.long_slots + (uint64_t)blockIdx.x * b.long_slot_bytes;
  const uint64_t* keys = (const uint64_t*)(slot + LongSlot::o_keys);
  for (uint32_t x = blockIdx.x; x < n_long; x += gridDim.x) {
    const uint32_t d = b.long_docs[x];
    const uint64_t o0 = b.offs[d], o1 = b.offs[d + 1];
    if (o1 - o0 > SG_LONG_MAX_TERMS) { if (lane == 0) atomicAdd(b.stats + 6, 1u); continue; }
    __syncthreads();
    const uint32_t A = long_tokenize(b.ix, false, b.docs + o0, (uint32_t)(o1 - o0), slot, lane);
    if (A == 0xFFFFFFFFu) { if (lane == 0) atomicAdd(b.stats + 6, 1u); continue; }   // more n-grams than the tables hold: unsupported, like too many bytes
    if (lane == 0) { b.doc_cnt[d] = A; atomicMax(b.stats + 0, A); }
    const uint64_t base = b.cap_off[d];
    for (uint32_t i = lane; i < A; i += 64) build_intern(b, d, i, keys[i], base);
    __syncthreads();
  }
}

__global__ void build_init_table(BuildSlot* table, uint32_t n_slots) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n_slots) { table[i].key = 0ull; table[i].stamp = ~0ull; }
}

__global__ void build_collect(const BuildSlot* table, uint32_t n_slots, const unsigned long long* zero_term, unsigned long long* stamps,
                              unsigned long long* keys, uint32_t* counter) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i == 0 && zero_term[0] != ~0ull) {
    const uint32_t at = atomicAdd(counter, 1u);
    stamps[at] = zero_term[0];
    keys[at] = 0ull;
  }
  if (i >= n_slots || table[i].key == 0ull) return;
  const uint32_t at = atomicAdd(counter, 1u);
  stamps[at] = table[i].stamp;
  keys[at] = table[i].key;
}

__device__ __forceinline__ uint32_t build_find(const BuildSlot* table, uint32_t mask, unsigned long long key) {
  uint32_t h = (uint32_t)d_mix64(key) & mask;
  while (table[h].key != key) h = (h + 1) & mask;
  return h;
}

__global__ void build_assign(BuildSlot* table, uint32_t mask, unsigned long long* zero_term, const unsigned long long* sorted_keys,
                             uint32_t n_terms) {
  const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= n_terms) return;
  if (sorted_keys[t] == 0ull) zero_term[0] = t;
  else table[build_find(table, mask, sorted_keys[t])].stamp = t;
}

__global__ __launch_bounds__(64) void build_emit(const BuildArgs b) {
  __shared__ uint32_t tid_lds[SG_MAX_A];
  const int lane = threadIdx.x;
  const uint32_t d = blockIdx.x;
  const uint32_t A = b.doc_cnt[d];
  const uint64_t base = b.cap_off[d];
  // term ids of the document's n-grams: in LDS, or — a long document — in the low words of its own key slots (every key
  // is read before the first id is written)
  const bool long_doc = A > SG_MAX_A;
  if (!long_doc) {
    for (uint32_t i = lane; i < A; i += 64) {
      const unsigned long long key = b.doc_keys[base + i];
      tid_lds[i] = (uint32_t)(key ? b.table[build_find(b.table, b.table_mask, key)].stamp : b.zero_term[0]);
    }
    __syncthreads();
  } else {
    for (uint32_t i0 = 0; i0 < A; i0 += 64) {
      const uint32_t i = i0 + (uint32_t)lane;
      unsigned long long key = 0;
      if (i < A) key = b.doc_keys[base + i];
      const uint32_t t = i < A ? (uint32_t)(key ? b.table[build_find(b.table, b.table_mask, key)].stamp : b.zero_term[0]) : 0u;
      if (i < A) b.doc_keys[base + i] = (unsigned long long)t | 0xABCD000000000000ull;      // (each lane rewrites only its own slot)
    }
    __threadfence();
    __syncthreads();
  }
  auto tid = [&](uint32_t j) -> uint32_t { return long_doc ? (uint32_t)__hip_atomic_load(b.doc_keys + base + j, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : tid_lds[j]; };
  for (uint32_t i = lane; i < A; i += 64) {
    const uint32_t t = tid(i);
    uint32_t before = 0, mult = 0;
    for (uint32_t j = 0; j < A; j++) { const bool eq = tid(j) == t; mult += eq; before += eq && j < i; }
    if (before) continue;                                       // the CSR keeps (term, doc) once
    b.sort_key[base + i] = t * b.S + A;
    b.sort_doc[base + i] = d;
    atomicAdd(b.list_len + (size_t)t * b.S + A, 1u);
    if (mult > 1) {                                             // SURVEY.md §A.2: the reference stores every occurrence
      const uint32_t at = atomicAdd(b.stats + 4, 1u);
      if (at < b.dup_cap) { b.dups[3 * at] = d; b.dups[3 * at + 1] = t; b.dups[3 * at + 2] = mult; }
      else atomicExch(b.stats + 5, 1u);
    }
  }
}

__global__ void build_chunks(const uint32_t* list_len, uint32_t n_lists, uint32_t* chunks) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n_lists) chunks[i] = (list_len[i] + 3u) >> 2;
}

__global__ void build_scatter(const uint32_t* sort_key, const uint32_t* sort_doc, uint64_t n_valid, const uint32_t* list_len,
                              const uint32_t* chunk_off, const uint32_t* src_off, uint32_t* postings) {
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n_valid) return;
  const uint32_t l = sort_key[i], d = sort_doc[i];
  const uint32_t pos = (uint32_t)(i - src_off[l]), len = list_len[l];
  uint32_t* p = postings + (uint64_t)chunk_off[l] * 4;
  p[pos] = d;
  if (pos == len - 1) for (uint32_t x = len; x < ((len + 3u) & ~3u); x++) p[x] = d;   // pad with the last docID
}

__global__ void build_seg_off(const uint32_t* chunk_off, uint32_t n_terms, uint32_t S, uint32_t total_chunks, uint32_t* seg_off) {
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= (uint64_t)n_terms * (S + 1)) return;
  const uint32_t t = (uint32_t)(i / (S + 1)), bseg = (uint32_t)(i % (S + 1));
  const uint64_t l = (uint64_t)t * S + bseg;
  seg_off[i] = l < (uint64_t)n_terms * S ? chunk_off[l] : total_chunks;
}

}  // namespace sg

namespace {

std::atomic<uint32_t> g_index_build_table_bits{0};      // sg_debug_index_build_table_bits (0: 20)
thread_local uint32_t t_index_build_report[4];          // the calling thread's last device build: tokenise passes, log2 of the final
                                                        // table, terms interned, documents the long tokeniser took (sg_debug_index_build_report)

int build_on_device(sg_index* ix, const uint8_t* utf8, const uint64_t* offs, uint32_t n_docs, int device) {
  HostIndex& h = ix->host;
  uint32_t* const report = t_index_build_report;
  report[0] = report[1] = report[2] = report[3] = 0;
  DeviceGuard dg;
  HIP_TRY(dg.set(device));
  h.n_docs = n_docs;
  BuildArgs b{};
  int rc;
  DeviceBlock mem;                                         // working memory, the description tables the tokeniser reads first: freed on return
  if ((rc = upload_description(h, mem, b.ix))) return rc;
  b.ix.slots = nullptr;
  b.n_docs = n_docs;
  if (n_docs == 0) { h.n_segments = 0; build_term_table(h); return SG_OK; }
  if (n_docs >= (1u << 26)) { set_error("more than 2^26 documents: beyond the device builder (a wavefront per document), use sg_index_build"); return SG_E_UNSUPPORTED; }

  // capacity of a document = the runes it can have (its bytes + the wrap), at most the tokeniser's limit
  const uint64_t wrap = h.wrap0.size() + h.wrap1.size();
  std::vector<uint64_t> cap_off((size_t)n_docs + 1, 0);
  uint64_t n_maybe_long = 0;                                  // (a document of at most 112 bytes fits the LDS tokeniser whatever it holds)
  for (uint32_t d = 0; d < n_docs; d++) {
    const uint64_t len = offs[d + 1] - offs[d];
    cap_off[d + 1] = cap_off[d] + len + wrap;
    n_maybe_long += len > 112;
  }
  const uint64_t cap_total = cap_off[n_docs];
  if (cap_total >= 0x7FFFFFF0ull) { set_error("dictionary too large for the device builder"); return SG_E_UNSUPPORTED; }

  uint8_t* d_docs; uint64_t *d_offs, *d_cap;
  uint32_t* d_stats;
  if ((rc = mem.alloc(&d_docs, (size_t)offs[n_docs])) || (rc = mem.alloc(&d_offs, (size_t)n_docs + 1)) ||
      (rc = mem.alloc(&d_cap, (size_t)n_docs + 1)) || (rc = mem.alloc(&b.doc_keys, (size_t)cap_total)) ||
      (rc = mem.alloc(&b.doc_cnt, (size_t)n_docs)) || (rc = mem.alloc(&d_stats, 8)) || (rc = mem.alloc(&b.zero_term, 2)) ||
      (rc = mem.alloc(&b.long_docs, (size_t)n_maybe_long + 1)))
    return rc;
  const uint32_t n_long_slots = (uint32_t)std::min<uint64_t>(n_maybe_long, 64);
  b.long_slot_bytes = LongSlot::bytes(0);
  if (n_long_slots && (rc = mem.alloc(&b.long_slots, (size_t)(b.long_slot_bytes * n_long_slots)))) return rc;
  HIP_TRY(hipMemcpy(d_docs, utf8, (size_t)offs[n_docs], hipMemcpyHostToDevice));
  HIP_TRY(hipMemcpy(d_offs, offs, ((size_t)n_docs + 1) * 8, hipMemcpyHostToDevice));
  HIP_TRY(hipMemcpy(d_cap, cap_off.data(), ((size_t)n_docs + 1) * 8, hipMemcpyHostToDevice));
  b.docs = d_docs; b.offs = d_offs; b.cap_off = d_cap; b.stats = d_stats;

  // K1 (the table is grown and the pass repeated if the dictionary has more distinct terms than guessed)
  uint32_t stats[8];
  uint32_t log2_table = 20;
  // (the test hook names the first table outright: under the capacity rule no dictionary could make it grow more than three times)
  if (const uint32_t bits = g_index_build_table_bits.load(std::memory_order_relaxed)) log2_table = bits;
  else while ((1ull << log2_table) < cap_total / 16 && log2_table < 26) log2_table++;
  for (;; log2_table += 2) {
    if (log2_table > 28) { set_error("too many distinct terms for the device builder"); return SG_E_UNSUPPORTED; }
    report[0]++;
    report[1] = log2_table;
    const size_t n_slots = (size_t)1 << log2_table;
    if ((rc = mem.alloc(&b.table, n_slots))) return rc;
    b.table_mask = (uint32_t)(n_slots - 1);
    hipLaunchKernelGGL(build_init_table, dim3((unsigned)((n_slots + 255) / 256)), dim3(256), 0, 0, b.table, (uint32_t)n_slots);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemset(d_stats, 0, 32));
    HIP_TRY(hipMemset(b.zero_term, 0xFF, 16));
    hipLaunchKernelGGL(build_tokenize, dim3(n_docs), dim3(64), 0, 0, b);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpy(stats, d_stats, 32, hipMemcpyDeviceToHost));
    if (stats[1] && !stats[3]) {                              // documents above 128 n-grams: the long tokeniser
      if (stats[1] > n_maybe_long || !n_long_slots) { set_error("internal: long-document list overrun"); return SG_E_INVALID; }
      hipLaunchKernelGGL(build_tokenize_long, dim3(std::min<uint32_t>(stats[1], n_long_slots)), dim3(64), 0, 0, b, stats[1]);
      HIP_TRY(hipGetLastError());
      HIP_TRY(hipMemcpy(stats, d_stats, 32, hipMemcpyDeviceToHost));
    }
    report[2] = stats[2];
    report[3] = stats[3] ? 0u : stats[1];
    if (!stats[3]) break;
  }
  if (stats[6]) { set_error("a document exceeds 65536 bytes: beyond the device builder, use sg_index_build"); return SG_E_UNSUPPORTED; }
  if (stats[0] + 1 > 0xFFFFu) { set_error("more than 65535 cardinality segments"); return SG_E_UNSUPPORTED; }
  const uint32_t n_terms = stats[2], S = std::max(stats[0] + 1, h.min_segments);   // indexer_writer.go:69-73
  const size_t n_slots = (size_t)b.table_mask + 1;
  if ((uint64_t)n_terms * S >= 0xFFFFFFF0ull) { set_error("terms x segments exceeds the device builder's 32-bit sort key"); return SG_E_UNSUPPORTED; }

  // K2: term numbering by first appearance
  unsigned long long *d_stamp, *d_key, *d_stamp2, *d_key2;
  uint32_t* d_counter;
  if ((rc = mem.alloc(&d_stamp, (size_t)n_terms)) || (rc = mem.alloc(&d_key, (size_t)n_terms)) || (rc = mem.alloc(&d_stamp2, (size_t)n_terms)) ||
      (rc = mem.alloc(&d_key2, (size_t)n_terms)) || (rc = mem.alloc(&d_counter, 4)))
    return rc;
  HIP_TRY(hipMemset(d_counter, 0, 4));
  hipLaunchKernelGGL(build_collect, dim3((unsigned)((n_slots + 255) / 256)), dim3(256), 0, 0, b.table, (uint32_t)n_slots, b.zero_term, d_stamp, d_key, d_counter);
  HIP_TRY(hipGetLastError());
  if ((rc = device_sort_pairs(mem, d_stamp, d_stamp2, d_key, d_key2, n_terms))) return rc;
  hipLaunchKernelGGL(build_assign, dim3((n_terms + 255) / 256), dim3(256), 0, 0, b.table, b.table_mask, b.zero_term, d_key2, n_terms);
  HIP_TRY(hipGetLastError());

  // K3
  b.S = S;
  b.dup_cap = (uint32_t)std::min<uint64_t>(cap_total, 1u << 23);   // (doc, term) pairs that repeat; beyond that: host builder
  if ((rc = mem.alloc(&b.sort_key, (size_t)cap_total)) || (rc = mem.alloc(&b.sort_doc, (size_t)cap_total)) ||
      (rc = mem.alloc(&b.list_len, (size_t)n_terms * S)) || (rc = mem.alloc(&b.dups, (size_t)b.dup_cap * 3)))
    return rc;
  HIP_TRY(hipMemset(b.sort_key, 0xFF, (size_t)cap_total * 4));
  HIP_TRY(hipMemset(b.list_len, 0, (size_t)n_terms * S * 4));
  hipLaunchKernelGGL(build_emit, dim3(n_docs), dim3(64), 0, 0, b);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipMemcpy(stats, d_stats, 32, hipMemcpyDeviceToHost));
  if (stats[5]) { set_error("too many documents with repeated terms for the device builder"); return SG_E_UNSUPPORTED; }

  // K4: stable sort by (term, segment); docIDs were emitted ascending
  uint32_t *d_key_s, *d_doc_s;
  if ((rc = mem.alloc(&d_key_s, (size_t)cap_total)) || (rc = mem.alloc(&d_doc_s, (size_t)cap_total))) return rc;
  if ((rc = device_sort_pairs(mem, b.sort_key, d_key_s, b.sort_doc, d_doc_s, (size_t)cap_total))) return rc;

  // K5
  const uint32_t n_cells = n_terms * S;
  uint32_t *d_chunks, *d_chunk_off, *d_src_off;
  if ((rc = mem.alloc(&d_chunks, (size_t)n_cells + 1)) || (rc = mem.alloc(&d_chunk_off, (size_t)n_cells + 1)) ||
      (rc = mem.alloc(&d_src_off, (size_t)n_cells + 1)))
    return rc;
  hipLaunchKernelGGL(build_chunks, dim3((n_cells + 255) / 256), dim3(256), 0, 0, b.list_len, n_cells, d_chunks);
  HIP_TRY(hipGetLastError());
  if ((rc = device_exclusive_sum(mem, d_chunks, d_chunk_off, n_cells)) || (rc = device_exclusive_sum(mem, b.list_len, d_src_off, n_cells))) return rc;
  // totals: last offset + last value, summed on the host in 64 bits
  h.list_len.resize(n_cells);
  HIP_TRY(hipMemcpy(h.list_len.data(), b.list_len, (size_t)n_cells * 4, hipMemcpyDeviceToHost));
  uint64_t total_chunks = 0, n_valid = 0;
  h.n_lists = 0;
  for (uint32_t l = 0; l < n_cells; l++) { total_chunks += (h.list_len[l] + 3u) >> 2; n_valid += h.list_len[l]; h.n_lists += h.list_len[l] != 0; }
  if (total_chunks >= 0xFFFFFFF0ull) { set_error("posting store exceeds 2^32 16-byte chunks"); return SG_E_UNSUPPORTED; }

  // K6: the posting store and the seg_off rows stay in HBM — the first sg_index_upload to this device adopts them
  // (no D2H + H2D round trip); the host copy below serves introspection, accounting and replicas on other GPUs
  uint32_t *d_postings, *d_seg_off;
  const size_t seg_n = (size_t)n_terms * (S + 1) + 1;
  DeviceBlock kept;
  if ((rc = kept.alloc(&d_postings, (size_t)total_chunks * 4)) || (rc = kept.alloc(&d_seg_off, seg_n))) return rc;
  HIP_TRY(hipMemset(d_seg_off, 0, seg_n * 4));
  if (n_valid) {
    hipLaunchKernelGGL(build_scatter, dim3((unsigned)((n_valid + 255) / 256)), dim3(256), 0, 0, d_key_s, d_doc_s, n_valid, b.list_len, d_chunk_off,
                       d_src_off, d_postings);
    HIP_TRY(hipGetLastError());
  }
  hipLaunchKernelGGL(build_seg_off, dim3((unsigned)((seg_n + 255) / 256)), dim3(256), 0, 0, d_chunk_off, n_terms, S, (uint32_t)total_chunks, d_seg_off);
  HIP_TRY(hipGetLastError());

  // back to the host index (introspection, accounting and sg_index_upload read it)
  h.n_segments = S;
  h.term_key.resize(n_terms);
  HIP_TRY(hipMemcpy(h.term_key.data(), d_key2, (size_t)n_terms * 8, hipMemcpyDeviceToHost));
  h.term_of.clear();
  h.term_of.reserve((size_t)n_terms * 2);
  for (uint32_t t = 0; t < n_terms; t++) h.term_of.emplace(h.term_key[t], t);
  h.seg_off.resize(seg_n);
  HIP_TRY(hipMemcpy(h.seg_off.data(), d_seg_off, seg_n * 4, hipMemcpyDeviceToHost));
  h.postings.resize((size_t)total_chunks * 4);
  HIP_TRY(hipMemcpy(h.postings.data(), d_postings, (size_t)total_chunks * 16, hipMemcpyDeviceToHost));
  h.n_postings = n_valid;
  {
    std::vector<uint32_t> cnt(n_docs);
    HIP_TRY(hipMemcpy(cnt.data(), b.doc_cnt, (size_t)n_docs * 4, hipMemcpyDeviceToHost));
    h.n_postings_raw = 0;
    for (uint32_t c : cnt) h.n_postings_raw += c;
    std::vector<uint32_t> dups((size_t)stats[4] * 3);
    if (stats[4]) HIP_TRY(hipMemcpy(dups.data(), b.dups, dups.size() * 4, hipMemcpyDeviceToHost));
    h.dups.clear();
    for (uint32_t i = 0; i < stats[4]; i++) h.dups.push_back(DupEntry{dups[3 * i + 1], cnt[dups[3 * i]], dups[3 * i], dups[3 * i + 2]});
    std::sort(h.dups.begin(), h.dups.end(), [](const DupEntry& x, const DupEntry& y) {
      if (x.term != y.term) return x.term < y.term;
      if (x.segment != y.segment) return x.segment < y.segment;
      return x.doc < y.doc;
    });
  }
  build_term_table(h);
  HIP_TRY(hipDeviceSynchronize());
  std::unique_ptr<Replica> keep(new Replica());
  keep->device = device;
  keep->mem = std::move(kept);
  keep->dix.postings = d_postings;
  keep->dix.seg_off = d_seg_off;
  ix->prebuilt = std::move(keep);
  return SG_OK;
}

}  // namespace
