// lm_build.inc — the language model built from a corpus on the device (sg_lm_build_device, lm_api.inc), included by engine.hip after
// capi.inc.  It uses host_base.inc's DeviceBlock, device_exclusive_sum and device_total and handles.inc's lm_alphabet_tables,
// behind the word tokeniser's helpers of engine.hip (d_next_rune, d_lower_pairs, d_lm_alpha_has, d_put_rune), which it reuses.
//
// What it restates: NGramBuilder.Build over NewSentenceRetriever (pkg/lm/ngram_builder.go:19-64, sentence_retriever.go:54-81),
// lm.NewTokenizer, buildDictionary's numbering (binary.go:140-198) and the vector builder as lm_load_google restates it — the
// result equals lm_build_google_files followed by lm_load_google on its files, array for array.
//
// Go's decoding makes rune starts locally decidable: a byte that is no continuation byte (10xxxxxx) always starts a rune; a
// continuation byte starts one (a U+FFFD of width 1) unless the nearest non-continuation byte at most three bytes before it
// begins a valid sequence that covers it.  So every thread can take a fixed slice of the text.
//
//   lm_build_walk<false>   a thread per 16-byte slice (a workgroup stages 4 KiB + halo in LDS with 16-byte loads): the runes
//                          that start in the slice are decoded, classified (separator / alphabet after lower-casing / other)
//                          and counted: bytes of lower-cased tokens, token ends, separators
//   3 x ExclusiveSum       where a slice's tokens, token bytes and sentences begin
//   lm_build_walk<true>    the same walk: the lower-cased token bytes go one token behind the other into a blob, every token
//                          records where it ends there (it begins where its predecessor ends) and its sentence number
//   lm_build_intern        a thread per token (+ the two markers, appended to the blob): FNV-1a of its bytes, open addressing
//                          on (hash tag << 32 | a token that spells the word); a hit is confirmed on the bytes, so two words
//                          with one hash stay two words.  Also flags the first token of every sentence with tokens.
//   ExclusiveSum           sentences with tokens before a token -> its place in the wrapped stream
//   lm_build_seq           seq[] = the table slots of <S> w1 .. wn </S> per sentence, eos[] marks the </S> positions
//   lm_build_count         count and first position per word: one atomicAdd + atomicMin per distinct word of a wavefront
//   lm_build_collect, lm_build_gather   the distinct words (count, first position, bytes) for the host, which numbers them
//   lm_build_ids           slots -> word ids in seq[]
//   per level k >= 2:      lm_build_keys (ctx[k-1][p] << 32 | seq[p+k-1]; a window must not run over a </S>), one radix sort,
//                          lm_build_heads + ExclusiveSum (run-length), lm_build_entries (ctx[k][p] = the entry of the k-gram at
//                          p), lm_build_values (word << 32 | count), lm_build_child_begin (a binary search per parent)
// On the host: word numbering (work per distinct word), the copy of the finished levels into HostLM (per distinct n-gram).

namespace sg {

#define SG_LMB_BLOCK_BYTES 4096u          // text bytes of a walk workgroup: 256 slices of 16
#define SG_LMB_INVALID 0xFFFFFFFFu        // ctx[k][p]: no k-gram starts at p
#define SG_LMB_EMPTY 0xFFFFFFFFFFFFFFFFull

struct LmRuneSet {                // alphabet.Has as d_lm_alpha_has reads it
  const uint2* alpha_ranges; uint32_t n_alpha_ranges;   // runes >= 128 as inclusive ranges, ascending
  uint64_t alpha_ascii[2];                              // ... and below 128 as a bitmap
};
struct LmLowerTable { const uint32_t* lower_from; const uint32_t* lower_to; uint32_t n_lower; };   // as d_lower_pairs reads it

struct LmBuildArgs {
  LmRuneSet alpha, sep;           // the model's alphabet; the sentence separators
  LmLowerTable lower;
  const uint8_t* text;            // readable from text - 16 to text + n_blocks * 4096 + 16 (zeros outside the corpus)
  uint64_t len;
  const uint32_t* sl_bytes; const uint32_t* sl_toks; const uint32_t* sl_seps;   // emit: [n_slices] where a slice's output begins
  uint32_t* o_bytes; uint32_t* o_toks; uint32_t* o_seps;                        // count: [n_slices] what a slice holds
  uint8_t* blob; uint32_t* tok_end; uint32_t* tok_sent;                         // emit
};

enum { LMB_OTHER = 0, LMB_ALPHA = 1, LMB_SEP = 2, LMB_END = 3 };

// the rune that starts at s (n bytes of text are left, capped): its class, its width in the text, its lower-cased form
__device__ __forceinline__ uint32_t lm_build_classify(const LmBuildArgs& a, const uint8_t* s, uint32_t n, uint32_t* adv, uint32_t* low) {
  const uint32_t r = d_next_rune(s, n, adv);
  if (d_lm_alpha_has(a.sep, r)) return LMB_SEP;                  // (the raw rune: sentence_retriever.go:60-70)
  *low = d_lower_pairs(a.lower, r);
  return d_lm_alpha_has(a.alpha, *low) ? LMB_ALPHA : LMB_OTHER;
}

template <bool kEmit>
__global__ __launch_bounds__(256) void lm_build_walk(const LmBuildArgs a) {
  __shared__ __align__(16) uint8_t s_raw[16 + SG_LMB_BLOCK_BYTES + 16];
  const uint32_t t = threadIdx.x;
  const uint64_t b0 = (uint64_t)blockIdx.x * SG_LMB_BLOCK_BYTES;
  ((uint4*)(s_raw + 16))[t] = ((const uint4*)(a.text + b0))[t];
  if (t == 0u) *(uint4*)s_raw = *(const uint4*)(a.text + b0 - 16);
  if (t == 1u) *(uint4*)(s_raw + 16 + SG_LMB_BLOCK_BYTES) = *(const uint4*)(a.text + b0 + SG_LMB_BLOCK_BYTES);
  __syncthreads();
  const uint8_t* s = s_raw + 16;                                 // s[i] = text[b0 + i], i = -16 .. 4096 + 15
  const uint32_t slice = blockIdx.x * 256u + t;
  const uint64_t left = a.len > b0 ? a.len - b0 : 0u;            // text bytes from b0 on
  const int rel_len = (int)min(left, (uint64_t)(SG_LMB_BLOCK_BYTES + 16u));   // ... as far as the staged bytes reach
  const int end = min((int)(t * 16u + 16u), min(rel_len, (int)SG_LMB_BLOCK_BYTES));
  auto n_at = [&](int i) { return (uint32_t)min(left - (uint64_t)((int64_t)i), (uint64_t)8); };   // (d_next_rune asks for 4 at most)
  // the first rune that starts in the slice: one of its first four bytes
  int i = (int)(t * 16u);
  for (; i < end; i++) {
    if ((s[i] & 0xC0u) != 0x80u) break;
    bool covered = false;
    for (int j = 1; j <= 3; j++) {
      if (b0 + (uint64_t)i < (uint64_t)j) break;                 // (the text begins here)
      if ((s[i - j] & 0xC0u) == 0x80u) continue;
      uint32_t adv;
      (void)d_next_rune(s + i - j, n_at(i - j), &adv);
      covered = adv > (uint32_t)j;
      break;
    }
    if (!covered) break;
  }
  uint32_t bytes = 0, toks = 0, seps = 0;
  if (kEmit) { bytes = a.sl_bytes[slice]; toks = a.sl_toks[slice]; seps = a.sl_seps[slice]; }
  if (i < end) {
    uint32_t adv = 1, low = 0;
    uint32_t cls = lm_build_classify(a, s + i, n_at(i), &adv, &low);
    while (i < end) {
      const int nxt = i + (int)adv;
      uint32_t n_adv = 1, n_low = 0, n_cls = LMB_END;
      if (nxt < rel_len) n_cls = lm_build_classify(a, s + nxt, n_at(nxt), &n_adv, &n_low);
      if (cls == LMB_ALPHA) {
        const uint32_t w = d_width(low);
        if (kEmit) d_put_rune(a.blob + bytes, low);
        bytes += w;
        if (n_cls != LMB_ALPHA) {                                // the token ends with this rune
          if (kEmit) { a.tok_end[toks] = bytes; a.tok_sent[toks] = seps; }
          toks++;
        }
      } else if (cls == LMB_SEP) seps++;
      i = nxt; cls = n_cls; adv = n_adv; low = n_low;
    }
  }
  if (!kEmit) { a.o_bytes[slice] = bytes; a.o_toks[slice] = toks; a.o_seps[slice] = seps; }
}

__device__ __forceinline__ bool lm_build_same_bytes(const uint8_t* x, const uint8_t* y, uint32_t n) {
  for (uint32_t i = 0; i < n; i++) if (x[i] != y[i]) return false;
  return true;
}

// token t (< n_tok; n_tok and n_tok + 1 are the start and end symbols) -> the table slot of its word.  table[s] is EMPTY or
// tag << 32 | a token that spells the slot's word: set once by the compare-and-swap that claims the slot, so whoever reads it finds
// the bytes to compare with (the blob was written by the launch before).
__global__ __launch_bounds__(256) void lm_build_intern(const uint8_t* blob, const uint32_t* tok_end, const uint32_t* tok_sent, uint32_t n_tok,
                                                       unsigned long long* table, uint32_t mask, uint32_t hash_bits, uint32_t* tok_slot,
                                                       uint32_t* first_flag, uint32_t* n_distinct) {
  const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= n_tok + 2u) return;
  const uint32_t s0 = t ? tok_end[t - 1u] : 0u, n = tok_end[t] - s0;
  const uint8_t* w = blob + s0;
  uint64_t h = SG_WORD_HASH_SEED;
  for (uint32_t i = 0; i < n; i++) h = d_word_hash_step(h, w[i]);
  if (hash_bits && hash_bits < 64u) h &= (1ull << hash_bits) - 1ull;          // sg_debug_lm_build_hash_bits
  h = d_mix64(h);
  const uint32_t tag = (uint32_t)(h >> 32);
  const unsigned long long mine = ((unsigned long long)tag << 32) | t;
  uint32_t s = (uint32_t)h & mask;
  for (;; s = (s + 1u) & mask) {                                               // (the table has twice as many slots as tokens)
    unsigned long long cur = table[s];
    if (cur == SG_LMB_EMPTY) {
      cur = atomicCAS(&table[s], SG_LMB_EMPTY, mine);
      if (cur == SG_LMB_EMPTY) { atomicAdd(n_distinct, 1u); break; }
    }
    if ((uint32_t)(cur >> 32) != tag) continue;
    const uint32_t rep = (uint32_t)cur, r0 = rep ? tok_end[rep - 1u] : 0u;
    if (tok_end[rep] - r0 == n && lm_build_same_bytes(blob + r0, w, n)) break;
  }
  tok_slot[t] = s;
  if (t < n_tok) first_flag[t] = (t == 0u || tok_sent[t] != tok_sent[t - 1u]) ? 1u : 0u;
}

// token t is word number t + 2 * S - 1 of the wrapped stream, S = sentences with tokens up to and with its own
__global__ __launch_bounds__(256) void lm_build_seq(const uint32_t* tok_slot, const uint32_t* tok_sent, const uint32_t* first_flag,
                                                    const uint32_t* first_pre, uint32_t n_tok, uint32_t* seq, uint8_t* eos) {
  const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= n_tok) return;
  const uint32_t pos = t + 2u * (first_pre[t] + first_flag[t]) - 1u;
  seq[pos] = tok_slot[t];
  if (first_flag[t]) seq[pos - 1u] = tok_slot[n_tok];
  if (t + 1u == n_tok || tok_sent[t + 1u] != tok_sent[t]) { seq[pos + 1u] = tok_slot[n_tok + 1u]; eos[pos + 1u] = 1; }
}

// count[slot] and the first position of every word.  A wavefront adds once per distinct word it holds: the markers and the
// commonest words are a fifth of a text, and an atomic per position would queue them all on a handful of addresses.
__global__ __launch_bounds__(256) void lm_build_count(const uint32_t* seq, uint32_t n_seq, uint32_t* count, uint32_t* first) {
  const uint32_t p = blockIdx.x * blockDim.x + threadIdx.x;
  const bool valid = p < n_seq;
  const uint32_t slot = valid ? seq[p] : 0u;
  const uint32_t lane = threadIdx.x & 63u;
  uint64_t todo = __ballot(valid);
  while (todo) {
    const int l = __ffsll((unsigned long long)todo) - 1;
    const uint32_t sl = (uint32_t)__shfl((int)slot, l);
    const uint64_t m = __ballot(valid && slot == sl);
    if (lane == (uint32_t)l) { atomicAdd(count + sl, (uint32_t)__popcll(m)); atomicMin(first + sl, p); }   // (its lowest lane: its first position)
    todo &= ~m;
  }
}

__global__ __launch_bounds__(256) void lm_build_collect(const unsigned long long* table, uint32_t n_slots, const uint32_t* tok_end, const uint32_t* count,
                                                        const uint32_t* first, uint32_t cap, uint32_t* counter, uint32_t* v_slot, uint32_t* v_count,
                                                        uint32_t* v_first, uint32_t* v_start, uint32_t* v_len) {
  const uint32_t s = blockIdx.x * blockDim.x + threadIdx.x;
  if (s >= n_slots || table[s] == SG_LMB_EMPTY) return;
  const uint32_t i = atomicAdd(counter, 1u);
  if (i >= cap) return;
  const uint32_t rep = (uint32_t)table[s], r0 = rep ? tok_end[rep - 1u] : 0u;
  v_slot[i] = s; v_count[i] = count[s]; v_first[i] = first[s]; v_start[i] = r0; v_len[i] = tok_end[rep] - r0;
}

__global__ __launch_bounds__(256) void lm_build_gather(const uint8_t* blob, const uint32_t* v_start, const uint32_t* v_off, uint32_t n_words, uint8_t* out) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n_words) return;
  const uint8_t* src = blob + v_start[i];
  for (uint32_t o = v_off[i], e = v_off[i + 1u]; o < e; o++) out[o] = *src++;
}

__global__ __launch_bounds__(256) void lm_build_slot_ids(const uint32_t* v_slot, const uint32_t* v_id, uint32_t n_words, uint32_t* id_of_slot) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n_words) id_of_slot[v_slot[i]] = v_id[i];
}

__global__ __launch_bounds__(256) void lm_build_ids(uint32_t* seq, uint32_t n_seq, const uint32_t* id_of_slot) {
  const uint32_t p = blockIdx.x * blockDim.x + threadIdx.x;
  if (p < n_seq) seq[p] = id_of_slot[seq[p]];
}

// level k (>= 2): key[p] = ctx[k-1][p] << 32 | seq[p+k-1] where a k-gram starts at p — a (k-1)-gram does and its last word is no
// </S> — and n_prev << 32, which sorts behind every key, elsewhere.  (eos[n_seq - 1] is set: p + k - 1 stays inside.)
__global__ __launch_bounds__(256) void lm_build_keys(const uint32_t* seq, const uint8_t* eos, const uint32_t* ctx_prev, uint32_t n_seq, uint32_t k,
                                                     uint32_t n_prev, unsigned long long* key, uint32_t* pos, uint32_t* n_valid) {
  const uint32_t p = blockIdx.x * blockDim.x + threadIdx.x;
  bool valid = false;
  if (p < n_seq) {
    const uint32_t c = ctx_prev[p];
    valid = c != SG_LMB_INVALID && !eos[p + k - 2u];
    key[p] = valid ? ((unsigned long long)c << 32) | seq[p + k - 1u] : (unsigned long long)n_prev << 32;
    pos[p] = p;
  }
  const uint64_t m = __ballot(valid);
  if ((threadIdx.x & 63u) == 0u && m) atomicAdd(n_valid, (uint32_t)__popcll(m));
}

__global__ __launch_bounds__(256) void lm_build_heads(const unsigned long long* key, uint32_t n_seq, uint32_t n_valid, uint32_t* head) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n_seq) head[i] = (i < n_valid && (i == 0u || key[i] != key[i - 1u])) ? 1u : 0u;
}

__global__ __launch_bounds__(256) void lm_build_entries(const unsigned long long* key, const uint32_t* pos, const uint32_t* head, const uint32_t* head_pre,
                                                        uint32_t n_seq, uint32_t n_valid, uint32_t* ctx, uint32_t* e_start, unsigned long long* e_key) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n_seq) return;
  if (i >= n_valid) { ctx[pos[i]] = SG_LMB_INVALID; return; }
  const uint32_t e = head_pre[i] + head[i] - 1u;
  ctx[pos[i]] = e;
  if (head[i]) { e_start[e] = i; e_key[e] = key[i]; }
}

__global__ __launch_bounds__(256) void lm_build_values(const uint32_t* e_start, const unsigned long long* e_key, uint32_t n_entries, uint32_t n_valid,
                                                       unsigned long long* values) {
  const uint32_t e = blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= n_entries) return;
  const uint32_t to = e + 1u < n_entries ? e_start[e + 1u] : n_valid;
  values[e] = (e_key[e] << 32) | (unsigned long long)(to - e_start[e]);
}

// child_begin[b], b = 0 .. n_prev + 1: the first entry whose parent is b or later (the bucket of orphans, b = n_prev, is empty:
// a corpus has no n-gram without its prefix)
__global__ __launch_bounds__(256) void lm_build_child_begin(const unsigned long long* e_key, uint32_t n_entries, uint32_t n_buckets, uint32_t* child_begin) {
  const uint32_t b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= n_buckets) return;
  uint32_t lo = 0, hi = n_entries;
  while (lo < hi) { const uint32_t mid = (lo + hi) >> 1; if ((uint32_t)(e_key[mid] >> 32) < b) lo = mid + 1u; else hi = mid; }
  child_begin[b] = lo;
}

}  // namespace sg

namespace {

std::atomic<uint32_t> g_lm_build_hash_bits{0};     // sg_debug_lm_build_hash_bits

// the model of a corpus without a token: what lm_load_google makes of empty count files
void lm_build_empty(HostLM& h, uint32_t order) {
  for (uint32_t k = 0; k < order; k++) { LmLevel lv; lv.child_begin.assign(2, 0); h.level.push_back(std::move(lv)); }
}

#define LMB_GRID(n) dim3((unsigned)(((size_t)(n) + 255) / 256)), dim3(256), 0, 0
#define LMB_LAUNCHED() HIP_TRY(hipGetLastError())

int lm_build_on_device(const uint8_t* text, uint64_t len, uint32_t order, const std::string& start_symbol, const std::string& end_symbol,
                       const std::vector<std::string>& separators, int id_order, int device, HostLM& h) {
  DeviceGuard dg;
  HIP_TRY(dg.set(device));
  DeviceBlock mem;
  int rc;
  LmBuildArgs a{};
  // ---- the tables of the walk
  {
    std::vector<uint2> ranges;
    lm_alphabet_tables(h.alphabet, a.alpha.alpha_ascii, ranges);
    if ((rc = mem.upload(ranges, &a.alpha.alpha_ranges))) return rc;
    a.alpha.n_alpha_ranges = (uint32_t)ranges.size();
    lm_alphabet_tables(separators, a.sep.alpha_ascii, ranges);
    if ((rc = mem.upload(ranges, &a.sep.alpha_ranges))) return rc;
    a.sep.n_alpha_ranges = (uint32_t)ranges.size();
    std::vector<uint32_t> lf, lt;
    for (const auto& pr : kLowerPairs) { lf.push_back(pr.from); lt.push_back(pr.to); }
    if ((rc = mem.upload(lf, &a.lower.lower_from)) || (rc = mem.upload(lt, &a.lower.lower_to))) return rc;
    a.lower.n_lower = (uint32_t)lf.size();
  }
  // ---- the text, with 16 readable bytes before it and the last workgroup's 4 KiB + 16 behind it
  const size_t n_blocks = (size_t)((len + SG_LMB_BLOCK_BYTES - 1) / SG_LMB_BLOCK_BYTES), n_slices = n_blocks * 256;
  const size_t text_cap = 16 + n_blocks * SG_LMB_BLOCK_BYTES + 16;
  uint8_t* d_text;
  if ((rc = mem.alloc(&d_text, text_cap))) return rc;
  HIP_TRY(hipMemset(d_text, 0, 16));
  HIP_TRY(hipMemset(d_text + 16 + len, 0, text_cap - 16 - (size_t)len));
  HIP_TRY(hipMemcpy(d_text + 16, text, (size_t)len, hipMemcpyHostToDevice));
  a.text = d_text + 16; a.len = len;
  uint32_t *c_bytes, *c_toks, *c_seps, *p_bytes, *p_toks, *p_seps;
  if ((rc = mem.alloc(&c_bytes, n_slices)) || (rc = mem.alloc(&c_toks, n_slices)) || (rc = mem.alloc(&c_seps, n_slices)) ||
      (rc = mem.alloc(&p_bytes, n_slices)) || (rc = mem.alloc(&p_toks, n_slices)) || (rc = mem.alloc(&p_seps, n_slices)))
    return rc;
  a.o_bytes = c_bytes; a.o_toks = c_toks; a.o_seps = c_seps;
  hipLaunchKernelGGL(lm_build_walk<false>, dim3((unsigned)n_blocks), dim3(256), 0, 0, a);
  LMB_LAUNCHED();
  if ((rc = device_exclusive_sum(mem, c_bytes, p_bytes, n_slices)) || (rc = device_exclusive_sum(mem, c_toks, p_toks, n_slices)) || (rc = device_exclusive_sum(mem, c_seps, p_seps, n_slices)))
    return rc;
  uint32_t blob_bytes = 0, n_tok = 0;                            // (a GiB of text holds 3 GiB of token bytes at most: invalid bytes
  if ((rc = device_total(c_bytes, p_bytes, n_slices, &blob_bytes)) || (rc = device_total(c_toks, p_toks, n_slices, &n_tok))) return rc;   //  as U+FFFD)
  if (n_tok == 0) { lm_build_empty(h, order); return SG_OK; }
  if ((uint64_t)blob_bytes + start_symbol.size() + end_symbol.size() >= 0xFFFFFFF0ull) { set_error("corpus too large for the device builder: its tokens pass 4 GiB"); return SG_E_UNSUPPORTED; }

  // ---- tokens: blob, where each ends, its sentence; the markers behind them
  const uint32_t n_all = n_tok + 2u;
  uint8_t* d_blob;
  uint32_t *tok_end, *tok_sent, *tok_slot, *first_flag, *first_pre, *d_counters;
  if ((rc = mem.alloc(&d_blob, (size_t)blob_bytes + start_symbol.size() + end_symbol.size())) || (rc = mem.alloc(&tok_end, (size_t)n_all)) ||
      (rc = mem.alloc(&tok_sent, (size_t)n_all)) || (rc = mem.alloc(&tok_slot, (size_t)n_all)) || (rc = mem.alloc(&first_flag, (size_t)n_tok)) ||
      (rc = mem.alloc(&first_pre, (size_t)n_tok)) || (rc = mem.alloc(&d_counters, 16)))
    return rc;
  HIP_TRY(hipMemset(d_counters, 0, 64));
  a.sl_bytes = p_bytes; a.sl_toks = p_toks; a.sl_seps = p_seps;
  a.blob = d_blob; a.tok_end = tok_end; a.tok_sent = tok_sent;
  hipLaunchKernelGGL(lm_build_walk<true>, dim3((unsigned)n_blocks), dim3(256), 0, 0, a);
  LMB_LAUNCHED();
  {
    const uint32_t ends[2] = {blob_bytes + (uint32_t)start_symbol.size(), blob_bytes + (uint32_t)(start_symbol.size() + end_symbol.size())};
    HIP_TRY(hipMemcpy(d_blob + blob_bytes, start_symbol.data(), start_symbol.size(), hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(d_blob + ends[0], end_symbol.data(), end_symbol.size(), hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(tok_end + n_tok, ends, 8, hipMemcpyHostToDevice));
  }
  // ---- vocabulary
  size_t n_slots = 16;
  while (n_slots < (size_t)n_all * 2) n_slots <<= 1;
  unsigned long long* table;
  uint32_t *w_count, *w_first;
  if ((rc = mem.alloc(&table, n_slots)) || (rc = mem.alloc(&w_count, n_slots)) || (rc = mem.alloc(&w_first, n_slots))) return rc;
  HIP_TRY(hipMemset(table, 0xFF, n_slots * 8));
  HIP_TRY(hipMemset(w_count, 0, n_slots * 4));
  HIP_TRY(hipMemset(w_first, 0xFF, n_slots * 4));
  hipLaunchKernelGGL(lm_build_intern, LMB_GRID(n_all), d_blob, tok_end, tok_sent, n_tok, table, (uint32_t)(n_slots - 1),
                     g_lm_build_hash_bits.load(std::memory_order_relaxed), tok_slot, first_flag, d_counters);
  LMB_LAUNCHED();
  if ((rc = device_exclusive_sum(mem, first_flag, first_pre, n_tok))) return rc;
  uint32_t n_sent = 0, n_words = 0;
  if ((rc = device_total(first_flag, first_pre, n_tok, &n_sent))) return rc;
  HIP_TRY(hipMemcpy(&n_words, d_counters, 4, hipMemcpyDeviceToHost));
  const uint64_t n_seq64 = (uint64_t)n_tok + 2ull * n_sent;
  if (n_seq64 >= 0x7FFFFFF0ull) { set_error("corpus too large for the device builder: tokens and markers pass 2^31"); return SG_E_UNSUPPORTED; }
  const uint32_t n_seq = (uint32_t)n_seq64;

  // ---- the wrapped stream, counts and first positions
  uint32_t* seq;
  uint8_t* eos;
  if ((rc = mem.alloc(&seq, (size_t)n_seq)) || (rc = mem.alloc(&eos, (size_t)n_seq + 8))) return rc;
  HIP_TRY(hipMemset(eos, 0, (size_t)n_seq + 8));
  hipLaunchKernelGGL(lm_build_seq, LMB_GRID(n_tok), tok_slot, tok_sent, first_flag, first_pre, n_tok, seq, eos);
  LMB_LAUNCHED();
  hipLaunchKernelGGL(lm_build_count, LMB_GRID(n_seq), seq, n_seq, w_count, w_first);
  LMB_LAUNCHED();
  uint32_t *v_slot, *v_count, *v_first, *v_start, *v_len, *v_off, *v_id;
  if ((rc = mem.alloc(&v_slot, (size_t)n_words)) || (rc = mem.alloc(&v_count, (size_t)n_words)) || (rc = mem.alloc(&v_first, (size_t)n_words)) ||
      (rc = mem.alloc(&v_start, (size_t)n_words)) || (rc = mem.alloc(&v_len, (size_t)n_words)) || (rc = mem.alloc(&v_off, (size_t)n_words + 1)) ||
      (rc = mem.alloc(&v_id, (size_t)n_words)))
    return rc;
  hipLaunchKernelGGL(lm_build_collect, LMB_GRID(n_slots), table, (uint32_t)n_slots, tok_end, w_count, w_first, n_words, d_counters + 1, v_slot, v_count,
                     v_first, v_start, v_len);
  LMB_LAUNCHED();
  // ---- on the host: the words and their numbering (work per distinct word)
  std::vector<uint32_t> hc(n_words), hf(n_words), hl(n_words), off((size_t)n_words + 1, 0);
  HIP_TRY(hipMemcpy(hc.data(), v_count, (size_t)n_words * 4, hipMemcpyDeviceToHost));
  HIP_TRY(hipMemcpy(hf.data(), v_first, (size_t)n_words * 4, hipMemcpyDeviceToHost));
  HIP_TRY(hipMemcpy(hl.data(), v_len, (size_t)n_words * 4, hipMemcpyDeviceToHost));
  uint64_t vocab_bytes = 0;
  for (uint32_t i = 0; i < n_words; i++) { off[i] = (uint32_t)vocab_bytes; vocab_bytes += hl[i]; }
  if (vocab_bytes >= 0xFFFFFFF0ull) { set_error("vocabulary too large"); return SG_E_UNSUPPORTED; }
  off[n_words] = (uint32_t)vocab_bytes;
  uint8_t* d_vbytes;
  if ((rc = mem.alloc(&d_vbytes, (size_t)vocab_bytes))) return rc;
  HIP_TRY(hipMemcpy(v_off, off.data(), ((size_t)n_words + 1) * 4, hipMemcpyHostToDevice));
  hipLaunchKernelGGL(lm_build_gather, LMB_GRID(n_words), d_blob, v_start, v_off, n_words, d_vbytes);
  LMB_LAUNCHED();
  std::string vbytes((size_t)vocab_bytes, '\0');
  if (vocab_bytes) HIP_TRY(hipMemcpy(&vbytes[0], d_vbytes, (size_t)vocab_bytes, hipMemcpyDeviceToHost));
  std::vector<uint32_t> by_id(n_words), id_of(n_words);          // by_id[id] = collected index; id_of = its inverse
  for (uint32_t i = 0; i < n_words; i++) by_id[i] = i;
  auto word_less = [&](uint32_t x, uint32_t y) {
    const int c = memcmp(vbytes.data() + off[x], vbytes.data() + off[y], std::min(hl[x], hl[y]));
    return c ? c < 0 : hl[x] < hl[y];
  };
  if (id_order == 0) std::sort(by_id.begin(), by_id.end(), [&](uint32_t x, uint32_t y) { return hf[x] < hf[y]; });   // 1-gm line order
  else std::sort(by_id.begin(), by_id.end(), [&](uint32_t x, uint32_t y) { return hc[x] != hc[y] ? hc[x] > hc[y] : word_less(x, y); });   // binary.go:141-199
  h.words.resize(n_words);
  h.id_of.reserve((size_t)n_words * 2);
  LmLevel uni;
  uni.word.resize(n_words); uni.count.resize(n_words);
  for (uint32_t id = 0; id < n_words; id++) {
    const uint32_t i = by_id[id];
    id_of[i] = id;
    h.words[id].assign(vbytes.data() + off[i], hl[i]);
    h.id_of.emplace(h.words[id], id);
    uni.word[id] = id; uni.count[id] = hc[i];
  }
  uni.child_begin = {0u, n_words};
  uni.total = n_seq;
  h.level.push_back(std::move(uni));
  HIP_TRY(hipMemcpy(v_id, id_of.data(), (size_t)n_words * 4, hipMemcpyHostToDevice));
  hipLaunchKernelGGL(lm_build_slot_ids, LMB_GRID(n_words), v_slot, v_id, n_words, w_count);   // (the counts are on the host: their array takes the ids)
  LMB_LAUNCHED();
  hipLaunchKernelGGL(lm_build_ids, LMB_GRID(n_seq), seq, n_seq, w_count);
  LMB_LAUNCHED();

  // ---- levels 2 .. order
  if (order > 1) {
    unsigned long long *key_a, *key_b, *e_key, *values;
    uint32_t *pos_a, *pos_b, *head, *head_pre, *e_start, *ctx[2], *child_begin;
    if ((rc = mem.alloc(&key_a, (size_t)n_seq)) || (rc = mem.alloc(&key_b, (size_t)n_seq)) || (rc = mem.alloc(&e_key, (size_t)n_seq)) ||
        (rc = mem.alloc(&values, (size_t)n_seq)) || (rc = mem.alloc(&pos_a, (size_t)n_seq)) || (rc = mem.alloc(&pos_b, (size_t)n_seq)) ||
        (rc = mem.alloc(&head, (size_t)n_seq)) || (rc = mem.alloc(&head_pre, (size_t)n_seq)) || (rc = mem.alloc(&e_start, (size_t)n_seq)) ||
        (rc = mem.alloc(&ctx[0], (size_t)n_seq)) || (rc = mem.alloc(&ctx[1], (size_t)n_seq)) || (rc = mem.alloc(&child_begin, (size_t)n_seq + 2)))
      return rc;
    size_t sort_bytes = 0, scan_bytes = 0;                       // one block of working memory for the sorts and the scans
    HIP_TRY(hipcub::DeviceRadixSort::SortPairs(nullptr, sort_bytes, key_a, key_b, pos_a, pos_b, (int)n_seq, 0, 64));
    HIP_TRY(hipcub::DeviceScan::ExclusiveSum(nullptr, scan_bytes, head, head_pre, (int)n_seq));
    uint8_t* sort_tmp;
    if ((rc = mem.alloc(&sort_tmp, std::max(sort_bytes, scan_bytes)))) return rc;
    const uint32_t* ctx_prev = seq;                               // the unigram of a word is entry number id
    uint32_t n_prev = n_words;
    for (uint32_t k = 2; k <= order; k++) {
      uint32_t n_valid = 0, n_entries = 0;
      if (n_prev) {
        uint32_t* ctx_cur = ctx[k & 1u];
        HIP_TRY(hipMemset(d_counters + 2, 0, 4));
        hipLaunchKernelGGL(lm_build_keys, LMB_GRID(n_seq), seq, eos, ctx_prev, n_seq, k, n_prev, key_a, pos_a, d_counters + 2);
        LMB_LAUNCHED();
        int end_bit = 33;                                         // the word, and the bits of 0 .. n_prev
        while (end_bit < 64 && ((uint64_t)n_prev >> (end_bit - 32))) end_bit++;
        HIP_TRY(hipcub::DeviceRadixSort::SortPairs(sort_tmp, sort_bytes, key_a, key_b, pos_a, pos_b, (int)n_seq, 0, end_bit));
        HIP_TRY(hipMemcpy(&n_valid, d_counters + 2, 4, hipMemcpyDeviceToHost));
        hipLaunchKernelGGL(lm_build_heads, LMB_GRID(n_seq), key_b, n_seq, n_valid, head);
        LMB_LAUNCHED();
        HIP_TRY(hipcub::DeviceScan::ExclusiveSum(sort_tmp, scan_bytes, head, head_pre, (int)n_seq));
        if ((rc = device_total(head, head_pre, n_seq, &n_entries))) return rc;
        hipLaunchKernelGGL(lm_build_entries, LMB_GRID(n_seq), key_b, pos_b, head, head_pre, n_seq, n_valid, ctx_cur, e_start, e_key);
        LMB_LAUNCHED();
        if (n_entries) {
          hipLaunchKernelGGL(lm_build_values, LMB_GRID(n_entries), e_start, e_key, n_entries, n_valid, values);
          LMB_LAUNCHED();
        }
        hipLaunchKernelGGL(lm_build_child_begin, LMB_GRID((size_t)n_prev + 2), e_key, n_entries, n_prev + 2u, child_begin);
        LMB_LAUNCHED();
        ctx_prev = ctx_cur;
      }
      // the finished level -> HostLM (work per distinct n-gram)
      LmLevel lv;
      lv.total = n_valid;
      lv.child_begin.assign((size_t)n_prev + 2, 0);
      if (n_prev) HIP_TRY(hipMemcpy(lv.child_begin.data(), child_begin, ((size_t)n_prev + 2) * 4, hipMemcpyDeviceToHost));
      std::vector<uint64_t> vals(n_entries);
      if (n_entries) HIP_TRY(hipMemcpy(vals.data(), values, (size_t)n_entries * 8, hipMemcpyDeviceToHost));
      lv.word.resize(n_entries); lv.count.resize(n_entries);
      for (uint32_t e = 0; e < n_entries; e++) { lv.word[e] = (uint32_t)(vals[e] >> 32); lv.count[e] = (uint32_t)vals[e]; }
      h.level.push_back(std::move(lv));
      n_prev = n_entries;
    }
  }
  HIP_TRY(hipDeviceSynchronize());
  return SG_OK;
}

}  // namespace
