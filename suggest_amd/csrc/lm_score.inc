// lm_score.inc — LanguageModel.ScoreSentence / ScoreWordIDs for a batch of sentences on the device (pkg/lm/language_model.go:55-92,
// ngram_model.go:44-62,163-175; the host restatement is lm_model_score / lm_score_word_ids in lm.cpp).  Included by engine.hip
// behind SpellArgs and the word tokeniser's helpers, which it reuses:
//   lm_text_tokenize_kernel  one thread per line: lm.NewTokenizer(alphabet).Tokenize (lower case, trim U+0020, maximal runs of
//                            alphabet runes).  The lower-cased tokens go one behind the other into the line's slot of w_blob and
//                            tok[] records where each one starts; the vocabulary lookups are left to the next launch, where every
//                            lane takes a token.
//   lm_score_kernel          a workgroup per group of sentences (text: lines): (text only) the vocabulary lookup of every token,
//                            its id written over its start; then the stupid-backoff walk of every window, one window per thread,
//                            and the sum per sentence in window order by the sentence's own thread.
// Windows: seq = [start] + ids + [end]; every run of `order` consecutive words of seq, left to right (generator.go:9-24).
// Score(window) backs off to the window's PREFIX, like the reference (c_i = the count of its first i words), not to its suffix.

#define SG_LM_GROUP 256u          // threads of a score workgroup = windows (tokens) per round; sentences per group at most

struct LmScoreArgs {
  SpellArgs sp;                   // level tables (values, child_begin, level_base, cb_base, n_parents, order) and the word
                                  // tokeniser's (q_blob = the text, alphabet, lower-case pairs, vocabulary, start_symbol)
  uint32_t n;                     // sentences
  uint32_t per_group;             // sentences per workgroup (1 .. SG_LM_GROUP)
  uint32_t end_symbol;
  uint32_t total0;                // CorpusCount of the unigram level: counts[0] of every window
  uint32_t n_uni;                 // entries of the unigram level
  uint32_t uni_dense;             // 1: the unigram level holds every word in id order (word w is entry w; checked by lm_upload)
  uint32_t text;                  // 1: text (tok[] holds the token starts, turned into ids in place); 0: the caller's ids
  uint32_t slot_mul;              // bytes of a line's slot in w_blob per byte of the line (2; 3 when U+FFFD is in the alphabet)
  uint64_t text_bytes;            // text: bytes of q_blob (offsets are clamped to it)
  const uint64_t* offs;           // [n + 1] text: byte offsets of the lines; ids: byte offsets of the sentences in ids
  const uint32_t* ids;            // ids: the word ids
  uint32_t* tok;                  // text: [text_bytes / 2 + n + 1]; line i owns tok[offs[i] / 2 + i ..] (a line of L bytes has at
                                  // most (L + 1) / 2 tokens)
  uint32_t* n_tok;                // text: [n] tokens of line i
  uint32_t* w_len;                // text: [n] bytes written to line i's slot
  uint8_t* w_blob;                // text: line i's slot is w_blob[slot_mul * offs[i] .. slot_mul * offs[i + 1])
  double* out_scores;             // [n]
  uint32_t* out_words;            // text: [n] tokens per line (may be null)
  uint32_t* out_unknown;          // text: [n] tokens without an id (may be null)
};

__device__ __forceinline__ void lm_line_range(const LmScoreArgs& a, uint32_t i, uint64_t* o0, uint64_t* o1) {
  *o0 = min(a.offs[i], a.text_bytes);                            // (device offsets are the caller's: every access stays in the
  *o1 = min(max(a.offs[i + 1], *o0), a.text_bytes);              //  buffers whatever they hold)
}

__global__ __launch_bounds__(256) void lm_text_tokenize_kernel(const LmScoreArgs a) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= a.n) return;
  const SpellArgs& p = a.sp;
  uint64_t o0, o1;
  lm_line_range(a, i, &o0, &o1);
  const uint8_t* q = p.q_blob + o0;
  uint32_t pos = 0, b = (uint32_t)(o1 - o0);
  while (pos < b && q[pos] == ' ') pos++;                        // (U+0020 is the byte 0x20 and nothing else)
  while (b > pos && q[b - 1] == ' ') b--;
  uint8_t* slot = a.w_blob + a.slot_mul * o0;
  uint32_t* tk = a.tok + (o0 >> 1) + i;
  uint32_t out = 0, start = 0, nt = 0;
  while (pos < b) {
    uint32_t adv;
    const uint32_t r = d_lower_pairs(p, d_next_rune(q + pos, b - pos, &adv));
    pos += adv;
    if (!d_lm_alpha_has(p, r)) {
      if (out != start) { tk[nt++] = start; start = out; }
      continue;
    }
    const uint32_t w = d_width(r);
    if (w == 1u) slot[out] = (uint8_t)r;
    else if (w == 2u) { slot[out] = (uint8_t)(0xC0u | (r >> 6)); slot[out + 1] = (uint8_t)(0x80u | (r & 0x3Fu)); }
    else if (w == 3u) { slot[out] = (uint8_t)(0xE0u | (r >> 12)); slot[out + 1] = (uint8_t)(0x80u | ((r >> 6) & 0x3Fu)); slot[out + 2] = (uint8_t)(0x80u | (r & 0x3Fu)); }
    else { slot[out] = (uint8_t)(0xF0u | (r >> 18)); slot[out + 1] = (uint8_t)(0x80u | ((r >> 12) & 0x3Fu)); slot[out + 2] = (uint8_t)(0x80u | ((r >> 6) & 0x3Fu)); slot[out + 3] = (uint8_t)(0x80u | (r & 0x3Fu)); }
    out += w;
  }
  if (out != start) tk[nt++] = start;
  a.n_tok[i] = nt;
  a.w_len[i] = out;
}

// Exclusive prefix over the group's values (thread t's v; 0 from t = S on): pre[0 .. SG_LM_GROUP]; returns the total.
// Every thread of the workgroup calls it.
__device__ uint32_t lm_group_scan(uint32_t* pre, uint32_t v, uint32_t t) {
  __syncthreads();                                               // (the previous readers of pre are done)
  pre[t + 1] = v;
  __syncthreads();
  if (t < 64u) {                                                 // four per lane of the first wave, one wave scan
    const uint32_t c0 = pre[4 * t + 1], c1 = pre[4 * t + 2], c2 = pre[4 * t + 3], c3 = pre[4 * t + 4];
    const uint32_t sum = c0 + c1 + c2 + c3, excl = wave_scan_incl(sum, (int)t) - sum;
    pre[4 * t + 1] = excl + c0; pre[4 * t + 2] = excl + c0 + c1; pre[4 * t + 3] = excl + c0 + c1 + c2; pre[4 * t + 4] = excl + sum;
    if (t == 0u) pre[0] = 0u;
  }
  __syncthreads();
  return pre[SG_LM_GROUP];
}

// the sentence of the group that item x (< pre[S]) belongs to: the largest j with pre[j] <= x (a sentence without items
// shares its start with the next one, which is the larger)
__device__ __forceinline__ uint32_t lm_group_find(const uint32_t* pre, uint32_t S, uint32_t x) {
  uint32_t lo = 0, hi = S - 1u;
  while (lo < hi) { const uint32_t mid = (lo + hi + 1u) >> 1; if (pre[mid] <= x) lo = mid; else hi = mid - 1u; }
  return lo;
}

// NGramModel.Score (ngram_model.go:44-62) of one window w[0 .. order): one binary search per level in one bucket — the parent's,
// or the orphans' (bucket n_parents[l]) after a miss — then calcScore (ngram_model.go:163-175) with its argument formed as the
// host forms it: factor * c_i / c_{i-1}, left to right in f64, factor = 0.4 multiplied once per level backed off.
__device__ double lm_window_score(const LmScoreArgs& a, const uint32_t* w) {
  const SpellArgs& p = a.sp;
  const uint32_t N = p.order;
  uint32_t counts[9];
  counts[0] = a.total0;
  uint32_t parent = kNoContext;
#pragma unroll
  for (uint32_t l = 0; l < 8u; l++) {
    counts[l + 1] = 0u;
    if (l < N) {
      const uint64_t* v = p.values + p.level_base[l];
      uint32_t at = kNoContext;
      if (l == 0u && a.uni_dense) {
        if (w[0] < a.n_uni) { at = w[0]; counts[1] = (uint32_t)v[at]; }
      } else if (parent == kNoContext || parent < p.n_parents[l]) {
        const uint32_t bucket = parent == kNoContext ? p.n_parents[l] : parent;
        const uint32_t* cb = p.child_begin + p.cb_base[l];
        uint32_t lo = cb[bucket], hi = cb[bucket + 1];
        const uint32_t end = hi, word = w[l];
        while (lo < hi) { const uint32_t mid = (lo + hi) >> 1; if ((uint32_t)(v[mid] >> 32) < word) lo = mid + 1u; else hi = mid; }
        if (lo < end) {
          const uint64_t e = v[lo];
          if ((uint32_t)(e >> 32) == word) { at = lo; counts[l + 1] = (uint32_t)e; }
        }
      }
      parent = at;
    }
  }
  double factor = 1.0;
  uint32_t num = 0, den = 0;
  bool found = false;
#pragma unroll
  for (uint32_t i = 8; i >= 1u; i--) {
    if (i <= N && !found) {
      if (counts[i] > 0u) { num = counts[i]; den = counts[i - 1]; found = true; }
      else factor *= 0.4;
    }
  }
  return found ? log(factor * (double)num / (double)den) : -100.0;
}

__global__ __launch_bounds__(256) void lm_score_kernel(const LmScoreArgs a) {
  __shared__ uint32_t s_pre[SG_LM_GROUP + 1];    // exclusive prefix of the group's tokens, then of its windows
  __shared__ uint32_t s_cnt[SG_LM_GROUP];        // words of sentence j
  __shared__ uint32_t s_unk[SG_LM_GROUP];        // its words without an id
  __shared__ uint64_t s_base[SG_LM_GROUP];       // its first word: in tok (text) or ids
  __shared__ uint64_t s_slot[SG_LM_GROUP];       // text: its slot in w_blob
  __shared__ double s_sc[SG_LM_GROUP];           // the round's window scores
  const uint32_t t = threadIdx.x, s0 = blockIdx.x * a.per_group;
  const uint32_t S = min(a.per_group, a.n - s0);
  const uint32_t N = a.sp.order;
  uint32_t len = 0;
  if (t < S) {
    const uint32_t i = s0 + t;
    if (a.text) {
      uint64_t o0, o1;
      lm_line_range(a, i, &o0, &o1);
      len = min(a.n_tok[i], (uint32_t)((o1 - o0 + 1u) >> 1));
      s_base[t] = (o0 >> 1) + i;
      s_slot[t] = a.slot_mul * o0;
    } else {
      const uint64_t o0 = a.offs[i] >> 2;
      len = (uint32_t)((a.offs[i + 1] >> 2) - o0);
      s_base[t] = o0;
    }
    s_cnt[t] = len;
    s_unk[t] = 0u;
  }
  if (a.text) {                                                  // (uniform) the vocabulary lookups, a token per thread
    const uint32_t total = lm_group_scan(s_pre, len, t);
    for (uint32_t xb = 0; xb < total; xb += SG_LM_GROUP) {
      const uint32_t x = xb + t;
      const bool mine = x < total;
      uint32_t j = 0, st = 0, en = 0;
      uint64_t at = 0;
      if (mine) {
        j = lm_group_find(s_pre, S, x);
        const uint32_t k = x - s_pre[j];
        at = s_base[j] + k;
        const uint32_t wl = a.w_len[s0 + j];                     // (clamped: lines that overlap cannot send a read past a slot)
        en = min(k + 1u < s_cnt[j] ? a.tok[at + 1] : wl, wl);
        st = min(a.tok[at], en);
      }
      __syncthreads();                                           // every start of the round is read before ids overwrite them
      if (mine) {
        const uint8_t* wb = a.w_blob + s_slot[j] + st;
        const uint32_t wl = en - st;
        uint64_t h = SG_WORD_HASH_SEED;
        for (uint32_t c = 0; c < wl; c++) h = d_word_hash_step(h, wb[c]);
        const uint32_t id = d_word_id(a.sp, h, wb, wl);
        a.tok[at] = id;
        if (id == kUnknownWord) atomicAdd(&s_unk[j], 1u);
      }
    }
    __syncthreads();                                             // (the group's ids are visible to all its threads)
  }
  const uint32_t* src = a.text ? a.tok : a.ids;
  const uint32_t n_win = len + 2u >= N ? len + 3u - N : 0u;
  const uint32_t total = lm_group_scan(s_pre, t < S ? n_win : 0u, t);
  double acc = 0.0;
  for (uint32_t xb = 0; xb < total; xb += SG_LM_GROUP) {
    const uint32_t x = xb + t;
    if (x < total) {
      const uint32_t j = lm_group_find(s_pre, S, x);
      const uint32_t k = x - s_pre[j], n = s_cnt[j];
      const uint32_t* ids = src + s_base[j];
      uint32_t w[8];
#pragma unroll
      for (uint32_t l = 0; l < 8u; l++) {
        const uint32_t m = k + l;                                // position in seq = [start] + ids + [end]
        w[l] = l >= N ? 0u : m == 0u ? a.sp.start_symbol : m == n + 1u ? a.end_symbol : ids[m - 1u];
      }
      s_sc[t] = lm_window_score(a, w);
    }
    __syncthreads();
    if (t < S) {                                                 // score += Score(window), in window order
      const uint32_t lo = max(s_pre[t], xb), hi = min(s_pre[t + 1], xb + SG_LM_GROUP);
      for (uint32_t y = lo; y < hi; y++) acc += s_sc[y - xb];
    }
    __syncthreads();
  }
  if (t < S) {
    const uint32_t i = s0 + t;
    a.out_scores[i] = acc;
    if (a.text && a.out_words) a.out_words[i] = len;
    if (a.text && a.out_unknown) a.out_unknown[i] = s_unk[t];
  }
}
