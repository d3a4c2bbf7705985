// lm_store.cpp — the host side of the language model's two reference formats that lm.cpp does not write:
//   mph_build            mph.Build + mph.Store (pkg/mph/mph.go:40-145,159-192): the minimal perfect hash RetrieveLMFromBinary reads
//                        straight after the model section of <name>.lm (pkg/lm/binary.go:59-98, table.Load)
//   lm_gm_check          what a model must be for its levels to be spelled as lines (sg_lm_store_google refuses the rest)
//   lm_store_google_host the plain writer of <dir>/<k>-gm, lines "w1 .. wk\tcount\n" (pkg/lm/ngram_writer.go:12,51-60): the referee
//                        the device writer of lm_store.inc is read against — both write identical files
// No HIP here: tests/cpp/lm_store_test.cpp compiles this file with the host compiler alone.
//
// The MPH stays on the host on purpose: the greedy places the buckets one after another in exactly the order the reference's
// sort leaves them (the fixture tests/golden/lm/test.lm pins values and auxiliary words, tie order included), and it is linear
// in the vocabulary.
#include <algorithm>
#include <chrono>
#include <cstring>

#include "sg_internal.h"

namespace sg {

uint32_t mph_hash(uint32_t h, const std::string& w) {     // mph.go:236-247: seed 0 stands for the FNV offset basis
  if (h == 0) h = 2166136261u;
  for (unsigned char c : w) { h *= 16777619u; h ^= c; }
  return h;
}

namespace {

// Go 1.14 sort.Slice (src/sort/zfuncversion.go: insertionSort_func, siftDown_func, heapSort_func, medianOfThree_func,
// doPivot_func, quickSort_func; slice.go: maxDepth) over positions 0 .. n, driven by a less and a swap on positions like Go's
// lessSwap.  The sort is unstable and mph.Build's less is not strict (len(i) >= len(j)), so WHICH order it leaves equal
// buckets in is part of the file format.  Restated on its own from the Go source; tests/mph_ref.py holds another restatement.
template <class Less, class Swap>
struct GoSliceSort {
  Less less;
  Swap swap;
  void insertion_sort(long a, long b) {
    for (long i = a + 1; i < b; i++)
      for (long j = i; j > a && less(j, j - 1); j--) swap(j, j - 1);
  }
  void sift_down(long lo, long hi, long first) {
    long root = lo;
    for (;;) {
      long child = 2 * root + 1;
      if (child >= hi) return;
      if (child + 1 < hi && less(first + child, first + child + 1)) child++;
      if (!less(first + root, first + child)) return;
      swap(first + root, first + child);
      root = child;
    }
  }
  void heap_sort(long a, long b) {
    const long first = a, lo = 0, hi = b - a;
    for (long i = (hi - 1) / 2; i >= 0; i--) sift_down(i, hi, first);
    for (long i = hi - 1; i >= 0; i--) { swap(first, first + i); sift_down(lo, i, first); }
  }
  void median_of_three(long m1, long m0, long m2) {
    if (less(m1, m0)) swap(m1, m0);
    if (less(m2, m1)) {
      swap(m2, m1);
      if (less(m1, m0)) swap(m1, m0);
    }
  }
  void do_pivot(long lo, long hi, long* midlo, long* midhi) {
    const long m = (long)((unsigned long)(lo + hi) >> 1);
    if (hi - lo > 40) {                                     // Tukey's ninther
      const long s = (hi - lo) / 8;
      median_of_three(lo, lo + s, lo + 2 * s);
      median_of_three(m, m - s, m + s);
      median_of_three(hi - 1, hi - 1 - s, hi - 1 - 2 * s);
    }
    median_of_three(lo, m, hi - 1);
    const long pivot = lo;
    long a = lo + 1, c = hi - 1;
    for (; a < c && less(a, pivot); a++) {}
    long b = a;
    for (;;) {
      for (; b < c && !less(pivot, b); b++) {}
      for (; b < c && less(pivot, c - 1); c--) {}
      if (b >= c) break;
      swap(b, c - 1);
      b++; c--;
    }
    bool protect = hi - c < 5;
    if (!protect && hi - c < (hi - lo) / 4) {
      int dups = 0;
      if (!less(pivot, hi - 1)) { swap(c, hi - 1); c++; dups++; }
      if (!less(b - 1, pivot)) { b--; dups++; }
      if (!less(m, pivot)) { swap(m, b - 1); b--; dups++; }
      protect = dups > 1;
    }
    if (protect) {
      for (;;) {
        for (; a < b && !less(b - 1, pivot); b--) {}
        for (; a < b && less(a, pivot); a++) {}
        if (a >= b) break;
        swap(a, b - 1);
        a++; b--;
      }
    }
    swap(pivot, b - 1);
    *midlo = b - 1; *midhi = c;
  }
  void quick_sort(long a, long b, int max_depth) {
    while (b - a > 12) {
      if (max_depth == 0) { heap_sort(a, b); return; }
      max_depth--;
      long mlo, mhi;
      do_pivot(a, b, &mlo, &mhi);
      if (mlo - a < b - mhi) { quick_sort(a, mlo, max_depth); a = mhi; }
      else { quick_sort(mhi, b, max_depth); b = mlo; }
    }
    if (b - a > 1) {
      for (long i = a + 6; i < b; i++)                      // a ShellSort pass with gap 6
        if (less(i, i - 6)) swap(i, i - 6);
      insertion_sort(a, b);
    }
  }
  void sort(long n) {
    int depth = 0;
    for (long i = n; i > 0; i >>= 1) depth++;
    quick_sort(0, n, depth * 2);
  }
};

template <class Less, class Swap>
void go_slice_sort(long n, Less less, Swap swap) { GoSliceSort<Less, Swap> s{less, swap}; s.sort(n); }

void put_u32(std::string& s, uint32_t v) { for (int i = 0; i < 4; i++) s.push_back((char)(v >> (8 * i))); }

}  // namespace

int mph_build(const std::vector<std::string>& words, std::vector<uint32_t>& values, std::vector<int32_t>& auxiliary, std::string& err) {
  const uint64_t n64 = words.size();
  values.clear(); auxiliary.clear();
  if (n64 == 0) return SG_OK;
  if (n64 >= 0x7FFFFFFFull) { err = "too many words for a minimal perfect hash (the auxiliary words are int32)"; return SG_E_UNSUPPORTED; }
  const uint32_t n = (uint32_t)n64;
  constexpr uint32_t kFree = 0xFFFFFFFFu;                   // math.MaxUint32
  values.assign(n, kFree);
  auxiliary.assign(n, 0);
  // Step 1: the ids of a bucket in id order (dict.Iterate goes by id), as one array with its bounds
  std::vector<uint32_t> home(n), begin((size_t)n + 1, 0), ids(n);
  for (uint32_t i = 0; i < n; i++) { home[i] = mph_hash(0, words[i]) % n; begin[home[i] + 1]++; }
  for (uint32_t b = 0; b < n; b++) begin[b + 1] += begin[b];
  {
    std::vector<uint32_t> at(begin.begin(), begin.end() - 1);
    for (uint32_t i = 0; i < n; i++) ids[at[home[i]]++] = i;
  }
  // Step 2: the buckets by size, largest first, in the order sort.Slice leaves them
  std::vector<uint32_t> order(n);
  for (uint32_t b = 0; b < n; b++) order[b] = b;
  auto size_of = [&](long p) { return begin[order[p] + 1] - begin[order[p]]; };
  go_slice_sort((long)n, [&](long i, long j) { return size_of(i) >= size_of(j); }, [&](long i, long j) { std::swap(order[i], order[j]); });
  uint32_t bucket_iter = 0;
  std::vector<uint32_t> slots;
  for (uint32_t p = 0; p < n; p++) {
    const uint32_t* bucket = ids.data() + begin[order[p]];
    const uint32_t len = (uint32_t)size_of(p);
    if (len <= 1) break;
    for (uint32_t i = 1; i < len; i++)                      // two equal words collide under every seed: the reference would not end
      for (uint32_t j = 0; j < i; j++)
        if (words[bucket[i]] == words[bucket[j]]) { err = "the dictionary lists the word \"" + words[bucket[i]] + "\" twice: no perfect hash exists"; return SG_E_UNSUPPORTED; }
    uint32_t d = 1, item = 0;
    slots.clear();
    while (item < len) {
      const uint32_t slot = mph_hash(d, words[bucket[item]]) % n;
      if (values[slot] != kFree || std::find(slots.begin(), slots.end(), slot) != slots.end()) {
        if (d == 0x7FFFFFFFu) { err = "no seed below 2^31 places a bucket of the minimal perfect hash"; return SG_E_UNSUPPORTED; }
        d++; item = 0; slots.clear();
      } else {
        slots.push_back(slot); item++;
      }
    }
    auxiliary[order[p]] = (int32_t)d;                       // hash(0, bucket[0]) % size is the bucket itself
    for (uint32_t i = 0; i < len; i++) values[slots[i]] = bucket[i];
    bucket_iter++;
  }
  // singletons: the last free slot each, marked by a negative auxiliary word
  std::vector<uint32_t> free_slots;
  for (uint32_t i = 0; i < n; i++) if (values[i] == kFree) free_slots.push_back(i);
  for (uint32_t p = bucket_iter; p < n; p++) {
    if (size_of(p) == 0 || free_slots.empty()) break;
    const uint32_t slot = free_slots.back();
    free_slots.pop_back();
    auxiliary[order[p]] = -(int32_t)slot - 1;
    values[slot] = ids[begin[order[p]]];
  }
  return SG_OK;
}

// mph.Store: u32 n, the values, u32 n, the auxiliary words, little endian; no words: the two zero lengths
int mph_section(const std::vector<std::string>& words, std::string& out, std::string& err) {
  std::vector<uint32_t> values;
  std::vector<int32_t> auxiliary;
  if (int rc = mph_build(words, values, auxiliary, err)) return rc;
  out.clear();
  out.reserve(8 + 8 * values.size());
  put_u32(out, (uint32_t)values.size());
  for (uint32_t v : values) put_u32(out, v);
  put_u32(out, (uint32_t)auxiliary.size());
  for (int32_t v : auxiliary) put_u32(out, (uint32_t)v);
  return SG_OK;
}

// ---- <dir>/<k>-gm ----

uint32_t lm_gm_slice_budget(int64_t set) {                  // sg_debug_lm_store_slice_bytes; set < 0: read it
  static std::atomic<uint32_t> g{0};
  if (set >= 0) g.store((uint32_t)set, std::memory_order_relaxed);
  const uint32_t v = g.load(std::memory_order_relaxed);
  return v ? v : kGmSliceBytes;
}

int lm_gm_check(const HostLM& lm, std::string& err) {
  const size_t n_words = lm.words.size();
  if (lm.level.empty() || lm.level.size() > 8) { err = "a model of 1 .. 8 levels is expected"; return SG_E_INVALID; }
  for (size_t k = 0; k < lm.level.size(); k++) {
    const LmLevel& lv = lm.level[k];
    const std::string at = "level " + std::to_string(k + 1) + ": ";
    const size_t n = lv.word.size(), n_parents = k ? lm.level[k - 1].word.size() : 0;
    if (n >= 0x7FFFFFF0ull) { err = at + "2^31 entries or more"; return SG_E_UNSUPPORTED; }
    if (lv.count.size() != n || lv.child_begin.size() != n_parents + 2 || lv.child_begin[0] != 0 || lv.child_begin.back() != n) { err = at + "malformed"; return SG_E_INVALID; }
    for (size_t b = 0; b + 1 < lv.child_begin.size(); b++)
      if (lv.child_begin[b] > lv.child_begin[b + 1]) { err = at + "malformed"; return SG_E_INVALID; }
    for (size_t e = 0; e < n; e++) {
      if (lv.word[e] == kUnknownWord) { err = at + "an entry ends in the unknown word, which has no spelling"; return SG_E_UNSUPPORTED; }
      if (lv.word[e] >= n_words) { err = at + "a word id outside the dictionary"; return SG_E_INVALID; }
    }
    if (k == 0) {
      bool ok = n == n_words;
      for (size_t e = 0; ok && e < n; e++) ok = lv.word[e] == e;
      if (!ok) { err = at + "not one entry per word in id order (a word listed twice, or one without a count)"; return SG_E_UNSUPPORTED; }
    } else if (lv.child_begin[n_parents] != n) {
      err = at + "entries without a context in the level below: their leading words are not recoverable";
      return SG_E_UNSUPPORTED;
    }
  }
  uint64_t longest = 0, bytes = 0;
  for (const auto& w : lm.words) { longest = std::max<uint64_t>(longest, w.size()); bytes += w.size(); }
  if (bytes >= 0xFFFFFFF0ull || longest * 8 + 32 >= 0x7FFFFFFFull) { err = "the words are too long for the n-gram writer"; return SG_E_UNSUPPORTED; }
  return SG_OK;
}

void lm_gm_parents(const LmLevel& lv, std::vector<uint32_t>& parent) {
  parent.assign(lv.word.size(), 0);
  for (size_t b = 0; b + 1 < lv.child_begin.size(); b++)
    for (uint32_t e = lv.child_begin[b]; e < lv.child_begin[b + 1]; e++) parent[e] = (uint32_t)b;
}

std::string lm_gm_path(const char* out_dir, size_t k) { return std::string(out_dir) + "/" + std::to_string(k) + "-gm"; }

GmFile::~GmFile() { if (f) fclose(f); }
int GmFile::open(const std::string& p, std::string& err) {
  path = p;
  f = fopen(p.c_str(), "wb");
  if (!f) { err = "failed to create an output: " + p; return SG_E_INVALID; }
  return SG_OK;
}
int GmFile::write(const void* data, size_t n, std::string& err) {
  if (n && fwrite(data, 1, n, f) != n) { err = "failed to write " + path; return SG_E_INVALID; }
  return SG_OK;
}
int GmFile::close(std::string& err) {
  const int rc = fclose(f);
  f = nullptr;
  if (rc) { err = "failed to write " + path; return SG_E_INVALID; }
  return SG_OK;
}

// 1-gm: a line per word in id order; k-gm: in level entry order (by context entry, then by word id) — the order in which
// sg_lm_load_google_ex(dir, id_order = 0) gives the model back array for array.  seconds[1] formatting, seconds[3] file writes.
int lm_store_google_host(const HostLM& lm, const char* out_dir, double seconds[4], std::string& err) {
  using clk = std::chrono::steady_clock;
  if (int rc = lm_gm_check(lm, err)) return rc;
  std::vector<std::vector<uint32_t>> parent(lm.level.size());
  std::string buf;
  for (size_t k = 0; k < lm.level.size(); k++) {
    auto t0 = clk::now();
    const LmLevel& lv = lm.level[k];
    if (k) lm_gm_parents(lv, parent[k]);
    seconds[1] += std::chrono::duration<double>(clk::now() - t0).count();
    GmFile out;
    if (int rc = out.open(lm_gm_path(out_dir, k + 1), err)) return rc;
    buf.clear();
    t0 = clk::now();
    for (size_t e = 0; e < lv.word.size(); e++) {
      uint32_t ids[8];
      uint32_t p = (uint32_t)e;
      for (size_t j = k + 1; j-- > 0;) { ids[j] = lm.level[j].word[p]; if (j) p = parent[j][p]; }
      for (size_t j = 0; j <= k; j++) { buf += lm.words[ids[j]]; buf.push_back(j < k ? ' ' : '\t'); }
      char digits[12];
      const int nd = snprintf(digits, sizeof digits, "%u", lv.count[e]);
      buf.append(digits, (size_t)nd);
      buf.push_back('\n');
      if (buf.size() >= (1u << 20) || e + 1 == lv.word.size()) {
        const auto tw = clk::now();
        if (int rc = out.write(buf.data(), buf.size(), err)) return rc;
        const double w = std::chrono::duration<double>(clk::now() - tw).count();
        seconds[3] += w; seconds[1] -= w;
        buf.clear();
      }
    }
    seconds[1] += std::chrono::duration<double>(clk::now() - t0).count();
    const auto tw = clk::now();
    if (int rc = out.close(err)) return rc;
    seconds[3] += std::chrono::duration<double>(clk::now() - tw).count();
  }
  return SG_OK;
}

}  // namespace sg
