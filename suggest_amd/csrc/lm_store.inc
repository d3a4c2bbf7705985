// lm_store.inc — the device writer behind sg_lm_store_google, included by engine.hip after index_store.inc (it uses HIP_TRY,
// DeviceGuard, DeviceBlock and StoreStream).  Replaces the walk of googleNGramFormatWriter.Write
// (pkg/lm/ngram_writer.go:32-76) over a trie of Go maps with the finished levels of a model spelled as lines
// "w1 .. wk\tcount\n"; the host writer the kernels are read against is lm_store_google_host (lm_store.cpp), and both write
// identical files.
//
// Per level, two passes with a prefix sum between them: bytes and offsets never depend on scheduling.
//   lm_gm_parent   a thread per entry: parent[e] = the bucket of child_begin that holds e, by binary search (buckets run from one
//                  child to most of a level, so not a thread per bucket)
//   lm_gm_size     a thread per entry: e -> parent -> .. up to level 1; the line is the word lengths, k + 1 separators and the
//                  decimal digits of the count
//   ExclusiveSum   hipcub, 64-bit: where each line begins
//   lm_gm_write    a thread per line, a wavefront per 64 consecutive lines (contiguous in the output): each lane formats its own
//                  line and stores it byte by byte.  Plain vector stores only; nothing reads or rewrites a dword it shares.
//                  (A form that built the 64 lines in LDS and copied them out with dword stores took the same time, to within
//                  2 % on the whole device part, and was removed: DESIGN.md 4g.)
// A level is formatted in slices of entries whose text fits lm_gm_slice_budget() bytes; each slice is copied back and appended
// to the file, so memory is bounded whatever the model.  Everything is staged from HostLM into memory of this call, on a
// stream of its own, and freed before it returns: nothing of lm_upload, Predict or scoring is read or written.

namespace sg {

struct GmArgs {
  const uint8_t* wbytes; const uint32_t* woff; uint32_t n_words;      // the words' bytes back to back, [n_words + 1] offsets
  const uint32_t* word[8]; const uint32_t* count[8]; const uint32_t* cbeg[8]; uint32_t* parent[8]; uint32_t n[8];   // per level
  uint32_t k;                                               // the level at work, 0-based
  uint64_t *len, *off;                                      // [n[k] + 1] line lengths (the last is 0) and their exclusive sum
  uint32_t e0, e1;                                          // the slice
  uint8_t* out; uint64_t out_bytes;                         // its text: off[e1] - off[e0] bytes
};

__global__ void lm_gm_parent(const GmArgs a) {
  const uint64_t e = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const uint32_t k = a.k;
  if (k == 0 || e >= a.n[k] || a.n[k - 1] == 0) return;
  const uint32_t* cb = a.cbeg[k];
  uint32_t lo = 0, hi = a.n[k - 1] + 1;                     // the first bucket bound above e, among cb[1 .. n_parents + 1]
  while (lo < hi) { const uint32_t mid = lo + ((hi - lo) >> 1); if (cb[mid + 1] > (uint32_t)e) hi = mid; else lo = mid + 1; }
  a.parent[k][e] = min(lo, a.n[k - 1] - 1u);
}

// the words of entry e of level a.k, first word first
__device__ __forceinline__ void gm_chain(const GmArgs& a, uint32_t e, uint32_t ids[8]) {
  uint32_t p = e;
#pragma unroll
  for (int j = 7; j >= 0; j--) {
    ids[j] = 0;
    if ((uint32_t)j <= a.k) {
      p = min(p, a.n[j] - 1u);
      ids[j] = min(a.word[j][p], a.n_words - 1u);
      if (j) p = a.parent[j][p];
    }
  }
}

__device__ __forceinline__ uint32_t gm_digits(uint32_t c) {
  return c < 10u ? 1u : c < 100u ? 2u : c < 1000u ? 3u : c < 10000u ? 4u : c < 100000u ? 5u : c < 1000000u ? 6u : c < 10000000u ? 7u : c < 100000000u ? 8u : c < 1000000000u ? 9u : 10u;
}

__global__ void lm_gm_size(const GmArgs a) {
  const uint64_t e = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (e > a.n[a.k]) return;
  if (e == a.n[a.k]) { a.len[e] = 0; return; }
  uint32_t ids[8];
  gm_chain(a, (uint32_t)e, ids);
  uint64_t bytes = a.k + 2u + gm_digits(a.count[a.k][e]);
#pragma unroll
  for (int j = 0; j < 8; j++) if ((uint32_t)j <= a.k) bytes += a.woff[ids[j] + 1] - a.woff[ids[j]];
  a.len[e] = bytes;
}

// the line of entry e, byte after byte into put(position, byte)
template <class Put>
__device__ __forceinline__ void gm_format(const GmArgs& a, uint32_t e, uint64_t at, Put put) {
  uint32_t ids[8];
  gm_chain(a, e, ids);
#pragma unroll
  for (int j = 0; j < 8; j++) {
    if ((uint32_t)j <= a.k) {
      const uint32_t from = a.woff[ids[j]], to = a.woff[ids[j] + 1];
      for (uint32_t i = from; i < to; i++) put(at++, a.wbytes[i]);
      put(at++, (uint32_t)j < a.k ? (uint32_t)' ' : (uint32_t)'\t');
    }
  }
  const uint32_t c = a.count[a.k][e];
  uint32_t pw = 1;
  while (c / pw >= 10u) pw *= 10u;
  for (; pw; pw /= 10u) put(at++, (uint32_t)'0' + (c / pw) % 10u);
  put(at, (uint32_t)'\n');
}

// A thread per line, a wavefront per 64 consecutive lines.  Byte stores only: neighbouring lines share dwords, and no lane reads
// or rewrites a byte of another's.
__global__ __launch_bounds__(64) void lm_gm_write(const GmArgs a) {
  const uint64_t e = (uint64_t)a.e0 + (uint64_t)blockIdx.x * 64u + threadIdx.x;
  if (e >= a.e1) return;
  const uint64_t base = a.off[a.e0], end = min(a.off[e + 1] - base, a.out_bytes);
  gm_format(a, (uint32_t)e, a.off[e] - base, [&](uint64_t at, uint32_t b) { if (at < end) a.out[at] = (uint8_t)b; });
}

}  // namespace sg

namespace {

thread_local double t_lm_store_seconds[4];                // the calling thread's last sg_lm_store_google: staging, kernels, copy-back, file writes

int lm_store_google_device(const HostLM& lm, const char* out_dir, int device, double seconds[4]) {
  std::string err;
  int rc;
  if ((rc = lm_gm_check(lm, err))) { set_error(err); return rc; }
  const size_t order = lm.level.size();
  DeviceGuard dg;
  HIP_TRY(dg.set(device));
  StoreStream ss;
  HIP_TRY(hipStreamCreateWithFlags(&ss.s, hipStreamNonBlocking));
  const hipStream_t st = ss.s;

  const auto t_stage = clk::now();
  GmArgs a{};
  DeviceBlock mem;
  std::vector<uint8_t> wbytes;
  std::vector<uint32_t> woff(lm.words.size() + 1, 0);
  for (size_t i = 0; i < lm.words.size(); i++) woff[i + 1] = woff[i] + (uint32_t)lm.words[i].size();
  wbytes.reserve(woff.back());
  for (const auto& w : lm.words) wbytes.insert(wbytes.end(), w.begin(), w.end());
  a.n_words = (uint32_t)lm.words.size();
  if ((rc = mem.upload(wbytes, &a.wbytes, st)) || (rc = mem.upload(woff, &a.woff, st))) return rc;
  size_t n_max = 0;
  for (size_t k = 0; k < order; k++) {
    const LmLevel& lv = lm.level[k];
    a.n[k] = (uint32_t)lv.word.size();
    n_max = std::max(n_max, lv.word.size());
    if ((rc = mem.upload(lv.word, &a.word[k], st)) || (rc = mem.upload(lv.count, &a.count[k], st)) ||
        (rc = mem.upload(lv.child_begin, &a.cbeg[k], st)) || (rc = mem.alloc(&a.parent[k], lv.word.size())))
      return rc;
  }
  if ((rc = mem.alloc(&a.len, n_max + 1)) || (rc = mem.alloc(&a.off, n_max + 1))) return rc;
  size_t scan_bytes = 0;
  HIP_TRY(hipcub::DeviceScan::ExclusiveSum(nullptr, scan_bytes, a.len, a.off, (int)(n_max + 1), st));
  uint8_t* scan_tmp;
  if ((rc = mem.alloc(&scan_tmp, scan_bytes))) return rc;
  HIP_TRY(hipStreamSynchronize(st));
  seconds[0] = since(t_stage);

  const uint64_t budget = lm_gm_slice_budget(-1);
  uint8_t* d_out = nullptr;                                 // grows to the largest slice met; freed with the call
  uint64_t d_out_cap = 0;
  std::vector<uint64_t> off;
  std::vector<uint8_t> text;
  for (size_t k = 0; k < order; k++) {
    const uint32_t n = a.n[k];
    a.k = (uint32_t)k;
    GmFile file;
    if ((rc = file.open(lm_gm_path(out_dir, k + 1), err))) { set_error(err); return rc; }
    uint64_t total = 0;
    if (n) {
      const auto t_k = clk::now();
      if (k) { hipLaunchKernelGGL(lm_gm_parent, dim3((n + 255u) / 256u), dim3(256), 0, st, a); HIP_TRY(hipGetLastError()); }
      hipLaunchKernelGGL(lm_gm_size, dim3(n / 256u + 1u), dim3(256), 0, st, a);
      HIP_TRY(hipGetLastError());
      HIP_TRY(hipcub::DeviceScan::ExclusiveSum(scan_tmp, scan_bytes, a.len, a.off, (int)(n + 1u), st));
      HIP_TRY(hipMemcpyAsync(&total, a.off + n, 8, hipMemcpyDeviceToHost, st));
      HIP_TRY(hipStreamSynchronize(st));
      seconds[1] += since(t_k);
    }
    if (total > budget) {                                   // more than one slice: their bounds come from the offsets
      const auto t_b = clk::now();
      off.resize((size_t)n + 1);
      HIP_TRY(hipMemcpyAsync(off.data(), a.off, ((size_t)n + 1) * 8, hipMemcpyDeviceToHost, st));
      HIP_TRY(hipStreamSynchronize(st));
      seconds[2] += since(t_b);
    }
    for (uint32_t e0 = 0; e0 < n;) {
      uint32_t e1 = n;
      uint64_t bytes = total;
      if (total > budget) {                                 // the entries whose text fits the budget, one at least
        e1 = (uint32_t)(std::upper_bound(off.begin() + e0, off.end(), off[e0] + budget) - off.begin()) - 1u;
        e1 = std::min(std::max(e1, e0 + 1u), n);
        bytes = off[e1] - off[e0];
      }
      if (bytes > d_out_cap) {
        if ((rc = mem.alloc(&d_out, (size_t)bytes))) return rc;
        d_out_cap = bytes;
      }
      a.e0 = e0; a.e1 = e1; a.out = d_out; a.out_bytes = bytes;
      const auto t_w = clk::now();
      hipLaunchKernelGGL(lm_gm_write, dim3((e1 - e0 + 63u) / 64u), dim3(64), 0, st, a);
      HIP_TRY(hipGetLastError());
      HIP_TRY(hipStreamSynchronize(st));
      seconds[1] += since(t_w);
      const auto t_b = clk::now();
      text.resize((size_t)bytes);
      if (bytes) HIP_TRY(hipMemcpyAsync(text.data(), d_out, (size_t)bytes, hipMemcpyDeviceToHost, st));
      HIP_TRY(hipStreamSynchronize(st));
      seconds[2] += since(t_b);
      const auto t_f = clk::now();
      if ((rc = file.write(text.data(), text.size(), err))) { set_error(err); return rc; }
      seconds[3] += since(t_f);
      e0 = e1;
    }
    const auto t_f = clk::now();
    if ((rc = file.close(err))) { set_error(err); return rc; }
    seconds[3] += since(t_f);
  }
  return SG_OK;
}

}  // namespace

extern "C" {

int sg_lm_store_google(const sg_lm* lm, const char* out_dir, int device) {
  SG_GUARD_BEGIN
  if (!lm || !out_dir) { set_error("null argument"); return SG_E_INVALID; }
  double* t = t_lm_store_seconds;
  t[0] = t[1] = t[2] = t[3] = 0;
  if (device >= 0) return lm_store_google_device(lm->host, out_dir, device, t);
  std::string err;
  const int rc = lm_store_google_host(lm->host, out_dir, t, err);
  if (rc) set_error(err);
  return rc;
  SG_GUARD_END(SG_RC)
}

int sg_debug_lm_store_slice_bytes(uint32_t bytes) {
  lm_gm_slice_budget((int64_t)bytes);
  return SG_OK;
}

int sg_debug_lm_store_times(double out[4]) {
  if (!out) { set_error("null argument"); return SG_E_INVALID; }
  for (int i = 0; i < 4; i++) out[i] = t_lm_store_seconds[i];
  return SG_OK;
}

}  // extern "C"
