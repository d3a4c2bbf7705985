// index_store.inc — the device encoder behind sg_index_store_reference, included by engine.hip after the host files (it uses the
// handle, HIP_TRY, DeviceGuard and DeviceBlock).  Replaces the single-threaded walk of Writer.Commit + index.NewEncoder
// (pkg/index/indexer_writer.go:88-167, pkg/index/codec.go:17-51) over the posting lists of a built index; the formats and
// the host encoder the kernels are read against are in index_store.cpp.
//
// Two passes with a prefix sum between them, no atomic allocation: bytes and positions never depend on scheduling.
//   size      sg_store_small_size   a wavefront per VB / skip list (raw <= 256): the raw list expanded in LDS from the stored list
//                                   and its slice of the repeats table, varint widths per lane, summed over blocks of 64
//             sg_store_roar_find    a wavefront per roaring list: a lane per high-16 key, container bounds by binary search,
//                                   compacted in key order into the list's container slots (__ballot rank)
//             sg_store_roar_runs    a wavefront per (list, container): cardinality, runs (compare with the neighbour, __ballot)
//             sg_store_roar_layout  a wavefront per roaring list: header size, container offsets (wave scan), list size
//   position  the sizes are copied back and scanned on the HOST in header order (one pass over n_lists words; the 4 GiB check
//             needs the 64-bit total anyway), the positions copied to the device
//   write     sg_store_small_write  a wavefront per block of 64 values of a VB / skip list: lane i holds delta i, a wave prefix
//                                   sum of the widths gives its byte offset, lane 0 the skip header
//             sg_store_roar_head    a wavefront per roaring list: cookie, run flags, (key, cardinality - 1), offsets
//             sg_store_roar_body    a wavefront per (list, container): arrays are a u16 copy, bitmaps are built in 8 KB of LDS
//                                   with atomicOr, runs are a compaction of run starts and ends
// Output goes out with BYTE stores only: adjacent lists share dwords and other wavefronts write them.  Everything is staged
// from the handle's host CSR into memory of this call, on a stream of its own, and freed before it returns: no replica,
// scratch block or knob of the search path is read or changed.

namespace sg {

struct StoreArgs {
  const uint32_t* post;                                   // the host CSR's posting array
  const uint64_t* l_src;                                  // [n_lists] per list in header order: first posting,
  const uint32_t *l_len, *l_raw, *l_dbeg, *l_dn;          //   stored length, raw length, its slice of d_doc / d_mult
  const uint32_t *d_doc, *d_mult;                         // the repeats table (doc, multiplicity), marker entries left out
  uint32_t n_lists;
  uint32_t* l_size;                                       // [n_lists] out of the size pass
  const uint32_t* l_pos;                                  // [n_lists] in to the write pass
  const uint32_t* items; uint32_t n_items;                // VB / skip work items: list | block << 30
  const uint32_t *r_list, *r_cbase; uint32_t n_r;         // roaring lists: list index, first container slot ([n_r + 1])
  uint32_t *r_ncont, *r_anyrun;                           // [n_r] containers found, 1 if one of them is a run container
  uint32_t *c_ri, *c_key, *c_beg, *c_card, *c_runs, *c_size, *c_off;   // [n_slots] per container slot (c_ri = 0xFFFFFFFF: unused)
  uint32_t n_slots;
  uint8_t* out; uint64_t out_bytes;
};

struct StoreLds { uint32_t s[256], m[256], e[256]; };     // stored values, multiplicities, the raw list

__device__ __forceinline__ uint32_t st_scan(uint32_t v, uint32_t lane) {   // inclusive prefix sum over the wavefront
  for (uint32_t d = 1; d < 64; d <<= 1) { const uint32_t o = __shfl_up(v, d, 64); if (lane >= d) v += o; }
  return v;
}
__device__ __forceinline__ uint32_t st_varint_len(uint32_t v) { return v < (1u << 7) ? 1u : v < (1u << 14) ? 2u : v < (1u << 21) ? 3u : v < (1u << 28) ? 4u : 5u; }
__device__ __forceinline__ void st_put(const StoreArgs& a, uint64_t at, uint32_t byte) { if (at < a.out_bytes) a.out[at] = (uint8_t)byte; }
__device__ __forceinline__ void st_put16(const StoreArgs& a, uint64_t at, uint32_t v) { st_put(a, at, v); st_put(a, at + 1, v >> 8); }
__device__ __forceinline__ void st_put32(const StoreArgs& a, uint64_t at, uint32_t v) { st_put16(a, at, v); st_put16(a, at + 2, v >> 16); }
// roaring's RunOptimize: a run container when it is no larger than the array or bitmap (ties go to the run)
__device__ __forceinline__ bool st_is_run(uint32_t card, uint32_t runs) { return 2u + 4u * runs <= min(8192u, 2u * card); }
__device__ __forceinline__ uint32_t st_body_size(uint32_t card, uint32_t runs) { return st_is_run(card, runs) ? 2u + 4u * runs : card <= 4096u ? 2u * card : 8192u; }
__device__ __forceinline__ uint32_t st_lower_bound(const uint32_t* p, uint32_t n, uint32_t x) {
  uint32_t lo = 0, hi = n;
  while (lo < hi) { const uint32_t mid = lo + ((hi - lo) >> 1); if (p[mid] < x) lo = mid + 1; else hi = mid; }
  return lo;
}

// One wavefront: the raw list of list l (at most 256 entries) into w.e; returns its length.
__device__ uint32_t st_expand(const StoreArgs& a, uint32_t l, StoreLds& w) {
  const uint32_t lane = threadIdx.x;
  const uint32_t len = min(a.l_len[l], 256u);
  const uint32_t* p = a.post + a.l_src[l];
  for (uint32_t j = lane; j < len; j += 64) { w.s[j] = p[j]; w.m[j] = 1u; }
  __syncthreads();
  const uint32_t nd = min(a.l_dn[l], len), db = a.l_dbeg[l];
  for (uint32_t d = lane; d < nd; d += 64) {                // a repeated document: found in the stored list, its multiplicity set
    const uint32_t doc = a.d_doc[db + d];
    const uint32_t at = st_lower_bound(w.s, len, doc);
    if (at < len && w.s[at] == doc) w.m[at] = max(a.d_mult[db + d], 1u);
  }
  __syncthreads();
  uint32_t run = 0;
  for (uint32_t base = 0; base < len; base += 64) {
    const uint32_t j = base + lane;
    const uint32_t mj = j < len ? w.m[j] : 0u, v = j < len ? w.s[j] : 0u;
    const uint32_t inc = st_scan(mj, lane);
    const uint32_t first = min(run + (inc - mj), 256u);
    for (uint32_t r = 0; r < mj && first + r < 256u; r++) w.e[first + r] = v;
    run = min(run + __shfl(inc, 63, 64), 256u);
  }
  __syncthreads();
  return run;
}

// delta i of a raw list: to its predecessor; in a skip list a block's first value is a delta to the previous block's first
__device__ __forceinline__ uint32_t st_delta(const StoreLds& w, uint32_t i, bool skip) {
  if (i == 0) return w.e[0];
  return w.e[i] - w.e[skip && (i & 63u) == 0 ? i - 64 : i - 1];
}

// A workgroup is one wavefront and every condition of an early return below (the list, its raw length, the block number) is
// the same in all of its lanes: no lane waits at a __syncthreads that another has left behind.
__global__ __launch_bounds__(64) void sg_store_small_size(const StoreArgs a) {
  __shared__ StoreLds w;
  const uint32_t l = blockIdx.x, lane = threadIdx.x;
  if (l >= a.n_lists || a.l_raw[l] > 256u) return;
  const bool skip = a.l_raw[l] > 65u;
  const uint32_t raw = st_expand(a, l, w);
  uint32_t total = 0;
  for (uint32_t base = 0; base < raw; base += 64) {
    const uint32_t i = base + lane;
    const uint32_t wd = i < raw ? st_varint_len(st_delta(w, i, skip)) : 0u;
    total += __shfl(st_scan(wd, lane), 63, 64) + (skip ? 2u : 0u);
  }
  if (lane == 0) a.l_size[l] = total;
}

__global__ __launch_bounds__(64) void sg_store_small_write(const StoreArgs a) {
  __shared__ StoreLds w;
  const uint32_t lane = threadIdx.x;
  if (blockIdx.x >= a.n_items) return;
  const uint32_t item = a.items[blockIdx.x], l = item & 0x3FFFFFFFu, blk = item >> 30;
  if (l >= a.n_lists || a.l_raw[l] > 256u) return;
  const bool skip = a.l_raw[l] > 65u;
  const uint32_t raw = st_expand(a, l, w);
  if (blk * 64u >= raw) return;
  uint64_t at = a.l_pos[l];
  for (uint32_t b = 0; b < blk; b++) {                      // the bytes of the blocks before this one
    const uint32_t i = b * 64u + lane;
    const uint32_t wd = i < raw ? st_varint_len(st_delta(w, i, skip)) : 0u;
    at += __shfl(st_scan(wd, lane), 63, 64) + (skip ? 2u : 0u);
  }
  const uint32_t i = blk * 64u + lane;
  uint32_t delta = i < raw ? st_delta(w, i, skip) : 0u;
  const uint32_t wd = i < raw ? st_varint_len(delta) : 0u;
  const uint32_t inc = st_scan(wd, lane), total = __shfl(inc, 63, 64);
  if (skip) {                                               // u16: the block's bytes with these two, bit 15 on the last block
    if (lane == 0) st_put16(a, at, (total + 2u) | ((blk + 1u) * 64u >= raw ? 0x8000u : 0u));
    at += 2;
  }
  if (i < raw) {
    uint64_t o = at + (inc - wd);
    while (delta >= 0x80u) { st_put(a, o++, delta | 0x80u); delta >>= 7; }
    st_put(a, o, delta);
  }
}

__global__ __launch_bounds__(64) void sg_store_roar_find(const StoreArgs a) {
  const uint32_t ri = blockIdx.x, lane = threadIdx.x;
  if (ri >= a.n_r) return;
  const uint32_t l = a.r_list[ri];
  if (l >= a.n_lists) return;
  const uint32_t len = a.l_len[l], cbase = a.r_cbase[ri], cend = min(a.r_cbase[ri + 1], a.n_slots);
  if (len == 0) { if (lane == 0) a.r_ncont[ri] = 0; return; }
  const uint32_t* p = a.post + a.l_src[l];
  const uint32_t k0 = p[0] >> 16, k1 = p[len - 1] >> 16;
  uint32_t count = 0;
  for (uint32_t kb = k0; kb <= k1; kb += 64) {
    const uint32_t k = kb + lane;
    uint32_t lo = 0, hi = 0;
    if (k <= k1) {
      lo = st_lower_bound(p, len, k << 16);
      hi = k >= 0xFFFFu ? len : st_lower_bound(p, len, (k + 1u) << 16);
    }
    const bool live = hi > lo;
    const unsigned long long mask = __ballot(live);
    const uint32_t slot = cbase + count + (uint32_t)__popcll(mask & ((1ull << lane) - 1ull));
    if (live && slot < cend) { a.c_ri[slot] = ri; a.c_key[slot] = k; a.c_beg[slot] = lo; a.c_card[slot] = hi - lo; }
    count += (uint32_t)__popcll(mask);
  }
  if (lane == 0) a.r_ncont[ri] = min(count, cend > cbase ? cend - cbase : 0u);
}

__global__ __launch_bounds__(64) void sg_store_roar_runs(const StoreArgs a) {
  const uint32_t s = blockIdx.x, lane = threadIdx.x;
  if (s >= a.n_slots) return;
  const uint32_t ri = a.c_ri[s];
  if (ri >= a.n_r) return;                                  // a slot the list did not need
  const uint32_t l = a.r_list[ri], card = a.c_card[s];
  const uint32_t* p = a.post + a.l_src[l] + a.c_beg[s];
  uint32_t runs = 0;
  for (uint32_t base = 0; base < card; base += 64) {
    const uint32_t i = base + lane;
    const bool start = i < card && (i == 0 || p[i] != p[i - 1] + 1u);
    runs += (uint32_t)__popcll(__ballot(start));
  }
  if (lane == 0) { a.c_runs[s] = runs; a.c_size[s] = st_body_size(card, runs); }
}

__global__ __launch_bounds__(64) void sg_store_roar_layout(const StoreArgs a) {
  const uint32_t ri = blockIdx.x, lane = threadIdx.x;
  if (ri >= a.n_r) return;
  const uint32_t l = a.r_list[ri], n = a.r_ncont[ri], cbase = a.r_cbase[ri];
  if (l >= a.n_lists) return;
  bool any = false;
  for (uint32_t base = 0; base < n; base += 64) {
    const uint32_t j = base + lane;
    any |= __ballot(j < n && st_is_run(a.c_card[cbase + j], a.c_runs[cbase + j])) != 0ull;
  }
  uint32_t run = any ? 4u + (n + 7u) / 8u + 4u * n + (n >= 4u ? 4u * n : 0u) : 8u + 8u * n;
  for (uint32_t base = 0; base < n; base += 64) {
    const uint32_t j = base + lane;
    const uint32_t sz = j < n ? a.c_size[cbase + j] : 0u;
    const uint32_t inc = st_scan(sz, lane);
    if (j < n) a.c_off[cbase + j] = run + (inc - sz);
    run += __shfl(inc, 63, 64);
  }
  if (lane == 0) { a.l_size[l] = run; a.r_anyrun[ri] = any ? 1u : 0u; }
}

__global__ __launch_bounds__(64) void sg_store_roar_head(const StoreArgs a) {
  const uint32_t ri = blockIdx.x, lane = threadIdx.x;
  if (ri >= a.n_r) return;
  const uint32_t l = a.r_list[ri], n = a.r_ncont[ri], cbase = a.r_cbase[ri];
  if (l >= a.n_lists || n == 0) return;
  const bool any = a.r_anyrun[ri] != 0u;
  uint64_t o = a.l_pos[l];
  if (lane == 0) st_put32(a, o, any ? 12347u | ((n - 1u) << 16) : 12346u);
  if (any) {
    const uint32_t nb = (n + 7u) / 8u;
    for (uint32_t b = lane; b < nb; b += 64) {
      uint32_t f = 0;
      for (uint32_t k = 0; k < 8u && 8u * b + k < n; k++) f |= (st_is_run(a.c_card[cbase + 8u * b + k], a.c_runs[cbase + 8u * b + k]) ? 1u : 0u) << k;
      st_put(a, o + 4 + b, f);
    }
    o += 4 + nb;
  } else {
    if (lane == 0) st_put32(a, o + 4, n);
    o += 8;
  }
  for (uint32_t j = lane; j < n; j += 64) { st_put16(a, o + 4ull * j, a.c_key[cbase + j]); st_put16(a, o + 4ull * j + 2, a.c_card[cbase + j] - 1u); }
  o += 4ull * n;
  if (!any || n >= 4u)
    for (uint32_t j = lane; j < n; j += 64) st_put32(a, o + 4ull * j, a.c_off[cbase + j]);
}

__global__ __launch_bounds__(64) void sg_store_roar_body(const StoreArgs a) {
  __shared__ uint32_t lds[2048];                            // a bitmap container's 8 KB; or the starts and ends of up to 2 047 runs
  const uint32_t s = blockIdx.x, lane = threadIdx.x;
  if (s >= a.n_slots) return;
  const uint32_t ri = a.c_ri[s];
  if (ri >= a.n_r) return;
  const uint32_t l = a.r_list[ri], card = a.c_card[s], runs = a.c_runs[s];
  const uint32_t* p = a.post + a.l_src[l] + a.c_beg[s];
  const uint64_t at = (uint64_t)a.l_pos[l] + a.c_off[s];
  if (st_is_run(card, runs)) {
    uint16_t* rs = (uint16_t*)lds;
    uint16_t* re = rs + 2048;
    uint32_t before = 0;
    for (uint32_t base = 0; base < card; base += 64) {
      const uint32_t i = base + lane;
      const bool in = i < card;
      const uint32_t v = in ? p[i] : 0u;
      const bool start = in && (i == 0 || v != p[i - 1] + 1u);
      const bool end = in && (i + 1u == card || p[i + 1] != v + 1u);
      const unsigned long long m = __ballot(start);
      const uint32_t r = before + (uint32_t)__popcll(m & ((2ull << lane) - 1ull)) - 1u;   // the run this value lies in
      if (start && r < 2048u) rs[r] = (uint16_t)v;
      if (end && r < 2048u) re[r] = (uint16_t)v;
      before += (uint32_t)__popcll(m);
    }
    __syncthreads();
    if (lane == 0) st_put16(a, at, runs);
    for (uint32_t r = lane; r < min(runs, 2048u); r += 64) { st_put16(a, at + 2 + 4ull * r, rs[r]); st_put16(a, at + 4 + 4ull * r, (uint32_t)(re[r] - rs[r]) & 0xFFFFu); }
  } else if (card <= 4096u) {
    for (uint32_t i = lane; i < card; i += 64) st_put16(a, at + 2ull * i, p[i] & 0xFFFFu);
  } else {
    for (uint32_t j = lane; j < 2048u; j += 64) lds[j] = 0u;
    __syncthreads();
    for (uint32_t i = lane; i < card; i += 64) { const uint32_t x = p[i] & 0xFFFFu; atomicOr(&lds[x >> 5], 1u << (x & 31u)); }
    __syncthreads();
    for (uint32_t b = lane; b < 8192u; b += 64) st_put(a, at + b, (lds[b >> 2] >> (8u * (b & 3u))) & 0xFFu);
  }
}

}  // namespace sg

namespace {

thread_local double t_store_seconds[4];                   // the calling thread's last sg_index_store_reference: encode, staging, header, all

struct StoreStream {                                      // the call's own stream
  hipStream_t s = nullptr;
  ~StoreStream() { if (s) (void)hipStreamDestroy(s); }
};

// The lists of `h` encoded on `device`: size[] and pos[] per list in header order, the bytes of the .dl in `dl`.
int store_encode_device(const HostIndex& h, const std::vector<StoreList>& lists, int device, std::vector<uint32_t>& size,
                        std::vector<uint32_t>& pos, uint64_t* total, std::vector<uint8_t>& dl, double seconds[2]) {
  const size_t n = lists.size();
  if (n >= (1u << 30)) { set_error("2^30 posting lists or more: beyond the device encoder, store with device < 0"); return SG_E_UNSUPPORTED; }
  DeviceGuard dg;
  HIP_TRY(dg.set(device));
  StoreStream ss;
  HIP_TRY(hipStreamCreateWithFlags(&ss.s, hipStreamNonBlocking));
  const hipStream_t st = ss.s;

  // what the kernels read, from the host CSR (counted as staging)
  const auto t_stage = clk::now();
  std::vector<uint64_t> l_src(n);
  std::vector<uint32_t> l_len(n), l_raw(n), l_dbeg(n), l_dn(n), d_doc, d_mult, items, r_list, r_cbase;
  d_doc.reserve(h.dups.size()); d_mult.reserve(h.dups.size());
  uint64_t n_slots = 0;
  for (size_t i = 0; i < n; i++) {
    const StoreList& l = lists[i];
    l_src[i] = l.src; l_len[i] = l.len; l_raw[i] = l.raw; l_dbeg[i] = (uint32_t)d_doc.size(); l_dn[i] = l.dup_n;
    for (uint32_t d = 0; d < l.dup_n; d++) { d_doc.push_back(h.dups[l.dup_begin + d].doc); d_mult.push_back(h.dups[l.dup_begin + d].mult); }
    if (l.raw <= 256u) {
      for (uint32_t b = 0; b * 64u < l.raw; b++) items.push_back((uint32_t)i | (b << 30));
    } else {                                                // container slots: no more than its postings or the keys it spans
      const uint32_t first = h.postings[l.src] >> 16, last = h.postings[l.src + l.len - 1] >> 16;
      r_list.push_back((uint32_t)i);
      r_cbase.push_back((uint32_t)n_slots);
      n_slots += std::min<uint64_t>(l.len, (uint64_t)last - first + 1);
      if (n_slots >= 0xFFFFFFF0ull) { set_error("too many roaring containers for the device encoder, store with device < 0"); return SG_E_UNSUPPORTED; }
    }
  }
  r_cbase.push_back((uint32_t)n_slots);
  if (items.size() >= 0x7FFFFFFFull) { set_error("too many blocks for the device encoder, store with device < 0"); return SG_E_UNSUPPORTED; }

  DeviceBlock mem;
  StoreArgs a{};
  int rc;
  a.n_lists = (uint32_t)n; a.n_items = (uint32_t)items.size(); a.n_r = (uint32_t)r_list.size(); a.n_slots = (uint32_t)n_slots;
  uint32_t* d_pos;
  if ((rc = mem.upload(h.postings, &a.post, st)) || (rc = mem.upload(l_src, &a.l_src, st)) || (rc = mem.upload(l_len, &a.l_len, st)) ||
      (rc = mem.upload(l_raw, &a.l_raw, st)) || (rc = mem.upload(l_dbeg, &a.l_dbeg, st)) || (rc = mem.upload(l_dn, &a.l_dn, st)) ||
      (rc = mem.upload(d_doc, &a.d_doc, st)) || (rc = mem.upload(d_mult, &a.d_mult, st)) || (rc = mem.upload(items, &a.items, st)) ||
      (rc = mem.upload(r_list, &a.r_list, st)) || (rc = mem.upload(r_cbase, &a.r_cbase, st)) ||
      (rc = mem.alloc(&a.l_size, n)) || (rc = mem.alloc(&d_pos, n)) || (rc = mem.alloc(&a.r_ncont, (size_t)a.n_r)) || (rc = mem.alloc(&a.r_anyrun, (size_t)a.n_r)))
    return rc;
  a.l_pos = d_pos;
  for (uint32_t** c : {&a.c_ri, &a.c_key, &a.c_beg, &a.c_card, &a.c_runs, &a.c_size, &a.c_off})
    if ((rc = mem.alloc(c, (size_t)n_slots))) return rc;
  if (n_slots) HIP_TRY(hipMemsetAsync(a.c_ri, 0xFF, (size_t)n_slots * 4, st));
  HIP_TRY(hipStreamSynchronize(st));
  seconds[1] = since(t_stage);

  const auto t_size = clk::now();
  hipLaunchKernelGGL(sg_store_small_size, dim3((unsigned)n), dim3(64), 0, st, a);
  HIP_TRY(hipGetLastError());
  if (a.n_r) {
    hipLaunchKernelGGL(sg_store_roar_find, dim3(a.n_r), dim3(64), 0, st, a);
    HIP_TRY(hipGetLastError());
    if (a.n_slots) { hipLaunchKernelGGL(sg_store_roar_runs, dim3(a.n_slots), dim3(64), 0, st, a); HIP_TRY(hipGetLastError()); }
    hipLaunchKernelGGL(sg_store_roar_layout, dim3(a.n_r), dim3(64), 0, st, a);
    HIP_TRY(hipGetLastError());
  }
  size.resize(n);
  HIP_TRY(hipMemcpyAsync(size.data(), a.l_size, n * 4, hipMemcpyDeviceToHost, st));
  HIP_TRY(hipStreamSynchronize(st));
  {
    std::string err;
    if ((rc = store_positions(size, pos, total, err))) { set_error(err); return rc; }
  }
  HIP_TRY(hipMemcpyAsync(d_pos, pos.data(), n * 4, hipMemcpyHostToDevice, st));
  if ((rc = mem.alloc(&a.out, (size_t)*total))) return rc;
  a.out_bytes = *total;
  if (a.n_items) { hipLaunchKernelGGL(sg_store_small_write, dim3(a.n_items), dim3(64), 0, st, a); HIP_TRY(hipGetLastError()); }
  if (a.n_r) {
    hipLaunchKernelGGL(sg_store_roar_head, dim3(a.n_r), dim3(64), 0, st, a);
    HIP_TRY(hipGetLastError());
    if (a.n_slots) { hipLaunchKernelGGL(sg_store_roar_body, dim3(a.n_slots), dim3(64), 0, st, a); HIP_TRY(hipGetLastError()); }
  }
  HIP_TRY(hipStreamSynchronize(st));
  seconds[0] = since(t_size);

  const auto t_back = clk::now();
  dl.resize((size_t)*total);
  if (*total) HIP_TRY(hipMemcpyAsync(dl.data(), a.out, (size_t)*total, hipMemcpyDeviceToHost, st));
  HIP_TRY(hipStreamSynchronize(st));
  seconds[1] += since(t_back);
  return SG_OK;
}

}  // namespace

extern "C" {

int sg_index_store_reference(sg_index* ix, const char* hd_path, const char* dl_path, int device) {
  SG_GUARD_BEGIN
  if (!ix || !hd_path || !dl_path) { set_error("null argument"); return SG_E_INVALID; }
  const auto t0 = clk::now();
  const HostIndex& h = ix->host;
  std::string err;
  std::vector<StoreList> lists;
  std::vector<uint32_t> size, pos;
  std::vector<uint8_t> dl;
  uint64_t total = 0;
  double* t = t_store_seconds;
  t[0] = t[1] = t[2] = t[3] = 0;
  int rc = store_lists(h, lists, err);
  if (rc) { set_error(err); return rc; }
  if (device >= 0 && !lists.empty()) {
    if ((rc = store_encode_device(h, lists, device, size, pos, &total, dl, t))) return rc;
  } else {
    const auto t_enc = clk::now();                         // (behind the list table, like the device path's clock)
    store_encode_host(h, lists, size, dl);
    if ((rc = store_positions(size, pos, &total, err))) { set_error(err); return rc; }
    t[0] = since(t_enc);
  }
  if ((rc = store_write_files(h, lists, size, pos, dl.data(), total, hd_path, dl_path, &t[2], err))) { set_error(err); return rc; }
  t[3] = since(t0);
  return SG_OK;
  SG_GUARD_END(SG_RC)
}

int sg_debug_index_store_times(double out[4]) {
  if (!out) { set_error("null argument"); return SG_E_INVALID; }
  for (int i = 0; i < 4; i++) out[i] = t_store_seconds[i];
  return SG_OK;
}

int sg_dictionary_store_cdb(const uint8_t* utf8, const uint64_t* offs, uint32_t n_docs, const char* cdb_path) {
  SG_GUARD_BEGIN
  if (!offs || !cdb_path || (!utf8 && n_docs && offs[n_docs] > offs[0])) { set_error("null argument"); return SG_E_INVALID; }
  for (uint32_t i = 0; i < n_docs; i++)
    if (offs[i + 1] < offs[i]) { set_error("document offsets must not decrease"); return SG_E_INVALID; }
  std::string err;
  const int rc = cdb_write_dictionary(cdb_path, n_docs, [&](size_t i, size_t* len) {
    *len = (size_t)(offs[i + 1] - offs[i]);
    return (const char*)utf8 + offs[i];
  }, err);
  if (rc) set_error(err);
  return rc;
  SG_GUARD_END(SG_RC)
}

}  // extern "C"
