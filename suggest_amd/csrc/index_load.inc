// index_load.inc — the device decoder behind sg_index_load_reference_ex, included by engine.hip after index_store.inc (it uses
// HIP_TRY, DeviceGuard, DeviceBlock, StoreStream and st_scan).  The reverse of index_store.inc: the VB / skip-VB / roaring
// posting lists of a reference-built <name>.dl become the host CSR's posting store.  Steps 1 and 3 of a load and the host
// decoders the kernels are read against are in ref_index_reader.cpp.
//
// Two passes with a host scan between them, no atomic allocation: positions never depend on scheduling.
//   count     sg_load_small_count   a wavefront per VB / skip list (raw <= 256): the bytes staged in LDS, a byte < 0x80 ends a
//                                   varint (__ballot ranks the values, the terminator's lane assembles its value), docIDs by a
//                                   wave prefix sum per block, repeats by comparing with the neighbour
//             sg_load_roar_head     a wavefront per roaring list: cookie, run flags, (key, cardinality - 1), the container starts
//                                   by walking the sizes (the file's offset header is skipped, never trusted)
//             sg_load_roar_count    a wavefront per (list, container): values, first and last, strictly ascending or not
//             sg_load_roar_sum      a wavefront per roaring list: each container's first output slot (wave scan), the list's words
//   position  the per-list words {status, stored, repeats, last value} are copied back; the HOST computes list_len, seg_off, the
//             repeat-table offsets and n_docs (ref_layout), and the chunk and repeat offsets go to the device
//   write     sg_load_small_write   a wavefront per VB / skip list: decoded again the same way, the de-duplicated docIDs to its
//                                   chunks, the last chunk padded, the {doc, multiplicity} entries to its repeat slots
//             sg_load_roar_write    a wavefront per (list, container): arrays are a widening copy, bitmaps go by popcount ranks,
//                                   run containers through a prefix sum of run lengths; the list's last container pads
// Every index derived from file bytes is compared with the list's end before it is used, the write pass writes no more than
// the count pass counted, and a malformed list only sets its status word.  A roaring list whose values do not strictly ascend
// (no writer emits one: the neighbour de-duplication would cross containers) has status LD_HOST and is decoded by the host's
// decoder into its slot.  Everything is memory of the call on a stream of its own, freed before return.

namespace sg {

enum : uint32_t { LD_OK = 0, LD_BAD = 1, LD_HOST = 2 };
enum : uint32_t { LD_ARRAY = 0, LD_BITMAP = 1, LD_RUN = 2 };
constexpr uint32_t kLoadLdsBytes = 2048;                  // a VB list is at most 325 bytes, a skip list of blocks of 64 about 1.3 KB

struct LoadInfo { uint32_t status, stored, ndup, last; };  // per list, out of the count pass

struct LoadArgs {
  const uint8_t* dl; uint64_t dl_bytes;                   // the .dl, zero bytes behind its end (dl_bytes: the file's)
  const uint64_t* l_pos; const uint32_t *l_size, *l_raw;  // [n_lists] per list in header order
  uint32_t n_lists;
  LoadInfo* info;                                         // [n_lists]
  const uint32_t *r_list, *r_cbase; uint32_t n_r;         // roaring lists: list index, first container slot ([n_r + 1])
  uint32_t* r_status;                                     // [n_r] out of sg_load_roar_head
  uint32_t *c_ri, *c_key, *c_kind, *c_n, *c_start;        // [n_slots] per container: its list, key, LD_*, cardinality or runs, first byte in the list
  uint32_t *c_count, *c_last, *c_flag, *c_out;            // [n_slots] values, last value, 1 = not strictly ascending, first output slot
  uint32_t n_slots;
  const uint32_t* l_chunk; const uint64_t* l_dup;         // [n_lists] in to the write pass: first 16-byte chunk, first repeat slot
  uint32_t* post; uint64_t post_words;
  uint32_t* dups; uint64_t n_dups;                        // {doc, multiplicity} pairs
};

struct LoadLds { uint8_t b[kLoadLdsBytes]; uint32_t v[256]; };

__device__ __forceinline__ uint32_t ld_u16(const uint8_t* b, uint64_t o) { return (uint32_t)b[o] | ((uint32_t)b[o + 1] << 8); }
__device__ __forceinline__ uint32_t ld_u32(const uint8_t* b, uint64_t o) { return ld_u16(b, o) | (ld_u16(b, o + 2) << 16); }
__device__ __forceinline__ uint32_t ld_below(unsigned long long m, uint32_t lane) { return (uint32_t)__popcll(m & ((1ull << lane) - 1ull)); }

// The range [pos, pos + size) of a list lies inside the uploaded file (checked on the host; again here).
__device__ __forceinline__ bool ld_inside(const LoadArgs& a, uint32_t l) { return a.l_pos[l] <= a.dl_bytes && a.l_size[l] <= a.dl_bytes - a.l_pos[l]; }

// One wavefront: the varints of b[beg, end) appended to w.v at rank `cnt` on (ranks past 255 are counted, not kept).  False: a
// varint of more than five bytes or one that runs off the end — as varints() of ref_index_reader.cpp judges.
__device__ bool ld_varints(const uint8_t* b, uint32_t beg, uint32_t end, LoadLds& w, uint32_t& cnt, uint32_t lane) {
  bool bad = end > beg && b[end - 1] >= 0x80u;
  for (uint32_t base = beg; base < end; base += 64) {
    const uint32_t i = base + lane;
    const uint32_t c = i < end ? b[i] : 0x80u;
    const bool term = c < 0x80u;
    const unsigned long long m = __ballot(term);
    bool mine = false;
    if (term) {
      uint32_t k = 0;                                       // continuation bytes in front of the terminator
      while (k < 5u && i - k > beg && b[i - k - 1] >= 0x80u) k++;
      mine = k >= 5u;
      uint32_t v = c << (7u * min(k, 4u));
      for (uint32_t j = 0; j < min(k, 4u); j++) v |= (uint32_t)(b[i - k + j] & 0x7Fu) << (7u * j);
      const uint32_t r = cnt + ld_below(m, lane);
      if (r < 256u) w.v[r] = v;
    }
    bad |= __ballot(mine) != 0ull;
    cnt += (uint32_t)__popcll(m);
  }
  return !bad;
}

// One wavefront: w.v[r0, r1) from deltas to docIDs, the first one added to `prev`.
__device__ void ld_prefix(LoadLds& w, uint32_t r0, uint32_t r1, uint32_t prev, uint32_t lane) {
  __syncthreads();
  for (uint32_t base = r0; base < r1; base += 64) {
    const uint32_t j = base + lane;
    const uint32_t d = j < r1 ? w.v[j] : 0u;
    const uint32_t inc = st_scan(d, lane);
    if (j < r1) w.v[j] = prev + inc;
    prev += __shfl(inc, 63, 64);
  }
  __syncthreads();
}

// One wavefront: list l (raw <= 256) decoded into w.v, repeats included.  False: malformed, as decode_vb / decode_skipping of
// ref_index_reader.cpp judge.  Every branch is uniform over the wavefront: all lanes read the same header bytes.
__device__ bool ld_small(const LoadArgs& a, uint32_t l, LoadLds& w) {
  const uint32_t lane = threadIdx.x, n = a.l_size[l], raw = a.l_raw[l];
  const uint8_t* b = a.dl + a.l_pos[l];
  if (n <= kLoadLdsBytes) {
    for (uint32_t i = lane; i < n; i += 64) w.b[i] = b[i];
    b = w.b;
  }
  __syncthreads();
  uint32_t cnt = 0;
  if (raw <= 65u) {
    if (n > 5u * 65u) return false;                         // more bytes than 65 varints hold
    if (!ld_varints(b, 0, n, w, cnt, lane) || cnt != raw) return false;
    ld_prefix(w, 0, cnt, 0u, lane);
    return cnt != 0u;
  }
  uint32_t i = 0, block_first = 0;
  for (;;) {                                                // blocks of any length: walked by their sizes
    if (n - i < 2u) return false;
    const uint32_t packed = ld_u16(b, i), size = packed & 0x7FFFu;
    if (size < 2u || size > n - i) return false;
    const uint32_t r0 = min(cnt, 256u);
    if (!ld_varints(b, i + 2u, i + size, w, cnt, lane)) return false;
    if (cnt > raw) return false;
    if (cnt > r0) { ld_prefix(w, r0, cnt, block_first, lane); block_first = w.v[r0]; }
    i += size;
    if (packed & 0x8000u) break;
  }
  return i == n && cnt == raw;
}

// A workgroup is one wavefront and every condition of an early return is the same in all of its lanes.
__global__ __launch_bounds__(64) void sg_load_small_count(const LoadArgs a) {
  __shared__ LoadLds w;
  const uint32_t l = blockIdx.x, lane = threadIdx.x;
  if (l >= a.n_lists || a.l_raw[l] > 256u) return;
  LoadInfo out{LD_BAD, 0u, 0u, 0u};
  if (ld_inside(a, l) && ld_small(a, l, w)) {
    const uint32_t raw = a.l_raw[l];
    uint32_t stored = 0, ndup = 0;
    for (uint32_t base = 0; base < raw; base += 64) {
      const uint32_t j = base + lane;
      const bool in = j < raw;
      const bool keep = in && (j == 0u || w.v[j] != w.v[j - 1]);
      stored += (uint32_t)__popcll(__ballot(keep));
      ndup += (uint32_t)__popcll(__ballot(keep && j + 1u < raw && w.v[j + 1] == w.v[j]));
    }
    out = LoadInfo{LD_OK, stored, ndup, w.v[raw - 1]};
  }
  if (lane == 0) a.info[l] = out;
}

__global__ __launch_bounds__(64) void sg_load_small_write(const LoadArgs a) {
  __shared__ LoadLds w;
  const uint32_t l = blockIdx.x, lane = threadIdx.x;
  if (l >= a.n_lists || a.l_raw[l] > 256u || a.info[l].status != LD_OK) return;
  if (!ld_inside(a, l) || !ld_small(a, l, w)) return;
  const uint32_t raw = a.l_raw[l], stored = a.info[l].stored, ndup = a.info[l].ndup;
  const uint64_t at = (uint64_t)a.l_chunk[l] * 4u, dat = a.l_dup[l];
  uint32_t kept = 0, reps = 0;
  for (uint32_t base = 0; base < raw; base += 64) {
    const uint32_t j = base + lane;
    const bool in = j < raw;
    const uint32_t v = in ? w.v[j] : 0u;
    const bool keep = in && (j == 0u || v != w.v[j - 1]);
    const bool rep = keep && j + 1u < raw && w.v[j + 1] == v;
    const unsigned long long mk = __ballot(keep), mr = __ballot(rep);
    const uint32_t o = kept + ld_below(mk, lane), d = reps + ld_below(mr, lane);
    if (keep && o < stored && at + o < a.post_words) a.post[at + o] = v;
    if (rep && d < ndup && dat + d < a.n_dups) {
      uint32_t mult = 2;
      while (j + mult < raw && w.v[j + mult] == v) mult++;
      a.dups[2u * (dat + d)] = v;
      a.dups[2u * (dat + d) + 1u] = mult;
    }
    kept += (uint32_t)__popcll(mk);
    reps += (uint32_t)__popcll(mr);
  }
  const uint32_t o = stored + lane;                         // the last chunk padded with the last value
  if (o < ((stored + 3u) & ~3u) && at + o < a.post_words) a.post[at + o] = w.v[raw - 1];
}

__global__ __launch_bounds__(64) void sg_load_roar_head(const LoadArgs a) {
  const uint32_t ri = blockIdx.x, lane = threadIdx.x;
  if (ri >= a.n_r) return;
  const uint32_t l = a.r_list[ri];
  if (l >= a.n_lists) return;
  if (lane == 0) a.r_status[ri] = LD_BAD;                   // until the walk below has reached its end
  if (!ld_inside(a, l)) return;
  const uint64_t n = a.l_size[l];
  const uint8_t* b = a.dl + a.l_pos[l];
  const uint32_t cbase = a.r_cbase[ri], cend = min(a.r_cbase[ri + 1], a.n_slots);
  if (n < 8u) return;
  const uint32_t cookie = ld_u32(b, 0);
  uint64_t i = 4, flags = 0;
  uint32_t cnt;
  bool has_runs = false;
  if ((cookie & 0xFFFFu) == 12347u) {
    cnt = (cookie >> 16) + 1u; has_runs = true;
    flags = i;
    i += (cnt + 7u) / 8u;
    if (i > n) return;
  } else if (cookie == 12346u) { cnt = ld_u32(b, 4); i = 8; }
  else return;
  if (i + 4ull * cnt > n || cbase > cend || cnt != cend - cbase) return;   // (the host sized the slots by the same header)
  const uint64_t keys = i;
  i += 4ull * cnt;
  if (!has_runs || cnt >= 4u) i += 4ull * cnt;              // the offset header
  for (uint32_t base = 0; base < cnt; base += 64) {
    const uint32_t k = base + lane;
    const bool in = k < cnt;
    const uint32_t key = in ? ld_u16(b, keys + 4ull * k) : 0u, card = in ? ld_u16(b, keys + 4ull * k + 2u) + 1u : 0u;
    const bool is_run = in && has_runs && ((b[flags + k / 8u] >> (k % 8u)) & 1u);
    uint32_t size = !in || is_run ? 0u : card > 4096u ? 8192u : 2u * card, runs = 0;
    uint64_t start;
    const unsigned long long mr = __ballot(is_run);
    if (mr == 0ull) {
      const uint32_t inc = st_scan(size, lane);
      start = i + (inc - size);
      i += __shfl(inc, 63, 64);
    } else {                                                // a run container's size stands at its start: one after the other
      start = 0;
      for (uint32_t j = 0; j < 64u && base + j < cnt; j++) {
        uint32_t sz = __shfl(size, j, 64);
        if ((mr >> j) & 1ull) {
          if (i + 2u > n) return;
          const uint32_t nr = ld_u16(b, i);
          sz = 2u + 4u * nr;
          if (lane == j) { runs = nr; size = sz; }
        }
        if (lane == j) start = i;
        i += sz;
      }
    }
    if (__ballot(in && start + size > n) != 0ull) return;   // a container past the list's end
    if (in) {
      const uint32_t s = cbase + k;
      a.c_ri[s] = ri; a.c_key[s] = key; a.c_start[s] = (uint32_t)start;
      a.c_kind[s] = is_run ? LD_RUN : card > 4096u ? LD_BITMAP : LD_ARRAY;
      a.c_n[s] = is_run ? runs : card;
    }
  }
  if (lane == 0) a.r_status[ri] = cnt ? LD_OK : LD_BAD;
}

__device__ __forceinline__ uint64_t ld_word(const uint8_t* p) { return (uint64_t)ld_u32(p, 0) | ((uint64_t)ld_u32(p, 4) << 32); }
__device__ __forceinline__ uint32_t ld_run_end(uint32_t s, uint32_t len) { return min(s + len, 0xFFFFu); }   // a run stays inside its container

// A container of a list whose header walk ended well: its bytes lie inside the list (sg_load_roar_head compared them).
__device__ __forceinline__ bool ld_slot(const LoadArgs& a, uint32_t s, uint32_t* ri) {
  if (s >= a.n_slots) return false;
  *ri = a.c_ri[s];
  return *ri < a.n_r && a.r_status[*ri] == LD_OK && a.r_list[*ri] < a.n_lists;
}

__global__ __launch_bounds__(64) void sg_load_roar_count(const LoadArgs a) {
  const uint32_t s = blockIdx.x, lane = threadIdx.x;
  uint32_t ri;
  if (!ld_slot(a, s, &ri)) return;
  const uint8_t* p = a.dl + a.l_pos[a.r_list[ri]] + a.c_start[s];
  const uint32_t kind = a.c_kind[s], n = a.c_n[s];
  unsigned long long count = 0;
  uint32_t last = 0, flag = 0;
  if (kind == LD_ARRAY) {
    for (uint32_t i = lane; i < n; i += 64) flag |= i && ld_u16(p, 2ull * i) <= ld_u16(p, 2ull * i - 2u) ? 1u : 0u;
    count = n;
    last = n ? ld_u16(p, 2ull * (n - 1u)) : 0u;
  } else if (kind == LD_BITMAP) {
    uint32_t c = 0, top = 0;
    for (uint32_t wd = lane; wd < 1024u; wd += 64) {
      const uint64_t x = ld_word(p + 8u * wd);
      c += (uint32_t)__popcll(x);
      if (x) top = wd * 64u + 63u - (uint32_t)__clzll(x);
    }
    for (uint32_t d = 32; d; d >>= 1) { c += __shfl_xor(c, d, 64); top = max(top, __shfl_xor(top, d, 64)); }
    count = c; last = top;
  } else {
    for (uint32_t r = lane; r < n; r += 64) {
      const uint32_t st = ld_u16(p, 2u + 4ull * r), e = ld_run_end(st, ld_u16(p, 4u + 4ull * r));
      count += e - st + 1u;
      if (r && st <= ld_run_end(ld_u16(p, 4ull * r - 2u), ld_u16(p, 4ull * r))) flag = 1u;
    }
    for (uint32_t d = 32; d; d >>= 1) count += __shfl_xor(count, d, 64);
    last = n ? ld_run_end(ld_u16(p, 4ull * n - 2u), ld_u16(p, 4ull * n)) : 0u;
  }
  const bool any = __ballot(flag != 0u) != 0ull || count > 65536ull;
  if (lane == 0) { a.c_count[s] = (uint32_t)min(count, 65536ull); a.c_last[s] = (a.c_key[s] << 16) | last; a.c_flag[s] = any ? 1u : 0u; }
}

__global__ __launch_bounds__(64) void sg_load_roar_sum(const LoadArgs a) {
  const uint32_t ri = blockIdx.x, lane = threadIdx.x;
  if (ri >= a.n_r) return;
  const uint32_t l = a.r_list[ri];
  if (l >= a.n_lists) return;
  LoadInfo out{LD_BAD, 0u, 0u, 0u};
  if (a.r_status[ri] == LD_OK) {
    const uint32_t cbase = a.r_cbase[ri], n = min(a.r_cbase[ri + 1], a.n_slots) - cbase;
    unsigned long long total = 0;
    bool host = false;
    uint32_t last = 0;
    for (uint32_t base = 0; base < n; base += 64) {
      const uint32_t k = base + lane;
      const bool in = k < n;
      const uint32_t c = in ? a.c_count[cbase + k] : 0u;
      const uint32_t inc = st_scan(c, lane);                // (64 containers of 65 536 values at most)
      if (in) a.c_out[cbase + k] = (uint32_t)min(total + (inc - c), 0xFFFFFFFFull);
      host |= __ballot(in && (a.c_flag[cbase + k] != 0u || (k && a.c_key[cbase + k] <= a.c_key[cbase + k - 1]))) != 0ull;
      const unsigned long long mc = __ballot(c != 0u);
      if (mc) last = __shfl(in ? a.c_last[cbase + k] : 0u, 63 - __clzll(mc), 64);
      total += __shfl(inc, 63, 64);
    }
    if (total > 0xFFFFFFFFull) host = true;
    if (total) out = LoadInfo{host ? LD_HOST : LD_OK, (uint32_t)min(total, 0xFFFFFFFFull), 0u, last};
  }
  if (lane == 0) a.info[l] = out;
}

__global__ __launch_bounds__(64) void sg_load_roar_write(const LoadArgs a) {
  const uint32_t s = blockIdx.x, lane = threadIdx.x;
  uint32_t ri;
  if (!ld_slot(a, s, &ri)) return;
  const uint32_t l = a.r_list[ri];
  if (a.info[l].status != LD_OK) return;
  const uint8_t* p = a.dl + a.l_pos[l] + a.c_start[s];
  const uint32_t kind = a.c_kind[s], n = a.c_n[s], count = a.c_count[s], first = a.c_out[s], stored = a.info[l].stored;
  const uint32_t high = a.c_key[s] << 16;
  const uint64_t at = (uint64_t)a.l_chunk[l] * 4u;
  // slot e of this container: inside what the count pass gave the container, the list and the store
  auto put = [&](uint32_t e, uint32_t low) {
    if (e < count && first <= stored && e < stored - first && at + first + e < a.post_words) a.post[at + first + e] = high | low;
  };
  if (kind == LD_ARRAY) {
    for (uint32_t i = lane; i < n; i += 64) put(i, ld_u16(p, 2ull * i));
  } else if (kind == LD_BITMAP) {
    uint32_t before = 0;
    for (uint32_t wd = lane; wd < 1024u; wd += 64) {
      uint64_t x = ld_word(p + 8u * wd);
      const uint32_t c = (uint32_t)__popcll(x), inc = st_scan(c, lane);
      uint32_t e = before + (inc - c);
      while (x) { put(e++, wd * 64u + (uint32_t)__ffsll((unsigned long long)x) - 1u); x &= x - 1u; }
      before += __shfl(inc, 63, 64);
    }
  } else {
    uint32_t before = 0;
    for (uint32_t base = 0; base < n; base += 64) {
      const uint32_t r = base + lane;
      const uint32_t st = r < n ? ld_u16(p, 2u + 4ull * r) : 0u;
      const uint32_t len = r < n ? ld_run_end(st, ld_u16(p, 4u + 4ull * r)) - st + 1u : 0u;
      const uint32_t inc = st_scan(len, lane);
      const uint32_t e = before + (inc - len);
      if (len < 64u) for (uint32_t t = 0; t < len; t++) put(e + t, st + t);
      unsigned long long big = __ballot(len >= 64u);        // a long run: the whole wavefront
      while (big) {
        const int j = __ffsll(big) - 1;
        const uint32_t sj = __shfl(st, j, 64), lj = __shfl(len, j, 64), ej = __shfl(e, j, 64);
        for (uint32_t t = lane; t < lj; t += 64) put(ej + t, sj + t);
        big &= big - 1ull;
      }
      before += __shfl(inc, 63, 64);
    }
  }
  if (s + 1u == a.r_cbase[ri + 1]) {                        // the list's last container pads the last chunk
    const uint32_t o = stored + lane;
    if (o < ((stored + 3u) & ~3u) && at + o < a.post_words) a.post[at + o] = a.info[l].last;
  }
}

}  // namespace sg

namespace {

thread_local double t_load_ms[7];                         // the calling thread's last load: read, parse, H2D, kernels, D2H, assembly, all

uint32_t load_roar_slots(const uint8_t* b, uint64_t n) {  // containers the header of a roaring list announces, 0 where it cannot hold them
  if (n < 8) return 0;
  const uint32_t cookie = (uint32_t)b[0] | ((uint32_t)b[1] << 8) | ((uint32_t)b[2] << 16) | ((uint32_t)b[3] << 24);
  uint64_t cnt, i;
  if ((cookie & 0xFFFF) == 12347) { cnt = (cookie >> 16) + 1; i = 4 + (cnt + 7) / 8; }
  else if (cookie == 12346) { cnt = (uint32_t)b[4] | ((uint32_t)b[5] << 8) | ((uint32_t)b[6] << 16) | ((uint32_t)b[7] << 24); i = 8; }
  else return 0;
  return i + 4 * cnt > n ? 0 : (uint32_t)cnt;
}

// Steps 2 and 3 with the lists decoded on `device`; seconds: [4] H2D, kernels, D2H, assembly.
int load_decode_device(HostIndex& ix, const RefFiles& f, int device, std::string& err, double seconds[4]) {
  const size_t n = f.lists.size();
  if (n >= (1u << 30)) { err = "2^30 posting lists or more: beyond the device decoder, load with device < 0"; return SG_E_UNSUPPORTED; }
  DeviceGuard dg;
  HIP_TRY(dg.set(device));
  StoreStream ss;
  HIP_TRY(hipStreamCreateWithFlags(&ss.s, hipStreamNonBlocking));
  const hipStream_t st = ss.s;

  auto t = clk::now();
  std::vector<uint64_t> l_pos(n);
  std::vector<uint32_t> l_size(n), l_raw(n), r_list, r_cbase;
  uint64_t n_slots = 0;
  for (size_t i = 0; i < n; i++) {
    const RefList& l = f.lists[i];
    l_pos[i] = l.pos; l_size[i] = l.size; l_raw[i] = l.raw;
    if (l.raw > 256u) {
      r_list.push_back((uint32_t)i);
      r_cbase.push_back((uint32_t)n_slots);
      n_slots += load_roar_slots(f.dl.data() + l.pos, l.size);
    }
  }
  r_cbase.push_back((uint32_t)n_slots);
  if (n_slots >= 0xFFFFFFF0ull) { err = "too many roaring containers for the device decoder, load with device < 0"; return SG_E_UNSUPPORTED; }

  DeviceBlock mem;
  LoadArgs a{};
  int rc;
  a.n_lists = (uint32_t)n; a.n_r = (uint32_t)r_list.size(); a.n_slots = (uint32_t)n_slots;
  a.dl_bytes = f.dl.size();
  const size_t padded = (f.dl.size() + 64 + 15) & ~(size_t)15;
  uint8_t* d_dl;
  uint32_t* d_chunk; uint64_t* d_dup;
  if ((rc = mem.alloc(&d_dl, padded)) || (rc = mem.upload(l_pos, &a.l_pos, st)) || (rc = mem.upload(l_size, &a.l_size, st)) ||
      (rc = mem.upload(l_raw, &a.l_raw, st)) || (rc = mem.upload(r_list, &a.r_list, st)) || (rc = mem.upload(r_cbase, &a.r_cbase, st)) ||
      (rc = mem.alloc(&a.info, n)) || (rc = mem.alloc(&a.r_status, (size_t)a.n_r)) || (rc = mem.alloc(&d_chunk, n)) || (rc = mem.alloc(&d_dup, n)))
    return rc;
  a.dl = d_dl; a.l_chunk = d_chunk; a.l_dup = d_dup;
  for (uint32_t** c : {&a.c_ri, &a.c_key, &a.c_kind, &a.c_n, &a.c_start, &a.c_count, &a.c_last, &a.c_flag, &a.c_out})
    if ((rc = mem.alloc(c, (size_t)n_slots))) return rc;
  if (!f.dl.empty()) HIP_TRY(hipMemcpyAsync(d_dl, f.dl.data(), f.dl.size(), hipMemcpyHostToDevice, st));
  HIP_TRY(hipMemsetAsync(d_dl + f.dl.size(), 0, padded - f.dl.size(), st));
  if (n) HIP_TRY(hipMemsetAsync(a.info, 0xFF, n * sizeof(LoadInfo), st));           // (a status that is none of LD_*)
  if (a.n_r) HIP_TRY(hipMemsetAsync(a.r_status, 0xFF, (size_t)a.n_r * 4, st));
  if (n_slots) HIP_TRY(hipMemsetAsync(a.c_ri, 0xFF, (size_t)n_slots * 4, st));
  HIP_TRY(hipStreamSynchronize(st));
  seconds[0] = since(t);

  t = clk::now();
  if (n) { hipLaunchKernelGGL(sg_load_small_count, dim3((unsigned)n), dim3(64), 0, st, a); HIP_TRY(hipGetLastError()); }
  if (a.n_r) {
    hipLaunchKernelGGL(sg_load_roar_head, dim3(a.n_r), dim3(64), 0, st, a);
    HIP_TRY(hipGetLastError());
    if (a.n_slots) { hipLaunchKernelGGL(sg_load_roar_count, dim3(a.n_slots), dim3(64), 0, st, a); HIP_TRY(hipGetLastError()); }
    hipLaunchKernelGGL(sg_load_roar_sum, dim3(a.n_r), dim3(64), 0, st, a);
    HIP_TRY(hipGetLastError());
  }
  HIP_TRY(hipStreamSynchronize(st));
  seconds[1] = since(t);

  t = clk::now();
  std::vector<LoadInfo> info(n);
  if (n) HIP_TRY(hipMemcpyAsync(info.data(), a.info, n * sizeof(LoadInfo), hipMemcpyDeviceToHost, st));
  HIP_TRY(hipStreamSynchronize(st));
  seconds[2] = since(t);

  // position: on the host
  t = clk::now();
  std::vector<uint32_t> stored(n), chunk(n);
  std::vector<uint64_t> dup_at(n);
  std::vector<std::pair<size_t, std::vector<uint32_t>>> by_host;                      // lists of status LD_HOST, de-duplicated
  uint32_t max_doc = 0;
  for (size_t i = 0; i < n; i++) {
    if (info[i].status != LD_OK && info[i].status != LD_HOST) return ref_malformed(f, f.lists[i], err);
    if (info[i].status == LD_HOST) {
      std::vector<uint32_t> v;
      if (!ref_decode_list(f, f.lists[i], v)) return ref_malformed(f, f.lists[i], err);
      info[i].last = v.back();
      by_host.emplace_back(i, std::move(v));
    }
    max_doc = std::max(max_doc, info[i].last);
  }
  if (f.fail_rc) { err = f.fail_err; return f.fail_rc; }
  ix.n_docs = n ? (uint64_t)max_doc + 1 : 0;
  uint64_t n_dups = 0;
  for (size_t i = 0, k = 0; i < n; i++) {
    dup_at[i] = n_dups;
    if (info[i].status == LD_HOST) {
      ref_dedup(ix, f.lists[i], by_host[k].second);         // its repeats and marker: straight into ix.dups
      stored[i] = (uint32_t)by_host[k++].second.size();
    } else {
      stored[i] = info[i].stored;
      n_dups += info[i].ndup;
    }
  }
  if ((rc = ref_layout(ix, f, stored.data(), err))) return rc;
  for (size_t i = 0; i < n; i++) chunk[i] = ix.seg_off[(size_t)f.lists[i].term * (ix.n_segments + 1) + f.lists[i].segment];
  seconds[3] = since(t);

  t = clk::now();
  a.post_words = ix.postings.size(); a.n_dups = n_dups;
  if ((rc = mem.alloc(&a.post, ix.postings.size())) || (rc = mem.alloc(&a.dups, (size_t)n_dups * 2))) return rc;
  if (n) {
    HIP_TRY(hipMemcpyAsync(d_chunk, chunk.data(), n * 4, hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(d_dup, dup_at.data(), n * 8, hipMemcpyHostToDevice, st));
  }
  HIP_TRY(hipMemsetAsync(a.post, 0, std::max<size_t>(ix.postings.size() * 4, 16), st));
  HIP_TRY(hipStreamSynchronize(st));
  seconds[0] += since(t);

  t = clk::now();
  if (n) { hipLaunchKernelGGL(sg_load_small_write, dim3((unsigned)n), dim3(64), 0, st, a); HIP_TRY(hipGetLastError()); }
  if (a.n_slots) { hipLaunchKernelGGL(sg_load_roar_write, dim3(a.n_slots), dim3(64), 0, st, a); HIP_TRY(hipGetLastError()); }
  HIP_TRY(hipStreamSynchronize(st));
  seconds[1] += since(t);

  t = clk::now();
  std::vector<uint32_t> dups((size_t)n_dups * 2);
  if (!ix.postings.empty()) HIP_TRY(hipMemcpyAsync(ix.postings.data(), a.post, ix.postings.size() * 4, hipMemcpyDeviceToHost, st));
  if (n_dups) HIP_TRY(hipMemcpyAsync(dups.data(), a.dups, dups.size() * 4, hipMemcpyDeviceToHost, st));
  HIP_TRY(hipStreamSynchronize(st));
  seconds[2] += since(t);

  t = clk::now();
  ix.dups.reserve(ix.dups.size() + (size_t)n_dups + 16);
  for (size_t i = 0; i < n; i++) {
    if (info[i].status == LD_HOST) continue;
    const RefList& l = f.lists[i];
    for (uint64_t d = dup_at[i]; d < dup_at[i] + info[i].ndup; d++) ix.dups.push_back(DupEntry{l.term, l.segment, dups[2 * d], dups[2 * d + 1]});
    ref_marker(ix, l, stored[i]);
  }
  for (const auto& h : by_host) ref_put_list(ix, f.lists[h.first], h.second);
  ref_finish(ix);
  seconds[3] += since(t);
  return SG_OK;
}

}  // namespace

extern "C" {

int sg_index_load_reference_ex(const char* hd_path, const char* dl_path, const sg_desc* desc, int device, sg_index** out) {
  SG_GUARD_BEGIN
  if (!out || !hd_path || !dl_path) { set_error("null argument"); return SG_E_INVALID; }
  const auto t0 = clk::now();
  std::unique_ptr<sg_index> ix(new (std::nothrow) sg_index());
  if (!ix) return SG_E_NOMEM;
  std::string err;
  double s[6] = {0, 0, 0, 0, 0, 0};                       // read, parse, H2D, kernels (the host decoders), D2H, assembly
  RefFiles f;
  int rc = ref_open(hd_path, dl_path, desc, ix->host, f, err, s);
  if (!rc) {
    // two descriptors of one (term, segment): the later one wins in header order, which only the host's walk reproduces
    if (device < 0 || f.lists.empty() || ref_pair_twice(ix->host, f)) {
      double hs[2] = {0, 0};
      rc = ref_decode_host(ix->host, f, err, hs);
      s[3] = hs[0]; s[5] = hs[1];
    } else {
      rc = load_decode_device(ix->host, f, device, err, s + 2);
      if (rc && err.empty()) return rc;                     // (a HIP error: HIP_TRY has set its message)
    }
  }
  if (rc) { set_error(err); return rc; }
  if (ix->host.wrap0.size() > SG_WRAP_MAX || ix->host.wrap1.size() > SG_WRAP_MAX) {
    set_error("wrap strings longer than 8 runes"); return SG_E_UNSUPPORTED;
  }
  for (int i = 0; i < 6; i++) t_load_ms[i] = s[i] * 1e3;
  t_load_ms[6] = since(t0) * 1e3;
  *out = ix.release();
  return SG_OK;
  SG_GUARD_END(SG_RC)
}

int sg_debug_index_load_times(double* out_ms, uint32_t cap) {
  if (!out_ms) { set_error("null argument"); return SG_E_INVALID; }
  for (uint32_t i = 0; i < cap && i < 7u; i++) out_ms[i] = t_load_ms[i];
  return SG_OK;
}

}  // extern "C"
