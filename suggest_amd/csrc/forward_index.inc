// forward_index.inc — the forward index (doc -> distinct terms) of a replica, derived on the GPU from the CSR that is
// already there.  Included by engine.hip after capi.inc; tune.inc's add_replica calls it.
//
// The reference verifies nothing: its mergers count exactly (pkg/merger/cp_merge.go:32-117).  The device path counts
// with lossy LDS counters and verifies every flagged document exactly (DESIGN.md §4); with only the inverted lists that
// costs a binary search in every query term's list (A searches x ~8 dependent probes, ~10 KB of scattered HBM lines per
// candidate).  With the doc's own term list at hand it is one contiguous read of <= 128 B and an LDS hash lookup per term.
//
//   fwd_count   one wavefront per (term, segment) list: cnt[doc] += 1 per posting (pad repeats skipped), card[doc] = segment
//   scan        chunk offsets of the docs' lists (a list is padded to 16 bytes with 0xFFFFFFFF)
//   fwd_fill    the same walk: fwd_terms[off[doc] * 4 + slot] = term, slot from an atomic cursor per doc
//   fwd_rec     {offset, card | distinct << 16}
namespace sg {

__global__ __launch_bounds__(64) void fwd_walk(const uint32_t* __restrict__ postings, const uint32_t* __restrict__ seg_off, uint32_t S, uint64_t n_lists,
                                               uint32_t n_docs, uint32_t* cnt, uint32_t* card, const uint32_t* off, uint32_t* terms) {
  // (grid-stride over the lists: terms x segments x 64 lanes passes HIP's 2^32 work-items per launch for dictionaries with
  //  many terms AND many cardinality segments — 341 k terms x 503 segments in a fuzz trial, where the lists beyond the
  //  limit silently went unwalked)
  for (uint64_t list = blockIdx.x; list < n_lists; list += gridDim.x) {
  const uint32_t t = (uint32_t)(list / S), b = (uint32_t)(list - (uint64_t)t * S);
  const uint32_t c0 = seg_off[(uint64_t)t * (S + 1) + b], c1 = seg_off[(uint64_t)t * (S + 1) + b + 1];
  for (uint32_t c = c0 + threadIdx.x; c < c1; c += 64) {
    const uint4 v = ((const uint4*)postings)[c];
    const uint32_t d[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
    for (int e = 0; e < 4; e++) {
      if (e > 0 && d[e] == d[e - 1]) continue;                 // padding repeats the last docID (lists are strictly ascending)
      if (d[e] >= n_docs) continue;
      if (!terms) { atomicAdd(cnt + d[e], 1u); card[d[e]] = b; }
      else terms[(uint64_t)off[d[e]] * 4 + atomicAdd(cnt + d[e], 1u)] = t;
    }
  }
  }
}

__global__ void fwd_chunks(const uint32_t* cnt, uint32_t n_docs, uint32_t* chunks) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n_docs) chunks[i] = (cnt[i] + 3u) >> 2;
}

__global__ void fwd_records(const uint32_t* off, const uint32_t* cnt, const uint32_t* card, uint32_t n_docs, uint2* rec) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n_docs) rec[i] = make_uint2(off[i], (card[i] & 0xFFFFu) | (cnt[i] << 16));
}

}  // namespace sg

namespace {

// builds fwd_rec / fwd_terms of replica `r` from its device CSR (postings, seg_off already set in r->dix)
int build_forward_index(const HostIndex& h, Replica* r) {
  DeviceIndex& d = r->dix;
  const uint32_t n_docs = (uint32_t)h.n_docs, S = h.n_segments, nT = (uint32_t)h.term_key.size();
  if (S > 0xFFFFu) { set_error("more than 65535 cardinality segments"); return SG_E_UNSUPPORTED; }
  uint2* rec = nullptr;
  int rc;
  if ((rc = r->mem.alloc(&rec, (size_t)n_docs))) return rc;
  d.fwd_rec = rec;
  if (!n_docs || !nT) { uint32_t* t = nullptr; if ((rc = r->mem.alloc(&t, 4))) return rc; d.fwd_terms = t; return SG_OK; }
  uint32_t *cnt = nullptr, *card = nullptr, *off = nullptr, *chunks = nullptr;
  DeviceBlock scratch;                                           // freed on return: not part of the replica
  if ((rc = scratch.alloc(&cnt, (size_t)n_docs)) || (rc = scratch.alloc(&card, (size_t)n_docs)) || (rc = scratch.alloc(&off, (size_t)n_docs + 1)) ||
      (rc = scratch.alloc(&chunks, (size_t)n_docs + 1)))
    return rc;
  HIP_TRY(hipMemset(cnt, 0, (size_t)n_docs * 4));
  HIP_TRY(hipMemset(card, 0, (size_t)n_docs * 4));
  const uint64_t n_lists = (uint64_t)nT * S;
  if (n_lists >= 0x7FFFFFFFull) { set_error("terms x segments exceeds a launch grid"); return SG_E_UNSUPPORTED; }
  hipLaunchKernelGGL(fwd_walk, dim3((unsigned)std::min<uint64_t>(n_lists, 1u << 22)), dim3(64), 0, 0, d.postings, d.seg_off, S, n_lists, n_docs, cnt, card, (const uint32_t*)nullptr, (uint32_t*)nullptr);
  HIP_TRY(hipGetLastError());
  hipLaunchKernelGGL(fwd_chunks, dim3((n_docs + 255) / 256), dim3(256), 0, 0, cnt, n_docs, chunks);
  HIP_TRY(hipGetLastError());
  uint64_t total_chunks = 0;
  if ((rc = device_exclusive_sum(scratch, chunks, off, n_docs)) || (rc = device_total(chunks, off, n_docs, &total_chunks))) return rc;
  if ((h.n_postings + 3) / 4 + n_docs >= 0xFFFFFFF0ull) { set_error("forward index exceeds 2^32 16-byte chunks"); return SG_E_UNSUPPORTED; }
  uint32_t* terms = nullptr;
  if ((rc = r->mem.alloc(&terms, (size_t)total_chunks * 4))) return rc;
  HIP_TRY(hipMemset(terms, 0xFF, std::max<size_t>((size_t)total_chunks * 16, 16)));
  hipLaunchKernelGGL(fwd_records, dim3((n_docs + 255) / 256), dim3(256), 0, 0, off, cnt, card, n_docs, rec);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipMemset(cnt, 0, (size_t)n_docs * 4));
  hipLaunchKernelGGL(fwd_walk, dim3((unsigned)std::min<uint64_t>(n_lists, 1u << 22)), dim3(64), 0, 0, d.postings, d.seg_off, S, n_lists, n_docs, cnt, card, (const uint32_t*)off, terms);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipDeviceSynchronize());
  d.fwd_terms = terms;
  return SG_OK;
}

}  // namespace
