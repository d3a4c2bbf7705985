// dict_rows.inc — result rows as strings from a dictionary held in HBM (sg_dictionary, include/suggest_hip.h; DESIGN.md §5c),
// included by engine.hip after mixed_batch.inc (it uses host_call.inc's run_host_call and IoCall, search_api.inc's
// search_enqueue, handles.inc's open_search, capi.inc's stream_scratch and poison_fill, d_copy_bytes, kCountFlagMin, read_cdb_words,
// HIP_TRY).  The reference's Service.Suggest maps every docID
// of a row through dict.Get (pkg/suggest/service.go:129-136); here the rows of any search stay on the device and
//   lengths   dict_lengths_kernel: a thread per slot finds the slot's row and its place in it — a division for a fixed stride, a
//             search of row_offs for ragged rows — and writes the string's length where the slot holds an entry, 0 where it
//             holds none (past the count, a flagged row, no row at all: the id is not read) or an id outside the dictionary
//             (counted in info[1]);
//   offsets   an exclusive sum over slots + 1 lengths: text_offs, and its last word the bytes needed (info[0]);
//   gather    dict_gather_kernel: 16 lanes per slot copy the string with d_copy_bytes, the byte copy of mixed_gather_kernel;
//             a string that would end past text_cap is not written.
// The step's own device memory is one block of the calling thread's per-stream scratch (SCRATCH_DICT: the lengths and the scan's
// working memory).  The host-buffer routes learn the total through pinned memory with one wait, then hold a text block of exactly
// the bytes needed — never more than the caller's text_cap — for the gather and the copy back.

namespace sg {

constexpr uint32_t kDictThreads = 256;
constexpr uint32_t kDictSub = 16;                     // lanes that copy one slot's string

struct DictView {            // a device-resident dictionary as the kernels read it
  const uint64_t* doc_offs;  // [n_docs + 1], from 0
  const uint8_t* blob;
  uint32_t n_docs;
};

// A thread per slot, thread `slots` closes the scan's input with a zero.  row_offs null: rows of `row` slots.
__global__ __launch_bounds__(kDictThreads) void dict_lengths_kernel(const DictView d, const uint32_t* __restrict__ ids, const uint32_t* __restrict__ counts,
                                                                     const uint64_t* __restrict__ row_offs, uint32_t n_rows, uint32_t row, uint64_t slots,
                                                                     uint64_t* __restrict__ lens, unsigned long long* __restrict__ info) {
  for (uint64_t s = (uint64_t)blockIdx.x * kDictThreads + threadIdx.x; s <= slots; s += (uint64_t)gridDim.x * kDictThreads) {
    uint64_t len = 0;
    bool in_row = false;
    uint32_t i = 0;
    uint64_t pos = 0, row_len = 0;
    if (s < slots && n_rows) {
      if (row_offs) {                              // the last row that begins at or before s
        uint32_t lo = 0, hi = n_rows;              // (row_offs[lo] <= s is not known yet; rows in [lo, hi))
        while (hi - lo > 1u) { const uint32_t mid = lo + (hi - lo) / 2u; if (row_offs[mid] <= s) lo = mid; else hi = mid; }
        const uint64_t b = row_offs[lo], e = row_offs[lo + 1];
        if (b <= s && s < e) { in_row = true; i = lo; pos = s - b; row_len = e - b; }
      } else if (row) {
        const uint64_t r = s / row;
        if (r < n_rows) { in_row = true; i = (uint32_t)r; pos = s - r * row; row_len = row; }
      }
    }
    if (in_row) {
      const uint32_t c = counts[i];
      if (c < kCountFlagMin && pos < c && pos < row_len) {
        const uint32_t id = ids[s];
        if (id < d.n_docs) len = d.doc_offs[(uint64_t)id + 1] - d.doc_offs[id];
        else atomicAdd(info + 1, 1ull);
      }
    }
    lens[s] = len;
  }
}

// kDictSub lanes per slot: the string of ids[s] goes to text[text_offs[s] .. text_offs[s + 1]).  A slot of length 0 holds no
// entry (or an empty string): its id is not read.
__global__ __launch_bounds__(kDictThreads) void dict_gather_kernel(const DictView d, const uint32_t* __restrict__ ids, const uint64_t* __restrict__ text_offs,
                                                                    uint64_t slots, uint8_t* __restrict__ text, uint64_t text_cap) {
  const uint32_t sub = threadIdx.x % kDictSub;
  const uint64_t per = kDictThreads / kDictSub;
  for (uint64_t s = (uint64_t)blockIdx.x * per + threadIdx.x / kDictSub; s < slots; s += (uint64_t)gridDim.x * per) {
    const uint64_t to = text_offs[s], end = text_offs[s + 1];
    if (end <= to || end > text_cap) continue;
    d_copy_bytes(text + to, d.blob + d.doc_offs[ids[s]], (uint32_t)(end - to), sub, kDictSub);
  }
}

}  // namespace sg

struct sg_dictionary {
  std::atomic<int> refs{1};
  int device = -1;                     // -1: host-resident
  uint32_t n_docs = 0, max_len = 0;
  uint64_t bytes = 0;
  std::vector<uint64_t> h_offs;        // host-resident: [n_docs + 1] from 0, and the blob
  std::vector<uint8_t> h_blob;
  DeviceBlock mem;                     // device-resident: owns the two arrays of `view`
  DictView view{nullptr, nullptr, 0};
  // device-resident: the handle's own copy of the simple lower-case pairs (edit_rank.inc folds case without an sg_index)
  const uint32_t* d_lower_from = nullptr; const uint32_t* d_lower_to = nullptr; uint32_t n_lower = 0;
};

namespace {

// What a thread keeps between its host-buffer dictionary calls: the pinned words the step's info comes back through and the
// text block of its last call.  A thread that ends hands them back (the main thread's are left to process exit).
struct DictThread {
  GrowBlock pin{true};
  void* text = nullptr; size_t text_bytes = 0; int text_device = -1;
  void drop_text() {
    if (!text) return;
    DeviceGuard dg;
    if (dg.set(text_device) == hipSuccess) (void)hipFree(text);
    text = nullptr; text_bytes = 0;
  }
  // a block of `needed` bytes at least and `cap` at most on `device` (needed <= cap, needed > 0)
  int text_block(int device, uint64_t needed, uint64_t cap, uint8_t** out) {
    if (!text || text_device != device || text_bytes < needed || text_bytes > cap) {
      drop_text();
      const hipError_t e = hipMalloc(&text, (size_t)needed);
      if (e != hipSuccess) { text = nullptr; set_error(std::string("hipMalloc: ") + hipGetErrorString(e)); return SG_E_NOMEM; }
      text_bytes = (size_t)needed; text_device = device;
    }
    *out = (uint8_t*)text;
    return SG_OK;
  }
  ~DictThread() {
    if (on_main_thread()) return;
    pin.release();
    drop_text();
  }
};
thread_local DictThread t_dict;

// the checks every route makes of a geometry
int dict_check_geometry(const void* row_offs, uint32_t n_rows, uint32_t row, uint64_t slots) {
  if (!row_offs && (uint64_t)n_rows * row > slots) { set_error("dictionary rows: slots is below n_rows * row"); return SG_E_INVALID; }
  if (slots > 0x7FFFFFF0ull) { set_error("dictionary rows: too many slots for one call"); return SG_E_INVALID; }   // (hipcub counts in int)
  return SG_OK;
}

// lengths and offsets on `st` (the caller has made dict->device current): text_offs[slots + 1], info[0] = the bytes needed,
// info[1] = entries outside the dictionary
int dict_offsets_enqueue(const sg_dictionary* dict, const uint32_t* ids, const uint32_t* counts, const uint64_t* row_offs, uint32_t n_rows,
                         uint32_t row, uint64_t slots, uint64_t* text_offs, uint64_t* info, hipStream_t st) {
  size_t tmp_bytes = 0;
  if (int rc = exclusive_sum_bytes<uint64_t>((size_t)slots + 1, &tmp_bytes)) return rc;
  Carve c;
  const size_t o_len = c.take(((size_t)slots + 1) * 8), o_tmp = c.take(tmp_bytes, 256);
  void* blk = nullptr;
  if (int rc = stream_scratch(dict->device, st, c.size(), &blk, SCRATCH_DICT)) return rc;
  uint64_t* lens = (uint64_t*)((char*)blk + o_len);
  if (poison_mode()) { if (int rc = poison_fill(lens, ((size_t)slots + 1) * 8, PZ_ROWS, st)) return rc; }
  HIP_TRY(hipMemsetAsync(info, 0, 16, st));
  const uint32_t blocks = (uint32_t)std::min<uint64_t>((slots + kDictThreads) / kDictThreads, 4096u);
  hipLaunchKernelGGL(dict_lengths_kernel, dim3(blocks), dim3(kDictThreads), 0, st, dict->view, ids, counts, row_offs, n_rows, row, slots, lens,
                     (unsigned long long*)info);
  HIP_TRY(hipGetLastError());
  if (int rc = device_exclusive_sum((char*)blk + o_tmp, tmp_bytes, (const uint64_t*)lens, text_offs, (size_t)slots + 1, st)) return rc;
  HIP_TRY(hipMemcpyAsync(info, text_offs + slots, 8, hipMemcpyDeviceToDevice, st));
  return SG_OK;
}

int dict_gather_enqueue(const sg_dictionary* dict, const uint32_t* ids, const uint64_t* text_offs, uint64_t slots, uint8_t* text, uint64_t text_cap,
                        hipStream_t st) {
  if (slots == 0) return SG_OK;
  const uint32_t blocks = (uint32_t)std::min<uint64_t>((slots * kDictSub + kDictThreads - 1) / kDictThreads, 4096u);
  hipLaunchKernelGGL(dict_gather_kernel, dim3(blocks), dim3(kDictThreads), 0, st, dict->view, ids, text_offs, slots, text, text_cap);
  HIP_TRY(hipGetLastError());
  return SG_OK;
}

// The second half of a host-buffer route, on `st` behind dict_offsets_enqueue: the first wait (info through pinned memory), then
// — where every id is inside and the text fits — the text block, the gather and the copy of the text to the caller's buffer,
// enqueued.  *status: SG_OK or the SG_E_INVALID the route answers once its rows are out (the error text is set here).
int dict_text_enqueue(const sg_dictionary* dict, const uint32_t* d_ids, const uint64_t* d_text_offs, const uint64_t* d_info, uint64_t slots,
                      uint8_t* text, uint64_t text_cap, uint64_t* needed, int* status, hipStream_t st) {
  DictThread& T = t_dict;
  if (int rc = T.pin.grow(16)) return rc;
  HIP_TRY(hipMemcpyAsync(T.pin.p, d_info, 16, hipMemcpyDeviceToHost, st));
  HIP_TRY(hipStreamSynchronize(st));
  const uint64_t need = ((const uint64_t*)T.pin.p)[0], outside = ((const uint64_t*)T.pin.p)[1];
  if (needed) *needed = need;
  *status = SG_OK;
  if (outside) { set_error("docID outside the dictionary"); *status = SG_E_INVALID; return SG_OK; }
  if (need > text_cap) { set_error("text buffer too small"); *status = SG_E_INVALID; return SG_OK; }
  if (need == 0) return SG_OK;
  if (!text) { set_error("null argument"); *status = SG_E_INVALID; return SG_OK; }
  uint8_t* d_text = nullptr;
  if (int rc = T.text_block(dict->device, need, text_cap, &d_text)) return rc;
  if (poison_mode()) { if (int rc = poison_fill(d_text, (size_t)need, PZ_ROWS, st)) return rc; }
  if (int rc = dict_gather_enqueue(dict, d_ids, d_text_offs, slots, d_text, need, st)) return rc;
  HIP_TRY(hipMemcpyAsync(text, d_text, (size_t)need, hipMemcpyDeviceToHost, st));
  return SG_OK;
}

// the host-resident handle: the reference's loop
int dict_rows_host(const sg_dictionary* dict, const uint32_t* ids, const uint32_t* counts, const uint64_t* row_offs, uint32_t n_rows, uint32_t row,
                   uint64_t slots, uint8_t* text, uint64_t text_cap, uint64_t* text_offs, uint64_t* needed) {
  // the offsets in one pass over the slots (the rows lie one behind the other: row_offs does not decrease), the bytes in a second
  uint64_t outside = 0, at = 0, s = 0;
  for (uint32_t i = 0; i < n_rows; i++) {
    const uint64_t b = row_offs ? row_offs[i] : (uint64_t)i * row, e = row_offs ? row_offs[i + 1] : b + row;
    for (; s < b && s < slots; s++) text_offs[s] = at;                       // (slots of no row, the last row's slots past its count)
    const uint64_t n = counts[i] >= kCountFlagMin ? 0 : std::min<uint64_t>(counts[i], e - b);
    for (; s < b + n && s < slots; s++) {
      text_offs[s] = at;
      const uint32_t id = ids[s];
      if (id >= dict->n_docs) { outside++; continue; }
      at += dict->h_offs[(size_t)id + 1] - dict->h_offs[id];
    }
  }
  for (; s < slots; s++) text_offs[s] = at;
  text_offs[slots] = at;
  if (needed) *needed = at;
  if (outside) { set_error("docID outside the dictionary"); return SG_E_INVALID; }
  if (at > text_cap) { set_error("text buffer too small"); return SG_E_INVALID; }
  if (at && !text) { set_error("null argument"); return SG_E_INVALID; }
  for (s = 0; s < slots; s++)
    if (text_offs[s + 1] > text_offs[s]) memcpy(text + text_offs[s], dict->h_blob.data() + dict->h_offs[ids[s]], (size_t)(text_offs[s + 1] - text_offs[s]));
  return SG_OK;
}

// a handle from strings in docID order; value(i, &len) = the bytes of string i
int dictionary_make(size_t n, const std::function<const uint8_t*(size_t, uint64_t*)>& value, int device, sg_dictionary** out) {
  if (n > 0xFFFFFFFFull) { set_error("dictionary: more than 2^32 - 1 strings"); return SG_E_UNSUPPORTED; }
  std::unique_ptr<sg_dictionary> d(new sg_dictionary);
  d->n_docs = (uint32_t)n;
  d->h_offs.resize(n + 1);
  uint64_t at = 0;
  for (size_t i = 0; i < n; i++) {
    uint64_t len = 0;
    (void)value(i, &len);
    if (len > 0xFFFFFFFFull) { set_error("dictionary: a string of 4 GiB or more"); return SG_E_UNSUPPORTED; }
    d->h_offs[i] = at; at += len;
    d->max_len = std::max(d->max_len, (uint32_t)len);
  }
  d->h_offs[n] = at;
  d->bytes = at;
  d->h_blob.resize((size_t)at);
  for (size_t i = 0; i < n; i++) {
    uint64_t len = 0;
    const uint8_t* p = value(i, &len);
    if (len) memcpy(d->h_blob.data() + d->h_offs[i], p, (size_t)len);
  }
  if (device >= 0) {
    int n_dev = 0;
    HIP_TRY(hipGetDeviceCount(&n_dev));
    if (device >= n_dev) { set_error("no such device"); return SG_E_INVALID; }
    DeviceGuard dg;
    HIP_TRY(dg.set(device));
    d->device = device;
    if (int rc = d->mem.upload(d->h_offs, &d->view.doc_offs)) return rc;
    if (int rc = d->mem.upload(d->h_blob, &d->view.blob)) return rc;
    d->view.n_docs = d->n_docs;
    std::vector<uint32_t> lf, lt;
    for (const auto& pr : kLowerPairs) { lf.push_back(pr.from); lt.push_back(pr.to); }
    if (int rc = d->mem.upload(lf, &d->d_lower_from)) return rc;
    if (int rc = d->mem.upload(lt, &d->d_lower_to)) return rc;
    d->n_lower = (uint32_t)lf.size();
    std::vector<uint64_t>().swap(d->h_offs);    // (the device copy is the dictionary: no second one on the host)
    std::vector<uint8_t>().swap(d->h_blob);
  }
  *out = d.release();
  return SG_OK;
}

int dict_check_rows_args(const sg_dictionary* dict, const void* ids, const void* counts, const void* row_offs, uint32_t n_rows, uint32_t row,
                         uint64_t slots, const void* text_offs) {
  if (!dict) { set_error("null dictionary"); return SG_E_INVALID; }
  if (!text_offs || (n_rows && !counts) || (slots && n_rows && !ids)) { set_error("null argument"); return SG_E_INVALID; }
  return dict_check_geometry(row_offs, n_rows, row, slots);
}

// sg_dictionary_rows on a device handle: the rows go in (row_offs null: an empty region); the slots + 1 text offsets come back (the
// scan writes every one: poisoned, never cleared); the step's two info words stay in the block — dict_text_enqueue reads them at
// its own wait.  The text itself is not part of the block.
enum { DR_TEXT_OFFS = 0, DR_INFO, DR_ROW_OFFS, DR_IDS, DR_COUNTS };
IoCall dict_rows_io(const uint32_t* ids, const uint32_t* counts, const uint64_t* row_offs, uint32_t n_rows, uint64_t slots, uint64_t* text_offs) {
  return IoCall().add(IO_OUT, text_offs, ((size_t)slots + 1) * 8, 8, false, PZ_OUT_IDS).add(IO_OUT, nullptr, 16, 8)
      .add(IO_IN, row_offs, row_offs ? ((size_t)n_rows + 1) * 8 : 0, 16).add(IO_IN, ids, (size_t)slots * 4, 16).add(IO_IN, counts, (size_t)n_rows * 4, 16);
}

// sg_suggest_batch_strings / sg_autocomplete_batch_strings: the plain call's staging, launch and copy-out, with the materialise
// step between the launch and the copy-out
int strings_host_call(sg_index* index, const uint8_t* q, const uint64_t* offs, uint32_t n_q, const LaunchReq& r, uint32_t* ids, double* scores,
                      uint32_t* counts, sg_dictionary* dict, uint8_t* text, uint64_t text_cap, uint64_t* text_offs, uint64_t* needed) {
  if (!dict) { set_error("null dictionary"); return SG_E_INVALID; }
  if (!text_offs) { set_error("null argument"); return SG_E_INVALID; }
  Replica* rep = find_replica(index, -1);
  if (dict->device != rep->device) { set_error("the dictionary is not on the device of the index's primary replica"); return SG_E_UNSUPPORTED; }
  const uint64_t slots = (uint64_t)n_q * r.k;
  if (int rc = dict_check_geometry(nullptr, n_q, r.k, slots)) return rc;
  if (needed) *needed = 0;
  if (n_q == 0) { text_offs[0] = 0; return SG_OK; }
  // a search's regions and, behind its rows in the one copy back, the text offsets and the step's two info words
  const IoCall call = search_io(q, offs, n_q, slots, ids, r.autocomplete ? nullptr : scores, counts, nullptr, true, text_offs);
  const Enqueue search = search_enqueue(index, rep, r, offs, n_q);
  int status = SG_OK;        // (answered once the rows are out; the step's error text stands: nothing behind it sets one unless it fails)
  const int rc = run_host_call(rep->device, call, [&](const IoCall& io, hipStream_t st) -> int {
    if (int rc2 = search(io, st)) return rc2;
    if (int rc2 = dict_offsets_enqueue(dict, io.at<uint32_t>(IO_IDS), io.at<uint32_t>(IO_COUNTS), nullptr, n_q, r.k, slots, io.at<uint64_t>(IO_TEXT_OFFS),
                                       io.at<uint64_t>(IO_INFO), st)) return rc2;
    return dict_text_enqueue(dict, io.at<uint32_t>(IO_IDS), io.at<uint64_t>(IO_TEXT_OFFS), io.at<uint64_t>(IO_INFO), slots, text, text_cap, needed, &status, st);
  });
  return rc ? rc : status;
}

}  // namespace

extern "C" {

int sg_dictionary_upload(const uint8_t* utf8, const uint64_t* offs, uint32_t n_docs, int device, sg_dictionary** out) {
  SG_GUARD_BEGIN
  if (!out || !offs || (!utf8 && n_docs && offs[n_docs] > offs[0])) { set_error("null argument"); return SG_E_INVALID; }
  for (uint32_t i = 0; i < n_docs; i++)
    if (offs[i + 1] < offs[i]) { set_error("document offsets must not decrease"); return SG_E_INVALID; }
  return dictionary_make(n_docs, [&](size_t i, uint64_t* len) { *len = offs[i + 1] - offs[i]; return utf8 + offs[i]; }, device, out);
  SG_GUARD_END(SG_RC)
}

int sg_dictionary_open_cdb(const char* cdb_path, int device, sg_dictionary** out) {
  SG_GUARD_BEGIN
  if (!out || !cdb_path) { set_error("null argument"); return SG_E_INVALID; }
  std::vector<std::string> words;
  std::string err;
  if (!read_cdb_words(cdb_path, words, err)) { set_error(err); return SG_E_INVALID; }
  return dictionary_make(words.size(), [&](size_t i, uint64_t* len) { *len = words[i].size(); return (const uint8_t*)words[i].data(); }, device, out);
  SG_GUARD_END(SG_RC)
}

void sg_dictionary_retain(sg_dictionary* d) { if (d) d->refs.fetch_add(1); }
void sg_dictionary_release(sg_dictionary* d) {
  if (!d) return;
  if (d->refs.fetch_sub(1) != 1) return;
  delete d;                                                // the DeviceBlock frees its HBM
}
uint32_t sg_dictionary_size(const sg_dictionary* d) { return d ? d->n_docs : 0; }
uint64_t sg_dictionary_bytes(const sg_dictionary* d) { return d ? d->bytes : 0; }
uint32_t sg_dictionary_max_len(const sg_dictionary* d) { return d ? d->max_len : 0; }
int sg_dictionary_device(const sg_dictionary* d) { return d ? d->device : -1; }

int sg_dictionary_rows_device(sg_dictionary* dict, const void* d_ids, const void* d_counts, const void* d_row_offs, uint32_t n_rows, uint32_t row,
                              uint64_t slots, void* d_text, uint64_t text_cap, void* d_text_offs, void* d_info, void* stream) {
  SG_GUARD_BEGIN
  if (int rc = dict_check_rows_args(dict, d_ids, d_counts, d_row_offs, n_rows, row, slots, d_text_offs)) return rc;
  if (!d_info || (!d_text && text_cap)) { set_error("null argument"); return SG_E_INVALID; }
  if (dict->device < 0) { set_error("a host-resident dictionary cannot serve a device call"); return SG_E_UNSUPPORTED; }
  DeviceGuard dg;
  HIP_TRY(dg.set(dict->device));
  hipStream_t st = (hipStream_t)stream;
  if (int rc = dict_offsets_enqueue(dict, (const uint32_t*)d_ids, (const uint32_t*)d_counts, (const uint64_t*)d_row_offs, n_rows, row, slots,
                                    (uint64_t*)d_text_offs, (uint64_t*)d_info, st)) return rc;
  return dict_gather_enqueue(dict, (const uint32_t*)d_ids, (const uint64_t*)d_text_offs, slots, (uint8_t*)d_text, text_cap, st);
  SG_GUARD_END(SG_RC)
}

int sg_dictionary_rows(sg_dictionary* dict, const uint32_t* ids, const uint32_t* counts, const uint64_t* row_offs, uint32_t n_rows, uint32_t row,
                       uint64_t slots, uint8_t* text, uint64_t text_cap, uint64_t* text_offs, uint64_t* needed) {
  SG_GUARD_BEGIN
  if (int rc = dict_check_rows_args(dict, ids, counts, row_offs, n_rows, row, slots, text_offs)) return rc;
  if (row_offs) for (uint32_t i = 0; i < n_rows; i++)
    if (row_offs[i + 1] < row_offs[i]) { set_error("row offsets must not decrease"); return SG_E_INVALID; }
  if (dict->device < 0) return dict_rows_host(dict, ids, counts, row_offs, n_rows, row, slots, text, text_cap, text_offs, needed);
  if (n_rows == 0 || slots == 0) { std::fill(text_offs, text_offs + slots + 1, 0); if (needed) *needed = 0; return SG_OK; }   // (no entry)
  int status = SG_OK;        // (as in strings_host_call)
  const int rc = run_host_call(dict->device, dict_rows_io(ids, counts, row_offs, n_rows, slots, text_offs), [&](const IoCall& io, hipStream_t st) -> int {
    if (int rc2 = dict_offsets_enqueue(dict, io.at<uint32_t>(DR_IDS), io.at<uint32_t>(DR_COUNTS), row_offs ? io.at<uint64_t>(DR_ROW_OFFS) : nullptr, n_rows, row, slots,
                                       io.at<uint64_t>(DR_TEXT_OFFS), io.at<uint64_t>(DR_INFO), st)) return rc2;
    return dict_text_enqueue(dict, io.at<uint32_t>(DR_IDS), io.at<uint64_t>(DR_TEXT_OFFS), io.at<uint64_t>(DR_INFO), slots, text, text_cap, needed, &status, st);
  });
  return rc ? rc : status;
  SG_GUARD_END(SG_RC)
}

int sg_suggest_batch_strings(sg_index* index, const uint8_t* q, const uint64_t* offs, uint32_t n_q, int metric, double similarity, uint32_t k,
                             uint32_t* ids, double* scores, uint32_t* counts, sg_dictionary* dict, uint8_t* text, uint64_t text_cap,
                             uint64_t* text_offs, uint64_t* needed) {
  SG_GUARD_BEGIN
  const SearchKey c = fuzzy_key(metric, similarity, k);
  if (int rc = open_search(index, c, true, {offs, ids, scores, counts})) return rc;
  return strings_host_call(index, q, offs, n_q, search_req(c), ids, scores, counts, dict, text, text_cap, text_offs, needed);
  SG_GUARD_END(SG_RC)
}

int sg_autocomplete_batch_strings(sg_index* index, const uint8_t* q, const uint64_t* offs, uint32_t n_q, uint32_t limit, uint32_t* ids,
                                  uint32_t* counts, sg_dictionary* dict, uint8_t* text, uint64_t text_cap, uint64_t* text_offs, uint64_t* needed) {
  SG_GUARD_BEGIN
  const SearchKey c = prefix_key(limit);
  if (int rc = open_search(index, c, false, {offs, ids, counts})) return rc;
  return strings_host_call(index, q, offs, n_q, search_req(c), ids, nullptr, counts, dict, text, text_cap, text_offs, needed);
  SG_GUARD_END(SG_RC)
}

}  // extern "C"
