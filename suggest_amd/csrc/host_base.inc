// host_base.inc — what every host file of libsuggest_hip stands on: the thread's error text, HIP_TRY and the extern "C" guards,
// DeviceGuard, DeviceBlock (the owner of held device memory) and the hipcub scan / sort helpers.  First of the host files
// engine.hip includes; it uses sg_internal.h alone.

#include <hipcub/hipcub.hpp>

// ------------------------------------------------------------------------------------------
// host side: handle, replicas, launches
// ------------------------------------------------------------------------------------------
namespace sg {
static thread_local std::string g_err;
void set_error(const std::string& m) { g_err = m; }
}  // namespace sg

using namespace sg;

#define HIP_TRY(expr)                                                                   \
  do {                                                                                  \
    hipError_t e_ = (expr);                                                             \
    if (e_ != hipSuccess) {                                                             \
      set_error(std::string(#expr) + ": " + hipGetErrorString(e_));                     \
      return SG_E_HIP;                                                                  \
    }                                                                                   \
  } while (0)

// Every extern "C" body runs inside this pair: no C++ exception crosses the C boundary (a cgo caller would abort).
#define SG_GUARD_BEGIN try {
#define SG_GUARD_END(on_fail)                                                           \
  } catch (const std::bad_alloc&) { set_error("out of host memory"); return on_fail(SG_E_NOMEM); } \
  catch (const std::exception& e_) { set_error(std::string("internal error: ") + e_.what()); return on_fail(SG_E_INVALID); }
#define SG_RC(x) (x)

// Makes a device the calling thread's current one for the rest of a scope and puts the previous one back at its end:
// `DeviceGuard dg; HIP_TRY(dg.set(device));`
struct DeviceGuard {
  int prev = -1, cur = -1;
  hipError_t set(int device) {
    if (prev < 0) {
      const hipError_t e = hipGetDevice(&prev);
      if (e != hipSuccess) { prev = -1; return e; }
      cur = prev;
    }
    if (device == cur) return hipSuccess;
    const hipError_t e = hipSetDevice(device);
    if (e == hipSuccess) cur = device;
    return e;
  }
  ~DeviceGuard() { if (prev >= 0 && cur != prev) (void)hipSetDevice(prev); }
};

// The one owner of device memory that is held, not reused (reuse buffers are GrowBlocks, below): a replica's arrays, a language
// model's tables, metric tables, the working memory of a build / store / load call.  Its blocks live on the device that was current
// at the first alloc(); the destructor frees them with that device current and puts the caller's back.  Movable: "commit on
// success" is to build in a local DeviceBlock and move it into the handle as the last step.  A failed hipMalloc is SG_E_NOMEM.
struct DeviceBlock {
  struct Block { void* p; size_t bytes; };
  std::vector<Block> blocks;
  int device = -1;
  uint64_t sum = 0;
  DeviceBlock() = default;
  DeviceBlock(DeviceBlock&& o) noexcept { swap(o); }
  DeviceBlock& operator=(DeviceBlock&& o) noexcept { clear(); swap(o); return *this; }
  ~DeviceBlock() { clear(); }
  void swap(DeviceBlock& o) { blocks.swap(o.blocks); std::swap(device, o.device); std::swap(sum, o.sum); }
  void clear() {
    if (blocks.empty()) return;
    DeviceGuard dg;
    if (dg.set(device) == hipSuccess) for (const Block& b : blocks) (void)hipFree(b.p);
    blocks.clear(); sum = 0;
  }
  template <class T> int alloc(T** out, size_t n) {   // n elements, 16 bytes at least
    if (device < 0) HIP_TRY(hipGetDevice(&device));
    void* p = nullptr;
    const size_t bytes = std::max<size_t>(n * sizeof(T), 16);
    const hipError_t e = hipMalloc(&p, bytes);
    if (e != hipSuccess) { set_error(std::string("hipMalloc: ") + hipGetErrorString(e)); return SG_E_NOMEM; }
    blocks.push_back(Block{p, bytes});
    sum += bytes;
    *out = (T*)p;
    return SG_OK;
  }
  // a block holding src[0 .. n): copied before the call returns, or on `st` when one is given (the caller synchronises it)
  template <class T> int upload(const T* src, size_t n, const T** out, hipStream_t st = nullptr) {
    T* p = nullptr;
    if (int rc = alloc(&p, n)) return rc;
    if (n && st) HIP_TRY(hipMemcpyAsync(p, src, n * sizeof(T), hipMemcpyHostToDevice, st));
    else if (n) HIP_TRY(hipMemcpy(p, src, n * sizeof(T), hipMemcpyHostToDevice));
    *out = p;
    return SG_OK;
  }
  template <class T> int upload(const std::vector<T>& src, const T** out, hipStream_t st = nullptr) { return upload(src.data(), src.size(), out, st); }
  const Block* find(const void* p) const { for (const Block& b : blocks) if (b.p == p) return &b; return nullptr; }
  size_t bytes_of(const void* p) const { const Block* b = find(p); return b ? b->bytes : 0; }   // 0: not a block of this owner
  uint64_t total() const { return sum; }
  void release(const void* p) {   // frees one block (null or unknown: nothing)
    const Block* b = p ? find(p) : nullptr;
    if (!b) return;
    DeviceGuard dg;
    if (dg.set(device) == hipSuccess) (void)hipFree(b->p);
    sum -= b->bytes;
    blocks.erase(blocks.begin() + (b - blocks.data()));
  }
};

// hipcub's two-call idiom, once: ask for the working memory's size, take it from `mem` (it goes when `mem` goes), run.  A loop that
// runs one sort or scan many times over one working block (lm_build.inc, lm_store.inc) calls hipcub itself.
template <class T>
int device_exclusive_sum(DeviceBlock& mem, const T* in, T* out, size_t n, hipStream_t st = nullptr) {
  size_t tb = 0;
  HIP_TRY(hipcub::DeviceScan::ExclusiveSum(nullptr, tb, in, out, (int)n, st));
  uint8_t* tmp;
  if (int rc = mem.alloc(&tmp, tb)) return rc;
  HIP_TRY(hipcub::DeviceScan::ExclusiveSum(tmp, tb, in, out, (int)n, st));
  return SG_OK;
}
// ... over working memory the caller holds already (a call on a caller's stream takes it from its scratch block: nothing is
// allocated or freed while the stream runs): exclusive_sum_bytes says how much a scan of n elements needs
template <class T>
int exclusive_sum_bytes(size_t n, size_t* bytes) {
  *bytes = 0;
  HIP_TRY(hipcub::DeviceScan::ExclusiveSum(nullptr, *bytes, (const T*)nullptr, (T*)nullptr, (int)n, (hipStream_t) nullptr));
  return SG_OK;
}
template <class T>
int device_exclusive_sum(void* tmp, size_t tmp_bytes, const T* in, T* out, size_t n, hipStream_t st) {
  HIP_TRY(hipcub::DeviceScan::ExclusiveSum(tmp, tmp_bytes, in, out, (int)n, st));
  return SG_OK;
}
template <class K, class V>   // stable, ascending by bits [begin_bit, end_bit) of the keys
int device_sort_pairs(DeviceBlock& mem, const K* keys_in, K* keys_out, const V* vals_in, V* vals_out, size_t n, int begin_bit = 0,
                      int end_bit = 8 * (int)sizeof(K), hipStream_t st = nullptr) {
  size_t tb = 0;
  HIP_TRY(hipcub::DeviceRadixSort::SortPairs(nullptr, tb, keys_in, keys_out, vals_in, vals_out, (int)n, begin_bit, end_bit, st));
  uint8_t* tmp;
  if (int rc = mem.alloc(&tmp, tb)) return rc;
  HIP_TRY(hipcub::DeviceRadixSort::SortPairs(tmp, tb, keys_in, keys_out, vals_in, vals_out, (int)n, begin_bit, end_bit, st));
  return SG_OK;
}
// the sum of val[0 .. n) from its exclusive prefix sums: last prefix + last value (n >= 1)
template <class Out>
int device_total(const uint32_t* val, const uint32_t* pre, size_t n, Out* out) {
  uint32_t a = 0, b = 0;
  HIP_TRY(hipMemcpy(&a, val + n - 1, 4, hipMemcpyDeviceToHost));
  HIP_TRY(hipMemcpy(&b, pre + n - 1, 4, hipMemcpyDeviceToHost));
  *out = (Out)a + b;
  return SG_OK;
}

using clk = std::chrono::steady_clock;   // the stopwatch of the store / load codecs' phase times
inline double since(clk::time_point t) { return std::chrono::duration<double>(clk::now() - t).count(); }
