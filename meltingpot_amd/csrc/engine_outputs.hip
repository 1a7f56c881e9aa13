// engine_outputs.hip — memory for a bound view (include/mp_engine.h: mp_alloc_output): views made
// of separately created physical chunks under one virtual range, their release, and the entry
// points torch's pluggable allocator calls.  Nothing here needs an engine.
#include <sys/types.h>

#include <map>
#include <mutex>
#include <vector>

#include "engine_state.h"

namespace {
struct MappedView { size_t bytes; size_t chunk; std::vector<hipMemGenericAllocationHandle_t> handles; };
std::map<void*, MappedView> g_mapped;   // views made of mapped chunks (plain ones are not listed)
std::mutex g_mapped_lock;
// Address space retired by released mapped views (free_output keeps their ranges reserved), and
// the bound beyond which nothing more is mapped: a process that places views for ever (a sweep
// that creates engine after engine) gets a clear error instead of an address space that silently
// fills up.  16 TiB: ~25,000 placed clean_up views.
int64_t g_retired_va = 0;
int64_t g_retired_va_limit = (int64_t)16 << 40;
}  // namespace

void retired_va(int64_t* bytes, int64_t* limit) {
  std::lock_guard<std::mutex> g(g_mapped_lock);
  if (bytes) *bytes = g_retired_va;
  if (limit) *limit = g_retired_va_limit;
}

// is `p` inside a view this library mapped?  (hipPointerGetAttributes does not know them)
bool in_mapped_view(const void* p) {
  std::lock_guard<std::mutex> g(g_mapped_lock);
  auto it = g_mapped.upper_bound(const_cast<void*>(p));
  if (it == g_mapped.begin()) return false;
  --it;
  return (const char*)p < (const char*)it->first + it->second.bytes;
}

namespace {
// undoes a partly built mapping (best effort) and reports `rc`
int mapped_failed(void* base, MappedView& v, size_t mapped, hipError_t rc, const char* what) {
  if (base) {
    if (mapped) (void)hipMemUnmap(base, mapped * v.chunk);
    (void)hipMemAddressFree(base, v.bytes);
  }
  for (auto h : v.handles) (void)hipMemRelease(h);
  (void)hipGetLastError();
  return fail(MP_ERR_HIP, "mp_alloc_output: %s failed: %s", what, hipGetErrorString(rc));
}
}  // namespace
extern "C" {

// One virtual range mapped onto separately created physical chunks: the view the frame launch
// writes evenly (a view whose physical pages lie next to each other — a contiguous extent,
// large pieces of a plain allocation — is written 25 - 45 % slower: profiles/r05_alloc_method.md;
// scattering the chunks FURTHER, pools and shuffles, added nothing there and is gone).
static int alloc_mapped(int device, uint64_t bytes, uint64_t chunk_bytes, void** out) {
  hipMemAllocationProp prop = {};
  prop.type = hipMemAllocationTypePinned;
  prop.location.type = hipMemLocationTypeDevice;
  prop.location.id = device;
  size_t gran = 0;
  HIP_TRY(hipMemGetAllocationGranularity(&gran, &prop, chunk_bytes >= (2u << 20)
                                                           ? hipMemAllocationGranularityRecommended
                                                           : hipMemAllocationGranularityMinimum));
  if (gran == 0) gran = 4096;
  MappedView v;
  v.chunk = ((size_t)chunk_bytes + gran - 1) / gran * gran;
  const size_t n = ((size_t)bytes + v.chunk - 1) / v.chunk;
  if (n > (1u << 20)) return fail(MP_ERR_INVALID, "mp_alloc_output: %zu chunks", n);
  v.bytes = n * v.chunk;
  {
    int64_t retired = 0, limit = 0;
    retired_va(&retired, &limit);
    if (retired + (int64_t)v.bytes > limit)
      return fail(MP_ERR_HIP, "mp_alloc_output: this process has retired %lld bytes of address space with "
                  "released mapped views (their ranges are never reused: stale translations); mapping %zu "
                  "more would pass the bound of %lld (mp_set_retired_va_limit) — reuse views instead of "
                  "placing new ones", (long long)retired, v.bytes, (long long)limit);
  }
  void* base = nullptr;
  hipError_t rc = hipMemAddressReserve(&base, v.bytes, v.chunk < (2u << 20) ? (2u << 20) : v.chunk, nullptr, 0);
  if (rc != hipSuccess) return mapped_failed(nullptr, v, 0, rc, "hipMemAddressReserve");
  v.handles.reserve(n);
  for (size_t i = 0; i < n; ++i) {
    hipMemGenericAllocationHandle_t h;
    rc = hipMemCreate(&h, v.chunk, &prop, 0);
    if (rc != hipSuccess) return mapped_failed(base, v, 0, rc, "hipMemCreate");
    v.handles.push_back(h);
  }
  for (size_t i = 0; i < n; ++i) {
    rc = hipMemMap((char*)base + i * v.chunk, v.chunk, 0, v.handles[i], 0);
    if (rc != hipSuccess) return mapped_failed(base, v, i, rc, "hipMemMap");
  }
  hipMemAccessDesc acc = {};
  acc.location.type = hipMemLocationTypeDevice;
  acc.location.id = device;
  acc.flags = hipMemAccessFlagsProtReadWrite;
  rc = hipMemSetAccess(base, v.bytes, &acc, 1);
  if (rc != hipSuccess) return mapped_failed(base, v, n, rc, "hipMemSetAccess");
  {
    std::lock_guard<std::mutex> g(g_mapped_lock);
    g_mapped[base] = v;
  }
  *out = base;
  return MP_OK;
}

int mp_alloc_output(int device, uint64_t bytes, uint64_t chunk_bytes, void** out) {
  if (!out || bytes == 0) return fail(MP_ERR_INVALID, "mp_alloc_output: bad argument");
  *out = nullptr;
  HIP_TRY(hipSetDevice(device));
  if (chunk_bytes == 0) {
    const hipError_t rc = hipMalloc(out, (size_t)bytes);
    if (rc != hipSuccess) {
      (void)hipGetLastError();
      *out = nullptr;
      return fail(MP_ERR_HIP, "mp_alloc_output: hipMalloc of %llu bytes failed: %s",
                  (unsigned long long)bytes, hipGetErrorString(rc));
    }
    return MP_OK;
  }
  return alloc_mapped(device, bytes, chunk_bytes, out);
}

}  // extern "C"

// The physical chunks go back to the driver; the VIRTUAL range stays reserved and is
// never handed out again (`keep_va`, always true in this library).  Measured on this
// stack (ROCm 7.2, gfx950): a range released with hipMemAddressFree is reused by the next
// hipMemAddressReserve, and kernels then write through translations of the OLD mapping —
// a second placed view came back with 267 - 1030 of 1030 worlds stale, no error anywhere
// (tools/gpu_r04_dbg_place.py).  Address space is not scarce (a placement retires
// ~12 x the view's size of it); correctness is.
int free_output(int device, void* ptr, bool keep_va) {
  if (!ptr) return MP_OK;
  HIP_TRY(hipSetDevice(device));
  MappedView v;
  bool mapped = false;
  {
    std::lock_guard<std::mutex> g(g_mapped_lock);
    auto it = g_mapped.find(ptr);
    if (it != g_mapped.end()) { v = it->second; g_mapped.erase(it); mapped = true; }
  }
  if (!mapped) {
    HIP_TRY(hipFree(ptr));   // (waits for the device's work on the buffer)
    return MP_OK;
  }
  // best effort: whatever fails, the rest is still released
  hipError_t first = hipDeviceSynchronize(), rc = hipMemUnmap(ptr, v.bytes);
  if (first == hipSuccess) first = rc;
  for (auto h : v.handles) {
    rc = hipMemRelease(h);
    if (first == hipSuccess) first = rc;
  }
  if (!keep_va) {
    rc = hipMemAddressFree(ptr, v.bytes);
    if (first == hipSuccess) first = rc;
  } else {
    std::lock_guard<std::mutex> g(g_mapped_lock);
    g_retired_va += (int64_t)v.bytes;
  }
  if (first != hipSuccess) {
    (void)hipGetLastError();
    return fail(MP_ERR_HIP, "mp_free_output: %s", hipGetErrorString(first));
  }
  return MP_OK;
}

extern "C" {

int mp_free_output(int device, void* ptr) { return free_output(device, ptr, true); }

// torch.cuda.memory.CUDAPluggableAllocator entry points (meltingpot_amd/memory.py): tensors a
// caller allocates inside `memory.mapped_allocations()` — a learner's own rollout buffers —
// come from scattered 2 MB chunks like the engine's own views (32 MB and up; below that an
// ordinary hipMalloc).  NULL on failure, as the allocator interface expects.
void* mp_torch_alloc(ssize_t size, int device, void* stream) {
  (void)stream;
  void* p = nullptr;
  if (size <= 0) return nullptr;
  if (mp_alloc_output(device, (uint64_t)size, size >= (ssize_t)(32 << 20) ? (2u << 20) : 0, &p) != MP_OK)
    return nullptr;
  return p;
}

void mp_torch_free(void* ptr, ssize_t size, int device, void* stream) {
  (void)size; (void)stream;
  (void)free_output(device, ptr, true);
}

int mp_set_retired_va_limit(int64_t bytes) {
  if (bytes < 0) return fail(MP_ERR_INVALID, "mp_set_retired_va_limit: %lld", (long long)bytes);
  std::lock_guard<std::mutex> g(g_mapped_lock);
  g_retired_va_limit = bytes;
  return MP_OK;
}

}  // extern "C"
