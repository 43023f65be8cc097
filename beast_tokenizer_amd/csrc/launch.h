// Host-only launch layer of the library: the stream's device (Queue), DeviceGuard, cu_count, the
// grid of a tile-walking kernel, the diagnostic knobs, and launch<kernel> -- the one path by which
// every translation unit starts a kernel and reports a failure.  Knows no kernel's argument types.
#pragma once

#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <cstdint>
#include <cstdlib>
#include <utility>

#include "common.h"

namespace {

// A launch's stream and the device it belongs to, queried once per C-ABI call: a tokenizer on
// cuda:1 may be called while another device is current, so nothing here asks for the current one.
struct Queue {
  hipStream_t s;
  int dev;
};
inline int queue_of(void* stream, Queue& q, const char* what) {
  q.s = beast::as_stream(stream);
  BEAST_HIP(hipStreamGetDevice(q.s, &q.dev), what);
  return BEAST_OK;
}

// Diagnostic knob: BEAST_DEBUG_PHASES=<bitmask> skips kernel phases (1 stage, 2 MFMA,
// 4 store, 8 quantise, 16 dequantise) to attribute time; default: all phases.
inline int debug_phases() {
  static const int v = [] {
    const char* e = getenv("BEAST_DEBUG_PHASES");
    return e ? atoi(e) : 0xFF;
  }();
  return v;
}

// Compute units of a device, cached per device (racing first calls store the same value).
inline int cu_count(int device) {
  static std::atomic<int> n[16] = {};
  const bool cached = device >= 0 && device < 16;
  int v = cached ? n[device].load(std::memory_order_relaxed) : 0;
  if (v == 0) {
    if (hipDeviceGetAttribute(&v, hipDeviceAttributeMultiprocessorCount, device) != hipSuccess || v <= 0) v = 256;
    if (cached) n[device].store(v, std::memory_order_relaxed);
  }
  return v;
}

// Diagnostic knob: BEAST_DEBUG_GRID_CAP=<n> caps the codec grids (tools/stamps uses it to
// give each workgroup a second tile, i.e. to time a tile with warm instruction cache).
inline int64_t debug_grid_cap() {
  static const int64_t v = [] {
    const char* e = getenv("BEAST_DEBUG_GRID_CAP");
    return e ? std::max<int64_t>(1, atoll(e)) : INT64_MAX;
  }();
  return v;
}

inline int64_t grid_for(int64_t ntiles, int lds_bytes, int device) {
  const int per_cu = std::max(1, std::min(8, (160 * 1024) / std::max(lds_bytes, 1)));
  const int64_t g = std::min<int64_t>(ntiles, (int64_t)cu_count(device) * per_cu * 2);
  return std::max<int64_t>(1, std::min(g, debug_grid_cap()));
}

// Makes `device` current for a scope, if it is not already, and restores the previous one on exit.
// status() reports a failed setup; the destructor never fails.
class DeviceGuard {
 public:
  explicit DeviceGuard(int device) {
    err_ = hipGetDevice(&prev_);
    if (err_ == hipSuccess && prev_ != device) {
      err_ = hipSetDevice(device);
      restore_ = err_ == hipSuccess;
    }
  }
  ~DeviceGuard() {
    if (restore_) (void)hipSetDevice(prev_);
  }
  DeviceGuard(const DeviceGuard&) = delete;
  DeviceGuard& operator=(const DeviceGuard&) = delete;
  hipError_t status() const { return err_; }

 private:
  int prev_ = 0;
  bool restore_ = false;
  hipError_t err_;
};

// What launch remembers of one kernel, per device.  Entries are atomics: the first launches on
// a device may race from several host threads, and every racer stores the same values.
struct FnCache {
  std::atomic<hipFunction_t> fn[16];
  std::atomic<bool> big_lds[16];   // dynamic LDS above 64 KB has been granted (up to the CU's 160 KB)
};
template <auto K>
FnCache& cache_of() {
  static FnCache c = {};
  return c;
}
template <class T>
struct same {
  using type = T;
};

// A kernel's function handle on the STREAM's device, cached.  hipGetFuncBySymbol resolves for the
// current device, so it is looked up under a guard that makes the stream's device current; the
// first request for more than 64 KB of dynamic LDS raises the kernel's limit under the same guard
// (the limit only bounds what a launch may ask for).
inline int function_of(const void* kernel, FnCache& cache, unsigned lds, const Queue& q, const char* what,
                       hipFunction_t& f) {
  const bool cached = q.dev >= 0 && q.dev < 16;
  f = cached ? cache.fn[q.dev].load(std::memory_order_acquire) : nullptr;
  const bool grant = lds > 65536 && !(cached && cache.big_lds[q.dev].load(std::memory_order_acquire));
  if (f != nullptr && !grant) return BEAST_OK;
  const DeviceGuard on(q.dev);
  BEAST_HIP(on.status(), what);
  BEAST_HIP(hipGetFuncBySymbol(&f, kernel), what);
  if (grant) {   // up to the CU's 160 KB, less what the kernel declares statically
    hipFuncAttributes fa;
    BEAST_HIP(hipFuncGetAttributes(&fa, kernel), what);
    BEAST_HIP(hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize,
                                  160 * 1024 - (int)fa.sharedSizeBytes), what);
  }
  if (cached) {
    cache.fn[q.dev].store(f, std::memory_order_release);
    if (grant) cache.big_lds[q.dev].store(true, std::memory_order_release);
  }
  return BEAST_OK;
}

// Host launch of a kernel through hipModuleLaunchKernel with the cached handle: the runtime skips
// hipLaunchKernel's host-function lookup and the GGL template's argument packing, ≈0.15 us of
// host time per launch (profiles/r02/launch_host_cost.json).  `args` are exactly the kernel's
// parameter types P..., so their addresses are what hipModuleLaunchKernel expects.  Returns the
// launch's own status.
template <class... P>
int launch_typed(void (*kernel)(P...), FnCache& cache, dim3 grid, unsigned block, unsigned lds, const Queue& q,
                 const char* what, typename same<P>::type... args) {
  hipFunction_t f;
  BEAST_TRY(function_of(reinterpret_cast<const void*>(kernel), cache, lds, q, what, f));
  void* params[] = {static_cast<void*>(&args)...};
  beast::g_last_launch_grid.store(grid.x, std::memory_order_relaxed);   // BEAST_OPT_LAST_LAUNCH_GRID
  BEAST_HIP(hipModuleLaunchKernel(f, grid.x, grid.y, grid.z, block, 1, 1, lds, q.s, params, nullptr), what);
  return BEAST_OK;
}

// launch<k>(grid, block, lds, q, "k", args...): the arguments convert to k's own parameter types
// at compile time (a wrong count or a type that does not convert is a compile error).
template <auto K, class... A>
int launch(dim3 grid, unsigned block, unsigned lds, const Queue& q, const char* what, A&&... a) {
  return launch_typed(K, cache_of<K>(), grid, block, lds, q, what, std::forward<A>(a)...);
}

// Workgroups of kernel K a CU of the stream's device holds at once at this block size and dynamic
// LDS, as launch<K> would start them (the LDS grant included); 0 when the runtime cannot say.
template <auto K>
int occupancy(int threads, unsigned lds, const Queue& q) {
  hipFunction_t f;
  int per = 0;
  if (function_of(reinterpret_cast<const void*>(K), cache_of<K>(), lds, q, "occupancy", f) != BEAST_OK) return 0;
  const DeviceGuard on(q.dev);
  if (on.status() != hipSuccess || hipOccupancyMaxActiveBlocksPerMultiprocessor(&per, K, threads, lds) != hipSuccess)
    return 0;
  return per;
}

}  // namespace
