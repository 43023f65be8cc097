// Host-only launch layer of codec.hip and deriv.hip: the stream's device, its CU count, the grid
// of a tile-walking kernel, the diagnostic knobs, and launch_fn -- the one path by which these two
// files start a kernel and report a failure.  Knows nothing of the codec's argument types.
#pragma once

#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <cstdint>
#include <cstdlib>

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

// What launch_fn remembers of one kernel, per device.  Entries are atomics: the first launches on
// a device may race from several host threads, and every racer stores the same values.
struct FnCache {
  std::atomic<hipFunction_t> fn[16];
  std::atomic<bool> big_lds[16];   // dynamic LDS above 64 KB has been granted (up to the CU's 160 KB)
};

// Host launch of a kernel through hipModuleLaunchKernel with a cached function handle: the
// runtime skips hipLaunchKernel's host-function lookup and the GGL template's argument packing,
// ≈0.15 us of host time per launch (profiles/r02/launch_host_cost.json).  The handle is the one
// of the STREAM's device (hipGetFuncBySymbol resolves for the current device, so it is looked up
// under a guard that makes the stream's device current); the first launch that asks for more
// than 64 KB of dynamic LDS raises the kernel's limit under the same guard.
template <class... Args>
int launch_fn(const void* kernel, FnCache& cache, unsigned grid, unsigned block, unsigned lds, const Queue& q,
              const char* what, Args... args) {
  const bool cached = q.dev >= 0 && q.dev < 16;
  hipFunction_t f = cached ? cache.fn[q.dev].load(std::memory_order_acquire) : nullptr;
  const bool grant = lds > 65536 && !(cached && cache.big_lds[q.dev].load(std::memory_order_acquire));
  if (f == nullptr || grant) {
    int cur = 0;
    BEAST_HIP(hipGetDevice(&cur), what);
    if (cur != q.dev) BEAST_HIP(hipSetDevice(q.dev), what);
    hipError_t e = hipGetFuncBySymbol(&f, kernel);
    if (e == hipSuccess && grant)
      e = hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
    if (cur != q.dev) BEAST_HIP(hipSetDevice(cur), what);
    BEAST_HIP(e, what);
    if (cached) {
      cache.fn[q.dev].store(f, std::memory_order_release);
      if (grant) cache.big_lds[q.dev].store(true, std::memory_order_release);
    }
  }
  void* params[] = {static_cast<void*>(&args)...};
  BEAST_HIP(hipModuleLaunchKernel(f, grid, 1, 1, block, 1, 1, lds, q.s, params, nullptr), what);
  return BEAST_OK;
}

}  // namespace
