// The B-spline basis on the device: the clipped linear phase and the Cox-de Boor recursion, the one
// definition k_basis (fit.hip) and the per-trajectory fit (fit_rows.hip) evaluate.  The library is
// built with -ffp-contract=off and IEEE fp32 division, so both get the same bits (the reference's
// fp32 recursion, uni_bspline_basis.py:82-113).
#pragma once

#include <hip/hip_runtime.h>

namespace {

// linear_phase.py:22-24: clip((t - delay) / tau, 0, 1); a NaN time stays NaN
__device__ __forceinline__ float phase_clip(float t, float tau, float delay) {
  float u = __fdiv_rn(__fsub_rn(t, delay), tau);
  u = (u < 0.0f) ? 0.0f : u;
  return (1.0f < u) ? 1.0f : u;
}

template <int K>
__device__ float bfun(int i, float u, const float* __restrict__ kv, int nctrl) {
  if constexpr (K == 0) {
    const float a = kv[i], b = kv[i + 1];
    const bool in = (i == nctrl - 1) ? (u >= a && u <= b) : (u >= a && u < b);
    return in ? 1.0f : 0.0f;
  } else {
    const float d1 = __fsub_rn(kv[i + K], kv[i]);
    const float d2 = __fsub_rn(kv[i + K + 1], kv[i + 1]);
    float t1 = 0.0f, t2 = 0.0f;
    if (!(d1 == 0.0f)) t1 = __fmul_rn(__fdiv_rn(__fsub_rn(u, kv[i]), d1), bfun<K - 1>(i, u, kv, nctrl));
    if (!(d2 == 0.0f)) t2 = __fmul_rn(__fdiv_rn(__fsub_rn(kv[i + K + 1], u), d2), bfun<K - 1>(i + 1, u, kv, nctrl));
    return __fadd_rn(t1, t2);
  }
}

}  // namespace
