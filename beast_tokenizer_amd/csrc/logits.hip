// Decode from logits for gfx950 (beast_logits_expect, beast_logits_expect_bwd): the expected
// normalised coefficient of a token under softmax(logits / tau), its greedy bin, and the adjoint.
//
//   k_logits_expect      zmax = lmax / tau, e_v = exp(l_v / tau - zmax), s = sum_v e_v,
//                        mean = clamp(sum_v e_v (2v - (V-1)) / (s (V-1)), -1, 1),
//                        amax = the lowest v with l_v == lmax
//   k_logits_expect_bwd  grad_l_v = (g / tau) (e_v / s) (x_v - mean),  x_v = (2v - (V-1)) / (V-1)
//
// Both are bandwidth-bound row kernels: the logits are the only large tensor and every element is
// read once per direction.  One wave owns a token row at a time.  A lane owns 16 bytes of
// consecutive elements of a chunk (4 fp32, 8 half / bf16) and a chunk is one wave-load, so element
// v of a row always belongs to lane (v / EPL) % 64: whether a row is read with 16-byte loads (its
// address is 16-byte aligned) or element by element (it is not, or the lane's piece crosses the
// row's end), the lanes hold the same elements and every sum has the same order.  A lane adds its
// elements in ascending order, the lanes of a 16-lane row are combined with DPP moves (xor 1,
// xor 2, half-row mirror, row mirror: every lane of the row ends with the same value) and the four
// row results in lane order, ((r0 + r1) + (r2 + r3)): no LDS, no atomics, and an order fixed by
// (V, element type) alone.  A row's outputs are therefore bitwise the same alone or in a batch,
// at any alignment, in any grid and from run to run.
//
// Rows of up to LG_MAX_CHUNKS chunks are held in registers: the exact maximum first, then one
// pass of exp.  Longer rows take the online form: every lane keeps a running maximum of its own
// elements and rescales its two sums when it grows; the lanes are brought to the row's maximum
// before they are combined.  A wave works on R rows at once (register form), or on LG_ONLINE_U
// chunks of one row (online form), so that several 16-byte loads are in flight per lane.
// e_v is computed as exp2((l_v * (1/tau) - zmax) * log2 e) with the product and the difference in
// one fma, in the forward and in the backward alike: zmax (stats[0]) is the only thing the
// backward needs to reproduce the forward's e_v.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <cmath>
#include <cstdint>
#include <cstdlib>

#include "common.h"
#include "launch.h"

namespace {

constexpr int LG_THREADS = 256;
constexpr int LG_WAVES = LG_THREADS / 64;
constexpr int LG_MAX_CHUNKS = 4;     // rows of up to this many wave-loads stay in registers
constexpr int LG_ONLINE_U = 4;       // online form: chunks loaded before any of them is used
constexpr int LG_MIN_V = 2;
constexpr int LG_MAX_V = 65536;
constexpr float LG_LOG2E = 1.44269504088896340736f;

// ------------------------------------------------------------------ element types --
struct ElemF32 {
  using raw = float;
  static constexpr int EPL = 4;
  static __device__ __forceinline__ float load(raw r) { return r; }
  static __device__ __forceinline__ raw store(float f) { return f; }
};
struct ElemF16 {
  using raw = _Float16;
  static constexpr int EPL = 8;
  static __device__ __forceinline__ float load(raw r) { return (float)r; }
  static __device__ __forceinline__ raw store(float f) { return (_Float16)f; }   // round to nearest even
};
struct ElemBF16 {
  using raw = uint16_t;
  static constexpr int EPL = 8;
  static __device__ __forceinline__ float load(raw r) { return __uint_as_float((uint32_t)r << 16); }
  static __device__ __forceinline__ raw store(float f) {                         // round to nearest even
    const uint32_t u = __float_as_uint(f);
    if (f != f) return (raw)((u >> 16) | 0x40u);                                 // a quiet NaN stays one
    return (raw)((u + 0x7FFFu + ((u >> 16) & 1u)) >> 16);
  }
};

struct LogitsArgs {
  const void* logits;
  int64_t sb, sk;        // element strides of the batch and the token axis
  int64_t rows;          // B * K
  int64_t K;             // tokens per batch element; `rows` (one batch element) where sb == K * sk
  int64_t gK;            // the same for grad_logits' strides
  int V;
  float inv_tau;         // 1 / tau
  float vm1;             // V - 1
  int64_t tok_offset;
  float* mean;           // forward: out (nullable); backward: in
  int64_t* amax;
  float* stats;          // forward: out (nullable); backward: in
  // backward only
  const float* grad_mean;
  void* grad;
  int64_t gsb, gsk;
};

// ------------------------------------------------------------- wave-level reductions --
template <int CTRL>
__device__ __forceinline__ float dpp_f(float x) {
  return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(x), CTRL, 0xF, 0xF, true));
}
template <int CTRL>
__device__ __forceinline__ int dpp_i(int x) {
  return __builtin_amdgcn_update_dpp(0, x, CTRL, 0xF, 0xF, true);
}
constexpr int DPP_XOR1 = 0xB1;          // quad_perm [1, 0, 3, 2]
constexpr int DPP_XOR2 = 0x4E;          // quad_perm [2, 3, 0, 1]
constexpr int DPP_HALF_MIRROR = 0x141;  // lane i <- lane 7 - i of its group of 8
constexpr int DPP_MIRROR = 0x140;       // lane i <- lane 15 - i of its row of 16

__device__ __forceinline__ float lane_f(float x, int lane) {
  return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(x), lane));
}

// Sum over the wave, the same value in every lane (all 64 lanes must be active).
__device__ __forceinline__ float wave_sum(float x) {
  x = __fadd_rn(x, dpp_f<DPP_XOR1>(x));
  x = __fadd_rn(x, dpp_f<DPP_XOR2>(x));
  x = __fadd_rn(x, dpp_f<DPP_HALF_MIRROR>(x));
  x = __fadd_rn(x, dpp_f<DPP_MIRROR>(x));
  return __fadd_rn(__fadd_rn(lane_f(x, 0), lane_f(x, 16)), __fadd_rn(lane_f(x, 32), lane_f(x, 48)));
}

// The larger value, and the lower index where the values are equal.
__device__ __forceinline__ void take_max(float& v, int& i, float ov, int oi) {
  const bool other = (ov > v) | ((ov == v) & (oi < i));   // no branch
  v = other ? ov : v;
  i = other ? oi : i;
}
template <int CTRL>
__device__ __forceinline__ void dpp_max(float& v, int& i) {
  const float ov = dpp_f<CTRL>(v);
  const int oi = dpp_i<CTRL>(i);
  take_max(v, i, ov, oi);
}
__device__ __forceinline__ void wave_max(float& v, int& i) {
  dpp_max<DPP_XOR1>(v, i);
  dpp_max<DPP_XOR2>(v, i);
  dpp_max<DPP_HALF_MIRROR>(v, i);
  dpp_max<DPP_MIRROR>(v, i);
  float rv = lane_f(v, 0);
  int ri = __builtin_amdgcn_readlane(i, 0);
#pragma unroll
  for (int r = 16; r < 64; r += 16) take_max(rv, ri, lane_f(v, r), __builtin_amdgcn_readlane(i, r));
  v = rv;
  i = ri;
}

// --------------------------------------------------------------------- row access --
// 16 bytes as one register quadruple: a true vector type, so that a load or store of it stays one
// 16-byte instruction.
typedef uint32_t Vec16 __attribute__((ext_vector_type(4)));

// Where the R consecutive rows from `first` start, in elements from the tensor's base; rows a
// group lacks at the end of the tensor repeat the last one.  The host folds a tensor whose batch
// stride is K token strides into one batch element (K = rows): no division then, and one 64-bit
// division per group otherwise.
template <int R>
__device__ __forceinline__ void group_offsets(int64_t first, int64_t rows, int64_t K, int64_t sb, int64_t sk,
                                              int64_t (&off)[R]) {
  if (K == rows) {
#pragma unroll
    for (int r = 0; r < R; ++r) off[r] = min(first + r, rows - 1) * sk;
    return;
  }
  int64_t b = first / K, k = first - b * K;
#pragma unroll
  for (int r = 0; r < R; ++r) {
    off[r] = b * sb + k * sk;
    if (first + r + 1 < rows && ++k == K) {
      k = 0;
      ++b;
    }
  }
}

// A lane's piece of a row, elements e0 .. e0+EPL, as the 16 bytes memory holds: one 16-byte load
// where the row is 16-byte aligned and the piece lies inside it, element loads otherwise (indices
// at or beyond V read element V-1 again: in bounds, and masked when the piece is unpacked).
// Nothing looks at the bytes here, so the loads of several pieces are in flight together.
template <class T>
__device__ __forceinline__ Vec16 load_piece(const typename T::raw* row, bool aligned, int e0, int V) {
  Vec16 q;
  if (aligned && e0 + T::EPL <= V) {
    q = *reinterpret_cast<const Vec16*>(row + e0);
  } else {
    typename T::raw r[T::EPL];
#pragma unroll
    for (int j = 0; j < T::EPL; ++j) r[j] = row[min(e0 + j, V - 1)];
    __builtin_memcpy(&q, r, 16);
  }
  return q;
}

// The piece as floats; elements at or beyond V become -inf (probability 0, never the maximum of
// a row that has a finite element).
template <class T>
__device__ __forceinline__ void unpack_piece(const Vec16& q, int e0, int V, float (&v)[T::EPL]) {
  typename T::raw r[T::EPL];
  __builtin_memcpy(r, &q, 16);
#pragma unroll
  for (int j = 0; j < T::EPL; ++j) v[j] = T::load(r[j]);
  if (e0 + T::EPL > V) {
#pragma unroll
    for (int j = 0; j < T::EPL; ++j) v[j] = (e0 + j < V) ? v[j] : -INFINITY;
  }
}

// ------------------------------------------------------------------ forward kernels --
// exp(l / tau - zmax), the way both directions compute it
__device__ __forceinline__ float exp_shifted(float l, float inv_tau, float zmax) {
  return __builtin_amdgcn_exp2f(__fmul_rn(fmaf(l, inv_tau, -zmax), LG_LOG2E));
}

__device__ __forceinline__ void store_row(const LogitsArgs& a, int64_t row, int lane, float zmax, float s, float wsum,
                                          int mi) {
  if (lane != 0) return;
  if (a.mean != nullptr) {
    const float m = __fdiv_rn(__fdiv_rn(wsum, s), a.vm1);
    a.mean[row] = fminf(fmaxf(m, -1.0f), 1.0f);     // a NaN row stays unspecified; nothing is indexed by it
  }
  if (a.amax != nullptr) a.amax[row] = (int64_t)mi + a.tok_offset;
  if (a.stats != nullptr) {
    a.stats[2 * row] = zmax;
    a.stats[2 * row + 1] = s;
  }
}

// Rows of up to NCH chunks, R of them per wave at a time, held in registers.
template <class T, int NCH, int R>
__global__ __launch_bounds__(LG_THREADS) void k_logits_expect(LogitsArgs a) {
  using raw = typename T::raw;
  constexpr int E = T::EPL, CH = 64 * E;
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int V = a.V;
  const bool sums = a.mean != nullptr || a.stats != nullptr;
  const int64_t ngroups = (a.rows + R - 1) / R;

  for (int64_t g = (int64_t)blockIdx.x * LG_WAVES + wave; g < ngroups; g += (int64_t)gridDim.x * LG_WAVES) {
    int64_t off[R];
    group_offsets<R>(g * R, a.rows, a.K, a.sb, a.sk, off);
    Vec16 q[R][NCH];
#pragma unroll
    for (int r = 0; r < R; ++r) {
      const raw* rowp = static_cast<const raw*>(a.logits) + off[r];
      const bool aligned = (reinterpret_cast<uintptr_t>(rowp) & 15) == 0;
#pragma unroll
      for (int c = 0; c < NCH; ++c) q[r][c] = load_piece<T>(rowp, aligned, c * CH + lane * E, V);
    }
#pragma unroll
    for (int r = 0; r < R; ++r) {
      float v[NCH][E];
#pragma unroll
      for (int c = 0; c < NCH; ++c) unpack_piece<T>(q[r][c], c * CH + lane * E, V, v[c]);
      // the exact maximum of the raw logits, lowest index first
      float mx = -INFINITY;
      int mi = lane * E;
#pragma unroll
      for (int c = 0; c < NCH; ++c)
#pragma unroll
        for (int j = 0; j < E; ++j)
          if (v[c][j] > mx) {
            mx = v[c][j];
            mi = c * CH + lane * E + j;
          }
      wave_max(mx, mi);
      float zmax = 0.0f, s = 0.0f, wsum = 0.0f;
      if (sums) {
        zmax = __fmul_rn(mx, a.inv_tau);
        float ls = 0.0f, lw = 0.0f;
#pragma unroll
        for (int c = 0; c < NCH; ++c) {
          float n = (float)(2 * (c * CH + lane * E)) - a.vm1;           // 2v - (V-1): exact
#pragma unroll
          for (int j = 0; j < E; ++j) {
            const float e = exp_shifted(v[c][j], a.inv_tau, zmax);
            ls = __fadd_rn(ls, e);
            lw = fmaf(e, n, lw);
            n = __fadd_rn(n, 2.0f);
          }
        }
        s = wave_sum(ls);
        wsum = wave_sum(lw);
      }
      const int64_t row = g * R + r;
      if (row < a.rows) store_row(a, row, lane, zmax, s, wsum, mi);
    }
  }
}

// Rows of any length: a running maximum per lane, rescaled sums.
template <class T>
__global__ __launch_bounds__(LG_THREADS) void k_logits_expect_online(LogitsArgs a) {
  using raw = typename T::raw;
  constexpr int E = T::EPL, CH = 64 * E, U = LG_ONLINE_U;
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int V = a.V;
  const bool sums = a.mean != nullptr || a.stats != nullptr;

  for (int64_t row = (int64_t)blockIdx.x * LG_WAVES + wave; row < a.rows; row += (int64_t)gridDim.x * LG_WAVES) {
    int64_t off[1];
    group_offsets<1>(row, a.rows, a.K, a.sb, a.sk, off);
    const raw* rowp = static_cast<const raw*>(a.logits) + off[0];
    const bool aligned = (reinterpret_cast<uintptr_t>(rowp) & 15) == 0;
    float ml = -INFINITY, zm = 0.0f, ls = 0.0f, lw = 0.0f;   // zm: ml / tau, 0 while ml is -inf
    int mi = lane * E;
    for (int c0 = 0; c0 < V; c0 += U * CH) {
      Vec16 q[U];
#pragma unroll
      for (int u = 0; u < U; ++u) q[u] = load_piece<T>(rowp, aligned, c0 + u * CH + lane * E, V);
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const int e0 = c0 + u * CH + lane * E;
        float v[E];
        unpack_piece<T>(q[u], e0, V, v);
        float cm = ml;
        int ci = mi;
#pragma unroll
        for (int j = 0; j < E; ++j)
          if (v[j] > cm) {
            cm = v[j];
            ci = e0 + j;
          }
        if (!sums) {
          ml = cm;
          mi = ci;
          continue;
        }
        if (cm > ml) {                                       // the lane's maximum grew: rescale its sums
          const float zn = __fmul_rn(cm, a.inv_tau);
          // nothing is summed yet while ml is -inf: a select, so that 0 * inf cannot arise
          const float f = (ml == -INFINITY) ? 0.0f : __builtin_amdgcn_exp2f(__fmul_rn(__fsub_rn(zm, zn), LG_LOG2E));
          ls = __fmul_rn(ls, f);
          lw = __fmul_rn(lw, f);
          ml = cm;
          mi = ci;
          zm = zn;
        }
        float n = (float)(2 * e0) - a.vm1;
#pragma unroll
        for (int j = 0; j < E; ++j) {
          const float e = exp_shifted(v[j], a.inv_tau, zm);
          ls = __fadd_rn(ls, e);
          lw = fmaf(e, n, lw);
          n = __fadd_rn(n, 2.0f);
        }
      }
    }
    float mx = ml;
    wave_max(mx, mi);
    float zmax = 0.0f, s = 0.0f, wsum = 0.0f;
    if (sums) {
      zmax = __fmul_rn(mx, a.inv_tau);
      const float f = (ml == -INFINITY) ? 0.0f : __builtin_amdgcn_exp2f(__fmul_rn(__fsub_rn(zm, zmax), LG_LOG2E));
      s = wave_sum(__fmul_rn(ls, f));
      wsum = wave_sum(__fmul_rn(lw, f));
    }
    store_row(a, row, lane, zmax, s, wsum, mi);
  }
}

// ----------------------------------------------------------------- backward kernels --
// grad_l_v = (g / tau) (e_v / s) (x_v - mean_exact).  Next to the bin that holds the mass x_v - mean
// cancels, and the forward's fp32 mean is only good to its own rounding there (a peaked row: the
// largest gradient of the row would be wrong in its leading digits).  So the backward uses the
// forward's mean only to pick a pivot, the bin c nearest to it, and measures everything from that
// bin in exact integers: with t_v = 2 (v - c) it sums delta = sum_v e_v t_v / s
// = (mean_exact - x_c) (V-1) -- the pivot's own term is exactly 0, so where one bin holds the mass
// nothing cancels -- and x_v - mean_exact = (t_v - delta) / (V-1).  The gradient is then accurate
// relative to itself, not to 1.  One wave sum per row; the row's e_v stay in registers between the
// two steps.
struct BwdRow {
  float zmax, coef, nc, s;   // coef: (g / tau) / (s (V-1)); nc = 2c - (V-1), the pivot bin
};
__device__ __forceinline__ BwdRow bwd_row(const LogitsArgs& a, int64_t row, float inv_vm1) {
  BwdRow w;
  w.zmax = a.stats[2 * row];
  w.s = a.stats[2 * row + 1];
  w.coef = __fmul_rn(__fdiv_rn(__fmul_rn(a.grad_mean[row], a.inv_tau), w.s), inv_vm1);
  const float c = rintf(__fmul_rn(__fmul_rn(__fadd_rn(a.mean[row], 1.0f), 0.5f), a.vm1));
  w.nc = __fsub_rn(__fmul_rn(2.0f, fminf(fmaxf(c, 0.0f), a.vm1)), a.vm1);   // exact: integers below 2^18
  return w;
}

// A lane's piece of the gradient: 16 bytes where the row allows it, its elements inside V otherwise.
template <class T>
__device__ __forceinline__ void store_piece(typename T::raw* row, bool aligned, int e0, int V,
                                            const typename T::raw (&o)[T::EPL]) {
  if (aligned && e0 + T::EPL <= V) {
    Vec16 w;
    __builtin_memcpy(&w, o, 16);
    *reinterpret_cast<Vec16*>(row + e0) = w;
  } else {
#pragma unroll
    for (int j = 0; j < T::EPL; ++j)
      if (e0 + j < V) row[e0 + j] = o[j];
  }
}

// Rows of up to NCH chunks, R of them per wave at a time, held in registers.
template <class T, int NCH, int R>
__global__ __launch_bounds__(LG_THREADS) void k_logits_expect_bwd(LogitsArgs a) {
  using raw = typename T::raw;
  constexpr int E = T::EPL, CH = 64 * E;
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int V = a.V;
  const float inv_vm1 = __fdiv_rn(1.0f, a.vm1);
  const int64_t ngroups = (a.rows + R - 1) / R;

  for (int64_t g = (int64_t)blockIdx.x * LG_WAVES + wave; g < ngroups; g += (int64_t)gridDim.x * LG_WAVES) {
    int64_t soff[R], doff[R];
    group_offsets<R>(g * R, a.rows, a.K, a.sb, a.sk, soff);
    group_offsets<R>(g * R, a.rows, a.gK, a.gsb, a.gsk, doff);
    Vec16 q[R][NCH];
#pragma unroll
    for (int r = 0; r < R; ++r) {
      const raw* src = static_cast<const raw*>(a.logits) + soff[r];
      const bool aligned = (reinterpret_cast<uintptr_t>(src) & 15) == 0;
#pragma unroll
      for (int c = 0; c < NCH; ++c) q[r][c] = load_piece<T>(src, aligned, c * CH + lane * E, V);
    }
#pragma unroll
    for (int r = 0; r < R; ++r) {
      const BwdRow w = bwd_row(a, min(g * R + r, a.rows - 1), inv_vm1);
      float e[NCH][E];
      float lw = 0.0f;
#pragma unroll
      for (int c = 0; c < NCH; ++c) {
        unpack_piece<T>(q[r][c], c * CH + lane * E, V, e[c]);
        float n = (float)(2 * (c * CH + lane * E)) - a.vm1;
#pragma unroll
        for (int j = 0; j < E; ++j) {
          e[c][j] = exp_shifted(e[c][j], a.inv_tau, w.zmax);
          lw = fmaf(e[c][j], __fsub_rn(n, w.nc), lw);
          n = __fadd_rn(n, 2.0f);
        }
      }
      const float delta = __fdiv_rn(wave_sum(lw), w.s);
      if (g * R + r >= a.rows) continue;                               // a row the group lacks
      raw* dst = static_cast<raw*>(a.grad) + doff[r];
      const bool aligned = (reinterpret_cast<uintptr_t>(dst) & 15) == 0;
#pragma unroll
      for (int c = 0; c < NCH; ++c) {
        const int e0 = c * CH + lane * E;
        if (c > 0 && c * CH >= V) break;
        raw o[E];
        float n = (float)(2 * e0) - a.vm1;
#pragma unroll
        for (int j = 0; j < E; ++j) {
          const float t = __fsub_rn(__fsub_rn(n, w.nc), delta);
          o[j] = T::store(__fmul_rn(__fmul_rn(w.coef, e[c][j]), t));    // e == 0 (a -inf logit) gives 0
          n = __fadd_rn(n, 2.0f);
        }
        store_piece<T>(dst, aligned, e0, V, o);
      }
    }
  }
}

// Rows of any length, one per wave: a pass for delta, then a pass for the gradient.  The second
// pass reads the row again -- LG_ONLINE_U chunks in flight, from the L2 a row of at most 256 KB
// has just been pulled through.
template <class T>
__global__ __launch_bounds__(LG_THREADS) void k_logits_expect_bwd_long(LogitsArgs a) {
  using raw = typename T::raw;
  constexpr int E = T::EPL, CH = 64 * E, U = LG_ONLINE_U;
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int V = a.V;
  const float inv_vm1 = __fdiv_rn(1.0f, a.vm1);

  for (int64_t row = (int64_t)blockIdx.x * LG_WAVES + wave; row < a.rows; row += (int64_t)gridDim.x * LG_WAVES) {
    int64_t soff[1], doff[1];
    group_offsets<1>(row, a.rows, a.K, a.sb, a.sk, soff);
    group_offsets<1>(row, a.rows, a.gK, a.gsb, a.gsk, doff);
    const raw* src = static_cast<const raw*>(a.logits) + soff[0];
    raw* dst = static_cast<raw*>(a.grad) + doff[0];
    const bool src_al = (reinterpret_cast<uintptr_t>(src) & 15) == 0;
    const bool dst_al = (reinterpret_cast<uintptr_t>(dst) & 15) == 0;
    const BwdRow w = bwd_row(a, row, inv_vm1);
    float lw = 0.0f;
    for (int c0 = 0; c0 < V; c0 += U * CH) {
      Vec16 q[U];
#pragma unroll
      for (int u = 0; u < U; ++u) q[u] = load_piece<T>(src, src_al, c0 + u * CH + lane * E, V);
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const int e0 = c0 + u * CH + lane * E;
        float v[E];
        unpack_piece<T>(q[u], e0, V, v);
        float n = (float)(2 * e0) - a.vm1;
#pragma unroll
        for (int j = 0; j < E; ++j) {
          lw = fmaf(exp_shifted(v[j], a.inv_tau, w.zmax), __fsub_rn(n, w.nc), lw);
          n = __fadd_rn(n, 2.0f);
        }
      }
    }
    const float delta = __fdiv_rn(wave_sum(lw), w.s);
    for (int c0 = 0; c0 < V; c0 += U * CH) {
      Vec16 q[U];
#pragma unroll
      for (int u = 0; u < U; ++u) q[u] = load_piece<T>(src, src_al, c0 + u * CH + lane * E, V);
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const int e0 = c0 + u * CH + lane * E;
        float v[E];
        unpack_piece<T>(q[u], e0, V, v);
        raw o[E];
        float n = (float)(2 * e0) - a.vm1;
#pragma unroll
        for (int j = 0; j < E; ++j) {
          const float t = __fsub_rn(__fsub_rn(n, w.nc), delta);
          o[j] = T::store(__fmul_rn(__fmul_rn(w.coef, exp_shifted(v[j], a.inv_tau, w.zmax)), t));
          n = __fadd_rn(n, 2.0f);
        }
        store_piece<T>(dst, dst_al, e0, V, o);
      }
    }
  }
}

// ------------------------------------------------------------------------ launching --
// Diagnostic knob: BEAST_DEBUG_LOGITS_ROWS=<1|2|4> rows a wave works on at once (timing tools);
// default 4 (tests/tools/logits_timing.py).  Results do not depend on it.
inline int rows_in_flight() {
  static const int v = [] {
    const char* e = getenv("BEAST_DEBUG_LOGITS_ROWS");
    const int r = e ? atoi(e) : 4;
    return (r == 1 || r == 2 || r == 4) ? r : 4;
  }();
  return v;
}

// Workgroups of K resident on the stream's device (launch.h's occupancy query, asked once per
// kernel and device).
template <auto K>
int64_t resident_workgroups(const Queue& q) {
  static std::atomic<int> per_cu[16] = {};
  const bool cached = q.dev >= 0 && q.dev < 16;
  int per = cached ? per_cu[q.dev].load(std::memory_order_relaxed) : 0;
  if (per == 0) {
    per = std::max(1, occupancy<K>(LG_THREADS, 0, q));
    if (cached) per_cu[q.dev].store(per, std::memory_order_relaxed);
  }
  return (int64_t)cu_count(q.dev) * per;
}

// Launches K over the rows, R per wave at a time, on the resident workgroups only; with
// `resident_rows` set it launches nothing and reports how many rows those workgroups hold.
template <auto K, int R>
int run_rows(const LogitsArgs& a, const Queue& q, const char* what, int64_t* resident_rows) {
  const int64_t wgs = resident_workgroups<K>(q);
  if (resident_rows != nullptr) {
    *resident_rows = wgs * LG_WAVES * R;
    return BEAST_OK;
  }
  const int64_t ngroups = (a.rows + R - 1) / R;
  const int64_t grid = std::max<int64_t>(1, std::min((ngroups + LG_WAVES - 1) / LG_WAVES, wgs));
  return launch<K>((unsigned)grid, LG_THREADS, 0, q, what, a);
}

template <class T>
int run_forward(const LogitsArgs& a, const Queue& q, int64_t* resident_rows) {
  const int chunks = (a.V + 64 * T::EPL - 1) / (64 * T::EPL);
  const int r = rows_in_flight();
  const char* what = "k_logits_expect";
  if (chunks == 1) {
    if (r == 1) return run_rows<k_logits_expect<T, 1, 1>, 1>(a, q, what, resident_rows);
    if (r == 2) return run_rows<k_logits_expect<T, 1, 2>, 2>(a, q, what, resident_rows);
    return run_rows<k_logits_expect<T, 1, 4>, 4>(a, q, what, resident_rows);
  }
  if (chunks == 2) {
    if (r == 1) return run_rows<k_logits_expect<T, 2, 1>, 1>(a, q, what, resident_rows);
    return run_rows<k_logits_expect<T, 2, 2>, 2>(a, q, what, resident_rows);
  }
  if (chunks <= LG_MAX_CHUNKS) return run_rows<k_logits_expect<T, LG_MAX_CHUNKS, 1>, 1>(a, q, what, resident_rows);
  return run_rows<k_logits_expect_online<T>, 1>(a, q, "k_logits_expect_online", resident_rows);
}

template <class T>
int run_backward(const LogitsArgs& a, const Queue& q, int64_t* resident_rows) {
  const int chunks = (a.V + 64 * T::EPL - 1) / (64 * T::EPL);
  const int r = rows_in_flight();
  const char* what = "k_logits_expect_bwd";
  if (chunks == 1) {
    if (r == 1) return run_rows<k_logits_expect_bwd<T, 1, 1>, 1>(a, q, what, resident_rows);
    if (r == 2) return run_rows<k_logits_expect_bwd<T, 1, 2>, 2>(a, q, what, resident_rows);
    return run_rows<k_logits_expect_bwd<T, 1, 4>, 4>(a, q, what, resident_rows);
  }
  if (chunks == 2) {
    if (r == 1) return run_rows<k_logits_expect_bwd<T, 2, 1>, 1>(a, q, what, resident_rows);
    return run_rows<k_logits_expect_bwd<T, 2, 2>, 2>(a, q, what, resident_rows);
  }
  if (chunks <= LG_MAX_CHUNKS) return run_rows<k_logits_expect_bwd<T, LG_MAX_CHUNKS, 1>, 1>(a, q, what, resident_rows);
  return run_rows<k_logits_expect_bwd_long<T>, 1>(a, q, "k_logits_expect_bwd_long", resident_rows);
}

int run_typed(int dtype, bool backward, const LogitsArgs& a, const Queue& q, int64_t* resident_rows) {
  switch (dtype) {
    case BEAST_LOGITS_F32:
      return backward ? run_backward<ElemF32>(a, q, resident_rows) : run_forward<ElemF32>(a, q, resident_rows);
    case BEAST_LOGITS_F16:
      return backward ? run_backward<ElemF16>(a, q, resident_rows) : run_forward<ElemF16>(a, q, resident_rows);
    default:
      return backward ? run_backward<ElemBF16>(a, q, resident_rows) : run_forward<ElemBF16>(a, q, resident_rows);
  }
}

// K as the kernels take it: B * K where the B batch elements lie K token strides apart (or there
// is only one), so that a row's offset is row * sk.
int64_t folded_k(int64_t B, int K, int64_t sb, int64_t sk) { return (B == 1 || sb == K * sk) ? B * K : K; }

// The checks both directions share (before any HIP call).
int check_common(const char* fn, const void* logits, int dtype, int64_t B, int K, int V, int64_t sb, int64_t sk,
                 float temperature) {
  BEAST_REQUIRE(logits != nullptr, "%s: null logits", fn);
  BEAST_REQUIRE(dtype == BEAST_LOGITS_F32 || dtype == BEAST_LOGITS_F16 || dtype == BEAST_LOGITS_BF16,
                "%s: unknown dtype code %d", fn, dtype);
  BEAST_REQUIRE(B >= 0 && K >= 1, "%s: bad shape B=%lld K=%d", fn, (long long)B, K);
  BEAST_REQUIRE(sb >= 0 && sk >= 0, "%s: strides must be >= 0 (sb=%lld, sk=%lld)", fn, (long long)sb, (long long)sk);
  BEAST_REQUIRE(temperature > 0.0f && temperature < INFINITY, "%s: temperature must be finite and > 0 (got %g)", fn,
                (double)temperature);
  BEAST_REQUIRE_CODE(V >= LG_MIN_V && V <= LG_MAX_V, BEAST_E_UNSUPPORTED, "%s supports %d <= V <= %d (V=%d)", fn,
                     LG_MIN_V, LG_MAX_V, V);
  return BEAST_OK;
}

}  // namespace

// =================================================================== C-ABI ==
extern "C" int beast_logits_expect(const void* logits, int dtype, int64_t B, int K, int V, int64_t sb, int64_t sk,
                                   float temperature, int64_t tok_offset, float* mean_out, int64_t* argmax_out,
                                   float* stats_out, void* hip_stream) {
  BEAST_TRY(check_common("beast_logits_expect", logits, dtype, B, K, V, sb, sk, temperature));
  BEAST_REQUIRE(mean_out || argmax_out || stats_out, "beast_logits_expect: no output requested");
  if (B == 0) return BEAST_OK;
  LogitsArgs a{};
  a.logits = logits; a.sb = sb; a.sk = sk; a.rows = B * K; a.K = folded_k(B, K, sb, sk); a.V = V;
  a.inv_tau = (float)(1.0 / (double)temperature); a.vm1 = (float)(V - 1); a.tok_offset = tok_offset;
  a.mean = mean_out; a.amax = argmax_out; a.stats = stats_out;
  Queue q;
  if (const int rc = queue_of(hip_stream, q, "beast_logits_expect")) return rc;
  return run_typed(dtype, false, a, q, nullptr);
}

extern "C" int beast_logits_expect_bwd(const void* logits, int dtype, int64_t B, int K, int V, int64_t sb, int64_t sk,
                                       float temperature, const float* mean, const float* stats,
                                       const float* grad_mean, void* grad_logits, int64_t gsb, int64_t gsk,
                                       void* hip_stream) {
  BEAST_TRY(check_common("beast_logits_expect_bwd", logits, dtype, B, K, V, sb, sk, temperature));
  BEAST_REQUIRE(mean && stats && grad_mean && grad_logits, "beast_logits_expect_bwd: null pointer");
  BEAST_REQUIRE(gsb >= 0 && gsk >= V, "beast_logits_expect_bwd: grad_logits rows must not overlap (gsb=%lld, "
                "gsk=%lld, V=%d)", (long long)gsb, (long long)gsk, V);
  if (B == 0) return BEAST_OK;
  LogitsArgs a{};
  a.logits = logits; a.sb = sb; a.sk = sk; a.rows = B * K; a.K = folded_k(B, K, sb, sk); a.V = V;
  a.gK = folded_k(B, K, gsb, gsk);
  a.inv_tau = (float)(1.0 / (double)temperature); a.vm1 = (float)(V - 1);
  a.mean = const_cast<float*>(mean); a.stats = const_cast<float*>(stats);
  a.grad_mean = grad_mean; a.grad = grad_logits; a.gsb = gsb; a.gsk = gsk;
  Queue q;
  if (const int rc = queue_of(hip_stream, q, "beast_logits_expect_bwd")) return rc;
  return run_typed(dtype, true, a, q, nullptr);
}

extern "C" int64_t beast_logits_resident_rows(int dtype, int V, int backward, void* hip_stream) {
  BEAST_REQUIRE(dtype == BEAST_LOGITS_F32 || dtype == BEAST_LOGITS_F16 || dtype == BEAST_LOGITS_BF16,
                "beast_logits_resident_rows: unknown dtype code %d", dtype);
  BEAST_REQUIRE_CODE(V >= LG_MIN_V && V <= LG_MAX_V, BEAST_E_UNSUPPORTED,
                     "beast_logits_resident_rows supports %d <= V <= %d (V=%d)", LG_MIN_V, LG_MAX_V, V);
  LogitsArgs a{};
  a.V = V;
  Queue q;
  if (const int rc = queue_of(hip_stream, q, "beast_logits_resident_rows")) return rc;
  int64_t rows = 0;
  if (const int rc = run_typed(dtype, backward != 0, a, q, &rows)) return rc;
  return rows;
}
