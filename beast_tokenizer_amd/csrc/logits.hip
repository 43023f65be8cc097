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
//
// The same machinery carries the training direction (beast_xent_rows, beast_xent_rows_bwd): the
// cross-entropy of a row against a token or against the two-hot target of an unquantised
// coefficient, k_xent / k_xent_online and k_xent_bwd / k_xent_bwd_long further down; and the
// rollout direction (beast_sample_rows): temperature / top-k / top-p draws with their
// log-probabilities, k_sample / k_sample_long after those; and the policy-gradient direction
// (beast_score_rows, beast_score_rows_bwd): the log-probability of given tokens, the entropy and the
// divergence from a reference under the sampler's distribution, k_score / k_score_long and
// k_score_bwd / k_score_bwd_long last.
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
constexpr float LG_LN2 = 0.693147180559945309417f;

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

// ------------------------------------------------------- two-hot cross-entropy kernels --
// beast_xent_rows / beast_xent_rows_bwd on the same row machinery.  With m = max_v l_v,
// e_v = exp(l_v - m), s = sum_v e_v and a target position u = i + f (i <= V-2, f in [0, 1]):
//   q_v    = (1-eps) [(1-f) (v == i) + f (v == i+1)] + eps / V
//   loss   = log s + (1-eps) [(1-f) (m - l_i) + f (m - l_{i+1})] + eps (sum_v (m - l_v)) / V
//   grad_v = g (e_v / s - q_v)
// Every term of the loss is >= 0: nothing cancels.  A term whose weight is exactly 0 is left out
// by a select, so a -inf logit under a zero weight gives neither NaN nor inf.  The target only
// ever meets v in a comparison: l_i and l_{i+1} are picked by select and the wave sum of one
// non-zero term is exact.  The temperature is 1, so e_v is exp_shifted(l_v, 1, m) in both
// directions and stats = (m, s) is all the backward needs.
struct XentArgs {
  const void* logits;
  int64_t sb, sk;        // element strides of the batch and the token axis
  int64_t rows;          // B * K
  int64_t K, gK;         // folded_k of the logits' and of grad_logits' strides
  int V;
  float vm1;             // V - 1
  const int64_t* tok;    // exactly one of tok, pos
  const float* pos;
  int64_t tok_offset, ignore_index;
  float eps, keep, eps_v;   // label smoothing, 1 - eps, eps / V
  float* loss;           // forward outputs, nullable
  float* stats;          // forward: out (nullable); backward: in
  int64_t* amax;
  // backward only
  const float* grad_loss;
  void* grad;
  int64_t gsb, gsk;
};

constexpr int XENT_TARGET = 0, XENT_IGNORED = 1, XENT_OUT_OF_RANGE = 2;
struct XentTarget {
  int i;       // the lower bin, <= V-2; matches no v where the row has no target
  float f;     // the weight of bin i+1
  int kind;
};
// Which two bins carry a row's target.  A coefficient x gives u = clamp(((x + 1) * 0.5) * (V-1),
// 0, V-1) with these three roundings in fp32 (the oracle replicates them); a token t gives u = t.
// A row's target as memory holds it: loaded at the top of a group of rows, beside the rows
// themselves, so that its latency is not paid row by row.
struct XentRaw {
  int64_t tok;
  float pos;
};
__device__ __forceinline__ XentRaw xent_load(const XentArgs& a, int64_t row) {
  XentRaw r{0, 0.0f};
  if (a.tok != nullptr) r.tok = a.tok[row];
  else r.pos = a.pos[row];
  return r;
}
__device__ __forceinline__ XentTarget xent_target(const XentArgs& a, const XentRaw& in) {
  XentTarget t{-2, 0.0f, XENT_TARGET};
  if (a.tok != nullptr) {
    const int64_t raw = in.tok;
    const int64_t tk = raw - a.tok_offset;
    if (raw == a.ignore_index) {
      t.kind = XENT_IGNORED;
    } else if (tk < 0 || tk >= a.V) {
      t.kind = XENT_OUT_OF_RANGE;
    } else {
      t.i = min((int)tk, a.V - 2);
      t.f = (float)((int)tk - t.i);
    }
    return t;
  }
  const float x = in.pos;
  if (x != x) {
    t.kind = XENT_IGNORED;
    return t;
  }
  const float u = fminf(fmaxf(__fmul_rn(__fmul_rn(__fadd_rn(x, 1.0f), 0.5f), a.vm1), 0.0f), a.vm1);
  t.i = min((int)u, a.V - 2);             // u >= 0: the conversion is the floor
  t.f = __fsub_rn(u, (float)t.i);         // exact
  return t;
}

// The wave's maximum alone, and the wave's lowest index, the same value in every lane: one DPP
// operation a step where the (value, index) pair of wave_max takes five.
__device__ __forceinline__ float wave_max_value(float x) {
  x = fmaxf(x, dpp_f<DPP_XOR1>(x));
  x = fmaxf(x, dpp_f<DPP_XOR2>(x));
  x = fmaxf(x, dpp_f<DPP_HALF_MIRROR>(x));
  x = fmaxf(x, dpp_f<DPP_MIRROR>(x));
  return fmaxf(fmaxf(lane_f(x, 0), lane_f(x, 16)), fmaxf(lane_f(x, 32), lane_f(x, 48)));
}
__device__ __forceinline__ int wave_min_index(int i) {
  i = min(i, dpp_i<DPP_XOR1>(i));
  i = min(i, dpp_i<DPP_XOR2>(i));
  i = min(i, dpp_i<DPP_HALF_MIRROR>(i));
  i = min(i, dpp_i<DPP_MIRROR>(i));
  return min(min(__builtin_amdgcn_readlane(i, 0), __builtin_amdgcn_readlane(i, 16)),
             min(__builtin_amdgcn_readlane(i, 32), __builtin_amdgcn_readlane(i, 48)));
}

// Element `rel` of a chunk (lane rel / EPL, slot rel % EPL) for a wave-uniform rel in [0, 64 EPL):
// the lane by a readlane of every slot, the slot by scalar compares among the results (in this order:
// a select chain over the register array itself would be folded into a dynamic index, which the
// compiler serves from scratch).  The target is compared, never an address.
template <int E>
__device__ __forceinline__ float pick_piece(const float (&v)[E], int rel) {
  const int ln = rel / E, j = rel & (E - 1);
  float x = lane_f(v[0], ln);
#pragma unroll
  for (int k = 1; k < E; ++k) {
    const float y = lane_f(v[k], ln);
    x = (j == k) ? y : x;
  }
  return x;
}

// What lane 0 stores for a row.  li, li1: l_i and l_{i+1}; sd: sum_v (m - l_v) (eps > 0 only).
__device__ __forceinline__ void xent_store(const XentArgs& a, int64_t row, int lane, const XentTarget& t, float m,
                                           float s, float li, float li1, float sd, int mi) {
  if (lane != 0) return;
  if (a.loss != nullptr) {
    float L = 0.0f;
    if (t.kind == XENT_OUT_OF_RANGE) {
      L = __builtin_nanf("");
    } else if (t.kind == XENT_TARGET) {
      const float w0 = __fsub_rn(1.0f, t.f);
      float hot = 0.0f;
      if (w0 != 0.0f) hot = __fmul_rn(w0, __fsub_rn(m, li));
      if (t.f != 0.0f) hot = __fadd_rn(hot, __fmul_rn(t.f, __fsub_rn(m, li1)));
      L = __fadd_rn(__fmul_rn(__builtin_amdgcn_logf(s), LG_LN2), __fmul_rn(a.keep, hot));   // s >= 1
      if (a.eps > 0.0f) L = __fadd_rn(L, __fmul_rn(a.eps_v, sd));
    }
    a.loss[row] = L;
  }
  if (a.amax != nullptr) a.amax[row] = (int64_t)mi + a.tok_offset;
  if (a.stats != nullptr) {
    a.stats[2 * row] = m;
    a.stats[2 * row + 1] = s;
  }
}

// Rows of up to NCH chunks, R of them per wave at a time, held in registers.
template <class T, int NCH, int R>
__global__ __launch_bounds__(LG_THREADS) void k_xent(XentArgs a) {
  using raw = typename T::raw;
  constexpr int E = T::EPL, CH = 64 * E;
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int V = a.V;
  const bool sums = a.loss != nullptr || a.stats != nullptr;
  const bool picks = a.loss != nullptr;
  const bool smooth = picks && a.eps > 0.0f;
  const int64_t ngroups = (a.rows + R - 1) / R;

  for (int64_t g = (int64_t)blockIdx.x * LG_WAVES + wave; g < ngroups; g += (int64_t)gridDim.x * LG_WAVES) {
    int64_t off[R];
    group_offsets<R>(g * R, a.rows, a.K, a.sb, a.sk, off);
    XentRaw in[R];
    if (picks) {
#pragma unroll
      for (int r = 0; r < R; ++r) in[r] = xent_load(a, min(g * R + r, a.rows - 1));
    }
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
      const int64_t row = min(g * R + r, a.rows - 1);
      float v[NCH][E];
#pragma unroll
      for (int c = 0; c < NCH; ++c) unpack_piece<T>(q[r][c], c * CH + lane * E, V, v[c]);
      // the exact maximum first; its lowest index only where the argmax is asked for
      float mx = -INFINITY;
#pragma unroll
      for (int c = 0; c < NCH; ++c)
#pragma unroll
        for (int j = 0; j < E; ++j) mx = fmaxf(mx, v[c][j]);
      mx = wave_max_value(mx);
      int mi = 0;
      if (a.amax != nullptr) {
        int first = LG_MAX_V;
#pragma unroll
        for (int c = NCH - 1; c >= 0; --c)
#pragma unroll
          for (int j = E - 1; j >= 0; --j) first = (v[c][j] == mx) ? c * CH + lane * E + j : first;
        mi = wave_min_index(first);
      }
      XentTarget t{-2, 0.0f, XENT_TARGET};
      float s = 0.0f, li = 0.0f, li1 = 0.0f, sd = 0.0f;
      if (sums) {
        float ls = 0.0f;
#pragma unroll
        for (int c = 0; c < NCH; ++c)
#pragma unroll
          for (int j = 0; j < E; ++j) ls = __fadd_rn(ls, exp_shifted(v[c][j], 1.0f, mx));
        s = wave_sum(ls);
      }
      if (picks) {
        t = xent_target(a, in[r]);
        const int ti = __builtin_amdgcn_readfirstlane(t.i);            // the row's, so the wave's
#pragma unroll
        for (int c = 0; c < NCH; ++c) {
          const int r0 = ti - c * CH, r1 = r0 + 1;
          if (r0 >= 0 && r0 < CH) li = pick_piece<E>(v[c], r0);
          if (r1 >= 0 && r1 < CH) li1 = pick_piece<E>(v[c], r1);
        }
        if (smooth) {
          float ld = 0.0f;
#pragma unroll
          for (int c = 0; c < NCH; ++c)
#pragma unroll
            for (int j = 0; j < E; ++j)                                  // padding is masked
              ld = __fadd_rn(ld, (c * CH + lane * E + j < V) ? __fsub_rn(mx, v[c][j]) : 0.0f);
          sd = wave_sum(ld);
        }
      }
      if (g * R + r < a.rows) xent_store(a, row, lane, t, mx, s, li, li1, sd, mi);
    }
  }
}

// Rows of any length: a running maximum per lane, its sums brought along when it grows.  The lane's
// sum of m - l_v grows by (elements so far) * (the maximum's growth): every term stays >= 0.
template <class T>
__global__ __launch_bounds__(LG_THREADS) void k_xent_online(XentArgs a) {
  using raw = typename T::raw;
  constexpr int E = T::EPL, CH = 64 * E, U = LG_ONLINE_U;
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int V = a.V;
  const bool sums = a.loss != nullptr || a.stats != nullptr;
  const bool picks = a.loss != nullptr;
  const bool smooth = picks && a.eps > 0.0f;

  for (int64_t row = (int64_t)blockIdx.x * LG_WAVES + wave; row < a.rows; row += (int64_t)gridDim.x * LG_WAVES) {
    int64_t off[1];
    group_offsets<1>(row, a.rows, a.K, a.sb, a.sk, off);
    const raw* rowp = static_cast<const raw*>(a.logits) + off[0];
    const bool aligned = (reinterpret_cast<uintptr_t>(rowp) & 15) == 0;
    XentTarget t{-2, 0.0f, XENT_TARGET};
    if (picks) t = xent_target(a, xent_load(a, row));
    const int ti = __builtin_amdgcn_readfirstlane(t.i);
    float ml = -INFINITY, zm = 0.0f, ls = 0.0f, li = 0.0f, li1 = 0.0f;   // zm: ml, 0 while ml is -inf
    float ld = 0.0f, cnt = 0.0f;      // sum of ml - l_v over the lane's cnt elements so far
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
        if (picks) {
          const int r0 = ti - (c0 + u * CH), r1 = r0 + 1;
          if (r0 >= 0 && r0 < CH) li = pick_piece<E>(v, r0);
          if (r1 >= 0 && r1 < CH) li1 = pick_piece<E>(v, r1);
        }
        if (cm > ml) {                                       // the lane's maximum grew
          // while ml is -inf nothing finite is summed: selects, so that 0 * inf and inf - inf cannot arise
          const bool first = ml == -INFINITY;
          const float f = first ? 0.0f : __builtin_amdgcn_exp2f(__fmul_rn(__fsub_rn(ml, cm), LG_LOG2E));
          ls = __fmul_rn(ls, f);
          if (smooth)
            ld = first ? (cnt > 0.0f ? INFINITY : 0.0f) : __fadd_rn(ld, __fmul_rn(cnt, __fsub_rn(cm, ml)));
          ml = cm;
          mi = ci;
          zm = cm;
        }
#pragma unroll
        for (int j = 0; j < E; ++j) {
          ls = __fadd_rn(ls, exp_shifted(v[j], 1.0f, zm));
          if (smooth) {
            const bool real = e0 + j < V;
            ld = __fadd_rn(ld, (real && ml != -INFINITY) ? __fsub_rn(ml, v[j]) : 0.0f);
            cnt = __fadd_rn(cnt, real ? 1.0f : 0.0f);
          }
        }
      }
    }
    float mx = ml;
    wave_max(mx, mi);
    float s = 0.0f, sd = 0.0f;
    if (sums) {
      const bool none = ml == -INFINITY;
      const float f = none ? 0.0f : __builtin_amdgcn_exp2f(__fmul_rn(__fsub_rn(ml, mx), LG_LOG2E));
      s = wave_sum(__fmul_rn(ls, f));
      if (smooth) {
        ld = none ? (cnt > 0.0f ? INFINITY : 0.0f) : __fadd_rn(ld, __fmul_rn(cnt, __fsub_rn(mx, ml)));
        sd = wave_sum(ld);
      }
    }
    xent_store(a, row, lane, t, mx, s, li, li1, sd, mi);
  }
}

// grad_v = g (e_v / s - q_v) = fma(g / s, e_v, -g q_v): no sum over the row, so a lane's piece goes
// from its load to its store.  q_v is eps / V except in bins i and i+1, whose owners are found as in
// the forward: the chunk and the slot by scalar compares, the lane by one compare per piece.
struct XentBwdRow {
  float m, gs;           // gs = g / s
  float nq, nqi, nqi1;   // -g q_v: elsewhere, in bin i, in bin i+1
  int i, kind;
};
struct XentBwdRaw {
  XentRaw target;
  float m, s, g;
};
__device__ __forceinline__ XentBwdRaw xent_bwd_load(const XentArgs& a, int64_t row) {
  return XentBwdRaw{xent_load(a, row), a.stats[2 * row], a.stats[2 * row + 1], a.grad_loss[row]};
}
__device__ __forceinline__ XentBwdRow xent_bwd_row(const XentArgs& a, const XentBwdRaw& in) {
  const XentTarget t = xent_target(a, in.target);
  XentBwdRow w;
  const float g = in.g;
  w.m = in.m;
  w.gs = __fmul_rn(g, __fdiv_rn(1.0f, in.s));
  w.nq = -__fmul_rn(g, a.eps_v);
  w.nqi = -__fmul_rn(g, __fadd_rn(a.eps_v, __fmul_rn(a.keep, __fsub_rn(1.0f, t.f))));
  w.nqi1 = -__fmul_rn(g, __fadd_rn(a.eps_v, __fmul_rn(a.keep, t.f)));
  w.i = __builtin_amdgcn_readfirstlane(t.i);
  w.kind = __builtin_amdgcn_readfirstlane(t.kind);
  return w;
}

// The piece as memory holds it.  bf16 goes through the compiler's own float -> bfloat conversion
// (round to nearest even, NaN stays NaN), which gfx950 has as one packed instruction.
template <class T>
__device__ __forceinline__ void pack_piece(const float (&d)[T::EPL], typename T::raw (&o)[T::EPL]) {
#pragma unroll
  for (int j = 0; j < T::EPL; ++j) o[j] = T::store(d[j]);
}
typedef float F32x2 __attribute__((ext_vector_type(2)));
typedef __bf16 BF16x2 __attribute__((ext_vector_type(2)));
template <>
__device__ __forceinline__ void pack_piece<ElemBF16>(const float (&d)[8], uint16_t (&o)[8]) {
#pragma unroll
  for (int j = 0; j < 8; j += 2) {
    const BF16x2 r = __builtin_convertvector(F32x2{d[j], d[j + 1]}, BF16x2);
    __builtin_memcpy(&o[j], &r, 4);
  }
}

// The gradient of the chunk at `cb` (a wave-uniform element index) of a row that has a target.
template <class T>
__device__ __forceinline__ void xent_bwd_piece(const XentBwdRow& w, int cb, int lane, const float (&v)[T::EPL],
                                               typename T::raw (&o)[T::EPL]) {
  constexpr int E = T::EPL, CH = 64 * E;
  float nq[E];
#pragma unroll
  for (int j = 0; j < E; ++j) nq[j] = w.nq;
  const int r0 = w.i - cb, r1 = r0 + 1;
  if (r0 >= 0 && r0 < CH) {
    const bool own = lane == r0 / E;
#pragma unroll
    for (int j = 0; j < E; ++j) nq[j] = (own && j == (r0 & (E - 1))) ? w.nqi : nq[j];
  }
  if (r1 >= 0 && r1 < CH) {
    const bool own = lane == r1 / E;
#pragma unroll
    for (int j = 0; j < E; ++j) nq[j] = (own && j == (r1 & (E - 1))) ? w.nqi1 : nq[j];
  }
  float d[E];
#pragma unroll
  for (int j = 0; j < E; ++j) d[j] = fmaf(w.gs, exp_shifted(v[j], 1.0f, w.m), nq[j]);   // a -inf logit: e == 0
  pack_piece<T>(d, o);
}

// A row without a target: zeros where it is ignored, NaN where its token is out of range.
template <class T>
__device__ __forceinline__ void xent_bwd_fill(int kind, typename T::raw (&o)[T::EPL]) {
  const typename T::raw fill = T::store(kind == XENT_IGNORED ? 0.0f : __builtin_nanf(""));
#pragma unroll
  for (int j = 0; j < T::EPL; ++j) o[j] = fill;
}

// Rows of up to NCH chunks, R of them per wave at a time, held in registers.
template <class T, int NCH, int R>
__global__ __launch_bounds__(LG_THREADS) void k_xent_bwd(XentArgs a) {
  using raw = typename T::raw;
  constexpr int E = T::EPL, CH = 64 * E;
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int V = a.V;
  const int64_t ngroups = (a.rows + R - 1) / R;

  for (int64_t g = (int64_t)blockIdx.x * LG_WAVES + wave; g < ngroups; g += (int64_t)gridDim.x * LG_WAVES) {
    int64_t soff[R], doff[R];
    group_offsets<R>(g * R, a.rows, a.K, a.sb, a.sk, soff);
    group_offsets<R>(g * R, a.rows, a.gK, a.gsb, a.gsk, doff);
    XentBwdRaw in[R];
#pragma unroll
    for (int r = 0; r < R; ++r) in[r] = xent_bwd_load(a, min(g * R + r, a.rows - 1));
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
      if (g * R + r >= a.rows) continue;                               // a row the group lacks
      const XentBwdRow w = xent_bwd_row(a, in[r]);
      raw* dst = static_cast<raw*>(a.grad) + doff[r];
      const bool aligned = (reinterpret_cast<uintptr_t>(dst) & 15) == 0;
#pragma unroll
      for (int c = 0; c < NCH; ++c) {
        const int e0 = c * CH + lane * E;
        if (c > 0 && c * CH >= V) break;
        raw o[E];
        if (w.kind == XENT_TARGET) {
          float v[E];
          unpack_piece<T>(q[r][c], e0, V, v);
          xent_bwd_piece<T>(w, c * CH, lane, v, o);
        } else {
          xent_bwd_fill<T>(w.kind, o);
        }
        store_piece<T>(dst, aligned, e0, V, o);
      }
    }
  }
}

// Rows of any length, one per wave: one pass, LG_ONLINE_U chunks in flight.
template <class T>
__global__ __launch_bounds__(LG_THREADS) void k_xent_bwd_long(XentArgs a) {
  using raw = typename T::raw;
  constexpr int E = T::EPL, CH = 64 * E, U = LG_ONLINE_U;
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int V = a.V;

  for (int64_t row = (int64_t)blockIdx.x * LG_WAVES + wave; row < a.rows; row += (int64_t)gridDim.x * LG_WAVES) {
    int64_t soff[1], doff[1];
    group_offsets<1>(row, a.rows, a.K, a.sb, a.sk, soff);
    group_offsets<1>(row, a.rows, a.gK, a.gsb, a.gsk, doff);
    const raw* src = static_cast<const raw*>(a.logits) + soff[0];
    raw* dst = static_cast<raw*>(a.grad) + doff[0];
    const bool src_al = (reinterpret_cast<uintptr_t>(src) & 15) == 0;
    const bool dst_al = (reinterpret_cast<uintptr_t>(dst) & 15) == 0;
    const XentBwdRow w = xent_bwd_row(a, xent_bwd_load(a, row));
    for (int c0 = 0; c0 < V; c0 += U * CH) {
      Vec16 q[U];
#pragma unroll
      for (int u = 0; u < U; ++u) q[u] = load_piece<T>(src, src_al, c0 + u * CH + lane * E, V);
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const int e0 = c0 + u * CH + lane * E;
        raw o[E];
        if (w.kind == XENT_TARGET) {
          float v[E];
          unpack_piece<T>(q[u], e0, V, v);
          xent_bwd_piece<T>(w, c0 + u * CH, lane, v, o);
        } else {
          xent_bwd_fill<T>(w.kind, o);
        }
        store_piece<T>(dst, dst_al, e0, V, o);
      }
    }
  }
}

// ---------------------------------------------------------------- sampling kernels --
// beast_sample_rows on the same row machinery: S inverse-CDF draws from one read of a row, under
// softmax(l / tau) truncated to the top-k and then the top-p (nucleus) bins.  With
// e_v = exp(l_v / tau - zmax) as everywhere above:
//   kept   = {v : l_v >= theta}; theta is the k-th largest logit, raised to the largest logit value
//            whose upper set still holds p of the top-k survivors' mass (whole tie groups stay)
//   C_v    = sum of e_w over kept w <= v, in ascending index;  S2 = C_{V-1}
//   tok_s  = the lowest kept v with e_v > 0 and C_v > u_s S2; the highest kept v with e_v > 0
//            where rounding leaves none
//   logprob_s = (l_tok / tau - zmax) - log S2
// Both thresholds are found on order-preserving integer keys of the raw logits by a bitwise binary
// search, most significant bit first: the number of keys >= a candidate (ballot + popcount) and the
// masked wave_sum of e are both monotone in the candidate (a fixed-order fp32 sum of non-negative
// terms cannot grow when terms are replaced by 0).  The prefix C is built with DPP row shifts and
// readlanes only: a lane's elements in ascending order, a shift-and-add scan over each 16-lane row,
// the four row totals in lane order, the chunks one after the other -- no LDS, no atomics, an
// order fixed by (V, element type).  Lane L's offset is bitwise lane L-1's inclusive value, and a
// chunk's base is bitwise the last C of the chunk before it.  The draws reuse the row's C in
// registers; tokens and log-probabilities of the S draws collect in lanes 0 .. S-1 and leave in one
// store each.  Nothing is addressed by a computed value: a token is a minimum over lane indices.
struct SampleArgs {
  const void* logits;
  int64_t sb, sk;        // element strides of the batch and the token axis
  int64_t rows;          // B * K
  int64_t K;             // folded_k of the strides
  int V;
  float inv_tau;
  int top_k;             // 0: no top-k
  float top_p;           // 1: no top-p
  const float* u;        // [S][rows]
  int S;
  int64_t tok_offset;
  int64_t* tok;          // [S][rows]
  float* logprob;        // nullable [S][rows]
  int32_t* kept;         // nullable [rows]
};

constexpr int DPP_ROW_SHR1 = 0x111, DPP_ROW_SHR2 = 0x112, DPP_ROW_SHR4 = 0x114, DPP_ROW_SHR8 = 0x118;

// An unsigned key with key(a) < key(b) exactly where a < b (-0 and +0 share one key): 32 bits for
// fp32; for the 16-bit types the 16 bits of the element itself, so the search takes 16 steps.
template <class T>
struct SampleKey {
  static constexpr int BITS = 16;
};
template <>
struct SampleKey<ElemF32> {
  static constexpr int BITS = 32;
};
__device__ __forceinline__ uint32_t ordered_key32(float f) {
  const uint32_t u = (f == 0.0f) ? 0u : __float_as_uint(f);
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
template <class T>
__device__ __forceinline__ uint32_t sample_key(float f) {
  return ordered_key32(f);
}
template <>
__device__ __forceinline__ uint32_t sample_key<ElemBF16>(float f) {
  return ordered_key32(f) >> 16;                 // a bf16 is the upper half of its float
}
template <>
__device__ __forceinline__ uint32_t sample_key<ElemF16>(float f) {
  const _Float16 h = (_Float16)f;                // exact: f came from an fp16
  uint16_t b;
  __builtin_memcpy(&b, &h, 2);
  const uint32_t u = (f == 0.0f) ? 0u : (uint32_t)b;
  return (u & 0x8000u) ? (~u & 0xFFFFu) : (u | 0x8000u);
}

__device__ __forceinline__ int wave_count(bool p) { return __builtin_popcountll(__builtin_amdgcn_ballot_w64(p)); }

// The exclusive prefix of x over the lanes (lane L: x_0 + .. + x_{L-1}, 0 in lane 0), and in
// `total` the sum over all 64, which is what lane 64 would hold.
__device__ __forceinline__ float wave_exclusive_scan(float x, int lane, float& total) {
  x = __fadd_rn(x, dpp_f<DPP_ROW_SHR1>(x));      // lanes a shift has no source for read 0
  x = __fadd_rn(x, dpp_f<DPP_ROW_SHR2>(x));
  x = __fadd_rn(x, dpp_f<DPP_ROW_SHR4>(x));
  x = __fadd_rn(x, dpp_f<DPP_ROW_SHR8>(x));      // inclusive within each row of 16
  const float r0 = lane_f(x, 15), r1 = lane_f(x, 31), r2 = lane_f(x, 47), r3 = lane_f(x, 63);
  const float b2 = __fadd_rn(r0, r1), b3 = __fadd_rn(b2, r2);
  const int rw = lane >> 4;
  const float rb = rw == 0 ? 0.0f : rw == 1 ? r0 : rw == 2 ? b2 : b3;
  total = __fadd_rn(b3, r3);
  return __fadd_rn(rb, dpp_f<DPP_ROW_SHR1>(x));
}

// One chunk's part of C: e (kept bins only) in, C out with -inf in the bins that cannot be drawn
// (e == 0), so that a draw is one compare per element; `base` moves on to the chunk's last C.
template <int E>
__device__ __forceinline__ void chunk_prefix(const float (&e)[E], int lane, float& base, float (&C)[E]) {
  float p = 0.0f, loc[E];
#pragma unroll
  for (int j = 0; j < E; ++j) {
    p = __fadd_rn(p, e[j]);
    loc[j] = p;
  }
  float total;
  const float off = __fadd_rn(base, wave_exclusive_scan(p, lane, total));
  float last = 0.0f;
#pragma unroll
  for (int j = 0; j < E; ++j) {
    last = __fadd_rn(off, loc[j]);
    C[j] = (e[j] > 0.0f) ? last : -INFINITY;
  }
  base = lane_f(last, 63);
}

// The highest index a lane holds with e > 0, as the wave's (-1: none).
__device__ __forceinline__ int wave_max_index(int i) { return -wave_min_index(-i); }

// The top-k / top-p search of a row held in registers (k_sample, k_score): v the raw logits
// (padding -inf), e their exp_shifted.  Leaves e == 0 outside the kept set, the elements' keys in
// `key` (padding: 0, below every candidate) and the threshold key in `theta`: kept = {key >= theta}.
// Returns |kept|.
template <class T, int NCH>
__device__ __forceinline__ int truncate_row(const float (&v)[NCH][T::EPL], float (&e)[NCH][T::EPL], int lane, int V,
                                            int top_k, float top_p, uint32_t (&key)[NCH][T::EPL], uint32_t& theta) {
  constexpr int E = T::EPL, CH = 64 * E;
  constexpr int BITS = SampleKey<T>::BITS;
#pragma unroll
  for (int c = 0; c < NCH; ++c)
#pragma unroll
    for (int j = 0; j < E; ++j) key[c][j] = (c * CH + lane * E + j < V) ? sample_key<T>(v[c][j]) : 0u;
  theta = 1;
  if (top_k > 0 && top_k < V) {                                    // the k-th largest key
    uint32_t t = 0;
#pragma unroll 1
    for (int b = BITS - 1; b >= 0; --b) {
      const uint32_t cand = t | (1u << b);
      int n = 0;
#pragma unroll
      for (int c = 0; c < NCH; ++c)
#pragma unroll
        for (int j = 0; j < E; ++j) n += wave_count(key[c][j] >= cand);
      t = (n >= top_k) ? cand : t;
    }
    theta = max(t, 1u);
#pragma unroll
    for (int c = 0; c < NCH; ++c)
#pragma unroll
      for (int j = 0; j < E; ++j) e[c][j] = (key[c][j] >= theta) ? e[c][j] : 0.0f;
  }
  if (top_p < 1.0f) {                           // the largest key whose upper set holds p of the mass
    float ls = 0.0f;
#pragma unroll
    for (int c = 0; c < NCH; ++c)
#pragma unroll
      for (int j = 0; j < E; ++j) ls = __fadd_rn(ls, e[c][j]);
    const float need = __fmul_rn(top_p, wave_sum(ls));
    uint32_t t = 0;
#pragma unroll 1
    for (int b = BITS - 1; b >= 0; --b) {
      const uint32_t cand = t | (1u << b);
      float lm = 0.0f;
#pragma unroll
      for (int c = 0; c < NCH; ++c)
#pragma unroll
        for (int j = 0; j < E; ++j) lm = __fadd_rn(lm, (key[c][j] >= cand) ? e[c][j] : 0.0f);
      t = (wave_sum(lm) >= need) ? cand : t;
    }
    theta = max(t, theta);
#pragma unroll
    for (int c = 0; c < NCH; ++c)
#pragma unroll
      for (int j = 0; j < E; ++j) e[c][j] = (key[c][j] >= theta) ? e[c][j] : 0.0f;
  }
  int kept = 0;
#pragma unroll
  for (int c = 0; c < NCH; ++c)
#pragma unroll
    for (int j = 0; j < E; ++j) kept += wave_count(key[c][j] >= theta);
  return kept;
}

// A row's online maximum and sum, LG_ONLINE_U chunks in flight (k_sample_long, k_score_long): the
// exact maximum mx of the raw elements, zmax = mx / tau and s = sum_v exp(l_v / tau - zmax), every
// lane rescaling its own sum when its maximum grows, the lanes brought to zmax before wave_sum.
template <class T>
__device__ __forceinline__ void online_max_sum(const typename T::raw* rowp, bool aligned, int V, int lane,
                                               float inv_tau, float& mx, float& zmax, float& s) {
  constexpr int E = T::EPL, CH = 64 * E, U = LG_ONLINE_U;
  float ml = -INFINITY, zm = 0.0f, ls = 0.0f;              // zm: ml / tau, 0 while ml is -inf
  for (int c0 = 0; c0 < V; c0 += U * CH) {
    Vec16 q[U];
#pragma unroll
    for (int k = 0; k < U; ++k) q[k] = load_piece<T>(rowp, aligned, c0 + k * CH + lane * E, V);
#pragma unroll
    for (int k = 0; k < U; ++k) {
      float v[E];
      unpack_piece<T>(q[k], c0 + k * CH + lane * E, V, v);
      float cm = ml;
#pragma unroll
      for (int j = 0; j < E; ++j) cm = fmaxf(cm, v[j]);
      if (cm > ml) {                                       // the lane's maximum grew: rescale its sum
        const float zn = __fmul_rn(cm, inv_tau);
        const float f = (ml == -INFINITY) ? 0.0f : __builtin_amdgcn_exp2f(__fmul_rn(__fsub_rn(zm, zn), LG_LOG2E));
        ls = __fmul_rn(ls, f);
        ml = cm;
        zm = zn;
      }
#pragma unroll
      for (int j = 0; j < E; ++j) ls = __fadd_rn(ls, exp_shifted(v[j], inv_tau, zm));
    }
  }
  mx = wave_max_value(ml);
  zmax = __fmul_rn(mx, inv_tau);
  const float f = (ml == -INFINITY) ? 0.0f : __builtin_amdgcn_exp2f(__fmul_rn(__fsub_rn(zm, zmax), LG_LOG2E));
  s = wave_sum(__fmul_rn(ls, f));
}

// Rows of up to NCH chunks, R of them per wave at a time, held in registers.  TRUNC: top-k / top-p.
template <class T, int NCH, int R, bool TRUNC>
__global__ __launch_bounds__(LG_THREADS) void k_sample(SampleArgs a) {
  using raw = typename T::raw;
  constexpr int E = T::EPL, CH = 64 * E;
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int V = a.V;
  const int64_t ngroups = (a.rows + R - 1) / R;

  for (int64_t g = (int64_t)blockIdx.x * LG_WAVES + wave; g < ngroups; g += (int64_t)gridDim.x * LG_WAVES) {
    int64_t off[R];
    group_offsets<R>(g * R, a.rows, a.K, a.sb, a.sk, off);
    float us[R];                                                       // lane s: the row's u_s
#pragma unroll
    for (int r = 0; r < R; ++r)
      us[r] = (lane < a.S) ? a.u[(int64_t)lane * a.rows + min(g * R + r, a.rows - 1)] : 0.0f;
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
      const int64_t row = g * R + r;
      if (row >= a.rows) continue;                                     // a row the group lacks (wave-uniform)
      float v[NCH][E];
#pragma unroll
      for (int c = 0; c < NCH; ++c) unpack_piece<T>(q[r][c], c * CH + lane * E, V, v[c]);
      float mx = -INFINITY;
#pragma unroll
      for (int c = 0; c < NCH; ++c)
#pragma unroll
        for (int j = 0; j < E; ++j) mx = fmaxf(mx, v[c][j]);
      mx = wave_max_value(mx);
      const float zmax = __fmul_rn(mx, a.inv_tau);
      float e[NCH][E];
#pragma unroll
      for (int c = 0; c < NCH; ++c)
#pragma unroll
        for (int j = 0; j < E; ++j) e[c][j] = exp_shifted(v[c][j], a.inv_tau, zmax);   // padding: 0

      int kept = V;
      if constexpr (TRUNC) {
        uint32_t key[NCH][E], theta;
        kept = truncate_row<T, NCH>(v, e, lane, V, a.top_k, a.top_p, key, theta);
      }

      float C[NCH][E];
      float s2 = 0.0f;
#pragma unroll
      for (int c = 0; c < NCH; ++c) chunk_prefix<E>(e[c], lane, s2, C[c]);
      const float ln_s2 = __fmul_rn(__builtin_amdgcn_logf(s2), LG_LN2);

      int my_tok = 0;
      float my_lp = 0.0f;
      for (int s = 0; s < a.S; ++s) {
        const float target = __fmul_rn(lane_f(us[r], s), s2);
        int first = LG_MAX_V;
#pragma unroll
        for (int c = NCH - 1; c >= 0; --c)
#pragma unroll
          for (int j = E - 1; j >= 0; --j) first = (C[c][j] > target) ? c * CH + lane * E + j : first;
        int tk = wave_min_index(first);
        if (tk >= LG_MAX_V) {                                          // rounding (or a NaN) left none
          int last = -1;
#pragma unroll
          for (int c = 0; c < NCH; ++c)
#pragma unroll
            for (int j = 0; j < E; ++j) last = (e[c][j] > 0.0f) ? c * CH + lane * E + j : last;
          tk = max(wave_max_index(last), 0);
        }
        float lt = 0.0f;
#pragma unroll
        for (int c = 0; c < NCH; ++c) {
          const int rel = tk - c * CH;
          if (rel >= 0 && rel < CH) lt = pick_piece<E>(v[c], rel);
        }
        const float lp = __fsub_rn(fmaf(lt, a.inv_tau, -zmax), ln_s2);
        my_tok = (lane == s) ? tk : my_tok;
        my_lp = (lane == s) ? lp : my_lp;
      }
      if (lane < a.S) {
        a.tok[(int64_t)lane * a.rows + row] = (int64_t)my_tok + a.tok_offset;
        if (a.logprob != nullptr) a.logprob[(int64_t)lane * a.rows + row] = my_lp;
      }
      if (lane == 0 && a.kept != nullptr) a.kept[row] = kept;
    }
  }
}

// Rows of any length, one per wave, no truncation.  Pass 1: the online maximum and sum.  Pass 2
// reads the row again (from the L2 pass 1 pulled it through), carries the running prefix chunk by
// chunk and holds the S targets one per lane: a draw is looked for in the first chunk whose last C
// exceeds its target.
template <class T>
__global__ __launch_bounds__(LG_THREADS) void k_sample_long(SampleArgs a) {
  using raw = typename T::raw;
  constexpr int E = T::EPL, CH = 64 * E, U = LG_ONLINE_U;
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int V = a.V;

  for (int64_t row = (int64_t)blockIdx.x * LG_WAVES + wave; row < a.rows; row += (int64_t)gridDim.x * LG_WAVES) {
    int64_t off[1];
    group_offsets<1>(row, a.rows, a.K, a.sb, a.sk, off);
    const raw* rowp = static_cast<const raw*>(a.logits) + off[0];
    const bool aligned = (reinterpret_cast<uintptr_t>(rowp) & 15) == 0;
    const float u = (lane < a.S) ? a.u[(int64_t)lane * a.rows + row] : 0.0f;
    float mx, zmax, s2;
    online_max_sum<T>(rowp, aligned, V, lane, a.inv_tau, mx, zmax, s2);
    const float ln_s2 = __fmul_rn(__builtin_amdgcn_logf(s2), LG_LN2);
    const float target = __fmul_rn(u, s2);

    bool open = lane < a.S;                                  // this lane's draw has no token yet
    int my_tok = 0, hi = -1;                                 // hi: the lane's highest index with e > 0
    float my_lt = 0.0f, hv = 0.0f;                           // hv: the logit there
    float base = 0.0f;
    for (int c0 = 0; c0 < V; c0 += U * CH) {
      Vec16 q[U];
#pragma unroll
      for (int k = 0; k < U; ++k) q[k] = load_piece<T>(rowp, aligned, c0 + k * CH + lane * E, V);
#pragma unroll
      for (int k = 0; k < U; ++k) {
        const int cb = c0 + k * CH, e0 = cb + lane * E;
        if (cb >= V) break;                                  // wave-uniform
        float v[E], e[E], C[E];
        unpack_piece<T>(q[k], e0, V, v);
#pragma unroll
        for (int j = 0; j < E; ++j) {
          e[j] = exp_shifted(v[j], a.inv_tau, zmax);
          hi = (e[j] > 0.0f) ? e0 + j : hi;
          hv = (e[j] > 0.0f) ? v[j] : hv;
        }
        chunk_prefix<E>(e, lane, base, C);
        uint64_t m = __builtin_amdgcn_ballot_w64(open && target < base);
        while (m != 0) {
          const int s = __builtin_ctzll(m);
          m &= m - 1;
          const float t = lane_f(target, s);
          int first = LG_MAX_V;
#pragma unroll
          for (int j = E - 1; j >= 0; --j) first = (C[j] > t) ? e0 + j : first;
          const int tk = wave_min_index(first);
          if (tk < LG_MAX_V) {                               // else: a later chunk, or the fallback
            const float lt = pick_piece<E>(v, tk - cb);
            const bool mine = lane == s;
            my_tok = mine ? tk : my_tok;
            my_lt = mine ? lt : my_lt;
            open = mine ? false : open;
          }
        }
      }
    }
    const int top = wave_max_index(hi);                      // rounding (or a NaN) left some draw open
    const float top_l = lane_f(hv, (max(top, 0) / E) & 63);
    if (open) {
      my_tok = max(top, 0);
      my_lt = top_l;
    }
    if (lane < a.S) {
      a.tok[(int64_t)lane * a.rows + row] = (int64_t)my_tok + a.tok_offset;
      if (a.logprob != nullptr)
        a.logprob[(int64_t)lane * a.rows + row] = __fsub_rn(fmaf(my_lt, a.inv_tau, -zmax), ln_s2);
    }
    if (lane == 0 && a.kept != nullptr) a.kept[row] = V;
  }
}

// ----------------------------------------------------------------- scoring kernels --
// beast_score_rows / beast_score_rows_bwd on the same row machinery: the log-probability of S given
// tokens per row, the entropy and the divergence from a reference row, under exactly the
// distribution k_sample draws from.  zmax, e, the kept set (truncate_row) and S2 (chunk_prefix's
// running total in registers, online_max_sum beyond four chunks) are the sampler's, so
//   log pi_v = (l_v / tau - zmax) - log S2          (kept v;  -inf, pi_v = 0 elsewhere)
// of a token has the bits of the sampler's logprob_out.  The S tokens sit one per lane; a draw's
// logit is picked by readlanes of a wave-uniform index (pick_piece), a token is never an address.
//   H  = -sum_kept pi_v log pi_v        KL = sum_kept pi_v (log pi_v - log rho_v),
//   log rho_v = (r_v / tau - zr) - log sr over all V bins of the reference row r
// with every pi_v == 0 term left out by a select.  The forward leaves in stats, per row,
//   [0] zmax  [1] S2  [2] theta (the lowest kept raw logit; -inf without a truncation)  [3] H  [4] KL
//   [5] zr  [6] sr  [7] 0  [8], [9] the low and high 32 bits (as bit patterns) of the mask of the
//   draws that take part in the backward: token in range, not ignored, logprob > -inf
// so that the backward repeats neither the threshold search nor a row sum:
//   grad_v = (1/tau) [ sum_s g_s 1[t_s = v] - pi_v (G + g_H (log pi_v + H) - g_KL (log pi_v - log rho_v - KL)) ]
// with G = sum_s g_s over the draws that take part (one per lane, wave_sum) and pi_v == 0 terms
// left out by a select: a bin outside the kept set, or with a -inf logit, gets exactly 0.
constexpr int SCORE_STATS = 10;
constexpr int SCORE_NO_TOKEN = -1, SCORE_BAD_TOKEN = -2;

struct ScoreArgs {
  const void* logits;
  int64_t sb, sk;        // element strides of the batch and the token axis
  int64_t rows;          // B * K
  int64_t K;             // folded_k of the strides
  const void* ref;       // nullable
  int64_t rsb, rsk, rK;
  int V;
  float inv_tau;
  int top_k;             // 0: no top-k
  float top_p;           // 1: no top-p
  const int64_t* tok;    // [S][rows]
  int S;
  int64_t tok_offset, ignore_index;
  float* logprob;        // forward outputs, nullable
  float* entropy;
  float* kl;
  int32_t* kept;
  float* stats;          // forward: out (nullable); backward: in
  // backward only
  const float* g_lp;     // nullable [S][rows]
  const float* g_h;      // nullable [rows]
  const float* g_kl;     // nullable [rows]
  void* grad;
  int64_t gsb, gsk, gK;
};

// Lane s: draw s's bin of the row, SCORE_NO_TOKEN where it is ignored (or s >= S), SCORE_BAD_TOKEN
// where it lies outside [tok_offset, tok_offset + V).
__device__ __forceinline__ int score_token(const ScoreArgs& a, int64_t row, int lane) {
  if (lane >= a.S) return SCORE_NO_TOKEN;
  const int64_t raw = a.tok[(int64_t)lane * a.rows + row];
  const int64_t tk = raw - a.tok_offset;
  if (raw == a.ignore_index) return SCORE_NO_TOKEN;
  if (tk < 0 || tk >= a.V) return SCORE_BAD_TOKEN;
  return (int)tk;
}

__device__ __forceinline__ float wave_min_value(float x) { return -wave_max_value(-x); }

__device__ __forceinline__ float ln_of(float s) { return __fmul_rn(__builtin_amdgcn_logf(s), LG_LN2); }

// One element's terms of H and KL: pi log pi and pi (log pi - log rho), 0 where pi == 0.
struct ScoreTerms {
  float h, k;
};
__device__ __forceinline__ void score_terms(float l, float e, float r, bool with_ref, float inv_tau, float zmax,
                                            float ln_s2, float inv_s2, float zr, float ln_sr, ScoreTerms& t) {
  const float p = __fmul_rn(e, inv_s2);
  const float lp = __fsub_rn(fmaf(l, inv_tau, -zmax), ln_s2);
  t.h = __fadd_rn(t.h, (p > 0.0f) ? __fmul_rn(p, lp) : 0.0f);
  if (with_ref) {
    const float lr = __fsub_rn(fmaf(r, inv_tau, -zr), ln_sr);
    t.k = __fadd_rn(t.k, (p > 0.0f) ? __fmul_rn(p, __fsub_rn(lp, lr)) : 0.0f);
  }
}

// What lane 0 stores for a row, and lanes 0 .. S-1 for its draws.
__device__ __forceinline__ void score_store(const ScoreArgs& a, int64_t row, int lane, int ti, float my_lp, float zmax,
                                            float s2, float theta, float H, float KL, float zr, float sr, int kept) {
  const bool part = ti >= 0 && my_lp > -INFINITY;
  const uint64_t mask = __builtin_amdgcn_ballot_w64(part);
  if (lane < a.S && a.logprob != nullptr) a.logprob[(int64_t)lane * a.rows + row] = my_lp;
  if (lane != 0) return;
  if (a.entropy != nullptr) a.entropy[row] = H;
  if (a.kl != nullptr) a.kl[row] = KL;
  if (a.kept != nullptr) a.kept[row] = kept;
  if (a.stats != nullptr) {
    float* st = a.stats + row * SCORE_STATS;
    st[0] = zmax; st[1] = s2; st[2] = theta; st[3] = H; st[4] = KL; st[5] = zr; st[6] = sr; st[7] = 0.0f;
    st[8] = __uint_as_float((uint32_t)mask);
    st[9] = __uint_as_float((uint32_t)(mask >> 32));
  }
}

// Rows of up to NCH chunks, R of them per wave at a time, held in registers.  TRUNC: top-k / top-p.
template <class T, int NCH, int R, bool TRUNC>
__global__ __launch_bounds__(LG_THREADS) void k_score(ScoreArgs a) {
  using raw = typename T::raw;
  constexpr int E = T::EPL, CH = 64 * E;
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int V = a.V;
  const bool with_ref = a.ref != nullptr && (a.kl != nullptr || a.stats != nullptr);
  const bool sums = with_ref || a.entropy != nullptr || a.stats != nullptr;
  const bool draws = a.S > 0 && (a.logprob != nullptr || a.stats != nullptr);
  const int64_t ngroups = (a.rows + R - 1) / R;

  for (int64_t g = (int64_t)blockIdx.x * LG_WAVES + wave; g < ngroups; g += (int64_t)gridDim.x * LG_WAVES) {
    int64_t off[R], roff[R];
    group_offsets<R>(g * R, a.rows, a.K, a.sb, a.sk, off);
    if (with_ref) group_offsets<R>(g * R, a.rows, a.rK, a.rsb, a.rsk, roff);
    int ti[R];                                                         // lane s: the row's token s
#pragma unroll
    for (int r = 0; r < R; ++r) ti[r] = draws ? score_token(a, min(g * R + r, a.rows - 1), lane) : SCORE_NO_TOKEN;
    Vec16 q[R][NCH], qr[R][NCH];
#pragma unroll
    for (int r = 0; r < R; ++r) {
      const raw* rowp = static_cast<const raw*>(a.logits) + off[r];
      const bool aligned = (reinterpret_cast<uintptr_t>(rowp) & 15) == 0;
#pragma unroll
      for (int c = 0; c < NCH; ++c) q[r][c] = load_piece<T>(rowp, aligned, c * CH + lane * E, V);
    }
#pragma unroll
    for (int r = 0; r < R; ++r) {
      if (with_ref) {
        const raw* refp = static_cast<const raw*>(a.ref) + roff[r];
        const bool aligned = (reinterpret_cast<uintptr_t>(refp) & 15) == 0;
#pragma unroll
        for (int c = 0; c < NCH; ++c) qr[r][c] = load_piece<T>(refp, aligned, c * CH + lane * E, V);
      } else {
#pragma unroll
        for (int c = 0; c < NCH; ++c) qr[r][c] = Vec16{0u, 0u, 0u, 0u};
      }
    }
#pragma unroll
    for (int r = 0; r < R; ++r) {
      const int64_t row = g * R + r;
      if (row >= a.rows) continue;                                     // a row the group lacks (wave-uniform)
      float v[NCH][E];
#pragma unroll
      for (int c = 0; c < NCH; ++c) unpack_piece<T>(q[r][c], c * CH + lane * E, V, v[c]);
      float mx = -INFINITY;
#pragma unroll
      for (int c = 0; c < NCH; ++c)
#pragma unroll
        for (int j = 0; j < E; ++j) mx = fmaxf(mx, v[c][j]);
      mx = wave_max_value(mx);
      const float zmax = __fmul_rn(mx, a.inv_tau);
      float e[NCH][E];
#pragma unroll
      for (int c = 0; c < NCH; ++c)
#pragma unroll
        for (int j = 0; j < E; ++j) e[c][j] = exp_shifted(v[c][j], a.inv_tau, zmax);   // padding: 0

      int kept = V;
      float theta = -INFINITY;
      if constexpr (TRUNC) {
        uint32_t key[NCH][E], tkey;
        kept = truncate_row<T, NCH>(v, e, lane, V, a.top_k, a.top_p, key, tkey);
        float lo = INFINITY;                                           // the lowest kept raw logit
#pragma unroll
        for (int c = 0; c < NCH; ++c)
#pragma unroll
          for (int j = 0; j < E; ++j) lo = fminf(lo, (key[c][j] >= tkey) ? v[c][j] : INFINITY);
        theta = wave_min_value(lo);
      }

      float s2 = 0.0f;                                                 // in the sampler's order
#pragma unroll
      for (int c = 0; c < NCH; ++c) {
        float C[E];
        chunk_prefix<E>(e[c], lane, s2, C);
      }
      const float ln_s2 = ln_of(s2);

      float H = 0.0f, KL = 0.0f, zr = 0.0f, sr = 0.0f;
      if (sums) {
        const float inv_s2 = __fdiv_rn(1.0f, s2);
        float rv[NCH][E];
        float ln_sr = 0.0f;
        if (with_ref) {
          float rmx = -INFINITY;
#pragma unroll
          for (int c = 0; c < NCH; ++c) {
            unpack_piece<T>(qr[r][c], c * CH + lane * E, V, rv[c]);
#pragma unroll
            for (int j = 0; j < E; ++j) rmx = fmaxf(rmx, rv[c][j]);
          }
          zr = __fmul_rn(wave_max_value(rmx), a.inv_tau);
          float ls = 0.0f;
#pragma unroll
          for (int c = 0; c < NCH; ++c)
#pragma unroll
            for (int j = 0; j < E; ++j) ls = __fadd_rn(ls, exp_shifted(rv[c][j], a.inv_tau, zr));
          sr = wave_sum(ls);
          ln_sr = ln_of(sr);
        } else {
#pragma unroll
          for (int c = 0; c < NCH; ++c)
#pragma unroll
            for (int j = 0; j < E; ++j) rv[c][j] = 0.0f;
        }
        ScoreTerms t{0.0f, 0.0f};
#pragma unroll
        for (int c = 0; c < NCH; ++c)
#pragma unroll
          for (int j = 0; j < E; ++j)
            score_terms(v[c][j], e[c][j], rv[c][j], with_ref, a.inv_tau, zmax, ln_s2, inv_s2, zr, ln_sr, t);
        H = -wave_sum(t.h);
        if (with_ref) KL = wave_sum(t.k);
      }

      float my_lp = 0.0f;
      if (draws) {
        for (int s = 0; s < a.S; ++s) {
          const int tk = __builtin_amdgcn_readlane(ti[r], s);
          float lp = 0.0f;
          if (tk >= 0) {
            float lt = 0.0f;
#pragma unroll
            for (int c = 0; c < NCH; ++c) {
              const int rel = tk - c * CH;
              if (rel >= 0 && rel < CH) lt = pick_piece<E>(v[c], rel);
            }
            lp = (lt >= theta) ? __fsub_rn(fmaf(lt, a.inv_tau, -zmax), ln_s2) : -INFINITY;
          } else if (tk == SCORE_BAD_TOKEN) {
            lp = __builtin_nanf("");
          }
          my_lp = (lane == s) ? lp : my_lp;
        }
      }
      score_store(a, row, lane, ti[r], my_lp, zmax, s2, theta, H, KL, zr, sr, kept);
    }
  }
}

// Rows of any length, one per wave, no truncation.  Pass 1: the online maximum and sum of the row
// (and of the reference row).  Pass 2 reads them again (from the L2 pass 1 pulled them through) for
// the draws' logits and the terms of H and KL.
template <class T>
__global__ __launch_bounds__(LG_THREADS) void k_score_long(ScoreArgs a) {
  using raw = typename T::raw;
  constexpr int E = T::EPL, CH = 64 * E, U = LG_ONLINE_U;
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int V = a.V;
  const bool with_ref = a.ref != nullptr && (a.kl != nullptr || a.stats != nullptr);
  const bool sums = with_ref || a.entropy != nullptr || a.stats != nullptr;
  const bool draws = a.S > 0 && (a.logprob != nullptr || a.stats != nullptr);

  for (int64_t row = (int64_t)blockIdx.x * LG_WAVES + wave; row < a.rows; row += (int64_t)gridDim.x * LG_WAVES) {
    int64_t off[1], roff[1] = {0};
    group_offsets<1>(row, a.rows, a.K, a.sb, a.sk, off);
    if (with_ref) group_offsets<1>(row, a.rows, a.rK, a.rsb, a.rsk, roff);
    const raw* rowp = static_cast<const raw*>(a.logits) + off[0];
    const raw* refp = with_ref ? static_cast<const raw*>(a.ref) + roff[0] : rowp;
    const bool aligned = (reinterpret_cast<uintptr_t>(rowp) & 15) == 0;
    const bool ref_al = (reinterpret_cast<uintptr_t>(refp) & 15) == 0;
    const int ti = draws ? score_token(a, row, lane) : SCORE_NO_TOKEN;
    float mx, zmax, s2;
    online_max_sum<T>(rowp, aligned, V, lane, a.inv_tau, mx, zmax, s2);
    const float ln_s2 = ln_of(s2);
    const float inv_s2 = __fdiv_rn(1.0f, s2);
    float rmx, zr = 0.0f, sr = 0.0f, ln_sr = 0.0f;
    if (with_ref) {
      online_max_sum<T>(refp, ref_al, V, lane, a.inv_tau, rmx, zr, sr);
      ln_sr = ln_of(sr);
    }
    ScoreTerms t{0.0f, 0.0f};
    float my_lt = 0.0f;
    if (sums || draws) {
      for (int c0 = 0; c0 < V; c0 += U * CH) {
        Vec16 q[U], qr[U];
#pragma unroll
        for (int k = 0; k < U; ++k) q[k] = load_piece<T>(rowp, aligned, c0 + k * CH + lane * E, V);
#pragma unroll
        for (int k = 0; k < U; ++k)
          qr[k] = with_ref ? load_piece<T>(refp, ref_al, c0 + k * CH + lane * E, V) : Vec16{0u, 0u, 0u, 0u};
#pragma unroll
        for (int k = 0; k < U; ++k) {
          const int cb = c0 + k * CH, e0 = cb + lane * E;
          if (cb >= V) break;                                          // wave-uniform
          float v[E], rv[E];
          unpack_piece<T>(q[k], e0, V, v);
          unpack_piece<T>(qr[k], e0, V, rv);
          if (sums) {
#pragma unroll
            for (int j = 0; j < E; ++j)
              score_terms(v[j], exp_shifted(v[j], a.inv_tau, zmax), rv[j], with_ref, a.inv_tau, zmax, ln_s2, inv_s2,
                          zr, ln_sr, t);
          }
          uint64_t m = __builtin_amdgcn_ballot_w64(ti >= cb && ti < cb + CH);
          while (m != 0) {
            const int s = __builtin_ctzll(m);
            m &= m - 1;
            const float lt = pick_piece<E>(v, __builtin_amdgcn_readlane(ti, s) - cb);
            my_lt = (lane == s) ? lt : my_lt;
          }
        }
      }
    }
    float H = 0.0f, KL = 0.0f;
    if (sums) {
      H = -wave_sum(t.h);
      if (with_ref) KL = wave_sum(t.k);
    }
    float my_lp = 0.0f;
    if (ti >= 0) my_lp = __fsub_rn(fmaf(my_lt, a.inv_tau, -zmax), ln_s2);
    else if (ti == SCORE_BAD_TOKEN) my_lp = __builtin_nanf("");
    score_store(a, row, lane, ti, my_lp, zmax, s2, -INFINITY, H, KL, zr, sr, V);
  }
}

// What the backward knows of a row before it meets the row's elements.
struct ScoreBwdRow {
  float zmax, ln_s2, inv_s2, theta, H, KL, zr, ln_sr;
  float gh, gk, G;       // the upstream gradients of H and KL; the sum of the draws' that take part
  float gs;              // lane s: g_s of draw s, 0 where it takes no part
  uint64_t part;         // the draws that take part
  bool bad;              // some token is out of range: a NaN row
};
__device__ __forceinline__ ScoreBwdRow score_bwd_row(const ScoreArgs& a, int64_t row, int lane, int ti, float g) {
  const float* st = a.stats + row * SCORE_STATS;
  ScoreBwdRow w;
  w.zmax = st[0];
  const float s2 = st[1];
  w.ln_s2 = ln_of(s2);
  w.inv_s2 = __fdiv_rn(1.0f, s2);
  w.theta = st[2];
  w.H = st[3];
  w.KL = st[4];
  w.zr = st[5];
  w.ln_sr = ln_of(st[6]);
  w.gh = a.g_h != nullptr ? a.g_h[row] : 0.0f;
  w.gk = a.g_kl != nullptr ? a.g_kl[row] : 0.0f;
  const uint64_t mask = (uint64_t)__float_as_uint(st[8]) | ((uint64_t)__float_as_uint(st[9]) << 32);
  w.part = mask & __builtin_amdgcn_ballot_w64(ti >= 0);
  w.gs = ((w.part >> lane) & 1) ? g : 0.0f;
  w.G = wave_sum(w.gs);
  w.bad = __builtin_amdgcn_ballot_w64(ti == SCORE_BAD_TOKEN) != 0;
  return w;
}

// The gradient of the chunk at `cb` (a wave-uniform element index): the draws whose token lies in it
// leave the sum of their g_s in the owner's slot; then the softmax terms.  The g_s of one token are
// summed by wave_sum over their lanes, the others 0 -- the order G is summed in, so that where every
// draw names one bin sum_s g_s 1[t_s = v] equals G to the bit and pi_v = 1 cancels it exactly.
template <class T>
__device__ __forceinline__ void score_bwd_piece(const ScoreArgs& a, const ScoreBwdRow& w, int cb, int lane, int ti,
                                                const float (&v)[T::EPL], const float (&rv)[T::EPL],
                                                typename T::raw (&o)[T::EPL]) {
  constexpr int E = T::EPL, CH = 64 * E;
  float d[E];
  if (w.bad) {
#pragma unroll
    for (int j = 0; j < E; ++j) d[j] = __builtin_nanf("");
    pack_piece<T>(d, o);
    return;
  }
  float acc[E];
#pragma unroll
  for (int j = 0; j < E; ++j) acc[j] = 0.0f;
  uint64_t m = w.part & __builtin_amdgcn_ballot_w64(ti >= cb && ti < cb + CH);
  while (m != 0) {                               // one turn per distinct token of the chunk
    const int tk = __builtin_amdgcn_readlane(ti, __builtin_ctzll(m));
    const uint64_t same = w.part & __builtin_amdgcn_ballot_w64(ti == tk);
    m &= ~same;
    const float g = wave_sum(((same >> lane) & 1) ? w.gs : 0.0f);
    const int rel = tk - cb;
    const bool own = lane == rel / E;
#pragma unroll
    for (int j = 0; j < E; ++j) acc[j] = (own && j == (rel & (E - 1))) ? g : acc[j];
  }
#pragma unroll
  for (int j = 0; j < E; ++j) {
    const float e = (v[j] >= w.theta) ? exp_shifted(v[j], a.inv_tau, w.zmax) : 0.0f;
    const float p = __fmul_rn(e, w.inv_s2);
    const float lp = __fsub_rn(fmaf(v[j], a.inv_tau, -w.zmax), w.ln_s2);
    float qv = w.G;
    if (a.g_h != nullptr) qv = fmaf(w.gh, __fadd_rn(lp, w.H), qv);
    if (a.g_kl != nullptr) {
      const float lr = __fsub_rn(fmaf(rv[j], a.inv_tau, -w.zr), w.ln_sr);
      qv = fmaf(-w.gk, __fsub_rn(__fsub_rn(lp, lr), w.KL), qv);
    }
    const float inner = __fsub_rn(acc[j], (p > 0.0f) ? __fmul_rn(p, qv) : 0.0f);
    d[j] = __fmul_rn(a.inv_tau, inner);
  }
  pack_piece<T>(d, o);
}

// Rows of up to NCH chunks, R of them per wave at a time, held in registers.
template <class T, int NCH, int R>
__global__ __launch_bounds__(LG_THREADS) void k_score_bwd(ScoreArgs a) {
  using raw = typename T::raw;
  constexpr int E = T::EPL, CH = 64 * E;
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int V = a.V;
  const bool with_ref = a.g_kl != nullptr;
  const int64_t ngroups = (a.rows + R - 1) / R;

  for (int64_t g = (int64_t)blockIdx.x * LG_WAVES + wave; g < ngroups; g += (int64_t)gridDim.x * LG_WAVES) {
    int64_t soff[R], roff[R], doff[R];
    group_offsets<R>(g * R, a.rows, a.K, a.sb, a.sk, soff);
    if (with_ref) group_offsets<R>(g * R, a.rows, a.rK, a.rsb, a.rsk, roff);
    group_offsets<R>(g * R, a.rows, a.gK, a.gsb, a.gsk, doff);
    int ti[R];
    float gl[R];
#pragma unroll
    for (int r = 0; r < R; ++r) {
      const int64_t row = min(g * R + r, a.rows - 1);
      ti[r] = a.g_lp != nullptr ? score_token(a, row, lane) : SCORE_NO_TOKEN;
      gl[r] = (a.g_lp != nullptr && lane < a.S) ? a.g_lp[(int64_t)lane * a.rows + row] : 0.0f;
    }
    Vec16 q[R][NCH], qr[R][NCH];
#pragma unroll
    for (int r = 0; r < R; ++r) {
      const raw* src = static_cast<const raw*>(a.logits) + soff[r];
      const bool aligned = (reinterpret_cast<uintptr_t>(src) & 15) == 0;
#pragma unroll
      for (int c = 0; c < NCH; ++c) q[r][c] = load_piece<T>(src, aligned, c * CH + lane * E, V);
    }
#pragma unroll
    for (int r = 0; r < R; ++r) {
      if (with_ref) {
        const raw* refp = static_cast<const raw*>(a.ref) + roff[r];
        const bool aligned = (reinterpret_cast<uintptr_t>(refp) & 15) == 0;
#pragma unroll
        for (int c = 0; c < NCH; ++c) qr[r][c] = load_piece<T>(refp, aligned, c * CH + lane * E, V);
      } else {
#pragma unroll
        for (int c = 0; c < NCH; ++c) qr[r][c] = Vec16{0u, 0u, 0u, 0u};
      }
    }
#pragma unroll
    for (int r = 0; r < R; ++r) {
      const int64_t row = g * R + r;
      if (row >= a.rows) continue;                                     // a row the group lacks
      const ScoreBwdRow w = score_bwd_row(a, row, lane, ti[r], gl[r]);
      raw* dst = static_cast<raw*>(a.grad) + doff[r];
      const bool aligned = (reinterpret_cast<uintptr_t>(dst) & 15) == 0;
#pragma unroll
      for (int c = 0; c < NCH; ++c) {
        const int e0 = c * CH + lane * E;
        if (c > 0 && c * CH >= V) break;
        float v[E], rv[E];
        unpack_piece<T>(q[r][c], e0, V, v);
        unpack_piece<T>(qr[r][c], e0, V, rv);
        raw o[E];
        score_bwd_piece<T>(a, w, c * CH, lane, ti[r], v, rv, o);
        store_piece<T>(dst, aligned, e0, V, o);
      }
    }
  }
}

// Rows of any length, one per wave: one pass, LG_ONLINE_U chunks in flight.
template <class T>
__global__ __launch_bounds__(LG_THREADS) void k_score_bwd_long(ScoreArgs a) {
  using raw = typename T::raw;
  constexpr int E = T::EPL, CH = 64 * E, U = LG_ONLINE_U;
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int V = a.V;
  const bool with_ref = a.g_kl != nullptr;

  for (int64_t row = (int64_t)blockIdx.x * LG_WAVES + wave; row < a.rows; row += (int64_t)gridDim.x * LG_WAVES) {
    int64_t soff[1], roff[1] = {0}, doff[1];
    group_offsets<1>(row, a.rows, a.K, a.sb, a.sk, soff);
    if (with_ref) group_offsets<1>(row, a.rows, a.rK, a.rsb, a.rsk, roff);
    group_offsets<1>(row, a.rows, a.gK, a.gsb, a.gsk, doff);
    const raw* src = static_cast<const raw*>(a.logits) + soff[0];
    const raw* refp = with_ref ? static_cast<const raw*>(a.ref) + roff[0] : src;
    raw* dst = static_cast<raw*>(a.grad) + doff[0];
    const bool src_al = (reinterpret_cast<uintptr_t>(src) & 15) == 0;
    const bool ref_al = (reinterpret_cast<uintptr_t>(refp) & 15) == 0;
    const bool dst_al = (reinterpret_cast<uintptr_t>(dst) & 15) == 0;
    const int ti = a.g_lp != nullptr ? score_token(a, row, lane) : SCORE_NO_TOKEN;
    const float gl = (a.g_lp != nullptr && lane < a.S) ? a.g_lp[(int64_t)lane * a.rows + row] : 0.0f;
    const ScoreBwdRow w = score_bwd_row(a, row, lane, ti, gl);
    for (int c0 = 0; c0 < V; c0 += U * CH) {
      Vec16 q[U], qr[U];
#pragma unroll
      for (int k = 0; k < U; ++k) q[k] = load_piece<T>(src, src_al, c0 + k * CH + lane * E, V);
#pragma unroll
      for (int k = 0; k < U; ++k)
        qr[k] = with_ref ? load_piece<T>(refp, ref_al, c0 + k * CH + lane * E, V) : Vec16{0u, 0u, 0u, 0u};
#pragma unroll
      for (int k = 0; k < U; ++k) {
        const int cb = c0 + k * CH, e0 = cb + lane * E;
        if (cb >= V) break;                                            // wave-uniform
        float v[E], rv[E];
        unpack_piece<T>(q[k], e0, V, v);
        unpack_piece<T>(qr[k], e0, V, rv);
        raw o[E];
        score_bwd_piece<T>(a, w, cb, lane, ti, v, rv, o);
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
template <auto K, int R, class Args>
int run_rows(const Args& a, const Queue& q, const char* what, int64_t* resident_rows) {
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

// The cross-entropy kernels: rows in flight per chunk count are the decode kernels' defaults.
template <class T>
int run_xent(bool backward, const XentArgs& a, const Queue& q) {
  const int chunks = (a.V + 64 * T::EPL - 1) / (64 * T::EPL);
  if (backward) {
    const char* what = "k_xent_bwd";
    if (chunks == 1) return run_rows<k_xent_bwd<T, 1, 4>, 4>(a, q, what, nullptr);
    if (chunks == 2) return run_rows<k_xent_bwd<T, 2, 2>, 2>(a, q, what, nullptr);
    if (chunks <= LG_MAX_CHUNKS) return run_rows<k_xent_bwd<T, LG_MAX_CHUNKS, 1>, 1>(a, q, what, nullptr);
    return run_rows<k_xent_bwd_long<T>, 1>(a, q, "k_xent_bwd_long", nullptr);
  }
  const char* what = "k_xent";
  if (chunks == 1) return run_rows<k_xent<T, 1, 4>, 4>(a, q, what, nullptr);
  if (chunks == 2) return run_rows<k_xent<T, 2, 2>, 2>(a, q, what, nullptr);
  if (chunks <= LG_MAX_CHUNKS) return run_rows<k_xent<T, LG_MAX_CHUNKS, 1>, 1>(a, q, what, nullptr);
  return run_rows<k_xent_online<T>, 1>(a, q, "k_xent_online", nullptr);
}

int run_xent_typed(int dtype, bool backward, const XentArgs& a, const Queue& q) {
  switch (dtype) {
    case BEAST_LOGITS_F32: return run_xent<ElemF32>(backward, a, q);
    case BEAST_LOGITS_F16: return run_xent<ElemF16>(backward, a, q);
    default: return run_xent<ElemBF16>(backward, a, q);
  }
}

// The checks both cross-entropy directions share (before any HIP call), and the arguments they share.
int check_xent(const char* fn, const void* logits, int dtype, int64_t B, int K, int V, int64_t sb, int64_t sk,
               const int64_t* target_tok, const float* target_pos, float smoothing) {
  BEAST_TRY(check_common(fn, logits, dtype, B, K, V, sb, sk, 1.0f));
  BEAST_REQUIRE((target_tok != nullptr) != (target_pos != nullptr),
                "%s: exactly one of target_tok and target_pos must be given", fn);
  BEAST_REQUIRE(smoothing >= 0.0f && smoothing < 1.0f, "%s: smoothing must lie in [0, 1) (got %g)", fn,
                (double)smoothing);
  return BEAST_OK;
}

XentArgs xent_args(const void* logits, int64_t B, int K, int V, int64_t sb, int64_t sk, const int64_t* target_tok,
                   const float* target_pos, int64_t tok_offset, int64_t ignore_index, float smoothing) {
  XentArgs a{};
  a.logits = logits; a.sb = sb; a.sk = sk; a.rows = B * K; a.K = folded_k(B, K, sb, sk); a.V = V;
  a.vm1 = (float)(V - 1);
  a.tok = target_tok; a.pos = target_pos; a.tok_offset = tok_offset; a.ignore_index = ignore_index;
  a.eps = smoothing; a.keep = 1.0f - smoothing; a.eps_v = smoothing / (float)V;
  return a;
}

// The sampling kernels: rows in flight per chunk count are the decode kernels' defaults; the
// truncating form only where a truncation is asked for.
template <class T>
int run_sample(const SampleArgs& a, bool trunc, const Queue& q) {
  const int chunks = (a.V + 64 * T::EPL - 1) / (64 * T::EPL);
  const char* what = "k_sample";
  if (chunks > LG_MAX_CHUNKS) return run_rows<k_sample_long<T>, 1>(a, q, "k_sample_long", nullptr);
  if (trunc) {
    if (chunks == 1) return run_rows<k_sample<T, 1, 4, true>, 4>(a, q, what, nullptr);
    if (chunks == 2) return run_rows<k_sample<T, 2, 2, true>, 2>(a, q, what, nullptr);
    return run_rows<k_sample<T, LG_MAX_CHUNKS, 1, true>, 1>(a, q, what, nullptr);
  }
  if (chunks == 1) return run_rows<k_sample<T, 1, 4, false>, 4>(a, q, what, nullptr);
  if (chunks == 2) return run_rows<k_sample<T, 2, 2, false>, 2>(a, q, what, nullptr);
  return run_rows<k_sample<T, LG_MAX_CHUNKS, 1, false>, 1>(a, q, what, nullptr);
}

constexpr int SAMPLE_MAX_S = 64;      // one draw per lane

// The scoring kernels: rows in flight and the truncating form as for the sampling kernels.
template <class T>
int run_score(bool backward, const ScoreArgs& a, bool trunc, const Queue& q) {
  const int chunks = (a.V + 64 * T::EPL - 1) / (64 * T::EPL);
  if (backward) {
    const char* what = "k_score_bwd";
    if (chunks == 1) return run_rows<k_score_bwd<T, 1, 4>, 4>(a, q, what, nullptr);
    if (chunks == 2) return run_rows<k_score_bwd<T, 2, 2>, 2>(a, q, what, nullptr);
    if (chunks <= LG_MAX_CHUNKS) return run_rows<k_score_bwd<T, LG_MAX_CHUNKS, 1>, 1>(a, q, what, nullptr);
    return run_rows<k_score_bwd_long<T>, 1>(a, q, "k_score_bwd_long", nullptr);
  }
  const char* what = "k_score";
  if (chunks > LG_MAX_CHUNKS) return run_rows<k_score_long<T>, 1>(a, q, "k_score_long", nullptr);
  if (trunc) {
    if (chunks == 1) return run_rows<k_score<T, 1, 4, true>, 4>(a, q, what, nullptr);
    if (chunks == 2) return run_rows<k_score<T, 2, 2, true>, 2>(a, q, what, nullptr);
    return run_rows<k_score<T, LG_MAX_CHUNKS, 1, true>, 1>(a, q, what, nullptr);
  }
  if (chunks == 1) return run_rows<k_score<T, 1, 4, false>, 4>(a, q, what, nullptr);
  if (chunks == 2) return run_rows<k_score<T, 2, 2, false>, 2>(a, q, what, nullptr);
  return run_rows<k_score<T, LG_MAX_CHUNKS, 1, false>, 1>(a, q, what, nullptr);
}

// The checks both scoring directions share (before any HIP call); `trunc`: a truncation truncates.
int check_score(const char* fn, const void* logits, int dtype, int64_t B, int K, int V, int64_t sb, int64_t sk,
                const void* ref_logits, int64_t rsb, int64_t rsk, float temperature, int top_k, float top_p,
                const int64_t* tokens, int S, bool* trunc) {
  BEAST_TRY(check_common(fn, logits, dtype, B, K, V, sb, sk, temperature));
  BEAST_REQUIRE(ref_logits == nullptr || (rsb >= 0 && rsk >= 0), "%s: strides must be >= 0 (rsb=%lld, rsk=%lld)", fn,
                (long long)rsb, (long long)rsk);
  BEAST_REQUIRE(top_k >= 0, "%s: top_k must be >= 0 (got %d)", fn, top_k);
  BEAST_REQUIRE(top_p > 0.0f && top_p <= 1.0f, "%s: top_p must lie in (0, 1] (got %g)", fn, (double)top_p);
  BEAST_REQUIRE(S >= 0 && S <= SAMPLE_MAX_S, "%s: S must lie in [0, %d] (got %d)", fn, SAMPLE_MAX_S, S);
  BEAST_REQUIRE(S == 0 || tokens != nullptr, "%s: null tokens with S=%d", fn, S);
  *trunc = (top_k > 0 && top_k < V) || top_p < 1.0f;
  const int epl = dtype == BEAST_LOGITS_F32 ? ElemF32::EPL : ElemF16::EPL;
  BEAST_REQUIRE_CODE(!*trunc || V <= LG_MAX_CHUNKS * 64 * epl, BEAST_E_UNSUPPORTED,
                     "%s supports top_k / top_p for V <= %d of this dtype (V=%d)", fn, LG_MAX_CHUNKS * 64 * epl, V);
  return BEAST_OK;
}

ScoreArgs score_args(const void* logits, int64_t B, int K, int V, int64_t sb, int64_t sk, const void* ref_logits,
                     int64_t rsb, int64_t rsk, float temperature, int top_k, float top_p, const int64_t* tokens,
                     int S, int64_t tok_offset, int64_t ignore_index) {
  ScoreArgs a{};
  a.logits = logits; a.sb = sb; a.sk = sk; a.rows = B * K; a.K = folded_k(B, K, sb, sk); a.V = V;
  a.ref = ref_logits; a.rsb = rsb; a.rsk = rsk; a.rK = folded_k(B, K, rsb, rsk);
  a.inv_tau = (float)(1.0 / (double)temperature);
  a.top_k = (top_k > 0 && top_k < V) ? top_k : 0; a.top_p = top_p;
  a.tok = tokens; a.S = S; a.tok_offset = tok_offset; a.ignore_index = ignore_index;
  return a;
}

int run_score_typed(int dtype, bool backward, const ScoreArgs& a, bool trunc, const Queue& q) {
  switch (dtype) {
    case BEAST_LOGITS_F32: return run_score<ElemF32>(backward, a, trunc, q);
    case BEAST_LOGITS_F16: return run_score<ElemF16>(backward, a, trunc, q);
    default: return run_score<ElemBF16>(backward, a, trunc, q);
  }
}

}  // namespace

// =================================================================== C-ABI ==
extern "C" int beast_sample_rows(const void* logits, int dtype, int64_t B, int K, int V, int64_t sb, int64_t sk,
                                 float temperature, int top_k, float top_p, const float* uniforms, int S,
                                 int64_t tok_offset, int64_t* tokens_out, float* logprob_out, int32_t* kept_out,
                                 void* stream) {
  BEAST_TRY(check_common("beast_sample_rows", logits, dtype, B, K, V, sb, sk, temperature));
  BEAST_REQUIRE(top_k >= 0, "beast_sample_rows: top_k must be >= 0 (got %d)", top_k);
  BEAST_REQUIRE(top_p > 0.0f && top_p <= 1.0f, "beast_sample_rows: top_p must lie in (0, 1] (got %g)", (double)top_p);
  BEAST_REQUIRE(S >= 1 && S <= SAMPLE_MAX_S, "beast_sample_rows: S must lie in [1, %d] (got %d)", SAMPLE_MAX_S, S);
  BEAST_REQUIRE(uniforms != nullptr && tokens_out != nullptr, "beast_sample_rows: null pointer");
  const bool trunc = (top_k > 0 && top_k < V) || top_p < 1.0f;
  const int epl = dtype == BEAST_LOGITS_F32 ? ElemF32::EPL : ElemF16::EPL;
  BEAST_REQUIRE_CODE(!trunc || V <= LG_MAX_CHUNKS * 64 * epl, BEAST_E_UNSUPPORTED,
                     "beast_sample_rows supports top_k / top_p for V <= %d of this dtype (V=%d)",
                     LG_MAX_CHUNKS * 64 * epl, V);
  if (B == 0) return BEAST_OK;
  SampleArgs a{};
  a.logits = logits; a.sb = sb; a.sk = sk; a.rows = B * K; a.K = folded_k(B, K, sb, sk); a.V = V;
  a.inv_tau = (float)(1.0 / (double)temperature);
  a.top_k = (top_k > 0 && top_k < V) ? top_k : 0; a.top_p = top_p;
  a.u = uniforms; a.S = S; a.tok_offset = tok_offset;
  a.tok = tokens_out; a.logprob = logprob_out; a.kept = kept_out;
  Queue q;
  if (const int rc = queue_of(stream, q, "beast_sample_rows")) return rc;
  switch (dtype) {
    case BEAST_LOGITS_F32: return run_sample<ElemF32>(a, trunc, q);
    case BEAST_LOGITS_F16: return run_sample<ElemF16>(a, trunc, q);
    default: return run_sample<ElemBF16>(a, trunc, q);
  }
}

extern "C" int beast_score_rows(const void* logits, int dtype, int64_t B, int K, int V, int64_t sb, int64_t sk,
                                const void* ref_logits, int64_t rsb, int64_t rsk, float temperature, int top_k,
                                float top_p, const int64_t* tokens, int S, int64_t tok_offset, int64_t ignore_index,
                                float* logprob_out, float* entropy_out, float* kl_out, int32_t* kept_out,
                                float* stats_out, void* stream) {
  const char* fn = "beast_score_rows";
  bool trunc = false;
  BEAST_TRY(check_score(fn, logits, dtype, B, K, V, sb, sk, ref_logits, rsb, rsk, temperature, top_k, top_p, tokens, S,
                        &trunc));
  BEAST_REQUIRE(logprob_out || entropy_out || kl_out || kept_out || stats_out, "%s: no output requested", fn);
  BEAST_REQUIRE(logprob_out == nullptr || S >= 1, "%s: logprob_out needs S >= 1", fn);
  BEAST_REQUIRE(kl_out == nullptr || ref_logits != nullptr, "%s: kl_out needs ref_logits", fn);
  if (B == 0) return BEAST_OK;
  ScoreArgs a = score_args(logits, B, K, V, sb, sk, ref_logits, rsb, rsk, temperature, top_k, top_p, tokens, S,
                           tok_offset, ignore_index);
  a.logprob = logprob_out; a.entropy = entropy_out; a.kl = kl_out; a.kept = kept_out; a.stats = stats_out;
  Queue q;
  if (const int rc = queue_of(stream, q, fn)) return rc;
  return run_score_typed(dtype, false, a, trunc, q);
}

extern "C" int beast_score_rows_bwd(const void* logits, int dtype, int64_t B, int K, int V, int64_t sb, int64_t sk,
                                    const void* ref_logits, int64_t rsb, int64_t rsk, float temperature, int top_k,
                                    float top_p, const int64_t* tokens, int S, int64_t tok_offset,
                                    int64_t ignore_index, const float* stats, const float* grad_logprob,
                                    const float* grad_entropy, const float* grad_kl, void* grad_logits, int64_t gsb,
                                    int64_t gsk, void* stream) {
  const char* fn = "beast_score_rows_bwd";
  bool trunc = false;
  BEAST_TRY(check_score(fn, logits, dtype, B, K, V, sb, sk, ref_logits, rsb, rsk, temperature, top_k, top_p, tokens, S,
                        &trunc));
  BEAST_REQUIRE(stats && grad_logits, "%s: null pointer", fn);
  BEAST_REQUIRE(grad_logprob || grad_entropy || grad_kl, "%s: no upstream gradient given", fn);
  BEAST_REQUIRE(grad_logprob == nullptr || S >= 1, "%s: grad_logprob needs S >= 1", fn);
  BEAST_REQUIRE(grad_kl == nullptr || ref_logits != nullptr, "%s: grad_kl needs ref_logits", fn);
  BEAST_REQUIRE(gsb >= 0 && gsk >= V, "%s: grad_logits rows must not overlap (gsb=%lld, gsk=%lld, V=%d)", fn,
                (long long)gsb, (long long)gsk, V);
  if (B == 0) return BEAST_OK;
  ScoreArgs a = score_args(logits, B, K, V, sb, sk, ref_logits, rsb, rsk, temperature, top_k, top_p, tokens, S,
                           tok_offset, ignore_index);
  a.stats = const_cast<float*>(stats); a.g_lp = grad_logprob; a.g_h = grad_entropy; a.g_kl = grad_kl;
  a.grad = grad_logits; a.gsb = gsb; a.gsk = gsk; a.gK = folded_k(B, K, gsb, gsk);
  Queue q;
  if (const int rc = queue_of(stream, q, fn)) return rc;
  return run_score_typed(dtype, true, a, trunc, q);
}

extern "C" int beast_logits_expect(const void* logits, int dtype, int64_t B, int K, int V, int64_t sb, int64_t sk,
                                   float temperature, int64_t tok_offset, float* mean_out, int64_t* argmax_out,
                                   float* stats_out, void* stream) {
  BEAST_TRY(check_common("beast_logits_expect", logits, dtype, B, K, V, sb, sk, temperature));
  BEAST_REQUIRE(mean_out || argmax_out || stats_out, "beast_logits_expect: no output requested");
  if (B == 0) return BEAST_OK;
  LogitsArgs a{};
  a.logits = logits; a.sb = sb; a.sk = sk; a.rows = B * K; a.K = folded_k(B, K, sb, sk); a.V = V;
  a.inv_tau = (float)(1.0 / (double)temperature); a.vm1 = (float)(V - 1); a.tok_offset = tok_offset;
  a.mean = mean_out; a.amax = argmax_out; a.stats = stats_out;
  Queue q;
  if (const int rc = queue_of(stream, q, "beast_logits_expect")) return rc;
  return run_typed(dtype, false, a, q, nullptr);
}

extern "C" int beast_logits_expect_bwd(const void* logits, int dtype, int64_t B, int K, int V, int64_t sb, int64_t sk,
                                       float temperature, const float* mean, const float* stats,
                                       const float* grad_mean, void* grad_logits, int64_t gsb, int64_t gsk,
                                       void* stream) {
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
  if (const int rc = queue_of(stream, q, "beast_logits_expect_bwd")) return rc;
  return run_typed(dtype, true, a, q, nullptr);
}

extern "C" int64_t beast_logits_resident_rows(int dtype, int V, int backward, void* stream) {
  BEAST_REQUIRE(dtype == BEAST_LOGITS_F32 || dtype == BEAST_LOGITS_F16 || dtype == BEAST_LOGITS_BF16,
                "beast_logits_resident_rows: unknown dtype code %d", dtype);
  BEAST_REQUIRE_CODE(V >= LG_MIN_V && V <= LG_MAX_V, BEAST_E_UNSUPPORTED,
                     "beast_logits_resident_rows supports %d <= V <= %d (V=%d)", LG_MIN_V, LG_MAX_V, V);
  LogitsArgs a{};
  a.V = V;
  Queue q;
  if (const int rc = queue_of(stream, q, "beast_logits_resident_rows")) return rc;
  int64_t rows = 0;
  if (const int rc = run_typed(dtype, backward != 0, a, q, &rows)) return rc;
  return rows;
}

extern "C" int beast_xent_rows(const void* logits, int dtype, int64_t B, int K, int V, int64_t sb, int64_t sk,
                               const int64_t* target_tok, const float* target_pos, int64_t tok_offset,
                               int64_t ignore_index, float smoothing, float* loss_out, float* stats_out,
                               int64_t* argmax_out, void* stream) {
  BEAST_TRY(check_xent("beast_xent_rows", logits, dtype, B, K, V, sb, sk, target_tok, target_pos, smoothing));
  BEAST_REQUIRE(loss_out || stats_out || argmax_out, "beast_xent_rows: no output requested");
  if (B == 0) return BEAST_OK;
  XentArgs a = xent_args(logits, B, K, V, sb, sk, target_tok, target_pos, tok_offset, ignore_index, smoothing);
  a.loss = loss_out; a.stats = stats_out; a.amax = argmax_out;
  Queue q;
  if (const int rc = queue_of(stream, q, "beast_xent_rows")) return rc;
  return run_xent_typed(dtype, false, a, q);
}

extern "C" int beast_xent_rows_bwd(const void* logits, int dtype, int64_t B, int K, int V, int64_t sb, int64_t sk,
                                   const int64_t* target_tok, const float* target_pos, int64_t tok_offset,
                                   int64_t ignore_index, float smoothing, const float* stats,
                                   const float* grad_loss, void* grad_logits, int64_t gsb, int64_t gsk,
                                   void* stream) {
  BEAST_TRY(check_xent("beast_xent_rows_bwd", logits, dtype, B, K, V, sb, sk, target_tok, target_pos, smoothing));
  BEAST_REQUIRE(stats && grad_loss && grad_logits, "beast_xent_rows_bwd: null pointer");
  BEAST_REQUIRE(gsb >= 0 && gsk >= V, "beast_xent_rows_bwd: grad_logits rows must not overlap (gsb=%lld, "
                "gsk=%lld, V=%d)", (long long)gsb, (long long)gsk, V);
  if (B == 0) return BEAST_OK;
  XentArgs a = xent_args(logits, B, K, V, sb, sk, target_tok, target_pos, tok_offset, ignore_index, smoothing);
  a.gK = folded_k(B, K, gsb, gsk);
  a.stats = const_cast<float*>(stats); a.grad_loss = grad_loss; a.grad = grad_logits; a.gsb = gsb; a.gsk = gsk;
  Queue q;
  if (const int rc = queue_of(stream, q, "beast_xent_rows_bwd")) return rc;
  return run_xent_typed(dtype, true, a, q);
}
