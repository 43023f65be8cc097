// Per-trajectory weighted ridge fit for gfx950: every trajectory on its own time stamps, with
// sample weights (UniformBSpline.learn_mp_params_from_trajs with times [*add_dim, T],
// mp/uni_bspline.py:471-602, plus the tokenizer's clamp / quantise / offset).
//
//   k_fit_rows<K>   one wave per (trajectory, kind): the basis is evaluated from the times (bfun,
//                   basis_device.h: the bits of k_basis), G = Phi^T diag(w) Phi + reg I and
//                   R = Phi^T diag(w) Y accumulate in float64 on v_mfma_f64_16x16x4_f64, the
//                   wave solves [G | R] in LDS by Gauss-Jordan with partial pivoting, rounds once
//                   to fp32 and quantises with beast::quantize_one (k_quantize's arithmetic).
// There is no shared projection here: the shared-grid fit is codec.hip's.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "basis_device.h"
#include "codec_device.h"
#include "common.h"
#include "launch.h"

namespace {

constexpr int ROWS_WAVES = 4;    // waves per workgroup, one (trajectory, kind) each
constexpr int ROWS_MAX_N = 16, ROWS_MAX_T = 256, ROWS_MAX_D = 64, ROWS_MAX_DEGREE = 8;
constexpr int ROWS_MAX_TILES = ROWS_MAX_D / 16;

typedef double double4_t __attribute__((ext_vector_type(4)));

struct RowsArgs {
  const float* traj;
  int64_t B, sb, st, sd;
  const int32_t* dof_src;
  const float* times;
  int64_t times_sb;
  const float* weights;   // nullable: all ones
  int64_t weights_sb;
  const float* kv[2];     // knot vectors of kind 0 (degree K) and kind 1 (degree 0)
  const float* w_min;
  const float* w_max;
  float* params_out;
  long long* tokens_out;
  int64_t tok_offset;
  double reg;
  float tau, delay, vm1;
  int T, D, nj, N;
  int k0, nk;             // the first kind that has DoFs, and how many kinds have
  int ld;                 // row stride (doubles) of a wave's [16][ld] system in LDS
};

// acc[r] += sum_k a(row = lk + 4 r, k) * b(k, col = lc) over the chunk's 4 steps k: lane l holds
// a(l & 15, l >> 4) and b(l >> 4, l & 15).  The f64 C/D map is col = l & 15, row = (l >> 4) + 4 r.
// BEAST_ROWS_FMA (measurements): the same sums by v_fma_f64 through a wave-private LDS stage.
__device__ __forceinline__ double4_t outer4(double pa, double pb, double4_t acc, double* stage, int lane) {
#ifdef BEAST_ROWS_FMA
  const int lc = lane & 15, lk = lane >> 4;
  stage[lane] = pa;
  stage[64 + lane] = pb;
  wave_sync();
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const double b = stage[64 + 16 * k + lc];
#pragma unroll
    for (int r = 0; r < 4; ++r) acc[r] = fma(stage[16 * k + lk + 4 * r], b, acc[r]);
  }
  wave_sync();
  return acc;
#else
  (void)stage; (void)lane;
  return __builtin_amdgcn_mfma_f64_16x16x4f64(pa, pb, acc, 0, 0, 0);
#endif
}

// column c of the system for the compact index cc >= k: G's columns cc < N, then R's from 16
__device__ __forceinline__ int sys_col(int cc, int N) { return cc < N ? cc : 16 + (cc - N); }

template <int K>
__global__ __launch_bounds__(ROWS_WAVES * 64) void k_fit_rows(RowsArgs a) {
  extern __shared__ double smem[];
  __shared__ float s_kv[2][32];   // degree + 1 + N <= 25 knots per kind
#ifdef BEAST_ROWS_FMA
  __shared__ double s_stage[ROWS_WAVES][128];
#endif
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  if (tid < 64) {
    const int k = tid >> 5, i = tid & 31;
    const int n_kn = (k == 0 ? K : 0) + 1 + a.N;
    s_kv[k][i] = (a.kv[k] != nullptr && i < n_kn) ? a.kv[k][i] : 0.0f;
  }
  __syncthreads();
  double* A = smem + wave * 16 * a.ld;
#ifdef BEAST_ROWS_FMA
  double* stage = s_stage[wave];
#else
  double* stage = nullptr;
#endif
  const int lc = lane & 15, lk = lane >> 4;
  const int N = a.N, ld = a.ld, DN = a.D * a.N;
  const int64_t items = a.B * a.nk;
  for (int64_t it = blockIdx.x * (int64_t)ROWS_WAVES + wave; it < items; it += (int64_t)gridDim.x * ROWS_WAVES) {
    const int64_t b = a.nk == 2 ? (it >> 1) : it;
    const int kind = a.nk == 2 ? (int)(it & 1) : a.k0;
    const int d0 = kind ? a.nj : 0, dk = kind ? a.D - a.nj : a.nj;
    const int ntile = (dk + 15) >> 4;
    const float* tb = a.times + b * a.times_sb;
    const float* wb = a.weights ? a.weights + b * a.weights_sb : nullptr;
    const float* yb = a.traj + b * a.sb;
    int64_t src[ROWS_MAX_TILES];
    bool dv[ROWS_MAX_TILES];
#pragma unroll
    for (int tl = 0; tl < ROWS_MAX_TILES; ++tl) {
      const int dl = tl * 16 + lc;
      dv[tl] = tl < ntile && dl < dk;
      src[tl] = dv[tl] ? a.dof_src[d0 + dl] * a.sd : 0;
    }
    // --- G and R over chunks of 4 steps: this lane's step is t0 + lk, its basis function lc ---
    double4_t g = {0.0, 0.0, 0.0, 0.0};
    double4_t r[ROWS_MAX_TILES] = {};
    for (int t0 = 0; t0 < a.T; t0 += 4) {
      const int t = t0 + lk;
      float w = 0.0f;
      if (t < a.T) w = wb ? wb[t] : 1.0f;
      // weight 0 skips the sample: its time and values are never used (they may be NaN)
      const bool use = t < a.T && !(w == 0.0f);
      float phi = 0.0f;
      if (use && lc < N) {
        const float u = phase_clip(tb[t], a.tau, a.delay);
        phi = kind ? bfun<0>(lc, u, s_kv[1], N) : bfun<K>(lc, u, s_kv[0], N);
      }
      const double pa = (double)phi, wd = use ? (double)w : 0.0;
      g = outer4(pa, wd * pa, g, stage, lane);
#pragma unroll
      for (int tl = 0; tl < ROWS_MAX_TILES; ++tl) {
        if (tl < ntile) {
          const float y = (use && dv[tl]) ? yb[t * a.st + src[tl]] : 0.0f;
          r[tl] = outer4(pa, wd * (double)y, r[tl], stage, lane);
        }
      }
    }
    // --- [G + reg I | R] into the wave's LDS image (rows and columns >= N are not read) ---
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int row = lk + 4 * q;
      A[row * ld + lc] = g[q] + (row == lc ? a.reg : 0.0);
#pragma unroll
      for (int tl = 0; tl < ROWS_MAX_TILES; ++tl)
        if (tl < ntile) A[row * ld + 16 + 16 * tl + lc] = r[tl][q];
    }
    wave_sync();
    // --- Gauss-Jordan with partial pivoting over the columns right of k: lane = (row lc, column
    //     group lk).  Column k itself is never written, so the factors need no snapshot. ---
    for (int k = 0; k < N; ++k) {
      int p = k;
      double best = fabs(A[k * ld + k]);
      for (int rr = k + 1; rr < N; ++rr) {
        const double v = fabs(A[rr * ld + k]);
        if (v > best) { best = v; p = rr; }
      }
      p = __builtin_amdgcn_readfirstlane(p);
      const int ncol = (N - k) + dk;   // compact columns k .. k + ncol - 1
      if (p != k) {
        for (int j = lane; j < ncol; j += 64) {
          const int c = sys_col(k + j, N);
          const double x = A[k * ld + c];
          A[k * ld + c] = A[p * ld + c];
          A[p * ld + c] = x;
        }
        wave_sync();
      }
      const double inv = 1.0 / A[k * ld + k];
      const double f = lc < N ? A[lc * ld + k] : 0.0;
      for (int j = 1 + lk; j < ncol; j += 4) {
        const int c = sys_col(k + j, N);
        const double pk = A[k * ld + c] * inv;
        if (lc == k) A[k * ld + c] = pk;
        else if (lc < N) A[lc * ld + c] -= f * pk;
      }
      wave_sync();
    }
    // --- W = G^-1 R sits in R's columns: round once, write (d n) params and (n d) tokens ---
    const int cnt = dk * N;
    if (a.params_out) {
      for (int i = lane; i < cnt; i += 64) {
        const int dl = i / N, n = i - dl * N;
        a.params_out[b * DN + (d0 + dl) * N + n] = (float)A[n * ld + 16 + dl];
      }
    }
    if (a.tokens_out) {
      for (int i = lane; i < cnt; i += 64) {
        const int n = i / dk, dl = i - n * dk, kk = (d0 + dl) * N + n;
        const float p = (float)A[n * ld + 16 + dl];
        a.tokens_out[b * DN + n * a.D + d0 + dl] = beast::quantize_one(p, a.w_min[kk], a.w_max[kk], a.vm1) + a.tok_offset;
      }
    }
    wave_sync();   // the next item overwrites the image
  }
}

}  // namespace

// =================================================================== C-ABI ==
extern "C" int beast_encode_rows_f32(const float* traj, int64_t B, int T, int64_t sb, int64_t st, int64_t sd, int D,
                                     int n_joint, const int32_t* dof_src, const float* times, int64_t times_sb,
                                     const float* weights, int64_t weights_sb, float tau, float delay,
                                     const float* knots_joint, int n_knots_joint, const float* knots_grip,
                                     int n_knots_grip, int degree, int N, double reg, const float* w_min,
                                     const float* w_max, int vocab, int64_t tok_offset, float* params_out,
                                     int64_t* tokens_out, void* stream) {
  BEAST_REQUIRE(traj && dof_src && times, "beast_encode_rows_f32: null input pointer");
  BEAST_REQUIRE(params_out || tokens_out, "beast_encode_rows_f32: no output requested");
  BEAST_REQUIRE(B >= 0, "beast_encode_rows_f32: batch size B=%lld must be >= 0", (long long)B);
  BEAST_REQUIRE(T >= 1 && N >= 1 && degree >= 0, "beast_encode_rows_f32: need T >= 1, N >= 1, degree >= 0 (T=%d N=%d degree=%d)",
                T, N, degree);
  BEAST_REQUIRE(D >= 1 && n_joint >= 0 && n_joint <= D, "beast_encode_rows_f32: bad DoF split D=%d n_joint=%d", D, n_joint);
  BEAST_REQUIRE(sb >= 0 && st >= 0 && sd >= 0 && times_sb >= 0 && weights_sb >= 0,
                "beast_encode_rows_f32: strides must be >= 0");
  BEAST_REQUIRE(n_joint == 0 || (knots_joint && n_knots_joint == degree + 1 + N),
                "beast_encode_rows_f32: joint knot vector size %d != degree+1+N", n_knots_joint);
  BEAST_REQUIRE(n_joint == D || (knots_grip && n_knots_grip == 1 + N),
                "beast_encode_rows_f32: gripper knot vector size %d != 1+N", n_knots_grip);
  BEAST_REQUIRE(!tokens_out || (w_min && w_max && vocab >= 2),
                "beast_encode_rows_f32: quantisation needs w_min/w_max and vocab >= 2");
  BEAST_REQUIRE_CODE(N <= ROWS_MAX_N && T <= ROWS_MAX_T && D <= ROWS_MAX_D && degree <= ROWS_MAX_DEGREE,
                     BEAST_E_UNSUPPORTED,
                     "beast_encode_rows_f32 supports N <= %d, T <= %d, D <= %d, degree <= %d (N=%d T=%d D=%d degree=%d)",
                     ROWS_MAX_N, ROWS_MAX_T, ROWS_MAX_D, ROWS_MAX_DEGREE, N, T, D, degree);
  if (B == 0) return BEAST_OK;
  RowsArgs a{};
  a.traj = traj; a.B = B; a.sb = sb; a.st = st; a.sd = sd; a.dof_src = dof_src;
  a.times = times; a.times_sb = times_sb; a.weights = weights; a.weights_sb = weights_sb;
  a.kv[0] = n_joint > 0 ? knots_joint : nullptr; a.kv[1] = n_joint < D ? knots_grip : nullptr;
  a.w_min = w_min; a.w_max = w_max; a.params_out = params_out;
  a.tokens_out = reinterpret_cast<long long*>(tokens_out); a.tok_offset = tok_offset; a.reg = reg;
  a.tau = tau; a.delay = delay; a.vm1 = (float)(vocab - 1);
  a.T = T; a.D = D; a.nj = n_joint; a.N = N;
  a.nk = (n_joint > 0) + (n_joint < D); a.k0 = n_joint > 0 ? 0 : 1;
  a.ld = 16 + round_up(std::max(n_joint, D - n_joint), 16) + 1;
  const unsigned lds = (unsigned)(ROWS_WAVES * 16 * a.ld * sizeof(double));
  Queue q;
  BEAST_TRY(queue_of(stream, q, "beast_encode_rows_f32"));
  const int64_t items = B * a.nk;
  const int64_t grid = std::max<int64_t>(1, std::min<int64_t>((items + ROWS_WAVES - 1) / ROWS_WAVES,
                                                              (int64_t)cu_count(q.dev) * 8));
#define BEAST_ROWS_CASE(K) \
  case K: return launch<k_fit_rows<K>>((unsigned)grid, ROWS_WAVES * 64, lds, q, "k_fit_rows", a);
  switch (degree) {
    BEAST_ROWS_CASE(0) BEAST_ROWS_CASE(1) BEAST_ROWS_CASE(2) BEAST_ROWS_CASE(3) BEAST_ROWS_CASE(4)
    BEAST_ROWS_CASE(5) BEAST_ROWS_CASE(6) BEAST_ROWS_CASE(7) BEAST_ROWS_CASE(8)
  }
#undef BEAST_ROWS_CASE
  return BEAST_OK;   // unreachable: degree is in [0, 8]
}
