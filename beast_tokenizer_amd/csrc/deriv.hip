// Fused multi-order reconstruct for gfx950: tokens -> positions, velocities and accelerations
// in one launch (beast_reconstruct_derivs_f32).
//
//   k_reconstruct_derivs  dequantise a tile of trajectories once into LDS, then
//                         out_o[j][t][c] = sum_n basis_o[kind][t][n] * W[j][d][n] for every
//                         requested derivative order o from that one copy of the coefficients
//
// The spline's derivatives are linear in the same control points (beast_bspline_basis_deriv_f32
// gives d^o/dt^o of the basis over them), so the three orders differ only in the basis slab.
// The kernel is bandwidth-bound like k_reconstruct_v: at T 50, D 14, N 10 it reads 1,120 B of
// tokens per trajectory and writes up to 3 x 2,800 B.  A thread owns four consecutive elements
// of the tile's contiguous output range and stores them with one 16-byte store per order, so
// every wave writes 1 KB runs without a pass through LDS.  The shared basis slabs are staged in
// LDS once per workgroup (zero-padded to a multiple of four columns, read as 16-byte vectors);
// the four elements of a thread share their time step's basis rows in registers (reloaded where
// the output row wraps), so LDS serves one W row per element and one set of basis rows per
// four.  Tiles are 16 trajectories and the resident workgroups stride over them; a batch too
// small to give every CU two such tiles takes tiles of 4, one per workgroup.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>

#include "common.h"
#include "launch.h"

namespace {

constexpr int DV_THREADS = 256;
constexpr int DV_STEP = DV_THREADS * 4;      // output elements per workgroup pass
constexpr int DV_TILE = 16;                  // trajectories per tile (bulk); 4 for small batches
constexpr int DV_TILE_SMALL = 4;
constexpr int DV_MAX_N = 16;                 // the envelope of beast_reconstruct_f32
constexpr int DV_MAX_D = 64;
constexpr int DV_MAX_T = 4096;
constexpr int DV_MAX_NDO = 4096;
constexpr int DV_BASIS_LDS = 48 * 1024;      // shared slabs up to this size are staged in LDS
constexpr int DV_ORDERS = 3;

struct DerivArgs {
  const long long* tokens;
  const float* ntokens;
  const float* w_min;
  const float* w_max;
  const float* basis;        // [3][2][Tout][N] (shared) or per trajectory with stride basis_sb
  const int32_t* dof_dst;
  const float* init_p;
  const int32_t* init_p_src;
  float* out[DV_ORDERS];     // pos, vel, acc; null = not requested
  int64_t B, ntiles, tok_offset, basis_sb, init_p_sb;
  int D, nj, N, vocab, Tout, ndo;
  int vec4;                  // every requested output is 16-byte aligned
  int phi_off[DV_ORDERS];    // float offset of order o's staged slab (LDS basis only)
  int off_phi, off_wlo, off_col;   // byte offsets into the dynamic LDS
  int step_j, step_t, step_c;      // DV_STEP output elements as (trajectories, time steps, columns)
  float inv_per, inv_D;
};

// x / d for 0 <= x < 2^14, 1 <= d <= 2^10: (x + 0.5) / d is at least 2^-11 from an integer and
// the fp32 product is within 2^-18 of it
__device__ __forceinline__ int small_div(int x, float inv_d) { return (int)(((float)x + 0.5f) * inv_d); }

// one output element of every requested order with the basis rows read from memory (per-row
// grids, or shared slabs too large for LDS): a sequential fma over n, as k_reconstruct_rows
__device__ __forceinline__ void deriv_dot_mem(const DerivArgs& a, const float* __restrict__ Wr, int kind,
                                              int64_t b, int t, float (&v)[DV_ORDERS]) {
  const int64_t slab = (int64_t)2 * a.Tout * a.N;
  const float* gb = a.basis + b * a.basis_sb + ((int64_t)kind * a.Tout + t) * a.N;
#pragma unroll
  for (int o = 0; o < DV_ORDERS; ++o) {
    if (a.out[o] == nullptr || (o > 0 && kind == 1)) continue;   // gripper DoFs: degree 0, derivatives 0
    const float* p = gb + o * slab;
    float acc = 0.0f;
    for (int n = 0; n < a.N; ++n) acc = fmaf(p[n], Wr[n], acc);
    v[o] = acc;
  }
}

template <int KS, bool LB, int TB>
__global__ __launch_bounds__(DV_THREADS) void k_reconstruct_derivs(DerivArgs a) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  constexpr int NP = 4 * KS;
  const int D = a.D, N = a.N, nj = a.nj, per = N * D, Tout = a.Tout, ndo = a.ndo;
  float* W = reinterpret_cast<float*>(smem);                  // [TB][D][NP]
  float* phi = reinterpret_cast<float*>(smem + a.off_phi);    // staged slabs (LB)
  float* wlo = reinterpret_cast<float*>(smem + a.off_wlo);    // [per]
  float* whi = wlo + per;                                     // [per]
  int* col2d = reinterpret_cast<int*>(smem + a.off_col);      // [ndo] output column -> DoF
  const int tid = threadIdx.x;
  const float vm1 = (float)(a.vocab - 1);
  const bool grip = nj < D;

  for (int i = tid; i < per; i += DV_THREADS) {
    wlo[i] = a.w_min[i];
    whi[i] = a.w_max[i];
  }
  for (int i = tid; i < TB * D * NP; i += DV_THREADS) W[i] = 0.0f;   // the pad columns stay 0
  for (int c = tid; c < ndo; c += DV_THREADS) col2d[c] = -1;
  if constexpr (LB) {
#pragma unroll
    for (int o = 0; o < DV_ORDERS; ++o) {
      if (a.out[o] == nullptr) continue;                      // a null output's slab is never read
      const int rows = ((o == 0 && grip) ? 2 : 1) * Tout;     // kind 1 is read for positions only
      const float* src = a.basis + (int64_t)o * 2 * Tout * N;
      float* dst = phi + a.phi_off[o];
      for (int i = tid; i < rows * NP; i += DV_THREADS) {
        const int r = i / NP, n = i - r * NP;
        dst[i] = (n < N) ? src[r * N + n] : 0.0f;
      }
    }
  }
  __syncthreads();
  for (int d = tid; d < D; d += DV_THREADS) {
    const int dd = a.dof_dst[d];
    if (dd >= 0 && dd < ndo) col2d[dd] = d;
  }

  const int row = Tout * ndo;                                 // elements per trajectory and order
  for (int64_t tile = blockIdx.x; tile < a.ntiles; tile += gridDim.x) {
    const int64_t b0 = tile * TB;
    const int nb = (int)min<int64_t>(TB, a.B - b0);
    __syncthreads();                                          // the previous tile's W is read out
    // ---- (n d) tokens -> W[j][d][n], once for every order (bit-exact discrete_to_continuous,
    // or denormalize_tensor's intent for normalised tokens; init_p for n = 0 of the joint DoFs)
    for (int e = tid; e < nb * per; e += DV_THREADS) {
      const int j = small_div(e, a.inv_per), r = e - j * per;
      const int n = small_div(r, a.inv_D), d = r - n * D, k = d * N + n;
      float w;
      if (a.init_p != nullptr && n == 0 && d < nj) w = a.init_p[(b0 + j) * a.init_p_sb + a.init_p_src[d]];
      else if (a.ntokens != nullptr) w = beast::denormalize_one(a.ntokens[b0 * per + e], wlo[k], whi[k]);
      else w = beast::dequantize_one(a.tokens[b0 * per + e] - a.tok_offset, wlo[k], whi[k], vm1);
      W[(j * D + d) * NP + n] = w;
    }
    __syncthreads();
    // ---- four consecutive output elements per thread, every requested order from the same W
    const int total = nb * row;                               // <= 16 * 4096 * 4096 = 2^28
    const int64_t gbase = b0 * row;
    int e0 = tid * 4;
    int j = e0 / row, t, c;                                   // this thread's first element, then
    {                                                         // stepped by DV_STEP without dividing
      const int r = e0 - j * row;
      t = r / ndo;
      c = r - t * ndo;
    }
    for (; e0 < total; e0 += DV_STEP) {
      const int cnt = min(4, total - e0);
      int jj = j, tt = t, cc = c;
      float v[4][DV_ORDERS];
      float4 p[DV_ORDERS][KS] = {}, pg[KS] = {};              // basis rows of time step tt (LB)
      auto load_rows = [&](int ts) {
#pragma unroll
        for (int o = 0; o < DV_ORDERS; ++o) {
          if (a.out[o] == nullptr) continue;
          const float4* src = reinterpret_cast<const float4*>(phi + a.phi_off[o] + ts * NP);
#pragma unroll
          for (int k = 0; k < KS; ++k) p[o][k] = src[k];
        }
        if (grip && a.out[0] != nullptr) {                    // kind 1 (degree 0): positions only
          const float4* src = reinterpret_cast<const float4*>(phi + a.phi_off[0] + (Tout + ts) * NP);
#pragma unroll
          for (int k = 0; k < KS; ++k) pg[k] = src[k];
        }
      };
      if constexpr (LB) load_rows(tt);
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        v[q][0] = v[q][1] = v[q][2] = 0.0f;
        if (q >= cnt) continue;
        const int d = col2d[cc];
        if (d >= 0) {                                         // else: a column dof_dst does not name
          const bool g1 = d >= nj;
          const float* Wr = W + (jj * D + d) * NP;
          if constexpr (LB) {
            float4 w[KS];
#pragma unroll
            for (int k = 0; k < KS; ++k) w[k] = reinterpret_cast<const float4*>(Wr)[k];
#pragma unroll
            for (int o = 0; o < DV_ORDERS; ++o) {
              if (a.out[o] == nullptr || (o > 0 && g1)) continue;   // gripper DoFs: derivatives 0
              float acc = 0.0f;
#pragma unroll
              for (int k = 0; k < KS; ++k) {                  // a sequential fma over n
                const float4 b = (o == 0 && g1) ? pg[k] : p[o][k];
                acc = fmaf(b.x, w[k].x, acc);
                acc = fmaf(b.y, w[k].y, acc);
                acc = fmaf(b.z, w[k].z, acc);
                acc = fmaf(b.w, w[k].w, acc);
              }
              v[q][o] = acc;
            }
          } else {
            deriv_dot_mem(a, Wr, g1 ? 1 : 0, b0 + jj, tt, v[q]);
          }
        }
        if (++cc == ndo) {                                    // the output row wraps: next time step
          cc = 0;
          if (++tt == Tout) { tt = 0; ++jj; }
          if constexpr (LB) {
            if (q + 1 < cnt) load_rows(tt);
          }
        }
      }
#pragma unroll
      for (int o = 0; o < DV_ORDERS; ++o) {
        if (a.out[o] == nullptr) continue;
        float* g = a.out[o] + gbase + e0;
        if (a.vec4 && cnt == 4) {
          *reinterpret_cast<float4*>(g) = make_float4(v[0][o], v[1][o], v[2][o], v[3][o]);
        } else {
#pragma unroll
          for (int q = 0; q < 4; ++q)
            if (q < cnt) g[q] = v[q][o];
        }
      }
      // (j, t, c) += DV_STEP elements: step_t < Tout and step_c < ndo, so one carry each
      c += a.step_c;
      if (c >= ndo) { c -= ndo; ++t; }
      t += a.step_t;
      if (t >= Tout) { t -= Tout; ++j; }
      j += a.step_j;
    }
  }
}

// LDS: W [TB][D][NP] | staged slabs | w_min, w_max [D*N] | col2d [num_dof_out]
template <int KS, bool LB, int TB>
int launch_derivs(DerivArgs a, int phi_bytes, int cus, const Queue& q) {
  a.ntiles = (a.B + TB - 1) / TB;
  a.off_phi = TB * a.D * 4 * KS * 4;
  a.off_wlo = a.off_phi + (LB ? phi_bytes : 0);
  a.off_col = a.off_wlo + 2 * a.N * a.D * 4;
  const int lds = a.off_col + a.ndo * 4;
  BEAST_REQUIRE_CODE(lds <= 160 * 1024, BEAST_E_UNSUPPORTED, "reconstruct derivs tile needs %d B of LDS", lds);
  // resident workgroups only: each stages the slabs once and strides over the tiles (half of
  // grid_for's cap, which lets a second round of workgroups queue up)
  const int per_cu = std::max(1, std::min(8, (160 * 1024) / std::max(lds, 1)));
  const int64_t grid = std::max<int64_t>(1, std::min<int64_t>(a.ntiles, (int64_t)cus * per_cu));
  return launch<k_reconstruct_derivs<KS, LB, TB>>((unsigned)grid, DV_THREADS, lds, q, "k_reconstruct_derivs", a);
}

template <int KS>
int launch_derivs_ks(const DerivArgs& a, bool lb, int phi_bytes, const Queue& q) {
  const int cus = cu_count(q.dev);
  if ((a.B + DV_TILE - 1) / DV_TILE < 2 * (int64_t)cus)   // latency regime: more, smaller tiles
    return lb ? launch_derivs<KS, true, DV_TILE_SMALL>(a, phi_bytes, cus, q)
              : launch_derivs<KS, false, DV_TILE_SMALL>(a, phi_bytes, cus, q);
  return lb ? launch_derivs<KS, true, DV_TILE>(a, phi_bytes, cus, q)
            : launch_derivs<KS, false, DV_TILE>(a, phi_bytes, cus, q);
}

}  // namespace

// =================================================================== C-ABI ==
extern "C" int beast_reconstruct_derivs_f32(const int64_t* tokens, int64_t B, int D, int n_joint, int N, int vocab,
                                            int64_t tok_offset, const float* w_min, const float* w_max,
                                            const float* basis, int64_t basis_sb, int T_out,
                                            const int32_t* dof_dst, int num_dof_out, const float* init_p,
                                            int64_t init_p_sb, const int32_t* init_p_src, float* pos_out,
                                            float* vel_out, float* acc_out, const float* ntokens, void* stream) {
  BEAST_REQUIRE((tokens || ntokens) && w_min && w_max && basis && dof_dst,
                "beast_reconstruct_derivs_f32: null input pointer");
  BEAST_REQUIRE(pos_out || vel_out || acc_out, "beast_reconstruct_derivs_f32: no output requested");
  BEAST_REQUIRE(N >= 1 && D >= 1 && n_joint >= 0 && n_joint <= D, "bad shape N=%d D=%d n_joint=%d", N, D, n_joint);
  BEAST_REQUIRE(T_out >= 1 && num_dof_out >= D, "reconstruct derivs: need T_out >= 1, num_dof_out >= D (T_out=%d, "
                "num_dof_out=%d, D=%d)", T_out, num_dof_out, D);
  BEAST_REQUIRE(vocab >= 2 || ntokens, "vocab must be >= 2");
  BEAST_REQUIRE(basis_sb >= 0, "basis_sb=%lld must be >= 0", (long long)basis_sb);
  BEAST_REQUIRE(!init_p || init_p_src, "init_p needs init_p_src");
  BEAST_REQUIRE(B >= 0, "batch size B=%lld must be >= 0", (long long)B);
  BEAST_REQUIRE_CODE(N <= DV_MAX_N && D <= DV_MAX_D && T_out <= DV_MAX_T && num_dof_out <= DV_MAX_NDO,
                     BEAST_E_UNSUPPORTED,
                     "reconstruct derivs supports N <= %d, D <= %d, T_out <= %d, num_dof_out <= %d (N=%d D=%d "
                     "T_out=%d num_dof_out=%d)", DV_MAX_N, DV_MAX_D, DV_MAX_T, DV_MAX_NDO, N, D, T_out, num_dof_out);
  if (B == 0) return BEAST_OK;
  DerivArgs a{};
  a.tokens = reinterpret_cast<const long long*>(tokens); a.ntokens = ntokens; a.w_min = w_min; a.w_max = w_max;
  a.basis = basis; a.dof_dst = dof_dst; a.init_p = init_p; a.init_p_src = init_p_src;
  a.out[0] = pos_out; a.out[1] = vel_out; a.out[2] = acc_out;
  a.B = B; a.tok_offset = tok_offset; a.basis_sb = basis_sb;
  a.init_p_sb = init_p_sb; a.D = D; a.nj = n_joint; a.N = N; a.vocab = vocab; a.Tout = T_out; a.ndo = num_dof_out;
  a.vec4 = ((((uintptr_t)pos_out) | ((uintptr_t)vel_out) | ((uintptr_t)acc_out)) & 15) == 0;
  a.inv_per = 1.0f / (float)(N * D);
  a.inv_D = 1.0f / (float)D;
  const int row = T_out * num_dof_out, rem = DV_STEP % row;
  a.step_j = DV_STEP / row; a.step_t = rem / num_dof_out; a.step_c = rem % num_dof_out;
  const int KS = (N + 3) / 4, NP = 4 * KS;
  int phi_floats = 0;
  for (int o = 0; o < DV_ORDERS; ++o) {
    a.phi_off[o] = phi_floats;
    if (a.out[o]) phi_floats += ((o == 0 && n_joint < D) ? 2 : 1) * T_out * NP;
  }
  const bool lb = basis_sb == 0 && (int64_t)phi_floats * 4 <= DV_BASIS_LDS;
  Queue q;
  if (const int rc = queue_of(stream, q, "beast_reconstruct_derivs_f32")) return rc;
  switch (KS) {
    case 1: return launch_derivs_ks<1>(a, lb, phi_floats * 4, q);
    case 2: return launch_derivs_ks<2>(a, lb, phi_floats * 4, q);
    case 3: return launch_derivs_ks<3>(a, lb, phi_floats * 4, q);
    default: return launch_derivs_ks<4>(a, lb, phi_floats * 4, q);
  }
}
