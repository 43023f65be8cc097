// Adjoint of the fused multi-order reconstruct for gfx950 (beast_reconstruct_derivs_bwd_f32):
// gradients of positions, velocities and accelerations -> gradient of the normalised tokens.
//
//   k_reconstruct_derivs_bwd  S[j][d][n] = sum_t sum_o basis_o[kind][t][n] * G_o[j][t][dof_dst[d]],
//                             grad_ntokens[j][n*D+d] = -1 <= x <= 1 ? S * (w_max - w_min) / 2 : 0
//
// The forward is a linear map of the control points, so its transpose serves every order at once.
// The kernel is bandwidth-bound: at T 50, D 14, N 10 it reads up to 3 x 2,800 B of gradients per
// trajectory and writes 560 B.  A tile's gradients travel through LDS in chunks of time steps:
// every wave reads 1 KB runs with 16-byte loads (element loads where a pointer or the row length
// is not 16-byte aligned), each element once, several loads in flight per thread.  A thread owns
// one (trajectory, DoF) pair and all N of its sums in registers, and walks t upwards and the
// orders 0, 1, 2 inside each t with one fma per term: the order of every sum is fixed by (t, o)
// alone, whatever the chunk length, the tile size, the batch or the workgroup, so results are
// bitwise reproducible and a row's gradient does not depend on the batch around it.  No atomics.
// The shared basis slabs are staged in LDS once per workgroup (zero-padded to a multiple of four
// columns, read as 16-byte vectors; a wave's lanes share t, so the reads broadcast); per-row
// grids and slabs too large for LDS are read from memory.  The number of gradients given is a
// template parameter and the walk has no branch: a gripper DoF, which only order 0 reaches,
// reads a row of zeros for the other orders, so the LDS reads of several steps are in flight at
// once.  Tiles are 16 trajectories and the resident workgroups stride over them; a batch too
// small to give every CU two such tiles takes tiles of 4.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>

#include "common.h"
#include "launch.h"

namespace {

constexpr int DB_THREADS = 256;
constexpr int DB_TILE = 16;                  // trajectories per tile (bulk); 4 for small batches
constexpr int DB_TILE_SMALL = 4;
constexpr int DB_MAX_N = 16;                 // the envelope of beast_reconstruct_derivs_f32
constexpr int DB_MAX_D = 64;
constexpr int DB_MAX_T = 4096;
constexpr int DB_MAX_NDO = 4096;
constexpr int DB_BASIS_LDS = 48 * 1024;      // shared slabs up to this size are staged in LDS
constexpr int DB_CHUNK_LDS = 24 * 1024;      // a chunk of gradients aims at this size ...
constexpr int DB_CHUNK_LDS_MAX = 64 * 1024;  // ... and never exceeds this one (the tile shrinks first)
constexpr int DB_ORDERS = 3;

struct DerivBwdArgs {
  const float* grad[DB_ORDERS];   // the upstream gradients given, compacted: slot s
  int ord[DB_ORDERS];             // slot s's derivative order (ascending)
  const float* ntokens;
  const float* w_min;
  const float* w_max;
  const float* basis;             // [3][2][Tout][N] (shared) or per trajectory with stride basis_sb
  const int32_t* dof_dst;
  const int32_t* init_p_src;      // non-null: the forward overwrote coefficient 0 of the joint DoFs
  float* grad_ntokens;
  float* grad_init_p;
  int64_t B, ntiles, basis_sb, grad_init_p_sb;
  int D, nj, N, Tout, ndo;
  int tb;                         // trajectories per tile: tb * D <= DB_THREADS
  int tc;                         // time steps per chunk
  int seg;                        // floats of one (slot, trajectory) segment of a chunk in LDS
  int vec4;                       // 16-byte loads: pointers, row length and chunk length allow them
  int lx_shift;                   // staging: 1 << lx_shift threads walk a segment, the rest its trajectories
  int phi_off[DB_ORDERS];         // float offset of slot s's staged slab (LDS basis only)
  int off_phi, off_scale, off_col, off_zero;   // byte offsets into the dynamic LDS
};

// One chunk of one tile: segment (s, jj) of Gs <- cnt elements of gradient s, trajectory jj, from
// its time step t0 on.  A thread loads the same piece of PF (1 or 2) trajectories and of every
// gradient before it stores any of them: PF * NS loads in flight.  Two pay for their registers
// with a workgroup per CU, which the bulk batches gain from and the small ones lose by.
template <int NS, int PF, class V>
__device__ __forceinline__ void stage_chunk(const DerivBwdArgs& a, float* Gs, int64_t first, int row, int nb,
                                            int units, int tx, int ty, int lx, int ny) {
  for (int jj = ty; jj < nb; jj += PF * ny) {
    const bool two = PF == 2 && jj + ny < nb;
    for (int i = tx; i < units; i += lx) {
      V v0[NS], v1[NS] = {};
#pragma unroll
      for (int s = 0; s < NS; ++s) v0[s] = reinterpret_cast<const V*>(a.grad[s] + first + (int64_t)jj * row)[i];
      if (two) {
#pragma unroll
        for (int s = 0; s < NS; ++s)
          v1[s] = reinterpret_cast<const V*>(a.grad[s] + first + (int64_t)(jj + ny) * row)[i];
      }
#pragma unroll
      for (int s = 0; s < NS; ++s) reinterpret_cast<V*>(Gs + (s * a.tb + jj) * a.seg)[i] = v0[s];
      if (two) {
#pragma unroll
        for (int s = 0; s < NS; ++s) reinterpret_cast<V*>(Gs + (s * a.tb + jj + ny) * a.seg)[i] = v1[s];
      }
    }
  }
}

template <int KS, int NS, bool LB, int PF>
__global__ __launch_bounds__(DB_THREADS) void k_reconstruct_derivs_bwd(DerivBwdArgs a) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  constexpr int NP = 4 * KS;
  const int D = a.D, N = a.N, nj = a.nj, per = N * D, Tout = a.Tout, ndo = a.ndo;
  float* lds = reinterpret_cast<float*>(smem);                     // Gs [NS][tb][seg] comes first
  float* phi = reinterpret_cast<float*>(smem + a.off_phi);         // staged slabs (LB)
  float* scale = reinterpret_cast<float*>(smem + a.off_scale);     // [per] (d n): d denormalize / dx
  int* dcol = reinterpret_cast<int*>(smem + a.off_col);            // [D] DoF -> output column, or -1
  const int tid = threadIdx.x;
  const bool grip = nj < D;

  for (int i = tid; i < per; i += DB_THREADS) scale[i] = __fmul_rn(0.5f, __fsub_rn(a.w_max[i], a.w_min[i]));
  for (int d = tid; d < D; d += DB_THREADS) {
    const int dd = a.dof_dst[d];
    dcol[d] = (dd >= 0 && dd < ndo) ? dd : -1;
  }
  if (tid < 16) lds[a.off_zero / 4 + tid] = 0.0f;                  // what a gripper DoF reads for orders 1, 2
  if constexpr (LB) {
#pragma unroll
    for (int s = 0; s < NS; ++s) {                                 // a null gradient's slab is never read
      const int rows = ((a.ord[s] == 0 && grip) ? 2 : 1) * Tout;   // kind 1 feeds positions only
      const float* src = a.basis + (int64_t)a.ord[s] * 2 * Tout * N;
      float* dst = phi + a.phi_off[s];
      for (int i = tid; i < rows * NP; i += DB_THREADS) {
        const int r = i / NP, n = i - r * NP;
        dst[i] = (n < N) ? src[r * N + n] : 0.0f;
      }
    }
  }
  __syncthreads();

  // this thread's (trajectory, DoF) pair of every tile: where its gradient element and its basis
  // row of time step 0 sit in LDS for each slot, and how far the next time step is
  const int j = tid / D, d = tid - j * D;
  const bool g1 = d >= nj;
  const int c = (j < a.tb) ? dcol[d] : -1;
  int g_at[NS], g_step[NS], p_at[NS], p_step[NS];
  bool skip[NS];
#pragma unroll
  for (int s = 0; s < NS; ++s) {
    skip[s] = g1 && a.ord[s] > 0;                                  // gripper DoFs: positions only
    g_at[s] = skip[s] ? a.off_zero / 4 : (s * a.tb + j) * a.seg + c;
    g_step[s] = skip[s] ? 0 : ndo;
    p_at[s] = skip[s] ? a.off_zero / 4 : a.off_phi / 4 + a.phi_off[s] + (g1 ? Tout * NP : 0);
    p_step[s] = skip[s] ? 0 : NP;
  }
  const int lx = 1 << a.lx_shift, tx = tid & (lx - 1), ty = tid >> a.lx_shift, ny = DB_THREADS >> a.lx_shift;
  const int row = Tout * ndo;                                      // elements per trajectory and order
  const int64_t slab = (int64_t)2 * Tout * N;

  for (int64_t tile = blockIdx.x; tile < a.ntiles; tile += gridDim.x) {
    const int64_t b0 = tile * a.tb;
    const int nb = (int)min<int64_t>(a.tb, a.B - b0);
    const bool mine = j < nb && c >= 0;
    float acc[NP];
#pragma unroll
    for (int n = 0; n < NP; ++n) acc[n] = 0.0f;

    for (int t0 = 0; t0 < Tout; t0 += a.tc) {
      const int tc = min(a.tc, Tout - t0);
      __syncthreads();                                             // the previous chunk is read out
      // ---- the chunk's gradients -> Gs[slot][jj][tt][column], each element read once
      if (a.vec4) stage_chunk<NS, PF, float4>(a, lds, b0 * row + (int64_t)t0 * ndo, row, nb, (tc * ndo) >> 2, tx, ty, lx, ny);
      else stage_chunk<NS, PF, float>(a, lds, b0 * row + (int64_t)t0 * ndo, row, nb, tc * ndo, tx, ty, lx, ny);
      __syncthreads();
      // ---- acc[n] += basis_o[kind][t][n] * G_o[j][t][c], t upwards, the orders inside each t
      if (mine) {
        int gi[NS], pi[NS];
#pragma unroll
        for (int s = 0; s < NS; ++s) {
          gi[s] = g_at[s];
          pi[s] = p_at[s] + t0 * p_step[s];
        }
#pragma unroll 1
        for (int tt = 0; tt < tc; ++tt) {
#pragma unroll
          for (int s = 0; s < NS; ++s) {
            const float g = lds[gi[s]];
            gi[s] += g_step[s];
            if constexpr (LB) {
              const float4* p = reinterpret_cast<const float4*>(lds + pi[s]);
              pi[s] += p_step[s];
#pragma unroll
              for (int k = 0; k < KS; ++k) {
                const float4 b = p[k];
                acc[4 * k + 0] = fmaf(b.x, g, acc[4 * k + 0]);
                acc[4 * k + 1] = fmaf(b.y, g, acc[4 * k + 1]);
                acc[4 * k + 2] = fmaf(b.z, g, acc[4 * k + 2]);
                acc[4 * k + 3] = fmaf(b.w, g, acc[4 * k + 3]);
              }
            } else if (!skip[s]) {
              const float* p = a.basis + (b0 + j) * a.basis_sb + a.ord[s] * slab +
                               ((int64_t)(g1 ? Tout : 0) + t0 + tt) * N;
#pragma unroll
              for (int n = 0; n < NP; ++n)
                if (n < N) acc[n] = fmaf(p[n], g, acc[n]);
            }
          }
        }
      }
    }
    // ---- scale, mask and store: (d n) sums -> (n d) gradient, consecutive lanes consecutive d
    if (j < nb) {
      const int64_t base = (b0 + j) * per;
      const bool ip = a.init_p_src != nullptr && !g1;              // coefficient 0 came from init_p
      float x[NP];
#pragma unroll
      for (int n = 0; n < NP; ++n) x[n] = a.ntokens[base + min(n, N - 1) * D + d];   // all loads in flight
#pragma unroll
      for (int n = 0; n < NP; ++n) {
        if (n >= N) continue;
        const bool pass = x[n] >= -1.0f && x[n] <= 1.0f && !(ip && n == 0);   // a select: NaN * 0 stays out
        a.grad_ntokens[base + n * D + d] = pass ? __fmul_rn(acc[n], scale[d * N + n]) : 0.0f;
      }
      if (ip && a.grad_init_p != nullptr) a.grad_init_p[(b0 + j) * a.grad_init_p_sb + a.init_p_src[d]] = acc[0];
    }
  }
}

// Workgroups of kernel K (four waves, one per SIMD) that a CU's 512 registers per lane hold, from
// the register count the compiler settled on (allocated in steps of 8); asked once per kernel.
template <auto K>
int workgroups_by_registers() {
  static const int v = [] {
    hipFuncAttributes fa;
    if (hipFuncGetAttributes(&fa, reinterpret_cast<const void*>(K)) != hipSuccess || fa.numRegs <= 0) return 8;
    return std::max(1, std::min(8, 512 / ((fa.numRegs + 7) & ~7)));
  }();
  return v;
}

// LDS: gradient chunk [NS][tb][seg] | staged slabs | scale [D*N] | dcol [D] | 16 zeros
template <int KS, int NS, bool LB, int PF>
int launch_derivs_bwd(DerivBwdArgs a, int phi_bytes, int tile, const Queue& q) {
  // the tile: one thread per (trajectory, DoF); the chunk: as many time steps as DB_CHUNK_LDS
  // holds, a multiple of four where it is cut (a cut then keeps 16-byte alignment)
  a.tb = std::max(1, std::min(tile, DB_THREADS / a.D));
  for (;; a.tb /= 2) {
    const int64_t per_t = (int64_t)NS * a.tb * a.ndo * 4;
    a.tc = (int)std::max<int64_t>(1, std::min<int64_t>(a.Tout, DB_CHUNK_LDS / per_t));
    if (a.tc < a.Tout && a.tc >= 4) a.tc &= ~3;
    a.seg = (a.tc * a.ndo + 3) & ~3;
    if ((int64_t)NS * a.tb * a.seg * 4 <= DB_CHUNK_LDS_MAX || a.tb == 1) break;
  }
  const int row = a.Tout * a.ndo;
  a.vec4 = a.vec4 && row % 4 == 0 && (a.tc == a.Tout || (a.tc * a.ndo) % 4 == 0);
  const int units = a.vec4 ? a.seg / 4 : a.tc * a.ndo;
  a.lx_shift = 0;
  while ((1 << a.lx_shift) < units && (1 << a.lx_shift) < DB_THREADS) ++a.lx_shift;
  a.ntiles = (a.B + a.tb - 1) / a.tb;
  a.off_phi = NS * a.tb * a.seg * 4;
  a.off_scale = a.off_phi + (LB ? phi_bytes : 0);
  a.off_col = a.off_scale + a.N * a.D * 4;
  a.off_zero = (a.off_col + a.D * 4 + 15) & ~15;
  const int lds = a.off_zero + 16 * 4;
  BEAST_REQUIRE_CODE(lds <= 160 * 1024, BEAST_E_UNSUPPORTED, "reconstruct derivs backward tile needs %d B of LDS",
                     lds);
  // resident workgroups only (by LDS and by registers): each stages the slabs once and strides
  // over the tiles, and none waits for a first round to end
  const int cus = cu_count(q.dev);
  const int per_cu = std::max(1, std::min(workgroups_by_registers<k_reconstruct_derivs_bwd<KS, NS, LB, PF>>(),
                                          (160 * 1024) / std::max(lds, 1)));
  const int64_t grid = std::max<int64_t>(1, std::min<int64_t>(a.ntiles, (int64_t)cus * per_cu));
  return launch<k_reconstruct_derivs_bwd<KS, NS, LB, PF>>((unsigned)grid, DB_THREADS, lds, q,
                                                          "k_reconstruct_derivs_bwd", a);
}

template <int KS, int NS>
int launch_derivs_bwd_ns(const DerivBwdArgs& a, bool lb, int phi_bytes, const Queue& q) {
  // latency regime: more, smaller tiles while a CU would get fewer than two tiles of 16
  if ((a.B + DB_TILE - 1) / DB_TILE < 2 * (int64_t)cu_count(q.dev))
    return lb ? launch_derivs_bwd<KS, NS, true, 1>(a, phi_bytes, DB_TILE_SMALL, q)
              : launch_derivs_bwd<KS, NS, false, 1>(a, phi_bytes, DB_TILE_SMALL, q);
  return lb ? launch_derivs_bwd<KS, NS, true, 2>(a, phi_bytes, DB_TILE, q)
            : launch_derivs_bwd<KS, NS, false, 2>(a, phi_bytes, DB_TILE, q);
}

template <int KS>
int launch_derivs_bwd_ks(const DerivBwdArgs& a, int ns, bool lb, int phi_bytes, const Queue& q) {
  switch (ns) {
    case 1: return launch_derivs_bwd_ns<KS, 1>(a, lb, phi_bytes, q);
    case 2: return launch_derivs_bwd_ns<KS, 2>(a, lb, phi_bytes, q);
    default: return launch_derivs_bwd_ns<KS, 3>(a, lb, phi_bytes, q);
  }
}

}  // namespace

// =================================================================== C-ABI ==
extern "C" int beast_reconstruct_derivs_bwd_f32(const float* grad_pos, const float* grad_vel, const float* grad_acc,
                                                int64_t B, int D, int n_joint, int N, const float* w_min,
                                                const float* w_max, const float* basis, int64_t basis_sb, int T_out,
                                                const int32_t* dof_dst, int num_dof_out, const float* ntokens,
                                                const int32_t* init_p_src, float* grad_ntokens, float* grad_init_p,
                                                int64_t grad_init_p_sb, void* stream) {
  BEAST_REQUIRE(ntokens && w_min && w_max && basis && dof_dst && grad_ntokens,
                "beast_reconstruct_derivs_bwd_f32: null pointer");
  BEAST_REQUIRE(grad_pos || grad_vel || grad_acc, "beast_reconstruct_derivs_bwd_f32: no gradient given");
  BEAST_REQUIRE(N >= 1 && D >= 1 && n_joint >= 0 && n_joint <= D, "bad shape N=%d D=%d n_joint=%d", N, D, n_joint);
  BEAST_REQUIRE(T_out >= 1 && num_dof_out >= D, "reconstruct derivs backward: need T_out >= 1, num_dof_out >= D "
                "(T_out=%d, num_dof_out=%d, D=%d)", T_out, num_dof_out, D);
  BEAST_REQUIRE(basis_sb >= 0, "basis_sb=%lld must be >= 0", (long long)basis_sb);
  BEAST_REQUIRE(!grad_init_p || init_p_src, "grad_init_p needs init_p_src");
  BEAST_REQUIRE(B >= 0, "batch size B=%lld must be >= 0", (long long)B);
  BEAST_REQUIRE_CODE(N <= DB_MAX_N && D <= DB_MAX_D && T_out <= DB_MAX_T && num_dof_out <= DB_MAX_NDO,
                     BEAST_E_UNSUPPORTED,
                     "reconstruct derivs backward supports N <= %d, D <= %d, T_out <= %d, num_dof_out <= %d (N=%d "
                     "D=%d T_out=%d num_dof_out=%d)", DB_MAX_N, DB_MAX_D, DB_MAX_T, DB_MAX_NDO, N, D, T_out,
                     num_dof_out);
  if (B == 0) return BEAST_OK;
  DerivBwdArgs a{};
  a.ntokens = ntokens; a.w_min = w_min; a.w_max = w_max; a.basis = basis; a.dof_dst = dof_dst;
  a.init_p_src = init_p_src; a.grad_ntokens = grad_ntokens; a.grad_init_p = grad_init_p;
  a.B = B; a.basis_sb = basis_sb; a.grad_init_p_sb = grad_init_p_sb;
  a.D = D; a.nj = n_joint; a.N = N; a.Tout = T_out; a.ndo = num_dof_out;
  a.vec4 = ((((uintptr_t)grad_pos) | ((uintptr_t)grad_vel) | ((uintptr_t)grad_acc)) & 15) == 0;
  const int KS = (N + 3) / 4, NP = 4 * KS;
  const float* given[DB_ORDERS] = {grad_pos, grad_vel, grad_acc};
  int phi_floats = 0, ns = 0;
  for (int o = 0; o < DB_ORDERS; ++o) {
    if (given[o] == nullptr) continue;
    a.grad[ns] = given[o];
    a.ord[ns] = o;
    a.phi_off[ns++] = phi_floats;
    phi_floats += ((o == 0 && n_joint < D) ? 2 : 1) * T_out * NP;
  }
  const bool lb = basis_sb == 0 && (int64_t)phi_floats * 4 <= DB_BASIS_LDS;
  Queue q;
  if (const int rc = queue_of(stream, q, "beast_reconstruct_derivs_bwd_f32")) return rc;
  switch (KS) {
    case 1: return launch_derivs_bwd_ks<1>(a, ns, lb, phi_floats * 4, q);
    case 2: return launch_derivs_bwd_ks<2>(a, ns, lb, phi_floats * 4, q);
    case 3: return launch_derivs_bwd_ks<3>(a, ns, lb, phi_floats * 4, q);
    default: return launch_derivs_bwd_ks<4>(a, ns, lb, phi_floats * 4, q);
  }
}
