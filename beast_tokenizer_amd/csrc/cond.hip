// Boundary conditions of the joint spline (init_cond_order / end_cond_order != 0, SURVEY.md §8f
// rank 4) for gfx950: the per-call work around the fit / reconstruct kernels.
//
//   k_cond_fixed  encode side: each (trajectory, joint DoF)'s init / end conditions and the fixed
//                 control points from y[0], y[1], y[T-2], y[T-1] (compute_init_params /
//                 compute_end_params, MP_lite_PyTorch/mp_pytorch/basis_gn/uni_bspline_basis.py
//                 :192-301, as uni_bspline.py:499-550 calls them), in the reference's fp32 op order
//   k_cond_add    reconstruct side: pos[j][t][joint d] += sum_k Phi_full[t][k] ext[j][d][k]
//                 + init_pos[j][d] over the fixed columns k (get_traj_pos, uni_bspline.py:126-166,
//                 end order -1 subtracting the end term from column C-2)
//   k_cond_add_long  the same sum, bit for bit, for T > 256 or C > 20 on a shared basis: tiles of
//                 trajectories x time rows, the fixed columns staged in LDS, rows moved 16 bytes at a time
// The fitted columns themselves run in the MFMA kernels of codec.hip with the conditioned
// projection (bspline.py:DeviceBasis); these replace about a dozen ATen launches per call.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "common.h"
#include "launch.h"

namespace {

struct CondArgs {
  int ic, ec, p, C;
  float tau;
};

// one thread per (trajectory j, joint d)
__global__ void k_cond_fixed(const float* __restrict__ y, int64_t B, int T, int64_t sb, int64_t st, int64_t sd,
                             const int32_t* __restrict__ jidx, int dj, const float* __restrict__ times,
                             const float* __restrict__ knots, CondArgs c, float* __restrict__ init_pos,
                             float* __restrict__ init_vel, float* __restrict__ end_pos, float* __restrict__ end_vel,
                             float* __restrict__ p_init, float* __restrict__ p_end) {
  const int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  if (i >= B * dj) return;
  const int64_t j = i / dj;
  const int d = (int)(i - j * dj);
  const float* yr = y + j * sb + (int64_t)jidx[d] * sd;
  const float inv_dt = __fdiv_rn(1.0f, __fsub_rn(times[1], times[0]));   // 1 / (t[1] - t[0])
  const float pf = (float)c.p;
  float ip = 0.0f;
  if (c.ic) {
    const float y0 = yr[0], y1 = yr[st];
    ip = y0;
    const float iv = __fmul_rn(__fsub_rn(y1, y0), inv_dt);
    init_pos[i] = y0;
    init_vel[i] = iv;
    p_init[i * c.ic] = 0.0f;
    if (c.ic == 2) {   // init_vel * tau * dk0 / p + 0
      const float dk0 = __fsub_rn(knots[1 + c.p], knots[1]);
      p_init[i * c.ic + 1] = __fadd_rn(__fdiv_rn(__fmul_rn(__fmul_rn(iv, c.tau), dk0), pf), 0.0f);
    }
  }
  if (c.ec) {
    const float ya = yr[(int64_t)(T - 1) * st], yb = yr[(int64_t)(T - 2) * st];
    const float ev = __fmul_rn(__fsub_rn(ya, yb), inv_dt);
    const float e = c.ic ? __fsub_rn(ya, ip) : ya;   // relative to init_pos when it exists
    const int ne = c.ec < 0 ? -c.ec : c.ec;
    const float dke = __fsub_rn(knots[c.C - 1 + c.p], knots[c.C - 1]);
    const float slope = __fdiv_rn(__fmul_rn(__fmul_rn(ev, c.tau), dke), pf);   // end_vel * tau * dke / p
    if (c.ec == -1) {
      p_end[i] = slope;
    } else if (c.ec == 1) {
      p_end[i] = e;
    } else {
      p_end[i * ne] = __fsub_rn(e, slope);
      p_end[i * ne + 1] = e;
    }
    end_pos[i] = c.ic ? __fadd_rn(e, ip) : e;
    end_vel[i] = ev;
  }
}

// one thread per (trajectory j, time t, joint d); Phi_full [T][C] shared (full_sb = 0) or per
// trajectory [B][T][C].  The fixed columns in ascending order, as the einsum's sum over k (the
// other columns are zero), then + init_pos, then added to the fitted positions.
__global__ void k_cond_add(float* __restrict__ pos, int64_t B, int T, int D, const int32_t* __restrict__ jidx,
                           int dj, const float* __restrict__ full, int64_t full_sb, CondArgs c,
                           const float* __restrict__ p_init, const float* __restrict__ p_end,
                           const float* __restrict__ init_pos) {
  const int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  if (i >= B * T * dj) return;
  const int64_t jt = i / dj;
  const int d = (int)(i - jt * dj);
  const int64_t j = jt / T;
  const int t = (int)(jt - j * T);
  const float* ph = full + j * full_sb + (int64_t)t * c.C;
  const int64_t jd = j * dj + d;
  float acc = 0.0f;
  bool any = false;
  auto term = [&](int k, float w) {
    const float v = __fmul_rn(ph[k], w);
    acc = any ? __fadd_rn(acc, v) : v;
    any = true;
  };
  for (int k = 0; k < c.ic; ++k) term(k, p_init[jd * c.ic + k]);
  if (c.ec == -1) {
    term(c.C - 2, -p_end[jd]);
  } else if (c.ec > 0) {
    for (int q = 0; q < c.ec; ++q) term(c.C - c.ec + q, p_end[jd * c.ec + q]);
  }
  if (c.ic) acc = __fadd_rn(acc, init_pos[jd]);
  float* o = pos + jt * D + jidx[d];
  *o = __fadd_rn(*o, acc);
}

// k_cond_add for long trajectories (T > 256 or C > 20) on a shared basis: a workgroup owns a tile
// of TB trajectories x CH time rows and walks the tiles grid-stride.  Per tile the LDS holds
//   sB [CH][nf]      the nf <= 4 fixed columns of Phi_full for the chunk's rows (never the whole row)
//   sW [TB][dj][nf]  each trajectory's fixed control points in column order (end order -1 negated)
//   sI [TB][dj]      init_pos
// and, for the kernel's life, sMap [D]: output column -> joint slot, -1 for a gripper column.  A
// trajectory's chunk is CH * D contiguous floats: it moves as 16-byte loads / stores between its
// first and last 16-byte boundary and as scalars outside them, whatever D and T are.  Each element
// takes k_cond_add's terms in k_cond_add's order, so its bits do not depend on the kernel.
__device__ __forceinline__ float cond_long_term(const float* __restrict__ bt, const float* __restrict__ w, int nf,
                                                bool has_init, float ip) {
  float acc = __fmul_rn(bt[0], w[0]);
  for (int f = 1; f < nf; ++f) acc = __fadd_rn(acc, __fmul_rn(bt[f], w[f]));
  return has_init ? __fadd_rn(acc, ip) : acc;
}

__global__ __launch_bounds__(256) void k_cond_add_long(float* __restrict__ pos, int64_t B, int T, int D,
                                                       const int32_t* __restrict__ jidx, int dj,
                                                       const float* __restrict__ full, CondArgs c, int CH, int TB,
                                                       const float* __restrict__ p_init,
                                                       const float* __restrict__ p_end,
                                                       const float* __restrict__ init_pos) {
  extern __shared__ float cond_lds[];
  const int tid = threadIdx.x;
  const int ne = c.ec == -1 ? 1 : c.ec;   // fixed end columns read
  const int nf = c.ic + ne;
  const bool has_init = c.ic != 0;
  float* sB = cond_lds;
  float* sW = sB + CH * nf;
  float* sI = sW + TB * dj * nf;
  int* sMap = reinterpret_cast<int*>(sI + TB * dj);
  for (int i = tid; i < D; i += 256) sMap[i] = -1;
  __syncthreads();
  for (int i = tid; i < dj; i += 256) {
    const int col = jidx[i];
    if (col >= 0 && col < D) sMap[col] = i;
  }
  const int nch = (T + CH - 1) / CH;
  const int64_t ntiles = ((B + TB - 1) / TB) * nch;
  for (int64_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
    const int64_t jt = tile / nch;
    const int t0 = (int)(tile - jt * nch) * CH;
    const int rows = min(CH, T - t0);
    const int64_t j0 = jt * TB;
    const int nb = (int)min<int64_t>(TB, B - j0);
    __syncthreads();   // the previous tile's readers are done with sB / sW / sI
    for (int i = tid; i < rows * nf; i += 256) {
      const int r = i / nf, f = i - r * nf;
      const int k = f < c.ic ? f : (c.ec == -1 ? c.C - 2 : c.C - c.ec + (f - c.ic));
      sB[i] = full[(int64_t)(t0 + r) * c.C + k];
    }
    for (int i = tid; i < nb * dj; i += 256) {
      const int64_t jd = j0 * dj + i;
      float* w = sW + i * nf;
      for (int k = 0; k < c.ic; ++k) w[k] = p_init[jd * c.ic + k];
      if (c.ec == -1) w[c.ic] = -p_end[jd];
      for (int q = 0; q < c.ec; ++q) w[c.ic + q] = p_end[jd * c.ec + q];
      if (has_init) sI[i] = init_pos[jd];
    }
    __syncthreads();
    const int n = rows * D;
    for (int b = 0; b < nb; ++b) {
      float* base = pos + ((j0 + b) * (int64_t)T + t0) * D;
      const float* w = sW + b * dj * nf;
      const float* ip = sI + b * dj;
      const int head = min(n, (int)((4 - ((reinterpret_cast<uintptr_t>(base) >> 2) & 3)) & 3));
      const int nvec = (n - head) >> 2;
      const int tail = head + nvec * 4;
      if (tid < head + (n - tail)) {   // at most 3 + 3 elements outside the 16-byte body
        const int l = tid < head ? tid : tail + (tid - head);
        const int t = l / D;
        const int d = sMap[l - t * D];
        if (d >= 0)
          base[l] = __fadd_rn(base[l], cond_long_term(sB + t * nf, w + d * nf, nf, has_init, has_init ? ip[d] : 0.0f));
      }
      for (int v = tid; v < nvec; v += 256) {
        const int l = head + 4 * v;
        int t = l / D, col = l - t * D;
        float4* p4 = reinterpret_cast<float4*>(base + l);
        const float4 x = *p4;
        float e[4] = {x.x, x.y, x.z, x.w};
        bool touched = false;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          const int d = sMap[col];
          if (d >= 0) {
            e[q] = __fadd_rn(e[q], cond_long_term(sB + t * nf, w + d * nf, nf, has_init, has_init ? ip[d] : 0.0f));
            touched = true;
          }
          if (++col == D) { col = 0; ++t; }
        }
        if (touched) *p4 = make_float4(e[0], e[1], e[2], e[3]);
      }
    }
  }
}

// Tile of k_cond_add_long that fits 48 KB of LDS: up to 256 rows x 8 trajectories, trajectories
// given up first.  False when not even one row of one trajectory fits (k_cond_add serves it).
bool cond_long_tile(int64_t B, int T, int D, int dj, int nf, int& CH, int& TB, unsigned& lds) {
  if (D > 4096) return false;
  auto bytes = [&](int ch, int tb) { return 4 * ((int64_t)ch * nf + (int64_t)tb * dj * (nf + 1) + D); };
  CH = std::min(T, 256);
  TB = (int)std::min<int64_t>(B, 8);
  while (bytes(CH, TB) > 48 * 1024 && TB > 1) TB = (TB + 1) / 2;
  while (bytes(CH, TB) > 48 * 1024 && CH > 1) CH = (CH + 1) / 2;
  lds = (unsigned)bytes(CH, TB);
  return bytes(CH, TB) <= 48 * 1024;
}

bool cond_orders_ok(int ic, int ec) { return ic >= 0 && ic <= 2 && ec >= -1 && ec <= 2 && (ic != 0 || ec != 0); }

}  // namespace

extern "C" int beast_cond_fixed_f32(const float* traj, int64_t B, int T, int64_t sb, int64_t st, int64_t sd,
                                    const int32_t* joint_idx, int dj, const float* times, const float* knots,
                                    int degree, int n_ctrl, float tau, int init_order, int end_order,
                                    float* init_pos, float* init_vel, float* end_pos, float* end_vel,
                                    float* params_init, float* params_end, void* stream) {
  BEAST_REQUIRE(cond_orders_ok(init_order, end_order), "beast_cond_fixed_f32: orders (%d, %d) out of range",
                init_order, end_order);
  BEAST_REQUIRE(B >= 0 && dj >= 0, "beast_cond_fixed_f32: B=%lld, dj=%d must be >= 0", (long long)B, dj);
  BEAST_REQUIRE(T >= 2, "index 1 is out of bounds for dimension 1 with size %d", T);
  BEAST_REQUIRE(degree >= 1 && n_ctrl >= 2, "beast_cond_fixed_f32: degree %d / control points %d", degree, n_ctrl);
  BEAST_REQUIRE(traj && joint_idx && times && knots, "beast_cond_fixed_f32: null input pointer");
  BEAST_REQUIRE(init_order == 0 || (init_pos && init_vel && params_init), "beast_cond_fixed_f32: null init output");
  BEAST_REQUIRE(end_order == 0 || (end_pos && end_vel && params_end), "beast_cond_fixed_f32: null end output");
  if (B == 0 || dj == 0) return BEAST_OK;
  Queue q;
  BEAST_TRY(queue_of(stream, q, "beast_cond_fixed_f32"));
  const CondArgs c{init_order, end_order, degree, n_ctrl, tau};
  const int64_t n = B * dj;
  return launch<k_cond_fixed>((unsigned)((n + 255) / 256), 256, 0, q, "k_cond_fixed", traj, B, T, sb, st, sd, joint_idx,
                              dj, times, knots, c, init_pos, init_vel, end_pos, end_vel, params_init, params_end);
}

extern "C" int beast_cond_add_f32(float* pos, int64_t B, int T, int D, const int32_t* joint_idx, int dj,
                                  const float* full_basis, int64_t full_sb, int n_ctrl, int init_order, int end_order,
                                  const float* params_init, const float* params_end, const float* init_pos,
                                  void* stream) {
  BEAST_REQUIRE(cond_orders_ok(init_order, end_order), "beast_cond_add_f32: orders (%d, %d) out of range",
                init_order, end_order);
  BEAST_REQUIRE(B >= 0 && T >= 0 && dj >= 0 && D >= dj, "beast_cond_add_f32: bad shape B=%lld T=%d D=%d dj=%d",
                (long long)B, T, D, dj);
  BEAST_REQUIRE(n_ctrl >= 2 && full_sb >= 0, "beast_cond_add_f32: control points %d / basis stride", n_ctrl);
  BEAST_REQUIRE(pos && joint_idx && full_basis, "beast_cond_add_f32: null pointer");
  BEAST_REQUIRE(init_order == 0 || (params_init && init_pos), "beast_cond_add_f32: null init condition");
  BEAST_REQUIRE(end_order == 0 || params_end, "beast_cond_add_f32: null end condition");
  if (B == 0 || T == 0 || dj == 0) return BEAST_OK;
  Queue q;
  BEAST_TRY(queue_of(stream, q, "beast_cond_add_f32"));
  const CondArgs c{init_order, end_order, 0, n_ctrl, 0.0f};
  // two kernels: k_cond_add (one thread per element) inside T <= 256 and n_ctrl <= 20 and for every
  // per-trajectory basis; k_cond_add_long (tiles, fixed columns in LDS, 16-byte rows) beyond
  int CH, TB;
  unsigned lds;
  if ((T > 256 || n_ctrl > 20) && full_sb == 0 &&
      cond_long_tile(B, T, D, dj, init_order + (end_order == -1 ? 1 : end_order), CH, TB, lds)) {
    const int64_t ntiles = ((B + TB - 1) / TB) * ((T + CH - 1) / CH);
    return launch<k_cond_add_long>((unsigned)grid_for(ntiles, (int)lds, q.dev), 256, lds, q, "k_cond_add_long", pos, B,
                                   T, D, joint_idx, dj, full_basis, c, CH, TB, params_init, params_end, init_pos);
  }
  const int64_t n = B * T * dj;
  return launch<k_cond_add>((unsigned)((n + 255) / 256), 256, 0, q, "k_cond_add", pos, B, T, D, joint_idx, dj,
                            full_basis, full_sb, c, params_init, params_end, init_pos);
}
