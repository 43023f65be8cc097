// Encode kernels (codec.hip's second layer): k_encode, the 4- / 7-wave tile walk for every shape,
// and k_encode_v, one wave per trajectory for the fixed BEAST shapes; their argument blocks and
// LDS layouts.  Tokens and params of the two are bit-identical (shared quantiser, same products
// in the same order).  A tile's fit and epilogue are enc_fit_tile / enc_store_tile, which
// windows.hip's k_encode_windows runs over its own image of the same layout.
#pragma once

#include "codec_device.h"

namespace {

constexpr int ECH = 4;    // encode: K-steps per LDS-operand chunk

// ----------------------------------------------------------------- encode --
struct EncArgs {
  const float* traj;
  int64_t B, sb, st, sd, ntiles;
  int row_elems, vocab, phases;
  const int32_t* dof_src;
  const float* proj;   // [kinds][16][Tp] fp32 rounding of the fp64 ridge projection
  const float* w_min;
  const float* w_max;
  int64_t tok_offset;
  float* params_out;
  long long* tokens_out;
  Geom g;
  const float* const* traj_list;   // list mode: batch i at traj_list[i], list_rows rows each
  int64_t list_rows;               //   (a multiple of the tile, so no tile straddles two batches)
};

struct EncVArgs {
  const int32_t* dof_src;
  const float* proj;
  const float* w_min;
  const float* w_max;
  long long* tokens_out;
  float* params_out;
  int64_t tok_offset;
  int vocab, phases;
};
// First trajectory of tile row b0 (FAST path: contiguous rows of stride sb)
__device__ __forceinline__ const float* enc_tile_src(const EncArgs& a, int64_t b0) {
  if (a.traj_list == nullptr) return a.traj + b0 * a.sb;
  const uint64_t bi = (uint64_t)b0 / (uint64_t)a.list_rows;
  return a.traj_list[bi] + (b0 - (int64_t)bi * a.list_rows) * a.sb;
}

struct EncSmem {
  int P, Y, pb, kq, wlo, whi, lcol, total;
};

// Every buffer an LDS-DMA fills is padded to whole wave-instructions (64 lanes x 16 B).
template <int TBT>
__host__ __device__ inline EncSmem enc_smem(int T, int Tp, int Dl, int D, int N, int nkinds) {
  EncSmem s;
  int o = 0;
  // DMA destinations padded to whole wave-instructions, plus slack for the MFMA loop's
  // one-step-ahead operand reads past the last row (never used)
  s.P = o;    o += round_up(nkinds * 16 * Tp * 4 + 64 * ECH, 1024);   // fp32 [16][Tp] projection per kind
  s.Y = o;    o += round_up(TBT * T * Dl * 4, 1024);
  s.pb = o;   o += round_up(TBT * D * N * 4, 16);        // params, (d n) per trajectory
  s.kq = o;   o += round_up(D * N * 16, 16);             // {lo, hi, scale, 0} per (d n) column
  s.wlo = o;  o += round_up(D * N * 4, 256);
  s.whi = o;  o += round_up(D * N * 4, 256);
  s.lcol = o; o += round_up(D * 4, 256);
  s.total = o;
  return s;
}

// The fit of one tile, shared by every kernel that walks tiles (k_encode, windows.hip's
// k_encode_windows): params[j][d][n] = sum_t P_kind[n][t] y[j][t][d]  (f32 MFMA 16x16x4; A = P,
// B = y) into the (d n) image pb.  A wave owns two column tiles per pass (two independent chains),
// operands pointer-stepped through LDS; rows t >= T (tail step) meet a zero A column.
// rows_of(j, base, last): trajectory j's sample t is row min(t, last) of the image, rows of Dl
// floats from float `base` of Y (last <= T - 1; a window that ends early repeats its last row);
// col_of(d): the column of DoF d inside a row.
template <int TBT, class S, class RowsOf, class ColOf>
__device__ __forceinline__ void enc_fit_tile(const Geom& g, const Dims<S>& m, const float* P, const float* Y, float* pb,
                                             int Dl, int nb, int wave, int lr, int lk, bool first, RowsOf rows_of,
                                             ColOf col_of) {
  constexpr int NW = S::W;
  const int D = m.D, N = m.N, T = m.T, Tp = m.Tp, DN = D * N;
  const int nq = n_coltiles<TBT>(m);
  for (int q0 = wave; q0 < nq; q0 += NW * 2) {
    int j0, d0, k0, j1, d1, k1;
    bool ok0, ok1;
    tile_col<TBT>(g, m, q0, lr, j0, d0, k0, ok0);
    tile_col<TBT>(g, m, min(q0 + NW, nq - 1), lr, j1, d1, k1, ok1);
    ok0 = ok0 && j0 < nb;
    ok1 = ok1 && j1 < nb && (q0 + NW < nq);
    const int c0 = col_of(d0);
    const int c1 = col_of(d1);
    int base0, last0, base1, last1;
    rows_of(j0, base0, last0);
    rows_of(j1, base1, last1);
    // K-steps in chunks of ECH: every LDS operand of a chunk is read before its MFMAs and
    // the next chunk's reads are issued before them too (one LDS round trip per chunk);
    // even / odd steps accumulate separately (two chains per tile).  Step s covers rows
    // t = 4s + lane/16, clamped to the trajectory's last row (the zero-padded P columns meet
    // the rows t >= T).
    const int nst = (T + 3) >> 2;
    const bool two = q0 + NW < nq;   // wave-uniform: a second column tile this pass
    const float* pa0 = P + (k0 * 16 + lr) * Tp + lk;
    const float* pa1 = P + (k1 * 16 + lr) * Tp + lk;
    const float* yc0 = Y + base0 + c0;
    const float* yc1 = Y + base1 + c1;
    float4_t acc0 = {0.0f, 0.0f, 0.0f, 0.0f}, acc1 = acc0, acc2 = acc0, acc3 = acc0;
    float xa[ECH], ya[ECH], xb[ECH], yb[ECH];
#pragma unroll
    for (int i = 0; i < ECH; ++i) {
      const int t = 4 * i + lk;
      xa[i] = pa0[4 * i]; ya[i] = yc0[min(t, last0) * Dl]; xb[i] = pa1[4 * i]; yb[i] = yc1[min(t, last1) * Dl];
    }
    for (int c = 0; c < nst; c += ECH) {
      float nxa[ECH], nya[ECH], nxb[ECH], nyb[ECH];
#pragma unroll
      for (int i = 0; i < ECH; ++i) {   // next chunk (reads past the end land in LDS slack, unused)
        const int st = c + ECH + i, t = 4 * st + lk;
        nxa[i] = pa0[4 * st]; nya[i] = yc0[min(t, last0) * Dl]; nxb[i] = pa1[4 * st]; nyb[i] = yc1[min(t, last1) * Dl];
      }
#pragma unroll
      for (int i = 0; i < ECH; ++i) {
        if (c + i < nst) {   // wave-uniform
          if (i & 1) acc1 = __builtin_amdgcn_mfma_f32_16x16x4f32(xa[i], ya[i], acc1, 0, 0, 0);
          else acc0 = __builtin_amdgcn_mfma_f32_16x16x4f32(xa[i], ya[i], acc0, 0, 0, 0);
          if (two) {
            if (i & 1) acc3 = __builtin_amdgcn_mfma_f32_16x16x4f32(xb[i], yb[i], acc3, 0, 0, 0);
            else acc2 = __builtin_amdgcn_mfma_f32_16x16x4f32(xb[i], yb[i], acc2, 0, 0, 0);
          }
        }
      }
#pragma unroll
      for (int i = 0; i < ECH; ++i) { xa[i] = nxa[i]; ya[i] = nya[i]; xb[i] = nxb[i]; yb[i] = nyb[i]; }
    }
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      acc0[r] = __fadd_rn(acc0[r], acc1[r]);
      acc2[r] = __fadd_rn(acc2[r], acc3[r]);
    }
    // f32 C/D map: col = lane & 15, row = (lane >> 4) * 4 + r.  Each lane writes its params
    // into the (d n) image; quantisation happens in the epilogue, spread over every thread.
    if (first && q0 == wave) STAMP(0, 8);
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int n = lk * 4 + r;
      if (n < N) {
        if (ok0) pb[j0 * DN + d0 * N + n] = acc0[r];
        if (ok1) pb[j1 * DN + d1 * N + n] = acc2[r];
      }
    }
  }
}

// The epilogue of one tile (rows b0 .. b0 + nb of the outputs): params (d n) out of the image pb,
// tokens (n d) quantised from it with the bounds kq / wlo / whi, both contiguous per tile.
template <class S>
__device__ __forceinline__ void enc_store_tile(const EncArgs& a, const Dims<S>& m, const float* pb, const float4* kq,
                                               const float* wlo, const float* whi, int64_t b0, int nb, float vm1,
                                               bool first) {
  constexpr int NT = S::W * 64;
  const Geom& g = a.g;
  const int D = m.D, N = m.N, per = m.per, DN = D * N;
  const int tid = threadIdx.x;
  const bool quant = a.tokens_out != nullptr;
  constexpr int SP = (S::W == 7) ? LAT_SP : 0;   // the 7-wave shape is the latency regime's
  if (a.params_out != nullptr && (a.phases & 4)) store_out<NT, SP>(a.params_out + b0 * DN, pb, nb * DN);
  if (first) STAMP(0, 5);
  if (quant && (a.phases & 8)) {
    // tokens in (n d) order: each thread quantises 4 consecutive tokens from the (d n)
    // params image (fast bins; the exactly-rounded chain only where one lies near a
    // rounding boundary), widens them to int64 + offset and stores 2 x 16 B.
    const int total = nb * per;
    long long* tout = a.tokens_out + b0 * per;
    const unsigned long long off = (unsigned long long)a.tok_offset;
    auto col_of = [&](int e, int& pj) {   // token e of the tile -> (d n) column, trajectory
      const int j = (int)div_by<S>((uint32_t)e, per, g.fd_per);
      const int r = e - j * per;
      const int n = (int)div_by<S>((uint32_t)r, D, g.fd_D);
      pj = j * DN;
      return (r - n * D) * N + n;
    };
    int done = 0;
    if ((((uintptr_t)tout) & 15) == 0) {
      const int n4 = total >> 2;
      for (int i = tid; i < n4; i += NT) {
        int bin[4], c[4], pj[4];
        float pv[4], lo[4], hi[4], k[4];
        // every LDS operand of the 4 tokens is requested before any is used (one round trip)
#pragma unroll
        for (int u = 0; u < 4; ++u) c[u] = col_of(4 * i + u, pj[u]);
#pragma unroll
        for (int u = 0; u < 4; ++u) {
          pv[u] = pb[pj[u] + c[u]];
          const float4 q = kq[c[u]];
          lo[u] = q.x; hi[u] = q.y; k[u] = q.z;
        }
        beast::quantize_bins(pv, lo, hi, vm1, bin, k);
        st16<SP>(tout + 4 * i, beast::widen_bin(bin[0], off), beast::widen_bin(bin[1], off));
        st16<SP>(tout + 4 * i + 2, beast::widen_bin(bin[2], off), beast::widen_bin(bin[3], off));
      }
      done = n4 << 2;
    }
    for (int e = done + tid; e < total; e += NT) {
      int pj;
      const int c = col_of(e, pj);
      tout[e] = beast::widen_bin(beast::quantize_bin(pb[pj + c], wlo[c], whi[c], vm1), off);
    }
  }
}

template <int TBT, bool FAST, class S>
__global__ __launch_bounds__(S::W * 64) void k_encode(EncArgs a) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  constexpr int NW = S::W, NT = NW * 64;
  const Geom& g = a.g;
  const Dims<S> m(g);
  const int D = m.D, N = m.N, T = m.T, Tp = m.Tp, DN = D * N;
  const int Dl = FAST ? (S::DL ? S::DL : a.row_elems) : D;
  const int nkinds = (m.nj < D) ? 2 : 1;
  const EncSmem L = enc_smem<TBT>(T, Tp, Dl, D, N, nkinds);
  float* P = reinterpret_cast<float*>(smem + L.P);
  float* Y = reinterpret_cast<float*>(smem + L.Y);
  float* pb = reinterpret_cast<float*>(smem + L.pb);
  float* wlo = reinterpret_cast<float*>(smem + L.wlo);
  float* whi = reinterpret_cast<float*>(smem + L.whi);
  float4* kq = reinterpret_cast<float4*>(smem + L.kq);
  int* lcol = reinterpret_cast<int*>(smem + L.lcol);
  const int tid = threadIdx.x;
  const bool quant = a.tokens_out != nullptr;
  const int tile_elems = T * a.row_elems;   // FAST: one trajectory, contiguous, % 4 == 0

  STAMP(0, 0);
  BSTAMP(0, 0);
  // ---- prologue: the first tile and every constant go HBM -> LDS by DMA in one round trip
  if (FAST && (a.phases & 1) && blockIdx.x < a.ntiles) {
    const int64_t b0 = (int64_t)blockIdx.x * TBT;
    const int nb = (int)min<int64_t>(TBT, a.B - b0);
    dma16<NT>(Y, enc_tile_src(a, b0), (nb * tile_elems) >> 2);
  }
  STAMP(0, 9);
  dma16<NT>(P, a.proj, nkinds * 4 * Tp);
  STAMP(0, 10);
  if (quant) {
    dma4<NT>(wlo, a.w_min, DN);
    dma4<NT>(whi, a.w_max, DN);
  }
  dma4<NT>(lcol, a.dof_src, D);
  STAMP(0, 11);

  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6), lane = tid & 63;
  const int lr = lane & 15, lk = lane >> 4;
  const float vm1 = (float)(a.vocab - 1);

  for (int64_t tile = blockIdx.x; tile < a.ntiles; tile += gridDim.x) {
    const int64_t b0 = tile * TBT;
    const int nb = (int)min<int64_t>(TBT, a.B - b0);

    // ---- the trajectory tile lands in LDS (the first one is already in flight)
    if (a.phases & 1) {
      if (FAST) {
        if (tile != blockIdx.x) dma16<NT>(Y, enc_tile_src(a, b0), (nb * tile_elems) >> 2);
      } else {
        const int pt = T * D;
        for (int e = tid; e < nb * pt; e += NT) {
          const int j = e / pt, r = e - j * pt, t = r / D, d = r - t * D;
          const int col = a.dof_src[d];
          Y[e] = (col >= 0 && col < a.row_elems)
                     ? a.traj[(b0 + j) * a.sb + (int64_t)t * a.st + (int64_t)col * a.sd] : 0.0f;
        }
      }
    }
    if (tile == blockIdx.x) STAMP(0, 1);
    __syncthreads();   // waits for the DMA (vmcnt) and the LDS stores
    if (tile == blockIdx.x) STAMP(0, 2);
    if (tile == blockIdx.x + gridDim.x) STAMP(0, 12);
    if (quant && tile == blockIdx.x)   // bounds landed with the first tile; read after the next barrier
      for (int i = tid; i < DN; i += NT)
        kq[i] = make_float4(wlo[i], whi[i], beast::quantize_scale(wlo[i], whi[i], vm1), 0.0f);

    // ---- fit: every trajectory's rows are its own T rows of the [j][t][Dl] image
    if (a.phases & 2)
      enc_fit_tile<TBT, S>(
          g, m, P, Y, pb, Dl, nb, wave, lr, lk, tile == blockIdx.x,
          [&](int j, int& base, int& last) { base = j * T * Dl; last = T - 1; },
          [&](int d) { return FAST ? min(max(lcol[d], 0), Dl - 1) : d; });
    if (tile == blockIdx.x) STAMP(0, 3);
    if (tile == blockIdx.x + gridDim.x) STAMP(0, 13);
    __syncthreads();
    if (tile == blockIdx.x) STAMP(0, 4);

    // ---- epilogue: params (d n) and tokens (n d), both contiguous per tile
    enc_store_tile<S>(a, m, pb, kq, wlo, whi, b0, nb, vm1, tile == blockIdx.x);
    if (tile == blockIdx.x) STAMP(0, 6);
    if (tile == blockIdx.x + gridDim.x) STAMP(0, 14);
  }
#ifdef BEAST_STAMPS
  __builtin_amdgcn_s_waitcnt(0);
  STAMP(0, 7);
  BSTAMP(0, 1);
#endif
}

// ------------------------------------------------------- encode, per-trajectory waves --
// waves = trajectories per tile of k_encode_v / k_reconstruct_v.  Round 6: 16 (one 1,024-thread
// workgroup per CU at B = 4,096) for both -- the encode -> reconstruct step is 2.4 % shorter than
// with 8-wave tiles (9.49-9.51 vs 9.70-9.75 us per step, outputs bitwise equal), although either
// kernel alone, launched back to back with itself, is 0.1 us slower; 16 / 8 mixed is slower than
// both (profiles/r06/codec_tile_width_ab_r06k.txt).  BEAST_RV_WE / _WR override (measurements).
// Bulk encode launches (more than one 16-trajectory tile per CU) keep 8-wave tiles: their 45 KB of
// LDS fit three workgroups -- 24 waves -- per CU, where a 16-wave tile's 84 KB fits one
// (B = 262,144: 232 vs 242 us, profiles/r06/).
#ifndef BEAST_RV_WE
#define BEAST_RV_WE 16
#endif
#ifndef BEAST_RV_WR
#define BEAST_RV_WR 16
#endif
constexpr int RV_WE = BEAST_RV_WE, RV_WR = BEAST_RV_WR, RV_WE_BULK = 8;
// Fixed shapes (the BEAST defaults), every batch size.  Wave j of the workgroup owns trajectory
// j of the W-trajectory tile: C[n][d] = sum_t P_kind[n][t] y[j][t][lcol[d]] on
// v_mfma_f32_16x16x4_f32 (A = P, B = y[j]: the columns are the trajectory's DoFs), then the wave
// quantises its own accumulators, writes its trajectory's params (d n) and tokens (n d) into an
// LDS image of its own and copies both out with 16-byte write-through stores -- no workgroup
// barrier after the prologue, so one wave's stores overlap the others' MFMAs.  It replaced round 2's
// pipelined kernel (two sub-tiles, DMA / MFMA waves and store waves; 4.70 vs 4.44 us at B = 4,096,
// 209 vs 214 us at B = 262,144, profiles/r05/).  Same products in the same K order with the same
// even / odd accumulators as k_encode, and the same quantiser, so params and tokens are
// bit-identical.  With gripper DoFs each kind's chain sees zero B columns for the other kind.
struct EvSmem {
  int Y, P, wlo, whi, lcol, pimg, timg, total;
};
template <class S, int W>
__host__ __device__ constexpr EvSmem ev_smem(int nkinds) {
  using PS = VShape<S>;
  EvSmem s{};
  int o = 0;
  s.Y = o;    o += round_up(W * PS::T * PS::DL * 4, 1024);
  s.P = o;    o += round_up(nkinds * 16 * PS::Tp * 4, 1024);
  s.wlo = o;  o += round_up(PS::DN * 4, 256);
  s.whi = o;  o += round_up(PS::DN * 4, 256);
  s.lcol = o; o += round_up(PS::D * 4, 256);
  s.pimg = o; o += W * round_up(PS::DN * 4, 16);
  s.timg = o; o += W * round_up(PS::DN * 8 + 8, 16);   // + one slot the padding lanes write to
  s.total = o;
  return s;
}

// Round 7: the chain that runs after the tile barrier is shorter.  The quantiser runs three slots
// per lane, not four: rows n = 4 lk + 3 of lanes lk < 2 move to slot 2 of lanes lk >= 2 (one
// v_permlane32_swap), whose own rows there are padding (N <= 10), so 192 slots serve the 140 values.
// The LDS addresses of a lane's operands, bounds and token-image slots depend on the lane alone and
// are computed before the barrier, while the DMA is in flight; padding slots write to a spare image
// slot instead of being predicated.  The bounds themselves still arrive by DMA: per-lane global
// loads of them before the barrier cost more vector-memory issue time than the chain saves
// (profiles/r07/codec_chain_ab.txt).
template <class S, int SP, int W>
__global__ __launch_bounds__(W * 64) void k_encode_v(const float* __restrict__ traj, int64_t B, EncVArgs a) {
  using PS = VShape<S>;
  static_assert(PS::D <= 16 && PS::N <= 10 && PS::DL == PS::D,
                "per-trajectory encode: D <= 16, rows of D, N <= 10 (three quantiser slots per lane)");
  constexpr int NT = W * 64, D = PS::D, N = PS::N, T = PS::T, Tp = PS::Tp, DN = PS::DN, NST = PS::NST;
  constexpr int NJ = S::NJ;
  constexpr int nkinds = NJ < D ? 2 : 1;
  constexpr EvSmem L = ev_smem<S, W>(nkinds);
  constexpr int PIMG = round_up(DN * 4, 16) / 4, TIMG = round_up(DN * 8 + 8, 16) / 8;
  constexpr int NQ = 3;   // quantiser slots per lane
  static_assert((T * D) % 4 == 0 && (DN % 2) == 0, "per-trajectory encode: whole 16-byte rows");
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  float* Y = reinterpret_cast<float*>(smem + L.Y);
  float* P = reinterpret_cast<float*>(smem + L.P);
  float* wlo = reinterpret_cast<float*>(smem + L.wlo);
  float* whi = reinterpret_cast<float*>(smem + L.whi);
  int* lcol = reinterpret_cast<int*>(smem + L.lcol);
  const int tid = threadIdx.x, wave = __builtin_amdgcn_readfirstlane(tid >> 6), lane = tid & 63;
  const int64_t b0 = (int64_t)blockIdx.x * W;
  const int nb = (int)min<int64_t>(W, B - b0);
  const bool quant = a.tokens_out != nullptr;
  STAMP(0, 0);
  BSTAMP(0, 0);
  // ---- prologue: the tile and every constant HBM -> LDS by DMA, all in flight together
  constexpr int tile16 = T * D / 4;   // float4 per trajectory
  dma16<NT>(Y, reinterpret_cast<const float4*>(traj) + b0 * tile16, nb * tile16);
  STAMP(0, 9);
  dma16<NT>(P, a.proj, nkinds * 4 * Tp);
  if (quant) {
    dma4<NT>(wlo, a.w_min, DN);
    dma4<NT>(whi, a.w_max, DN);
  }
  dma4<NT>(lcol, a.dof_src, D);
  // ---- lane-only LDS addresses, computed while the DMA is in flight.  Lane (lr, lk): DoF d = lr;
  //      slot u holds row n = 4 lk + u, slot 2 of lanes lk >= 2 row 4 (lk - 2) + 3
  const int j = wave;
  const int lr = lane & 15, lk = lane >> 4;
  const bool dok = lr < D;
  const float vm1 = (float)(a.vocab - 1);
  int tq[NQ];   // byte offset of the slot's token in this wave's (n d) image
  int kq[NQ];   // byte offset of the slot's (d n) column in a bounds array, clamped for the padding slots
#pragma unroll
  for (int u = 0; u < NQ; ++u) {
    const int n = slot_row<true>(lk, u);
    kq[u] = (min(lr, D - 1) * N + min(n, N - 1)) * 4;
    tq[u] = L.timg + (j * TIMG + ((dok && n < N) ? n * D + lr : DN)) * 8;
    pin(kq[u]); pin(tq[u]);
  }
  int yb = L.Y + (j * T * D + lk * D) * 4;
  int yt = yb + (min(4 * (NST - 1) + lk, T - 1) - lk) * D * 4;   // the last K-step's row, clamped to T - 1
  int pb = L.P + (lr * Tp + lk) * 4;
  pin(yb); pin(yt); pin(pb);
  __syncthreads();
  STAMP(0, 2);
  if (j >= nb) return;   // no barrier follows
  // the DMA's clamped tail filled lcol[D ..] with the last DoF's column: no select for lanes lr >= D
  const int c4 = min(max(lcol[lr], 0), D - 1) * 4;
  yb += c4;
  yt += c4;
  float qlo[NQ] = {0.0f, 0.0f, 0.0f}, qhi[NQ] = {0.0f, 0.0f, 0.0f};
  if (quant) {   // wave-uniform; read with the fit's operands
#pragma unroll
    for (int u = 0; u < NQ; ++u) {
      qlo[u] = *reinterpret_cast<const float*>(smem + L.wlo + kq[u]);
      qhi[u] = *reinterpret_cast<const float*>(smem + L.whi + kq[u]);
    }
  }
  // ---- fit: lane (lr, lk): A = P_kind[n = lr][t = 4 st + lk], B = y[j][t][lcol[d = lr]] (t clamped
  //      to T - 1: the zero-padded P columns meet those rows), even / odd steps accumulate apart.
  //      B columns d >= D are never stored, so with one kind they need no zeroing.
  float4_t acc0 = {0.0f, 0.0f, 0.0f, 0.0f}, acc1 = acc0;
#pragma unroll
  for (int kd = 0; kd < nkinds; ++kd) {
    const bool mine = nkinds == 1 || (dok && ((lr < NJ) == (kd == 0)));
    float xa[NST], ya[NST];
#pragma unroll
    for (int st = 0; st < NST; ++st) {   // every operand read before the chain (one LDS round trip)
      xa[st] = *reinterpret_cast<const float*>(smem + pb + (kd * 16 * Tp + 4 * st) * 4);
      const float y = *reinterpret_cast<const float*>(smem + (st + 1 < NST ? yb + 4 * st * D * 4 : yt));
      ya[st] = mine ? y : 0.0f;
    }
#pragma unroll
    for (int st = 0; st < NST; ++st) {
      if (st & 1) acc1 = __builtin_amdgcn_mfma_f32_16x16x4f32(xa[st], ya[st], acc1, 0, 0, 0);
      else acc0 = __builtin_amdgcn_mfma_f32_16x16x4f32(xa[st], ya[st], acc0, 0, 0, 0);
    }
  }
  STAMP(0, 3);
  // ---- C/D map: row n = lk * 4 + r, column d = lr.  Params (d n) and tokens (n d) of the trajectory
  //      into this wave's images; the quantiser is k_encode's (fast bins, the exact chain near a
  //      rounding boundary or for NaN / inf)
  float* pimg = reinterpret_cast<float*>(smem + L.pimg) + j * PIMG;
  const long long* timg = reinterpret_cast<const long long*>(smem + L.timg) + j * TIMG;
  float pv[4];
#pragma unroll
  for (int r = 0; r < 4; ++r) pv[r] = __fadd_rn(acc0[r], acc1[r]);
  if (dok) {
    float* q = pimg + lr * N + 4 * lk;
#pragma unroll
    for (int r = 0; r < 4; r += 2) {
      if (4 * lk + r + 1 < N) *reinterpret_cast<float2*>(q + r) = make_float2(pv[r], pv[r + 1]);
      else if (4 * lk + r < N) q[r] = pv[r];
    }
  }
  if (quant) {
    float qv[NQ];
    int bin[NQ];
    slot_values<true>(pv, qv);
    beast::quantize_bins(qv, qlo, qhi, vm1, bin);
    if (a.tok_offset == 0) {   // wave-uniform: no 64-bit add
#pragma unroll
      for (int u = 0; u < NQ; ++u) *reinterpret_cast<long long*>(smem + tq[u]) = beast::widen_bin(bin[u], 0ull);
    } else {
      const unsigned long long off = (unsigned long long)a.tok_offset;
#pragma unroll
      for (int u = 0; u < NQ; ++u) *reinterpret_cast<long long*>(smem + tq[u]) = beast::widen_bin(bin[u], off);
    }
  }
  wave_sync();
  STAMP(0, 5);
  // ---- 16-byte write-through stores of the trajectory's params (DN floats) and tokens (DN int64)
  if (a.phases & 4) {
    if (a.params_out != nullptr) wave_copy_out<SP, DN / 4>(a.params_out + (b0 + j) * DN, pimg, lane);
    if (quant) wave_copy_out<SP, DN / 2>(a.tokens_out + (b0 + j) * DN, timg, lane);
  }
  STAMP(0, 7);
#ifdef BEAST_STAMPS
  __builtin_amdgcn_s_waitcnt(0);
  STAMP(0, 8);
  BSTAMP(0, 1);
#endif
}

}  // namespace
