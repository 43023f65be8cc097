// Reconstruct kernels (codec.hip's third layer): k_reconstruct, the 4- / 7-wave tile walk on the
// MFMA, k_reconstruct_v, one wave per trajectory for the fixed BEAST shapes in the latency regime,
// and k_reconstruct_rows, the VALU path for per-row bases and decode-only calls; their argument
// blocks and LDS layouts.  Needs codec_encode.h only for RV_WR, the tile width it shares with
// k_encode_v's.
#pragma once

#include "codec_device.h"
#include "codec_encode.h"

namespace {

// ------------------------------------------------------------ reconstruct --
struct RecArgs {
  const long long* tokens;
  const float* ntokens;
  int64_t B, ntiles, tok_offset, basis_sb, init_p_sb;
  int vocab, Tout, ndo, phases, lut_n, tbt;
  const float* w_min;
  const float* w_max;
  const float* basis;      // [2][Tout][N] (shared) or per trajectory with stride basis_sb
  const int32_t* dof_dst;
  const float* init_p;
  const int32_t* init_p_src;
  float* params_out;
  float* pos_out;
  Geom g;
  FastDiv fd_row;          // Tout * ndo
};

// The per-trajectory kernels' argument blocks: only what k_encode_v / k_reconstruct_v read (their
// shapes are compile-time), 64 / 88 bytes instead of EncArgs' / RecArgs' ~260.  The runtime copies
// every launch's argument block into the kernarg ring, and a 224-byte block costs the host ~0.28 us
// more per launch than an 8- or 64-byte one (tools/launch/launch_bench.hip, profiles/r06/).
struct RecVArgs {
  const float* w_min;
  const float* w_max;
  const float* basis;
  const int32_t* dof_dst;
  const float* init_p;
  const int32_t* init_p_src;
  float* pos_out;
  int64_t tok_offset, init_p_sb;
  int vocab;
  float rinv;   // RN(1 / (vocab - 1)), IEEE-divided on the host: beast::exact_quotient's r
  int phases;
};

constexpr int LUT_MAX = 4096;   // dequantise LUT tok / (vocab - 1), IEEE-divided once
constexpr int RT_REG = 4;       // row tiles (64 output rows) whose basis operands live in registers

// W[j][d][n] from the staged tile: bit-exact discrete_to_continuous (beast/utils.py:20-25)
// or, for normalised tokens, denormalize_tensor's intent (utils.py:38-44).
__device__ __forceinline__ float rec_weight(const RecArgs& a, const unsigned char* tokl, int e, int k,
                                            const float* wlo, const float* whi, const float* lut, float vm1) {
  const float lo = wlo[k], hi = whi[k];
  if (a.ntokens) return beast::denormalize_one(reinterpret_cast<const float*>(tokl)[e], lo, hi);
  const long long t[1] = {reinterpret_cast<const long long*>(tokl)[e] - a.tok_offset};
  float nrm[1];
  lut_quotients(t, lut, a.lut_n, vm1, nrm);
  return beast::dequantize_quotient(nrm[0], lo, hi);
}

// B operand of one MFMA lane for KS K-steps: W[j][d][n], n = lk * KS + ks (clamped to N - 1
// for the read; the caller zeroes n >= N).  rec_weight's arithmetic, with every LDS read of
// the KS steps issued before any is used: tokens and bounds in one round trip, the LUT in
// a second; tokens outside the LUT (rare) take the IEEE division behind an exec branch.
template <int KS>
__device__ __forceinline__ void rec_weights(const RecArgs& a, const unsigned char* tokl, int j, int d, int lk,
                                            int N, int D, int per, const float* wlo, const float* whi,
                                            const float* lut, float vm1, float (&w)[KS]) {
  float lo[KS], hi[KS];
  int e[KS];
#pragma unroll
  for (int ks = 0; ks < KS; ++ks) {
    const int n = min(lk * KS + ks, N - 1), k = d * N + n;
    e[ks] = j * per + n * D + d;
    lo[ks] = wlo[k];
    hi[ks] = whi[k];
  }
  if (a.ntokens) {
#pragma unroll
    for (int ks = 0; ks < KS; ++ks)
      w[ks] = beast::denormalize_one(reinterpret_cast<const float*>(tokl)[e[ks]], lo[ks], hi[ks]);
    return;
  }
  long long t[KS];
#pragma unroll
  for (int ks = 0; ks < KS; ++ks) t[ks] = reinterpret_cast<const long long*>(tokl)[e[ks]] - a.tok_offset;
  float nrm[KS];
  lut_quotients(t, lut, a.lut_n, vm1, nrm);
#pragma unroll
  for (int ks = 0; ks < KS; ++ks) w[ks] = beast::dequantize_quotient(nrm[ks], lo[ks], hi[ks]);
}

struct RecSmem {
  int phi, tok, wlo, whi, lut, dst, out, pb, pmap, col2d, total;
  int Np4, RTR;   // padded basis width, padded output rows
  bool stage;
};

// Shared basis (KS > 0, MFMA): the basis operands are in registers (RT = RT_REG, T_out <= 64)
// or in LDS (RT = 0).  Per-row basis (KS == 0, VALU): W in LDS, rows of the basis from HBM.
template <int TBT, int KS, int RT>
__host__ __device__ inline RecSmem rec_smem(int Tout, int D, int N, int ndo, int nkinds, int lut_n) {
  RecSmem s;
  const int per = N * D;
  s.Np4 = KS ? 4 * KS : round_up(N, 4);
  s.RTR = KS ? round_up(Tout, 64) : Tout;   // row tiles in groups of four
  int o = 0;
  // basis in LDS: RT == 0 the zero-padded [kinds][RTR][Np4] image; RT > 0 the raw [kinds][Tout][N] (DMA)
  s.phi = o;   o += KS ? (RT == 0 ? round_up(nkinds * s.RTR * s.Np4 * 4, 16) : round_up(nkinds * Tout * N * 4, 1024)) : 0;
  s.tok = o;   o += round_up(TBT * per * 8, 1024);   // DMA destinations: whole wave-instructions
  s.wlo = o;   o += round_up(per * 4, 256);
  s.whi = o;   o += round_up(per * 4, 256);
  s.lut = o;   o += round_up(lut_n * 4, 16);
  s.dst = o;   o += round_up(D * 4, 256);
  s.pb = o;    o += KS ? 0 : round_up(TBT * D * s.Np4 * 4, 16);
  s.pmap = o;  o += KS ? 0 : round_up(per * 2, 16);   // (n d) slot -> W offset d*Np4 + n
  s.col2d = o; o += KS ? 0 : round_up(ndo * 4, 16);
  const int outb = round_up(TBT * s.RTR * ndo * 4, 16);
  s.stage = KS ? true : (o + outb) <= 96 * 1024;
  s.out = o;   o += s.stage ? outb : 0;
  s.total = o;
  return s;
}

// Shared-basis positions run on the MFMA (k_reconstruct*) while the padded output tile fits LDS,
// else in k_reconstruct_rows' sequential FMA order (k_roundtrip and k_blend_windows reproduce
// whichever applies).
template <int TBT>
inline bool rec_mfma_fits(int Tout, int D, int N, int ndo, int lut_n) {
  return rec_smem<TBT, 4, 0>(Tout, D, N, ndo, 2, lut_n).total <= 112 * 1024;
}

// decode-only output (params_out, (d n) order) straight from the staged tokens
template <int NT = NTHREADS>
__device__ __forceinline__ void rec_params_out(const RecArgs& a, const unsigned char* tokl, int64_t b0, int nb,
                                               const float* wlo, const float* whi, const float* lut, float vm1) {
  const Geom& g = a.g;
  const int per = g.per, D = g.D, N = g.N;
  float* pout = a.params_out + b0 * per;
  for (int e = threadIdx.x; e < nb * per; e += NT) {
    const uint32_t j = fdiv(e, g.fd_per);
    const int k = e - j * per;                 // (d n) index
    const uint32_t d = fdiv(k, g.fd_N);
    const int n = k - d * N;
    pout[e] = rec_weight(a, tokl, j * per + n * D + d, k, wlo, whi, lut, vm1);
  }
}

// ob rows [0, Tout) of each trajectory -> one contiguous HBM tile
template <class S>
__device__ __forceinline__ void rec_store(const RecArgs& a, float* gout, const float* ob, int nb, int RTR) {
  const int Tout = S::T ? S::T : a.Tout, ndo = S::DL ? S::DL : a.ndo;
  const int rowlen = Tout * ndo;
  if ((rowlen & 3) == 0 && ((RTR * ndo) & 3) == 0 && ((((uintptr_t)gout) & 15) == 0)) {
    const int n4 = nb * rowlen / 4;
    for (int i = threadIdx.x; i < n4; i += S::W * 64) {
      const uint32_t e = 4 * i;
      const uint32_t j = div_by<S>(e, rowlen, a.fd_row);
      st16<(S::W == 7) ? LAT_SP : 0>(reinterpret_cast<float4*>(gout) + i,
                                     *reinterpret_cast<const float4*>(ob + j * RTR * ndo + (e - j * rowlen)));
    }
  } else {
    for (int e = threadIdx.x; e < nb * rowlen; e += S::W * 64) {
      const uint32_t j = div_by<S>(e, rowlen, a.fd_row);
      gout[e] = ob[j * RTR * ndo + (e - j * rowlen)];
    }
  }
}

// tsrc (the token rows: a.tokens, or a.ntokens with esz 4), B and esz lead the argument list for
// kernarg preloading, as in k_encode_v: the first tile's DMA needs nothing else.
template <int TBT, int KS, int RT, class S>
__global__ __launch_bounds__(S::W * 64) void k_reconstruct(const void* __restrict__ tsrc, int64_t B, int esz,
                                                           RecArgs a) {
  static_assert(KS > 0, "shared-basis kernel");
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  constexpr int NW = S::W, NT = NW * 64;
  const Geom& g = a.g;
  const Dims<S> m(g);
  const int D = m.D, N = m.N, nj = m.nj, per = m.per;
  const int Tout = S::T ? S::T : a.Tout, ndo = S::DL ? S::DL : a.ndo;
  const int nkinds = (nj < D) ? 2 : 1;
  const int nq = n_coltiles<TBT>(m);
  const RecSmem L = rec_smem<TBT, KS, RT>(Tout, D, N, ndo, nkinds, a.lut_n);
  constexpr int Np4 = 4 * KS;
  const int RTR = L.RTR;
  float* phi = reinterpret_cast<float*>(smem + L.phi);
  const unsigned char* tokl = smem + L.tok;
  float* wlo = reinterpret_cast<float*>(smem + L.wlo);
  float* whi = reinterpret_cast<float*>(smem + L.whi);
  float* lut = reinterpret_cast<float*>(smem + L.lut);
  int* dst = reinterpret_cast<int*>(smem + L.dst);
  float* ob = reinterpret_cast<float*>(smem + L.out);
  const int tid = threadIdx.x, wave = __builtin_amdgcn_readfirstlane(tid >> 6), lane = tid & 63;
  const int lr = lane & 15, lk = lane >> 4;
  const float vm1 = (float)(a.vocab - 1);

  STAMP(1, 0);
  BSTAMP(1, 0);
  // ---- prologue: the first token tile, the bounds and the DoF map by DMA; the basis
  //      operands (registers or LDS) by clamped loads -- all in flight together
  // the first tile (the grid never exceeds the tile count); BEAST_DEBUG_PHASES does not skip it
  stage_rows<NT>(smem + L.tok, tsrc, B, esz, (int64_t)blockIdx.x * TBT, per, TBT);
  STAMP(1, 9);
  dma4<NT>(wlo, a.w_min, per);
  dma4<NT>(whi, a.w_max, per);
  dma4<NT>(dst, a.dof_dst, D);
  STAMP(1, 10);
  // A operand of MFMA row tile rt, K-step ks: Phi_kind[rt*16 + lr][n], n = lane/16 * KS + ks,
  // zero outside [Tout) x [N).  RT > 0: the raw basis [kinds][Tout][N] is DMA'd to LDS with
  // the first token tile and the operands are read into registers once, after it lands.
  float phr[2][RT > 0 ? RT : 1][KS];
  if constexpr (RT > 0) {
    const int pbytes = nkinds * Tout * N * 4;
    if ((pbytes & 15) == 0 && (((uintptr_t)a.basis) & 15) == 0) dma16<NT>(phi, a.basis, pbytes >> 4);
    else dma4<NT>(phi, a.basis, pbytes >> 2);
  } else {
    const int tot = nkinds * RTR * Np4, tn = RTR * Np4;
    for (int base = 0; base < tot; base += 8 * NT) {
      float v[8];
#pragma unroll
      for (int u = 0; u < 8; ++u) {
        const int i = min(base + u * NT + tid, tot - 1);
        const int k = i >= tn ? 1 : 0, r = i - k * tn, t = r / Np4, n = r - t * Np4;
        const float x = a.basis[(int64_t)k * Tout * N + min(t, Tout - 1) * N + min(n, N - 1)];
        const uint32_t keep = 0u - (uint32_t)((t < Tout) & (n < N));
        v[u] = __uint_as_float(__float_as_uint(x) & keep);
      }
#pragma unroll
      for (int u = 0; u < 8; ++u) phi[min(base + u * NT + tid, tot - 1)] = v[u];
    }
  }
  STAMP(1, 11);
  lut_fill(lut, a.lut_n, vm1, NT);
  STAMP(1, 12);
  // num_dof_out > D: the output columns dof_dst does not name are zeros (as k_reconstruct_rows
  // writes them).  The MFMA loop never touches them, so the image is cleared once.
  if (ndo > D)
    for (int i = tid; i < TBT * RTR * ndo; i += NT) ob[i] = 0.0f;

  for (int64_t tile = blockIdx.x; tile < a.ntiles; tile += gridDim.x) {
    const int64_t b0 = tile * TBT;
    const int nb = (int)min<int64_t>(TBT, a.B - b0);

    if ((a.phases & 1) && tile != blockIdx.x) stage_rows<NT>(smem + L.tok, tsrc, B, esz, b0, per, TBT);
    if (tile == blockIdx.x) STAMP(1, 1);
    __syncthreads();   // tokens (DMA), bounds, DoF map, LDS basis and LUT are in place
    if (tile == blockIdx.x) STAMP(1, 2);
    if constexpr (RT > 0) {
      if (tile == blockIdx.x) {
#pragma unroll
        for (int kd = 0; kd < 2; ++kd)
#pragma unroll
          for (int rt = 0; rt < RT; ++rt)
#pragma unroll
            for (int ks = 0; ks < KS; ++ks) {
              const int t = rt * 16 + lr, n = lk * KS + ks;
              const float x = phi[(min(kd, nkinds - 1) * Tout + min(t, Tout - 1)) * N + min(n, N - 1)];
              phr[kd][rt][ks] = (t < Tout && n < N && kd < nkinds) ? x : 0.0f;
            }
      }
    }
    if (a.params_out != nullptr) rec_params_out<NT>(a, tokl, b0, nb, wlo, whi, lut, vm1);

    // ---- pos[j][t][dst(d)] = sum_n Phi_kind[t][n] W[j][d][n]  (f32 MFMA 16x16x4; A = Phi, B = W).
    //      A wave owns a column tile (j, d) and dequantises its own B operand (K-step ks
    //      holds n = 4*ks + lane/16) straight from the token tile; the basis operands
    //      are reused across the wave's column tiles; rows past Tout land in ob's padding.
    for (int q = wave; (a.phases & 2) && q < nq; q += NW) {
      int j, d, kind;
      bool ok;
      tile_col<TBT>(g, m, q, lr, j, d, kind, ok);
      ok = ok && j < nb;
      float w[KS];   // B operand, K-step ks: W[j][d][n], n = lane/16 * KS + ks
      rec_weights<KS>(a, tokl, j, d, lk, N, D, per, wlo, whi, lut, vm1, w);
#pragma unroll
      for (int ks = 0; ks < KS; ++ks) w[ks] = (ok && lk * KS + ks < N) ? w[ks] : 0.0f;
      if (a.init_p != nullptr && lk == 0 && ok && d < nj)   // coefficient n = 0 of the joint DoFs <- init_p
        w[0] = a.init_p[(b0 + j) * a.init_p_sb + a.init_p_src[d]];   // (reference :505-510)
      float* oc = ob + (j * RTR + lk * 4) * ndo + min(max(dst[d], 0), ndo - 1);
      if constexpr (RT > 0) {
        float4_t acc[RT];
#pragma unroll
        for (int i = 0; i < RT; ++i) acc[i] = float4_t{0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
        for (int ks = 0; ks < KS; ++ks)
#pragma unroll
          for (int i = 0; i < RT; ++i)
            acc[i] = __builtin_amdgcn_mfma_f32_16x16x4f32(kind ? phr[1][i][ks] : phr[0][i][ks], w[ks], acc[i], 0,
                                                          0, 0);
        // f32 C/D map: col = lane & 15, row = (lane >> 4) * 4 + r
        if (ok) {
#pragma unroll
          for (int i = 0; i < RT; ++i)
#pragma unroll
            for (int r = 0; r < 4; ++r) oc[(i * 16 + r) * ndo] = acc[i][r];
        }
      } else {
        const float* Ph = phi + (kind * RTR + lr) * Np4 + lk * KS;
        for (int rt = 0; rt < RTR / 16; rt += 4) {   // four row tiles: four independent chains
          float av[4][KS];
#pragma unroll
          for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int ks = 0; ks < KS; ++ks) av[i][ks] = Ph[((rt + i) * 16) * Np4 + ks];
          float4_t acc[4];
#pragma unroll
          for (int i = 0; i < 4; ++i) acc[i] = float4_t{0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
          for (int ks = 0; ks < KS; ++ks)
#pragma unroll
            for (int i = 0; i < 4; ++i)
              acc[i] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[i][ks], w[ks], acc[i], 0, 0, 0);
          if (ok) {
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
              for (int r = 0; r < 4; ++r) oc[((rt + i) * 16 + r) * ndo] = acc[i][r];
          }
        }
      }
    }
    if (tile == blockIdx.x) STAMP(1, 5);
    __syncthreads();
    if (tile == blockIdx.x) STAMP(1, 6);
    if (a.phases & 4) rec_store<S>(a, a.pos_out + b0 * (int64_t)Tout * ndo, ob, nb, RTR);
    if (tile == blockIdx.x) STAMP(1, 7);
  }
#ifdef BEAST_STAMPS
  __builtin_amdgcn_s_waitcnt(0);
  STAMP(1, 8);
  BSTAMP(1, 1);
#endif
}

// ------------------------------------------------ reconstruct, per-trajectory waves --
// Latency regime, fixed shapes with num_dof_out == D.  The dispatch (rec_v, launch_rec_v in codec.hip)
// takes this kernel while the batch would give k_reconstruct at most two of its 8-trajectory tiles per
// CU; its own tiles are 16 trajectories, one wave each, so that is at most one 16-wave tile per CU
// (B <= 16 CUs, e.g. the bench's B = 4,096), the range in which it stores write-through.
// k_reconstruct computes pos^T (rows t, columns (trajectory, DoF)), so a
// lane's accumulators are 4 rows of one output column, 4 * ndo bytes apart: they go through an
// LDS image, a workgroup barrier and a cooperative store, and HBM sits idle while the whole chip
// computes.  Here the MFMA computes pos[j] itself: wave j owns trajectory j of the tile, A = W
// (16 rows = output columns c, K = basis n), B = Phi^T (columns t), so a lane's accumulator
// holds columns c = 4 kk .. 4 kk + 3 of one row t -- contiguous bytes of pos[j][t][.] -- and each
// wave stores its trajectory straight from registers as soon as its own chain is done (no LDS
// image, no barrier): the stores of the first waves overlap the MFMAs of the others.
// Same K mapping (n = kk * KS + s) and the same products summed in the same order as
// k_reconstruct (a product's operands only swap roles), so positions are bit-identical.  With
// gripper DoFs the rows of the other kind are zero in each kind's chain: the joint chain then
// the gripper chain, each adding exact zeros to the other kind's rows.

// Round 7: the chain after the tile barrier is shorter.  Whatever depends on the lane alone is
// computed before the barrier, while the DMA is in flight: the inverse DoF map (scalar loads of
// a.dof_dst), and the LDS addresses of the lane's tokens, bounds, W-image slots and Phi^T operands.
// Operands that must be zero (rows past T, K-steps past N, rows no DoF maps to) are read from a
// zeroed LDS region instead of being selected, and slots past the trajectory's tokens write to a
// spare W-image slot instead of being predicated.  Bounds and basis still arrive by DMA:
// per-lane global loads of them cost more vector-memory issue time than the chain saves
// (profiles/r07/codec_chain_ab.txt).
//
// Round 11: the lane-only values are no longer computed sixteen times per workgroup.  What hangs on
// a.dof_dst -- the inverse DoF map and with it the W-image address of each A operand and the
// kind mask -- is computed by one wave (RV_BUILDER) for its 64 lanes, without the wave's own
// offset, into a 1 KB LDS table of 16-byte entries; after the barrier every wave reads its lanes'
// entries in the round trip that fetches its tokens and bounds, and adds its W-image offset.  The
// dequantise slots map lanes to (n d) without a division (d = lane & 15, n = lane / 16 + 4 u: 192
// slots for the 140 values), so their offsets, the Phi^T operands' and the output image's stay
// inline: a handful of VALU each, cheaper than a table read.  The quotient t / (vocab - 1) is
// beast::exact_quotient (three VALU per slot): no LUT, no fill, no second LDS round trip; tokens
// outside [0, EXACT_QUOTIENT_MAX) and larger vocabularies take the IEEE division behind one branch.
// Nothing derived from the bounds or the DoF map outlives the launch.
#ifndef BEAST_RV_BUILDER
#define BEAST_RV_BUILDER 3
#endif
constexpr int RV_BUILDER = BEAST_RV_BUILDER < RV_WR ? BEAST_RV_BUILDER : RV_WR - 1;   // the wave that fills the lane table
struct RvSmem {
  int tok, wlo, whi, phi, zero, tab, wimg, img, total;
};
template <class S>
__host__ __device__ constexpr int rv_zero_bytes(int nkinds) {   // every Phi^T operand offset, from a zero base
  return round_up(((nkinds - 1) * S::T + round_up(S::T, 16)) * S::N * 4, 16);
}
template <class S>
__host__ __device__ constexpr RvSmem rv_smem(int nkinds) {
  RvSmem s{};
  constexpr int per = S::D * S::N;
  int o = 0;
  s.tok = o;  o += round_up(RV_WR * per * 8, 1024);           // DMA: whole wave-instructions
  s.wlo = o;  o += round_up(per * 4, 256);
  s.whi = o;  o += round_up(per * 4, 256);
  s.phi = o;  o += round_up(nkinds * S::T * S::N * 4, 1024);
  s.zero = o; o += rv_zero_bytes<S>(nkinds);
  s.tab = o;  o += 64 * 16;                                      // lane table: {wa[0..2], am[0]} per lane
  s.wimg = o; o += round_up(RV_WR * (per + 4) * 4, 16);        // W[j][d][n] (d n) + a spare and a zero slot, one per wave
  s.img = o;  o += RV_WR * round_up(S::T * S::D * 4, 16);        // pos[j] [T][D], one per wave
  // A 16-wave tile keeps a CU to itself, as it did while the LUT made it larger than half the CU's
  // 160 KB: without the LUT the layout is 78 KB and two tiles could share a CU while others idle.
  // The request is padded past 80 KB so that placement stays what every measurement of this kernel
  // was made with; nothing uses the pad.  Unpadded, 3 of 26 runs of the B = 4,096 step came out at
  // 9.0 - 13.5 us against 8.6; padded 0 of 20, the parent 0 of 26: too few to name the cause
  // (profiles/r11/reconstruct_lane_table_ab.txt).
  s.total = (RV_WR == 16 && o <= 84 * 1024) ? 84 * 1024 : o;
  return s;
}

typedef __attribute__((address_space(4))) const int32_t const_i32;   // constant memory: uniform reads are scalar loads

template <int KS, class S, int SP>
__global__ __launch_bounds__(RV_WR * 64) void k_reconstruct_v(const void* __restrict__ tsrc, int64_t B, int esz,
                                                             RecVArgs a) {
  static_assert(S::fixed && S::T > 0 && S::T <= 64 && S::D <= 16 && S::DL == S::D && 4 * KS >= S::N,
                "per-trajectory reconstruct: fixed shape, T <= 64, D <= 16, ndo == D");
  constexpr int NT = RV_WR * 64, D = S::D, N = S::N, T = S::T, per = D * N;
  constexpr int NJ = S::NJ;
  constexpr int nkinds = NJ < D ? 2 : 1;
  constexpr RvSmem L = rv_smem<S>(nkinds);
  constexpr int RV_IMG = round_up(T * D * 4, 16) / 4;   // floats per wave's output image
  constexpr int WIMG = per + 4;                         // floats per wave's W image; [per] spare, [per + 1] zero
  constexpr int DP = D <= 4 ? 4 : D <= 8 ? 8 : 16;      // lanes per coefficient row of the dequantise slots
  constexpr int RPS = 64 / DP;                          // coefficient rows per slot
  constexpr int NU = (N + RPS - 1) / RPS;               // dequantise slots per lane
  constexpr int NTT = (T + 15) / 16;                    // 16-row tiles of the output
  static_assert((T * D) % 4 == 0, "per-trajectory reconstruct: whole 16-byte rows");
  static_assert(KS <= 3, "per-trajectory reconstruct: a lane-table entry holds three A-operand offsets and a mask");
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  float* wlo = reinterpret_cast<float*>(smem + L.wlo);
  float* whi = reinterpret_cast<float*>(smem + L.whi);
  float* phi = reinterpret_cast<float*>(smem + L.phi);
  const int tid = threadIdx.x, wave = __builtin_amdgcn_readfirstlane(tid >> 6), lane = tid & 63;
  const int64_t b0 = (int64_t)blockIdx.x * RV_WR;
  STAMP(1, 0);
  BSTAMP(1, 0);
  // ---- prologue: the token tile, bounds and raw basis by DMA, all in flight together
  stage_rows<NT>(smem + L.tok, tsrc, B, esz, b0, per, RV_WR);
  STAMP(1, 9);
  dma4<NT>(wlo, a.w_min, per);
  dma4<NT>(whi, a.w_max, per);
  {
    constexpr int pbytes = nkinds * T * N * 4;
    if ((pbytes & 15) == 0 && (((uintptr_t)a.basis) & 15) == 0) dma16<NT>(phi, a.basis, pbytes >> 4);
    else dma4<NT>(phi, a.basis, pbytes >> 2);
  }
  STAMP(1, 13);
  const float vm1 = (float)(a.vocab - 1);
  const int qn = a.vocab <= beast::EXACT_QUOTIENT_MAX ? beast::EXACT_QUOTIENT_MAX : 0;
  for (int i = tid; i < rv_zero_bytes<S>(nkinds) / 4; i += NT) reinterpret_cast<float*>(smem + L.zero)[i] = 0.0f;
  STAMP(1, 12);
  const int j = wave;
  const int nb = (int)min<int64_t>(RV_WR, B - b0);
  const int c = lane & 15, kk = lane >> 4;
  // ---- lane-only values that are cheaper inline than read from a table, while the DMA is in flight
  // the wave's zero slot: A operands that must be zero are read from it
  *reinterpret_cast<float*>(smem + L.wimg + (j * WIMG + per + 1) * 4) = 0.0f;
  // dequantise slot u: DoF d = lane % DP, coefficient n = lane / DP + RPS u -> token (n d), W column
  // k = d N + n; slots outside the trajectory read its token 0 and write the spare W-image slot
  int te[NU], kb[NU], wk[NU];   // byte offsets: the token, its column in a bounds array, its W-image slot
  {
    const int sd = lane & (DP - 1), sn = lane / DP;
#pragma unroll
    for (int u = 0; u < NU; ++u) {
      const int n = sn + RPS * u;
      const bool ok = sd < D && n < N;
      te[u] = L.tok + (j * per + (ok ? n * D + sd : 0)) * 8;
      kb[u] = ok ? (sd * N + n) * 4 : 0;
      wk[u] = L.wimg + (j * WIMG + (ok ? sd * N + n : per)) * 4;
      pin(te[u]); pin(kb[u]); pin(wk[u]);
    }
  }
  // B = Phi_kind^T: column t = 16 tt + c, K-step s: n = kk * KS + s.  pa: the whole row tiles
  // (t < T for every c), pt: the last, partial one; kind and tile are constant offsets
  int pa[KS], pt[KS];
#pragma unroll
  for (int s2 = 0; s2 < KS; ++s2) {
    const int n = kk * KS + s2, tl = (NTT - 1) * 16 + c;
    pa[s2] = n < N ? L.phi + (c * N + n) * 4 : L.zero;
    pt[s2] = (n < N && tl < T) ? L.phi + (c * N + n) * 4 : L.zero;
    pin(pa[s2]); pin(pt[s2]);
  }
  // this lane's part of pos[j]: row t = 16 tt + c, columns 4 kk .. 4 kk + 3
  int ia = L.img + (j * RV_IMG + c * D + 4 * kk) * 4;
  pin(ia);
  STAMP(1, 14);
  // ---- the lane table, by one wave: A = W, row c = lane & 15 is output column c, i.e. DoF d with
  //      dof_dst[d] == c; K-step s holds n = kk * KS + s (k_reconstruct's mapping), zero past N, past D
  //      and for the other kind.  Entry: the byte offsets of W[dd][n] in a wave's W image (or of its
  //      zero slot), s < KS, and the mask that is ~0 where the row belongs to the joint kind's chain.
  if (wave == RV_BUILDER) {
    int dsrc = -1;
    const_i32* dof_dst = (const_i32*)a.dof_dst;
#pragma unroll
    for (int d = 0; d < D; ++d) dsrc = dof_dst[d] == c ? d : dsrc;
    const bool row_ok = dsrc >= 0;
    const int dd = row_ok ? dsrc : 0;
    int ent[4] = {0, 0, 0, 0};
#pragma unroll
    for (int s2 = 0; s2 < KS; ++s2) {
      const int n = kk * KS + s2;
      ent[s2] = L.wimg + ((row_ok && n < N) ? dd * N + n : per + 1) * 4;
    }
    ent[3] = (nkinds == 1 || dd < NJ) ? -1 : 0;
    *reinterpret_cast<int4*>(smem + L.tab + lane * 16) = make_int4(ent[0], ent[1], ent[2], ent[3]);
  }
  STAMP(1, 15);
  STAMP(1, 1);
  __syncthreads();   // every DMA, the lane table and the zeros are in place
  STAMP(1, 2);
  if (j >= nb) return;   // no barrier follows
  // ---- W[j][d][n] of this wave's trajectory (bit-exact discrete_to_continuous, init_p for n = 0 of
  //      the joint DoFs: reference :505-510) into its LDS image: the slots' tokens and bounds and
  //      the lane's table entry in one LDS round trip
  long long tv[NU];
  float lo[NU], hi[NU];
#pragma unroll
  for (int u = 0; u < NU; ++u) {
    tv[u] = *reinterpret_cast<const long long*>(smem + te[u]) - a.tok_offset;
    lo[u] = *reinterpret_cast<const float*>(smem + L.wlo + kb[u]);
    hi[u] = *reinterpret_cast<const float*>(smem + L.whi + kb[u]);
  }
  const int4 ent = *reinterpret_cast<const int4*>(smem + L.tab + lane * 16);
  float nrm[NU];
  fma_quotients(tv, qn, vm1, a.rinv, nrm);
#pragma unroll
  for (int u = 0; u < NU; ++u) {
    float w = beast::dequantize_quotient(nrm[u], lo[u], hi[u]);
    if (u == 0 && a.init_p != nullptr && lane < NJ)   // slot 0 of lanes d < NJ is n = 0 of the joint DoFs
      w = a.init_p[(b0 + j) * a.init_p_sb + a.init_p_src[lane]];
    *reinterpret_cast<float*>(smem + wk[u]) = w;
  }
  int wa[KS];            // byte offset of W[dd][n], or of the wave's zero slot
  unsigned am[nkinds];   // ~0 where the row belongs to the kind's chain
  {
    const int et[3] = {ent.x, ent.y, ent.z};
#pragma unroll
    for (int s2 = 0; s2 < KS; ++s2) wa[s2] = et[s2] + j * WIMG * 4;
#pragma unroll
    for (int kd = 0; kd < nkinds; ++kd) am[kd] = kd == 0 ? (unsigned)ent.w : ~(unsigned)ent.w;
  }
  wave_sync();
  STAMP(1, 3);
  float4_t acc[NTT];
#pragma unroll
  for (int tt = 0; tt < NTT; ++tt) acc[tt] = float4_t{0.0f, 0.0f, 0.0f, 0.0f};
  float wv[KS];
#pragma unroll
  for (int s2 = 0; s2 < KS; ++s2) wv[s2] = *reinterpret_cast<const float*>(smem + wa[s2]);
#pragma unroll
  for (int kd = 0; kd < nkinds; ++kd) {
    float bv[NTT][KS];
#pragma unroll
    for (int tt = 0; tt < NTT; ++tt)
#pragma unroll
      for (int s2 = 0; s2 < KS; ++s2)
        bv[tt][s2] = *reinterpret_cast<const float*>(smem + (tt * 16 + 15 < T ? pa[s2] : pt[s2]) +
                                                     (kd * T + tt * 16) * N * 4);
#pragma unroll
    for (int s2 = 0; s2 < KS; ++s2) {
      const float ak = nkinds == 1 ? wv[s2] : __uint_as_float(__float_as_uint(wv[s2]) & am[kd]);
#pragma unroll
      for (int tt = 0; tt < NTT; ++tt)
        acc[tt] = __builtin_amdgcn_mfma_f32_16x16x4f32(ak, bv[tt][s2], acc[tt], 0, 0, 0);
    }
  }
  STAMP(1, 5);
  // ---- f32 C/D map: row (column c of pos) = kk * 4 + r, column (t) = lane & 15: this lane holds
  //      pos[j][16 tt + (lane & 15)][4 kk .. 4 kk + 3].  Those are 8-byte aligned (t * D * 4 is a
  //      multiple of 16 only for even t), and 8-byte write-through stores are one fabric write each,
  //      so the wave puts its trajectory's [T][D] image into LDS (its own region: no workgroup
  //      barrier) and copies it out as 16-byte write-through stores.
  float* img = reinterpret_cast<float*>(smem + L.img) + j * RV_IMG;
#pragma unroll
  for (int tt = 0; tt < NTT; ++tt) {
    const int t = tt * 16 + c;
    if (t < T) {
      float* q = reinterpret_cast<float*>(smem + ia + tt * 16 * D * 4);
      if (4 * kk + 1 < D) *reinterpret_cast<float2*>(q) = make_float2(acc[tt][0], acc[tt][1]);
      else if (4 * kk < D) q[0] = acc[tt][0];
      if (4 * kk + 3 < D) *reinterpret_cast<float2*>(q + 2) = make_float2(acc[tt][2], acc[tt][3]);
      else if (4 * kk + 2 < D) q[2] = acc[tt][2];
    }
  }
  wave_sync();
  STAMP(1, 6);
  if (a.phases & 4)
    wave_copy_out<SP, T * D / 4>(reinterpret_cast<float4*>(a.pos_out + (b0 + j) * (int64_t)T * D),
                                 reinterpret_cast<const float4*>(img), lane);
  STAMP(1, 7);
#ifdef BEAST_STAMPS
  __builtin_amdgcn_s_waitcnt(0);
  STAMP(1, 8);
  BSTAMP(1, 1);
#endif
}

// Per-trajectory basis rows (custom times per row, KS == 0): decode W into LDS, then a
// sequential fma over n per output (the MFMA chain's order) on the VALU; also the
// decode-only path when no positions are requested.
template <int TBT>
__global__ __launch_bounds__(NTHREADS) void k_reconstruct_rows(RecArgs a) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const Geom& g = a.g;
  const int D = g.D, N = g.N, nj = g.nj, per = g.per;
  const int Tout = a.Tout, ndo = a.ndo;
  const bool pos = a.pos_out != nullptr;
  const RecSmem L = rec_smem<TBT, 0, 0>(Tout, D, N, ndo, (nj < D) ? 2 : 1, a.lut_n);
  const int Np4 = L.Np4;
  const unsigned char* tokl = smem + L.tok;
  float* pb = reinterpret_cast<float*>(smem + L.pb);
  float* wlo = reinterpret_cast<float*>(smem + L.wlo);
  float* whi = reinterpret_cast<float*>(smem + L.whi);
  float* lut = reinterpret_cast<float*>(smem + L.lut);
  uint16_t* pmap = reinterpret_cast<uint16_t*>(smem + L.pmap);
  int* dst = reinterpret_cast<int*>(smem + L.dst);
  int* col2d = reinterpret_cast<int*>(smem + L.col2d);
  float* ob = reinterpret_cast<float*>(smem + L.out);
  const int tid = threadIdx.x;
  const float vm1 = (float)(a.vocab - 1);

  const void* tsrc = a.ntokens ? static_cast<const void*>(a.ntokens) : static_cast<const void*>(a.tokens);
  const int esz = a.ntokens ? 4 : 8;
  if (blockIdx.x < a.ntiles) stage_rows(smem + L.tok, tsrc, a.B, esz, (int64_t)blockIdx.x * TBT, per, TBT);
  dma4(wlo, a.w_min, per);
  dma4(whi, a.w_max, per);
  if (pos) dma4(dst, a.dof_dst, D);
  lut_fill(lut, a.lut_n, vm1, NTHREADS);
  for (int r = tid; r < per; r += NTHREADS) {
    const int n = r / D, d = r - n * D;
    pmap[r] = (uint16_t)(d * Np4 + n);
  }
  if (pos) {   // output column -> DoF (after the DMA of dst)
    __syncthreads();
    for (int c = tid; c < ndo; c += NTHREADS) col2d[c] = -1;
    __syncthreads();
    if (tid < D) {
      const int dd = dst[tid];
      if (dd >= 0 && dd < ndo) col2d[dd] = tid;
    }
  }

  for (int64_t tile = blockIdx.x; tile < a.ntiles; tile += gridDim.x) {
    const int64_t b0 = tile * TBT;
    const int nb = (int)min<int64_t>(TBT, a.B - b0);
    if (tile != blockIdx.x) stage_rows(smem + L.tok, tsrc, a.B, esz, b0, per, TBT);
    __syncthreads();
    if (a.params_out != nullptr) rec_params_out(a, tokl, b0, nb, wlo, whi, lut, vm1);
    if (!pos) continue;
    for (int e = tid; e < nb * per; e += NTHREADS) {   // (n d) tokens -> W[j][d][n]
      const uint32_t j = fdiv(e, g.fd_per);
      const int r = e - j * per;
      const uint32_t n = fdiv(r, g.fd_D);
      const int d = r - n * D;
      pb[j * D * Np4 + pmap[r]] = rec_weight(a, tokl, e, d * N + n, wlo, whi, lut, vm1);
    }
    __syncthreads();
    if (a.init_p != nullptr) {   // coefficient 0 of the joint DoFs <- init_p (reference :505-510)
      for (int e = tid; e < nb * nj; e += NTHREADS) {
        const int j = e / nj, d = e - j * nj;
        pb[(j * D + d) * Np4] = a.init_p[(b0 + j) * a.init_p_sb + a.init_p_src[d]];
      }
      __syncthreads();
    }
    float* gout = a.pos_out + b0 * (int64_t)Tout * ndo;
    for (int e = tid; e < nb * Tout * ndo; e += NTHREADS) {
      const int j = e / (Tout * ndo), r = e - j * Tout * ndo, t = r / ndo, c = r - t * ndo;
      const int d = col2d[c];
      float acc = 0.0f;
      if (d >= 0) {
        const int kind = (d < nj) ? 0 : 1;
        const float* Phr = a.basis + (b0 + j) * a.basis_sb + (int64_t)kind * Tout * N + (int64_t)t * N;
        const float* Wr = pb + (j * D + d) * Np4;
        for (int n = 0; n < N; ++n) acc = fmaf(Phr[n], Wr[n], acc);
      }
      if (L.stage) ob[e] = acc; else gout[e] = acc;
    }
    __syncthreads();
    if (L.stage) store_out(gout, ob, nb * Tout * ndo);   // (per-row path: DynShape)
  }
}

}  // namespace
