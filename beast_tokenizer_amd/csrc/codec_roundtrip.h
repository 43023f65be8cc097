// Round trip (codec.hip's fourth layer): k_roundtrip, encode -> quantise -> dequantise ->
// reconstruct -> error statistics of a trajectory in one launch, its argument block and LDS layout.
// Fit and reconstruct chains are its own (runtime dimensions).
#pragma once

#include "codec_reconstruct.h"

namespace {

// ------------------------------------------------ round trip: encode -> reconstruct statistics --
// One wave per trajectory; a workgroup walks tiles of W trajectories (grid-stride, constants staged
// once, the grid capped as k_encode's).  The wave fits its trajectory
// as k_encode_v does (A = P_kind, B = y, the same K-steps into the same even / odd accumulators),
// quantises its accumulators with k_encode's quantiser, dequantises the bins (bit-exact
// discrete_to_continuous, the IEEE quotients from k_reconstruct's LUT) and writes both the
// dequantised and the raw params into wave-private W images, zero-padded to [16 ct][4 KS].  Two
// reconstruct chains (A = Phi_kind, rows = time steps; B = W, columns = DoFs; K mapping
// n = lane/16 * KS + s, one accumulator over s, the joint kind before the gripper kind:
// k_reconstruct's products in its order) give the positions of the tokens and of the unquantised
// fit; where beast_reconstruct_f32 would leave the MFMA for k_reconstruct_rows (rec_mfma_fits)
// both are that kernel's sequential FMAs over n instead.  A lane then holds, for one DoF, the
// errors at the time steps t = 16 tt + 4 (lane / 16) + r: it accumulates its own in order and the
// 4 lanes of a DoF combine in a fixed order, so the statistics are run-to-run identical without
// float atomics.  Clip counts go through LDS counters and leave right after the fit of the
// workgroup's last tile, one integer atomic per non-zero column and workgroup, so that they retire
// under the quantiser and the reconstruct stage: every workgroup of a launch adds to the same 18
// cache lines at about the same time (B = 4,096, default shape: flushed at the kernel's end 14.1 us,
// after the quantiser 10.4 us, after the fit 9.7 us; without counters 8.1 us), and one flush per
// tile cost 150 us at B = 262,144.  The time follows the VALU instruction count (the 16 waves of a
// tile share 4 SIMDs: about 150 instructions per us), so: operands that must be zero come from the
// zero-padded images, not from selects; the maximum of |e| is an unsigned integer maximum of the bit
// patterns (which orders non-negative floats and puts NaN above inf: torch.amax's propagation for
// free); e^2 and f^2 are accumulated by FMA; the quantiser runs three slots per lane at N <= 10.
// S fixed: the BEAST default shapes, contiguous rows, everything staged by LDS-DMA; otherwise
// runtime dims, the wave gathers its trajectory into a [T][D] image as k_encode does and the
// constants are copied through registers.
struct RtArgs {
  int64_t sb, st, sd, tok_offset;
  const int32_t* dof_src;
  const float* proj;
  const float* basis;
  const float* w_min;
  const float* w_max;
  long long* tokens_out;
  float* stats_out;
  unsigned* clip;
  int row_elems, vocab, D, nj, N, T, seq, lut_n;
};

constexpr int RT_W = 16, RT_W_BULK = 8;   // waves (trajectories) per tile of the fixed shapes

struct RtSmem {
  int P, phi, wlo, whi, lcol, clip, lut, Y, wq, wr, wimg, total;
};
// DMA destinations are padded to whole wave-instructions
__host__ __device__ constexpr RtSmem rt_smem(int T, int D, int N, int nkinds, int W, int lut_n) {
  RtSmem s{};
  const int Tp = round_up(T, 4), DN = D * N;
  int o = 0;
  s.P = o;    o += round_up(nkinds * 16 * Tp * 4, 1024);
  s.phi = o;  o += round_up(nkinds * T * N * 4, 1024);
  s.wlo = o;  o += round_up(DN * 4, 256);
  s.whi = o;  o += round_up(DN * 4, 256);
  s.lcol = o; o += round_up(D * 4, 256);
  s.clip = o; o += round_up(2 * DN * 4, 16);
  s.lut = o;  o += round_up(lut_n * 4, 16);
  s.Y = o;    o += round_up(W * T * D * 4, 1024);
  s.wimg = round_up(D, 16) * round_up(N, 4) * 4;   // W[d][n], rows of 4 KS floats, 16 rows per column tile
  s.wq = o;   o += W * s.wimg;
  s.wr = o;   o += W * s.wimg;
  s.total = o;
  return s;
}

// k_roundtrip keeps its own lines for the slot mapping, the quantise loop and the LUT dequantise
// (elsewhere slot_row / slot_values / lut_quotients and beast::quantize_bins): through the shared
// helpers its fixed shapes measured 0.6-1.1 % slower than before, outside the run-to-run spread
// (profiles/r08/codec_refactor_ab.txt).  tests/test_gpu_roundtrip.py holds the two bitwise equal.
// The params of an MFMA lane (C/D map: rows n = 4 lk + r) as quantiser slots: four, or three (Q3).
template <bool Q3>
__device__ __forceinline__ int rt_slot_row(int lk, int u) {
  return (Q3 && u == 2 && lk >= 2) ? 4 * (lk - 2) + 3 : 4 * lk + u;
}
template <bool Q3, int NQ>
__device__ __forceinline__ void rt_slots(const float4_t& acc0, const float4_t& acc1, int lk, float (&p)[NQ], int (&nn)[NQ]) {
  float p4[4];
#pragma unroll
  for (int r = 0; r < 4; ++r) p4[r] = __fadd_rn(acc0[r], acc1[r]);
  if constexpr (Q3) {   // slot 2: lanes lk < 2 keep their row 4 lk + 2, lanes lk >= 2 take row 4 (lk - 2) + 3 of lane - 32
    const auto sw = __builtin_amdgcn_permlane32_swap(__float_as_uint(p4[2]), __float_as_uint(p4[3]), false, false);
    p[0] = p4[0]; p[1] = p4[1]; p[2] = __uint_as_float(sw[0]);
  } else {
#pragma unroll
    for (int r = 0; r < 4; ++r) p[r] = p4[r];
  }
#pragma unroll
  for (int u = 0; u < NQ; ++u) nn[u] = rt_slot_row<Q3>(lk, u);
}

// (the runtime-shape instantiation cannot unroll the loops the fixed shapes unroll)
#pragma clang diagnostic push
#pragma clang diagnostic ignored "-Wpass-failed"
template <class S, int WF>
__global__ __launch_bounds__(S::fixed ? WF * 64 : 1024) void k_roundtrip(const float* __restrict__ traj, int64_t B,
                                                                        RtArgs a) {
  constexpr bool DMA = S::fixed;
  // N <= 10 (fixed shapes): three quantiser slots per lane, not four, as in k_encode_v -- rows 4 lk + 3
  // of lanes lk < 2 move to slot 2 of lanes lk >= 2, whose own rows there are padding
  constexpr bool Q3 = S::fixed && S::N > 0 && S::N <= 10;
  constexpr int NQ = Q3 ? 3 : 4;
  const int D = S::D ? S::D : a.D, nj = S::fixed ? S::NJ : a.nj, N = S::N ? S::N : a.N, T = S::T ? S::T : a.T;
  const int Tp = round_up(T, 4), DN = D * N;
  const int W = S::fixed ? WF : (int)(blockDim.x >> 6), NT = W * 64;
  const int nkinds = nj < D ? 2 : 1;
  const int NCT = (D + 15) >> 4, NST = Tp >> 2, NTT = (T + 15) >> 4, KS = (N + 3) >> 2, NP = 4 * KS;
  const int lut_n = a.lut_n;
  const RtSmem L = rt_smem(T, D, N, nkinds, W, lut_n);
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  float* P = reinterpret_cast<float*>(smem + L.P);
  float* phi = reinterpret_cast<float*>(smem + L.phi);
  float* wlo = reinterpret_cast<float*>(smem + L.wlo);
  float* whi = reinterpret_cast<float*>(smem + L.whi);
  int* lcol = reinterpret_cast<int*>(smem + L.lcol);
  unsigned* clipl = reinterpret_cast<unsigned*>(smem + L.clip);
  float* lut = reinterpret_cast<float*>(smem + L.lut);
  const int tid = threadIdx.x, wave = __builtin_amdgcn_readfirstlane(tid >> 6), lane = tid & 63;
  const int lr = lane & 15, lk = lane >> 4;
  const int j = wave;
  float* Yj = reinterpret_cast<float*>(smem + L.Y) + j * T * D;
  float* Wq = reinterpret_cast<float*>(smem + L.wq + j * L.wimg);
  float* Wr = reinterpret_cast<float*>(smem + L.wr + j * L.wimg);
  const float vm1 = (float)(a.vocab - 1);
  const int64_t ntiles = (B + W - 1) / W;
  const int tile16 = T * D / 4;   // DMA: float4 per trajectory

  // ---- prologue: the first tile and every constant into LDS (DMA: all in flight together)
  if constexpr (DMA) {
    constexpr int NTC = WF * 64;
    const int64_t f0 = (int64_t)blockIdx.x * W;   // the grid never exceeds the tile count
    dma16<NTC>(smem + L.Y, reinterpret_cast<const float4*>(traj) + f0 * tile16, (int)min<int64_t>(W, B - f0) * tile16);
    dma16<NTC>(P, a.proj, nkinds * 4 * Tp);
    dma4<NTC>(wlo, a.w_min, DN);
    dma4<NTC>(whi, a.w_max, DN);
    dma4<NTC>(lcol, a.dof_src, D);
    const int pbytes = nkinds * T * N * 4;
    if ((pbytes & 15) == 0 && (((uintptr_t)a.basis) & 15) == 0) dma16<NTC>(phi, a.basis, pbytes >> 4);
    else dma4<NTC>(phi, a.basis, pbytes >> 2);
  } else {
    for (int i = tid; i < nkinds * 16 * Tp; i += NT) P[i] = a.proj[i];
    for (int i = tid; i < nkinds * T * N; i += NT) phi[i] = a.basis[i];
    for (int i = tid; i < DN; i += NT) { wlo[i] = a.w_min[i]; whi[i] = a.w_max[i]; }
  }
  lut_fill(lut, lut_n, vm1, NT);
  for (int i = lane; i < L.wimg / 4; i += 64) Wq[i] = Wr[i] = 0.0f;          // the padding stays zero for every tile
  if (a.clip != nullptr)
    for (int i = tid; i < 2 * DN; i += NT) clipl[i] = 0u;

  // a workgroup walks its tiles (grid-stride): the constants are staged and the clip counts flushed once
  for (int64_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
    const int64_t b0 = tile * W;
    const int nb = (int)min<int64_t>(W, B - b0);
    if constexpr (DMA) {
      if (tile != blockIdx.x) {
        __syncthreads();   // every wave is done with the previous tile's trajectories
        dma16<WF * 64>(smem + L.Y, reinterpret_cast<const float4*>(traj) + b0 * tile16, nb * tile16);
      }
    } else if (j < nb) {   // the wave's own trajectory, gathered into [T][D]; columns outside the row read as zero
      const float* src = traj + (b0 + j) * a.sb;
      for (int e = lane; e < T * D; e += 64) {
        const int t = e / D, d = e - t * D;
        const int col = a.dof_src[d];
        Yj[e] = (col >= 0 && col < a.row_elems) ? src[(int64_t)t * a.st + (int64_t)col * a.sd] : 0.0f;
      }
    }
    __syncthreads();   // the tile (and, the first time, the constants) landed

    if (j < nb) {
      // ---- fit: lane (lr, lk): A = P_kind[n = lr][t = 4 st + lk], B = y[t][d = 16 ct + lr] (t clamped to
      //      T - 1: the zero-padded P columns meet those rows); a kind's chain sees zero B columns for
      //      the other kind's DoFs and is skipped where a column tile holds none of its own
      for (int ct = 0; ct < NCT; ++ct) {
        const int d = ct * 16 + lr, dc = min(d, D - 1);
        const bool dok = d < D;
        const int yc = DMA ? min(max(lcol[dc], 0), D - 1) : dc;
        float4_t acc0 = {0.0f, 0.0f, 0.0f, 0.0f}, acc1 = acc0;
        for (int kd = 0; kd < nkinds; ++kd) {
          if (nkinds == 2 && !(kd == 0 ? ct * 16 < nj : ct * 16 + 16 > nj)) continue;   // wave-uniform
          const bool mine = nkinds == 1 || (dok && ((d < nj) == (kd == 0)));
          const float* pa = P + (kd * 16 + lr) * Tp + lk;
#pragma unroll
          for (int st = 0; st < NST; st += 2) {
            const float x0 = pa[4 * st], y0 = Yj[min(4 * st + lk, T - 1) * D + yc];
            acc0 = __builtin_amdgcn_mfma_f32_16x16x4f32(x0, mine ? y0 : 0.0f, acc0, 0, 0, 0);
            if (st + 1 < NST) {
              const float x1 = pa[4 * st + 4], y1 = Yj[min(4 * st + 4 + lk, T - 1) * D + yc];
              acc1 = __builtin_amdgcn_mfma_f32_16x16x4f32(x1, mine ? y1 : 0.0f, acc1, 0, 0, 0);
            }
          }
        }
        // ---- C/D map: row n = 4 lk + r, column d: the raw params into their W image, and the clip
        //      counts at once, so that they can leave before the quantiser runs
        float p[NQ];
        int nn[NQ];
        rt_slots<Q3, NQ>(acc0, acc1, lk, p, nn);
#pragma unroll
        for (int u = 0; u < NQ; ++u) {
          if (dok && nn[u] < N) {   // the images' padding (n >= N, d >= D) stays zero
            const int k = d * N + nn[u];
            Wr[d * NP + nn[u]] = p[u];
            if (a.clip != nullptr) {
              if (p[u] < wlo[k]) atomicAdd(&clipl[k], 1u);
              if (p[u] > whi[k]) atomicAdd(&clipl[DN + k], 1u);
            }
          }
        }
      }
    }
    // ---- the workgroup's clip counts leave after its last tile's fit: the atomics retire under that
    //      tile's quantiser and reconstruct stage
    if (a.clip != nullptr && tile + gridDim.x >= ntiles) {   // workgroup-uniform
      __syncthreads();
      for (int i = tid; i < 2 * DN; i += NT) {
        const unsigned c = clipl[i];
        if (c) atomicAdd(&a.clip[i], c);
      }
    }

    if (j < nb) {
      // ---- quantise (k_encode's fast bins, the exact chain near a rounding boundary or for NaN / inf)
      //      and dequantise: each lane takes back the params it wrote
      const unsigned long long off = (unsigned long long)a.tok_offset;
      long long* tout = a.tokens_out ? a.tokens_out + (b0 + j) * DN : nullptr;
      for (int ct = 0; ct < NCT; ++ct) {
        const int d = ct * 16 + lr, dc = min(d, D - 1);
        const bool dok = d < D;
        float p[NQ], lo[NQ], hi[NQ], nrm[NQ];
        int bin[NQ], nn[NQ];
        bool ex = false, far = false;
#pragma unroll
        for (int u = 0; u < NQ; ++u) {
          nn[u] = rt_slot_row<Q3>(lk, u);
          const int nc = min(nn[u], N - 1), k = dc * N + nc;
          p[u] = Wr[dc * NP + nc];
          lo[u] = wlo[k];
          hi[u] = whi[k];
        }
#pragma unroll
        for (int u = 0; u < NQ; ++u)
          bin[u] = beast::quantize_bin_k(p[u], lo[u], hi[u], beast::quantize_scale(lo[u], hi[u], vm1), vm1, ex);
        if (ex) {
#pragma unroll
          for (int u = 0; u < NQ; ++u) bin[u] = beast::quantize_bin(p[u], lo[u], hi[u], vm1);
        }
#pragma unroll
        for (int u = 0; u < NQ; ++u) {
          const bool in = (unsigned)bin[u] < (unsigned)lut_n;
          far = far | !in;
          nrm[u] = lut[in ? bin[u] : 0];
        }
        if (far) {   // no LUT (vocab above its size, or no room), or the NaN bin: INT64_MIN as a token
#pragma unroll
          for (int u = 0; u < NQ; ++u)
            if (!((unsigned)bin[u] < (unsigned)lut_n))
              nrm[u] = __fdiv_rn(bin[u] == (int)0x80000000 ? -9223372036854775808.0f : (float)bin[u], vm1);
        }
#pragma unroll
        for (int u = 0; u < NQ; ++u) {
          if (dok && nn[u] < N) {
            Wq[d * NP + nn[u]] = beast::clamp_t(__fadd_rn(__fmul_rn(nrm[u], __fsub_rn(hi[u], lo[u])), lo[u]), lo[u], hi[u]);
            if (tout != nullptr) tout[nn[u] * D + d] = beast::widen_bin(bin[u], off);
          }
        }
      }
      wave_sync();
    }

    if (j < nb) {
      // ---- reconstruct both W images and reduce the errors.  A = Phi_kind: row = time step 16 tt + lr,
      //      read clamped (rows t >= T never reach a statistic); B = W: column = DoF 16 ct + lr (zero for
      //      n >= N, masked to the chain's kind).  C/D: this lane holds steps 16 tt + 4 lk + r of DoF
      //      16 ct + lr: it accumulates them in order, and the 4 lanes of a DoF combine in a fixed order
      const bool st16b = (((uintptr_t)a.stats_out) & 15) == 0;
      const bool seq = !S::fixed && a.seq;   // the fixed shapes' positions are k_reconstruct_v's
      float* sout = a.stats_out + (b0 + j) * (int64_t)D * 4;
      for (int ct = 0; ct < NCT; ++ct) {
        const int d = ct * 16 + lr, dc = min(d, D - 1);
        const int yc = DMA ? min(max(lcol[dc], 0), D - 1) : dc;
        float se = 0.0f, se2 = 0.0f, sf2 = 0.0f;
        unsigned mx = 0u;
#pragma unroll
        for (int tt = 0; tt < NTT; ++tt) {
          float4_t aq = {0.0f, 0.0f, 0.0f, 0.0f}, ar = aq;
          if (!seq) {
            const int ta = min(tt * 16 + lr, T - 1);
            for (int kd = 0; kd < nkinds; ++kd) {
              if (nkinds == 2 && !(kd == 0 ? ct * 16 < nj : ct * 16 + 16 > nj)) continue;   // wave-uniform
              const unsigned colk = (nkinds == 1 || ((d < nj) == (kd == 0))) ? ~0u : 0u;
#pragma unroll
              for (int s = 0; s < KS; ++s) {
                const int n = lk * KS + s;
                const float ph = phi[(kd * T + ta) * N + min(n, N - 1)];
                const float wq = __uint_as_float(__float_as_uint(Wq[d * NP + n]) & colk);
                const float wr = __uint_as_float(__float_as_uint(Wr[d * NP + n]) & colk);
                aq = __builtin_amdgcn_mfma_f32_16x16x4f32(ph, wq, aq, 0, 0, 0);
                ar = __builtin_amdgcn_mfma_f32_16x16x4f32(ph, wr, ar, 0, 0, 0);
              }
            }
          } else {
#pragma unroll
            for (int r = 0; r < 4; ++r) {
              const float* ph = phi + ((dc < nj ? 0 : 1) * T + min(tt * 16 + 4 * lk + r, T - 1)) * N;
              float q = 0.0f, f = 0.0f;
              for (int n = 0; n < N; ++n) {
                q = fmaf(ph[n], Wq[dc * NP + n], q);
                f = fmaf(ph[n], Wr[dc * NP + n], f);
              }
              aq[r] = q;
              ar[r] = f;
            }
          }
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            const int t = tt * 16 + 4 * lk + r;
            const bool tok = t < T;
            const float y = Yj[min(t, T - 1) * D + yc];
            const float e = tok ? __fsub_rn(y, aq[r]) : 0.0f, f = tok ? __fsub_rn(y, ar[r]) : 0.0f;
            se = __fadd_rn(se, e);
            se2 = fmaf(e, e, se2);
            mx = max(mx, __float_as_uint(e) & 0x7fffffffu);
            sf2 = fmaf(f, f, sf2);
          }
        }
#pragma unroll
        for (int o = 16; o <= 32; o <<= 1) {
          se = __fadd_rn(se, __shfl_xor(se, o));
          se2 = __fadd_rn(se2, __shfl_xor(se2, o));
          mx = max(mx, (unsigned)__shfl_xor((int)mx, o));
          sf2 = __fadd_rn(sf2, __shfl_xor(sf2, o));
        }
        if (lk == 0 && d < D) {
          float* q = sout + d * 4;
          if (st16b) {
            *reinterpret_cast<float4*>(q) = make_float4(se, se2, __uint_as_float(mx), sf2);
          } else {
            q[0] = se; q[1] = se2; q[2] = __uint_as_float(mx); q[3] = sf2;
          }
        }
      }
    }
  }
}
#pragma clang diagnostic pop

}  // namespace
