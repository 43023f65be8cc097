// Wide action spaces (codec.hip's sixth layer): k_encode_dof and k_reconstruct_dof, the fit and the
// reconstruction at 65 <= D <= WIDE_MAX_D DoFs, any N <= 32 and T <= 4096, reached through
// beast_encode_f32 / beast_encode_list_f32 / beast_reconstruct_f32 by the value of D alone.
//
// Work split.  One trajectory of more than 128 DoFs does not fit the 8 MFMA column tiles (4 waves x
// ST_CT) a workgroup accumulates, so the work item is (trajectory, DoF block).  dof_plan cuts the DoFs,
// in the kernels' kind-grouped order (joint DoFs, then gripper DoFs), into the fewest equal blocks of
// bd DoFs whose column tiles number at most 8: a column tile is kind-pure (its 16 columns share one A
// operand), so the block that straddles the joint / gripper boundary carries both kinds and pads each
// to whole tiles.  Items are numbered trajectory-major (item = b * nblk + block) and a persistent grid
// strides over them.  A column of the MFMA never meets another column, and the chunk lengths below
// depend on (N, kinds) alone, so an output is the same bits in whichever block, batch or grid it sits.
//
// k_encode_dof, LDS per item: two buffers of a y chunk [TC][bdn] (the block's bdn columns only, not
// whole rows) and of the projection chunk [kind][Np][TC] (fetched once per chunk, shared by all eight
// column tiles), the block's params image [bdn][N], and one int per block (below).  Both operands are
// streamed at every T: chunk c + 1 is in flight while chunk c is multiplied, one barrier per chunk.
//   Source.  Where the element stride is 1 and the block's dof_src entries are an ascending run
//   c0, c0 + 1, ... inside the row (decided on the device, once per workgroup: dof_src is device
//   memory), a whole chunk's row segments go by LDS-DMA: 16-byte units where every segment starts on
//   one and bdn % 4 == 0, else 4-byte units.  Any other layout, and the last, partial chunk of every
//   layout, is gathered through the strides, with ZEROS stored for the steps t >= T up to the multiple
//   of 4: nothing past a trajectory's last sample is read.
//   Sums.  Accumulators stay in registers for the whole trajectory (all NRT row tiles, v_mfma_f32_16x16x4_f32);
//   a chunk's K-steps alternate between two chains from the chunk's first step and the chains meet
//   once, exactly as k_encode_stream sums.
//   Epilogue.  params (d n): the image is one contiguous run of the output row.  tokens (n d): the
//   image is quantised (clamp, beast::quantize_one, offset: k_quantize's expression, so tokens_out is
//   bitwise beast_quantize_f32 mode 0 of params_out) into an int64 image [N][bdn] that reuses the chunk
//   buffers, and each of its N runs is stored in 16-byte pairs from the first even element of the
//   output on, single elements at a ragged head or tail.
//   LIST: the trajectory's rows come from the pointer table (contiguous rows, params only).
//
// k_reconstruct_dof, LDS per item: the W image [bdn][RW_WS] of the block's dequantised tokens (zero
// for n >= N), two buffers of a Phi chunk [kind][RC][N], the staged positions [RC][bdn], the block's
// clamped dof_dst entries, and (num_dof_out > D only) a byte per output column: named or not.
//   Tokens are dequantised once per item (beast::exact_quotient / dequantize_quotient through
//   fma_quotients, beast::denormalize_one for ntokens); params_out is written from the image.  A wave
//   holds the B operands of its two column tiles in registers, init_p in coefficient 0 of the joint
//   DoFs.  Sum order, for every N (N <= 16 included): one accumulator per output row tile, started at
//   0, K ascending over KS = ceil(N / 4) v_mfma_f32_16x16x4_f32, step ks covering n = 4 ks .. 4 ks + 3.
//   Output.  A chunk's positions are staged in BLOCK order [RC][bdn] and stored by one block-indexed
//   scatter, pos[b][t][dof_dst[d0 + i]] <- staged[t][i]: a block's column span is whatever its own
//   dof_dst entries name, contiguous or a permutation alike, and no block writes another's columns.
//   The columns dof_dst names nowhere are zeroed by block 0's item alone, chunk by chunk.
//   One chunk of Phi serves every item of a workgroup when T_out <= RC.  A params_out-only call reads
//   neither Phi nor dof_dst.
#pragma once

#include "codec_stream.h"

namespace {

constexpr int WIDE_MAX_D = 256;
constexpr int WD_COLS = ST_NW * ST_CT * 16;   // MFMA columns a workgroup accumulates

// ------------------------------------------------------------------ plans --
// column tiles of the DoFs [d0, d1): the joint ones, then the gripper ones
__host__ __device__ __forceinline__ int wd_coltiles(int d0, int d1, int nj) {
  const int j = nj <= d0 ? 0 : (nj >= d1 ? d1 - d0 : nj - d0);
  return (j + 15) / 16 + (d1 - d0 - j + 15) / 16;
}
struct DofPlan {
  int nblk, bd;   // blocks; DoFs per block (the last one may hold fewer)
};
inline DofPlan dof_plan(int D, int nj) {
  for (int n = (D + WD_COLS - 1) / WD_COLS;; ++n) {   // ends: 112 DoFs of two kinds fit 8 tiles
    const int bd = (D + n - 1) / n;
    bool fits = true;
    for (int d0 = 0; d0 < D; d0 += bd) fits = fits && wd_coltiles(d0, std::min(D, d0 + bd), nj) <= ST_NW * ST_CT;
    if (fits) return DofPlan{(D + bd - 1) / bd, bd};
  }
}
// Time steps per encode chunk / output rows per reconstruct chunk: both buffers of a chunk of the
// widest block (WD_COLS columns) within ST_BYTES, so a function of (N, kinds) alone.
inline int wd_enc_chunk(int N, int nkinds) {
  return std::min(ST_MAX_TC, (ST_BYTES / 8) / (WD_COLS + nkinds * (N <= 16 ? 16 : 32))) & ~3;
}
inline int wd_rec_rows(int N, int nkinds) {
  return std::min(ST_MAX_TC, ST_BYTES / (2 * nkinds * N * 4 + WD_COLS * 4)) & ~15;
}

// One work item: trajectory b, the DoFs [d0, d0 + bdn) of which the first njb are joint DoFs.
struct DofItem {
  int64_t b;
  int blk, d0, bdn, njb, nq0, nq;
};
__device__ __forceinline__ DofItem dof_item(int64_t item, int nblk, int bd, int D, int nj) {
  DofItem w;
  w.b = item / nblk;
  w.blk = (int)(item - w.b * nblk);
  w.d0 = w.blk * bd;
  w.bdn = min(bd, D - w.d0);
  w.njb = min(max(nj - w.d0, 0), w.bdn);
  w.nq0 = (w.njb + 15) >> 4;
  w.nq = w.nq0 + ((w.bdn - w.njb + 15) >> 4);
  return w;
}
// MFMA column lc of the item's column tile q: the DoF's index inside the block, its kind, and whether
// the column holds a DoF at all (else it repeats the kind's last one).
__device__ __forceinline__ void dof_col(const DofItem& w, int q, int lc, int& dd, int& kind, bool& valid) {
  kind = q < w.nq0 ? 0 : 1;
  const int c = kind ? w.njb + (q - w.nq0) * 16 + lc : q * 16 + lc;
  const int end = kind ? w.bdn : w.njb;
  valid = c < end;
  dd = valid ? c : end - 1;
}

// ----------------------------------------------------------------- encode --
struct WeSmem {
  int Y, ybuf, P, pbuf, pb, run, total;   // Y / P: buffer 0; buffer 1 lies ybuf / pbuf bytes on
};
__host__ __device__ __forceinline__ WeSmem wd_enc_smem(int tc, int bd, int N, int Np, int nkinds, int nblk) {
  WeSmem s;
  int o = 0;
  s.ybuf = round_up(tc * bd * 4, 1024);   // DMA destinations: whole wave-instructions
  s.pbuf = round_up(nkinds * Np * tc * 4, 1024);
  s.Y = o;   o += 2 * s.ybuf > N * bd * 8 ? 2 * s.ybuf : round_up(N * bd * 8, 16);   // and the token image
  s.P = o;   o += 2 * s.pbuf;
  s.pb = o;  o += round_up(bd * N * 4, 16);
  s.run = o; o += round_up(nblk * 4, 16);
  s.total = o;
  return s;
}

template <int NRT, bool LIST>
__global__ BEAST_NO_PK_F32 __launch_bounds__(ST_NT) void k_encode_dof(EncArgs a, int nblk, int bd, int TC) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  constexpr int Np = 16 * NRT;
  const int D = a.g.D, N = a.g.N, T = a.g.T, Tp = a.g.Tp, nj = a.g.nj, DN = D * N;
  const int nkinds = (nj < D) ? 2 : 1;
  const WeSmem L = wd_enc_smem(TC, bd, N, Np, nkinds, nblk);
  float* pb = reinterpret_cast<float*>(smem + L.pb);
  int* run = reinterpret_cast<int*>(smem + L.run);
  const int tid = threadIdx.x, wave = __builtin_amdgcn_readfirstlane(tid >> 6), lane = tid & 63;
  const int lr = lane & 15, lk = lane >> 4;
  const bool quant = !LIST && a.tokens_out != nullptr;
  const float vm1 = (float)(a.vocab - 1);
  const int nch = (T + TC - 1) / TC;

  // run[blk]: the first source column of the block where its dof_src entries are an ascending run
  // of a unit-stride row, else -1 (gathered)
  for (int i = tid; i < nblk; i += ST_NT) run[i] = a.sd == 1 ? a.dof_src[i * bd] : -1;
  st_sync();
  if (a.sd == 1)
    for (int d = tid; d < D; d += ST_NT) {
      const int blk = d / bd;
      if (a.dof_src[d] != a.dof_src[blk * bd] + (d - blk * bd)) run[blk] = -1;
    }
  st_sync();

  for (int64_t item = blockIdx.x; item < a.ntiles; item += gridDim.x) {
    const DofItem w = dof_item(item, nblk, bd, D, nj);
    const int d0 = w.d0, bdn = w.bdn;
    const float* src;
    if constexpr (LIST) {
      const uint64_t bi = (uint64_t)w.b / (uint64_t)a.list_rows;
      src = a.traj_list[bi] + (w.b - (int64_t)bi * a.list_rows) * a.sb;
    } else {
      src = a.traj + w.b * a.sb;
    }
    const int c0 = run[w.blk];
    const bool dma = c0 >= 0 && c0 + bdn <= a.row_elems;   // workgroup-uniform, as v16
    const bool v16 = dma && (bdn & 3) == 0 && (a.st & 3) == 0 && (((uintptr_t)(src + c0)) & 15) == 0;
    // this wave's column tiles: DoF inside the block (the column of a chunk's rows) and kind
    int cd[ST_CT], ck[ST_CT];
    bool cok[ST_CT], act[ST_CT];
#pragma unroll
    for (int i = 0; i < ST_CT; ++i) {
      const int q = wave + ST_NW * i;
      act[i] = q < w.nq;   // wave-uniform
      dof_col(w, min(q, w.nq - 1), lr, cd[i], ck[i], cok[i]);
      cok[i] = cok[i] && act[i];
    }

    // chunk c of both operands -> buffer c & 1
    auto load_chunk = [&](int c) ST_INLINE {
      const int t0 = c * TC, tc = min(TC, T - t0);
      float* Pb = reinterpret_cast<float*>(smem + L.P + (c & 1) * L.pbuf);
      float* Yb = reinterpret_cast<float*>(smem + L.Y + (c & 1) * L.ybuf);
      dma_segments<4>(Pb, a.proj + t0, nkinds * Np, TC >> 2, Tp, min(TC, Tp - t0) >> 2);
      if (dma && tc == TC) {
        const float* y0 = src + (int64_t)t0 * a.st + c0;
        if (v16) dma_segments<4>(Yb, y0, TC, bdn >> 2, a.st, bdn >> 2);
        else dma_segments<1>(Yb, y0, TC, bdn, a.st, bdn);
      } else {
        const int rows = round_up(tc, 4);
        for (int e = tid; e < rows * bdn; e += ST_NT) {
          const int t = e / bdn, col = a.dof_src[d0 + e - t * bdn];
          const bool in = t < tc && col >= 0 && col < a.row_elems;
          Yb[e] = in ? src[(int64_t)(t0 + t) * a.st + (int64_t)col * a.sd] : 0.0f;
        }
      }
    };

    float4_t acc[ST_CT][NRT][2];
#pragma unroll
    for (int i = 0; i < ST_CT; ++i)
#pragma unroll
      for (int rt = 0; rt < NRT; ++rt) acc[i][rt][0] = acc[i][rt][1] = float4_t{0.0f, 0.0f, 0.0f, 0.0f};

    load_chunk(0);
    for (int c = 0; c < nch; ++c) {
      // chunk c has landed (this wave's DMA: the explicit wait, as in k_encode_stream_list; the
      // gather: LDS stores); chunk c - 1 is consumed
      __builtin_amdgcn_s_waitcnt(0);
      st_sync();
      if (c + 1 < nch) load_chunk(c + 1);
      const float* Pb = reinterpret_cast<const float*>(smem + L.P + (c & 1) * L.pbuf);
      const float* Yb = reinterpret_cast<const float*>(smem + L.Y + (c & 1) * L.ybuf);
      const int nst = (min(TC, T - c * TC) + 3) >> 2;
      // K-step s covers t = 4 s + lane / 16 of the chunk; steps in pairs, even -> chain 0, odd -> chain 1
      for (int s = 0; s < nst; s += 2) {
        const bool two = s + 1 < nst;   // wave-uniform
        const int r0 = 4 * s + lk, r1 = two ? r0 + 4 : r0;
#pragma unroll
        for (int i = 0; i < ST_CT; ++i) {
          if (!act[i]) continue;
          const float y0 = Yb[r0 * bdn + cd[i]], y1 = Yb[r1 * bdn + cd[i]];
          float x0[NRT], x1[NRT];
#pragma unroll
          for (int rt = 0; rt < NRT; ++rt) {
            const float* pa = Pb + (ck[i] * Np + rt * 16 + lr) * TC;
            x0[rt] = pa[r0];
            x1[rt] = pa[r1];
          }
#pragma unroll
          for (int rt = 0; rt < NRT; ++rt) {
            acc[i][rt][0] = __builtin_amdgcn_mfma_f32_16x16x4f32(x0[rt], y0, acc[i][rt][0], 0, 0, 0);
            if (two) acc[i][rt][1] = __builtin_amdgcn_mfma_f32_16x16x4f32(x1[rt], y1, acc[i][rt][1], 0, 0, 0);
          }
        }
      }
    }
    // f32 C/D map: column = lane & 15, row n = 16 rt + 4 (lane >> 4) + r; the two chains meet once
#pragma unroll
    for (int i = 0; i < ST_CT; ++i)
#pragma unroll
      for (int rt = 0; rt < NRT; ++rt)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int n = rt * 16 + lk * 4 + r;
          if (cok[i] && n < N) pb[cd[i] * N + n] = __fadd_rn(acc[i][rt][0][r], acc[i][rt][1][r]);
        }
    st_sync();   // the image is whole; the chunk buffers are free

    // ---- epilogue: params (d n), one run of the row; tokens (n d), N runs of bdn
    if (a.params_out != nullptr && (a.phases & 4))
      store_out<ST_NT>(a.params_out + w.b * DN + (int64_t)d0 * N, pb, bdn * N);
    if (quant && (a.phases & 8)) {
      long long* tl = reinterpret_cast<long long*>(smem + L.Y);
      for (int e = tid; e < bdn * N; e += ST_NT) {
        const int dd = e / N, n = e - dd * N, k = d0 * N + e;
        tl[n * bdn + dd] = beast::quantize_one(pb[e], a.w_min[k], a.w_max[k], vm1) + a.tok_offset;
      }
      st_sync();
      long long* trow = a.tokens_out + w.b * DN + d0;
      const int spr = (bdn >> 1) + 1;   // 16-byte slots of a run, a half slot at a ragged head or tail included
      for (int s = tid; s < N * spr; s += ST_NT) {
        const int n = s / spr;
        long long* g = trow + (int64_t)n * D;
        const long long* t = tl + n * bdn;
        const int e0 = 2 * (s - n * spr) - (int)((((uintptr_t)g) >> 3) & 1);   // g + e0 is 16-byte aligned
        if (e0 >= 0 && e0 + 1 < bdn) st16<0>(g + e0, t[e0], t[e0 + 1]);
        else if (e0 >= 0 && e0 < bdn) g[e0] = t[e0];
        else if (e0 == -1) g[0] = t[0];
      }
    }
    st_sync();   // the images are free for the next item's chunks
  }
}

// ------------------------------------------------------------ reconstruct --
struct WrSmem {
  int wimg, phi, pbuf, out, dst, named, total;   // phi: buffer 0; buffer 1 lies pbuf bytes on
};
__host__ __device__ __forceinline__ WrSmem wd_rec_smem(int rc, int bd, int D, int N, int ndo, int nkinds, bool pos) {
  WrSmem s;
  int o = 0;
  s.wimg = o;  o += round_up(bd * RW_WS * 4, 16);
  s.pbuf = pos ? round_up(nkinds * rc * N * 4, 1024) : 0;   // DMA destinations: whole wave-instructions
  s.phi = o;   o += 2 * s.pbuf;
  s.out = o;   o += pos ? round_up(rc * bd * 4, 16) : 0;
  s.dst = o;   o += pos ? round_up(bd * 4, 16) : 0;
  s.named = o; o += pos && ndo > D ? round_up(ndo, 16) : 0;
  s.total = o;
  return s;
}

template <int KS>
__global__ BEAST_NO_PK_F32 __launch_bounds__(ST_NT) void k_reconstruct_dof(RecArgs a, int nblk, int bd, int RC,
                                                                           float rinv) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const int D = a.g.D, N = a.g.N, nj = a.g.nj, per = a.g.per;
  const int Tout = a.Tout, ndo = a.ndo;
  const int nkinds = (nj < D) ? 2 : 1;
  const bool pos = a.pos_out != nullptr;
  const WrSmem L = wd_rec_smem(RC, bd, D, N, ndo, nkinds, pos);
  float* wimg = reinterpret_cast<float*>(smem + L.wimg);
  float* ob = reinterpret_cast<float*>(smem + L.out);
  int* dstl = reinterpret_cast<int*>(smem + L.dst);
  unsigned char* named = smem + L.named;
  const int tid = threadIdx.x, wave = __builtin_amdgcn_readfirstlane(tid >> 6), lane = tid & 63;
  const int lr = lane & 15, lk = lane >> 4;
  const float vm1 = (float)(a.vocab - 1);
  const int qn = a.vocab <= beast::EXACT_QUOTIENT_MAX ? beast::EXACT_QUOTIENT_MAX : 0;
  const int nch = pos ? (Tout + RC - 1) / RC : 0;
  // 16-byte DMA units where every kind's rows of every chunk start on one
  const bool p16 = pos && ((Tout * N) & 3) == 0 && (((uintptr_t)a.basis) & 15) == 0;
  auto load_phi = [&](int c) ST_INLINE {
    const int r0 = c * RC;
    float* Pb = reinterpret_cast<float*>(smem + L.phi + (c & 1) * L.pbuf);
    const float* src = a.basis + (int64_t)r0 * N;
    const int left = (Tout - r0) * N;   // floats of a kind from row r0 on
    if (p16) dma_segments<4>(Pb, src, nkinds, (RC * N) >> 2, (int64_t)Tout * N, min(RC * N, left) >> 2);
    else dma_segments<1>(Pb, src, nkinds, RC * N, (int64_t)Tout * N, min(RC * N, left));
  };
  const bool spare = pos && ndo > D;   // output columns no DoF names: block 0 zeroes them
  if (spare) {
    for (int c = tid; c < ndo; c += ST_NT) named[c] = 0;
    st_sync();
    for (int d = tid; d < D; d += ST_NT) named[min(max(a.dof_dst[d], 0), ndo - 1)] = 1;   // read behind an item's barrier
  }

  for (int64_t item = blockIdx.x; item < a.ntiles; item += gridDim.x) {
    const DofItem w = dof_item(item, nblk, bd, D, nj);
    const int d0 = w.d0, bdn = w.bdn;
    int cd[ST_CT], ck[ST_CT];
    bool cok[ST_CT], act[ST_CT];
#pragma unroll
    for (int i = 0; i < ST_CT; ++i) {
      const int q = wave + ST_NW * i;
      act[i] = pos && q < w.nq;   // wave-uniform
      dof_col(w, min(q, w.nq - 1), lr, cd[i], ck[i], cok[i]);
      cok[i] = cok[i] && act[i];
    }
    if (pos && (nch > 1 || item == blockIdx.x)) load_phi(0);
    if (pos)
      for (int i = tid; i < bdn; i += ST_NT) dstl[i] = min(max(a.dof_dst[d0 + i], 0), ndo - 1);
    // ---- the block's tokens (n d) -> W image [dd][n], zero past N
    for (int e = tid; e < N * bdn; e += ST_NT) {
      const int n = e / bdn, dd = e - n * bdn, k = (d0 + dd) * N + n;
      const int64_t r = w.b * per + n * D + d0 + dd;
      const float lo = a.w_min[k], hi = a.w_max[k];
      float v;
      if (a.ntokens) {
        v = beast::denormalize_one(a.ntokens[r], lo, hi);
      } else {
        const long long t[1] = {a.tokens[r] - a.tok_offset};
        float nrm[1];
        fma_quotients(t, qn, vm1, rinv, nrm);
        v = beast::dequantize_quotient(nrm[0], lo, hi);
      }
      wimg[dd * RW_WS + n] = v;
    }
    for (int e = tid; e < bdn * (4 * KS - N); e += ST_NT) {
      const int dd = e / (4 * KS - N);
      wimg[dd * RW_WS + N + e - dd * (4 * KS - N)] = 0.0f;
    }
    st_sync();
    if (a.params_out != nullptr) {   // (d n), as decode(): the block's run of the row
      float* pout = a.params_out + w.b * per + (int64_t)d0 * N;
      for (int e = tid; e < bdn * N; e += ST_NT) {
        const int dd = e / N;
        pout[e] = wimg[dd * RW_WS + e - dd * N];
      }
    }
    float wb[ST_CT][KS];   // B operand, K-step ks: W[dd][4 ks + lane / 16]
#pragma unroll
    for (int i = 0; i < ST_CT; ++i) {
      if (!act[i]) continue;
      const float* wr = wimg + cd[i] * RW_WS + lk;
#pragma unroll
      for (int ks = 0; ks < KS; ++ks) wb[i][ks] = cok[i] ? wr[4 * ks] : 0.0f;
      if (a.init_p != nullptr && lk == 0 && cok[i] && ck[i] == 0)   // n = 0 of the joint DoFs <- init_p
        wb[i][0] = a.init_p[w.b * a.init_p_sb + a.init_p_src[d0 + cd[i]]];
    }

    for (int c = 0; c < nch; ++c) {
      const int r0 = c * RC, rcv = min(RC, Tout - r0), nrt = (rcv + 15) >> 4;
      __builtin_amdgcn_s_waitcnt(0);
      st_sync();   // Phi chunk c has landed; chunk c - 1 is consumed and its staged rows are stored
      if (c + 1 < nch) load_phi(c + 1);
      const float* Pb = reinterpret_cast<const float*>(smem + L.phi + ((nch > 1 ? c : 0) & 1) * L.pbuf);
#pragma unroll
      for (int i = 0; i < ST_CT; ++i) {
        if (!act[i]) continue;
        // A operand: Phi_kind[r0 + 16 rt + lr][4 ks + lk], zero past N; four row tiles, four chains
        const float* ph = Pb + (ck[i] * RC + lr) * N;
        float4_t acc[4];
#pragma unroll
        for (int rt = 0; rt < 4; ++rt) acc[rt] = float4_t{0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
        for (int ks = 0; ks < KS; ++ks) {
          const int n = 4 * ks + lk;
#pragma unroll
          for (int rt = 0; rt < 4; ++rt) {
            if (rt < nrt) {   // wave-uniform
              const float x = n < N ? ph[rt * 16 * N + min(n, N - 1)] : 0.0f;
              acc[rt] = __builtin_amdgcn_mfma_f32_16x16x4f32(x, wb[i][ks], acc[rt], 0, 0, 0);
            }
          }
        }
        // f32 C/D map: column = lane & 15, row = 16 rt + 4 (lane >> 4) + r; rows past the chunk's
        // last land in the image's padding rows and are not stored
        if (cok[i]) {
          float* oc = ob + lk * 4 * bdn + cd[i];
#pragma unroll
          for (int rt = 0; rt < 4; ++rt)
            if (rt < nrt)
#pragma unroll
              for (int r = 0; r < 4; ++r) oc[(rt * 16 + r) * bdn] = acc[rt][r];
        }
      }
      st_sync();
      float* prow = a.pos_out + (w.b * (int64_t)Tout + r0) * ndo;
      for (int e = tid; e < rcv * bdn; e += ST_NT) {
        const int t = e / bdn;
        prow[(int64_t)t * ndo + dstl[e - t * bdn]] = ob[e];
      }
      if (spare && w.blk == 0)
        for (int e = tid; e < rcv * ndo; e += ST_NT)
          if (!named[e % ndo]) prow[e] = 0.0f;
    }
    st_sync();   // the W image, the dof_dst entries and the staged rows are free for the next item
  }
}

}  // namespace
