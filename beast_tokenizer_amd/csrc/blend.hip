// Blend window tokens back into episode frames: beast_reconstruct_windows_f32, the way back from
// beast_encode_windows_f32.  Every window of a (start, end) table over a flat [R] row buffer holds the
// tokens of T samples; output row r is the blend-weighted mean, over the windows that own r in table
// order, of their reconstructed samples (ACT's temporal ensembling, or with other weights a
// receding-horizon rule).
//
// k_blend_windows gathers per output row instead of scattering per window, so there is no atomic on
// an output and a row's bits depend on its own contributors and their table order alone.  A workgroup
// walks tiles of BL_S consecutive rows.  Per tile: the candidate windows [a, b) by binary search
// (blend_index.h), then chunks of C_w of them in ascending order -- token rows HBM -> LDS by DMA
// (stage_rows), dequantised into W[j][d][n] with the row kernels' arithmetic, then every thread runs
// its fixed (row, DoF) elements over the chunk's windows j ascending: membership, the blend != 0 test,
// the n-chain against the basis row in LDS, num = fma(blend, y, num), den += blend.  num, den and the
// count stay in registers across chunks, so any number of candidates (duplicate starts are unbounded)
// is summed in the same order.  The next chunk's DMA is issued before the current chunk's chains.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "common.h"
#include "launch.h"
#include "codec_device.h"
#include "codec_reconstruct.h"
#include "blend_index.h"

namespace {

constexpr int BL_MAX_T = 256, BL_MAX_N = 16, BL_MAX_D = 64, BL_MAX_NDO = 4096;
constexpr int BL_S = 64;          // output rows per tile
constexpr int BL_CW = 16;         // windows per chunk, fewer where 12 bytes per coefficient of them exceed BL_CHUNK_BYTES
constexpr int BL_CHUNK_BYTES = 48 * 1024;
constexpr int BL_STAGE_BYTES = 32 * 1024;   // the tile's output image is staged in LDS up to this size

struct BlendArgs {
  const void* tsrc;          // token rows: int64 (esz 8) or fp32 normalised (esz 4)
  int esz;
  int64_t W, R, ntiles, tok_offset, out_sr;
  int D, nj, N, T, ndo, vocab, cw;
  FastDiv fd_per, fd_D;
  unsigned long long posq;   // 4 bits per basis function n: its place in the fma chain (blend_chain_places)
  float rinv, fill;          // RN(1 / (vocab - 1)), IEEE-divided on the host: beast::exact_quotient's r
  const float* w_min;
  const float* w_max;
  const float* basis;        // [2][T][N]
  const float* blend;        // [T]
  const long long* win_start;
  const long long* win_end;
  const int32_t* dof_dst;
  float* out;
  int32_t* coverage;
  float* weight;
  uint32_t* tile_counts;     // nullable: [0] += chunks walked, [1] += 1 per tile that walked more than one
};

struct BlendSmem {
  int phi, bl, wlo, whi, dst, tok, wimg, rel, rows, col2d, out, total;
  bool stage;
};

__host__ __device__ inline int blend_chunk(int per) {
  return std::max(1, std::min(BL_CW, BL_CHUNK_BYTES / (per * 12)));
}

// The order in which beast_reconstruct_f32 sums a sample's N products for this shape, as the place
// of each basis function in one fma chain from 0.  Where it runs on the MFMA (rec_mfma_fits; K-step
// ks of v_mfma_f32_16x16x4_f32 holds n = k * KS + ks for k = 0 .. 3, KS = ceil(N / 4), and the
// instruction adds its four products to the accumulator one after another, k ascending) the chain
// is ks-major; in k_reconstruct_rows it is n ascending.  Products with n >= N are exact zeros there
// and are left out here.
inline unsigned long long blend_chain_places(int N, bool mfma) {
  unsigned long long q = 0;
  const int KS = (N + 3) / 4;
  int place = 0;
  if (mfma) {
    for (int ks = 0; ks < KS; ++ks)
      for (int k = 0; k < 4; ++k)
        if (k * KS + ks < N) q |= (unsigned long long)place++ << (4 * (k * KS + ks));
  } else {
    for (int n = 0; n < N; ++n) q |= (unsigned long long)place++ << (4 * n);
  }
  return q;
}
__device__ __forceinline__ int chain_place(unsigned long long q, int n) { return (int)(q >> (4 * n)) & 15; }

// DMA destinations are whole wave-instructions (1 KB of 16-byte lanes, 256 B of 4-byte ones): a
// partial instruction's padding lanes land inside the region they pad, on nothing else.
__host__ __device__ inline BlendSmem blend_smem(int T, int D, int N, int ndo, int nkinds, int cw) {
  BlendSmem s;
  const int per = N * D;
  int o = 0;
  s.phi = o;   o += round_up(nkinds * T * N * 4, 1024);
  s.tok = o;   o += round_up(cw * per * 8, 1024);
  s.bl = o;    o += round_up(T * 4, 256);
  s.wlo = o;   o += round_up(per * 4, 256);
  s.whi = o;   o += round_up(per * 4, 256);
  s.dst = o;   o += round_up(D * 4, 256);
  s.wimg = o;  o += round_up(cw * per * 4, 16);
  s.rel = o;   o += round_up(cw * 4, 16);
  s.rows = o;  o += round_up(cw * 4, 16);
  s.stage = BL_S * ndo * 4 <= BL_STAGE_BYTES;
  s.col2d = o; o += s.stage ? 0 : round_up(ndo * 4, 16);
  s.out = o;   o += s.stage ? round_up(BL_S * ndo * 4, 16) : 0;
  s.total = o;
  return s;
}

// One sample: the fma chain from 0 over the N slots of a basis row and a W row, both in chain order.
// Every operand is requested before the first fma (one LDS round trip, not N).  NN > 0: N at compile
// time; an even NN reads 8-byte pairs (both rows then start on 8 bytes: every offset is a multiple
// of N floats from a 16-byte aligned base).  NN == 0: any N <= BL_MAX_N behind uniform branches.
template <int NN>
__device__ __forceinline__ float blend_chain(const float* Ph, const float* Wr, int N) {
  float y = 0.0f;
  if constexpr (NN > 0 && NN % 2 == 0) {
    float2 p[NN / 2], w[NN / 2];
#pragma unroll
    for (int c = 0; c < NN / 2; ++c) {
      p[c] = reinterpret_cast<const float2*>(Ph)[c];
      w[c] = reinterpret_cast<const float2*>(Wr)[c];
    }
#pragma unroll
    for (int c = 0; c < NN / 2; ++c) {
      y = fmaf(p[c].x, w[c].x, y);
      y = fmaf(p[c].y, w[c].y, y);
    }
  } else {
    float p[BL_MAX_N], w[BL_MAX_N];
#pragma unroll
    for (int c = 0; c < BL_MAX_N; ++c)
      if (c < N) {
        p[c] = Ph[c];
        w[c] = Wr[c];
      }
#pragma unroll
    for (int c = 0; c < BL_MAX_N; ++c)
      if (c < N) y = fmaf(p[c], w[c], y);
  }
  return y;
}

// EPT: (row, DoF) elements per thread, BL_S * D <= EPT * NTHREADS.  NN: num_basis at compile time
// (the default 10), or 0 for any.
template <int EPT, int NN>
__global__ __launch_bounds__(NTHREADS) void k_blend_windows(BlendArgs a) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  constexpr int NT = NTHREADS;
  const int D = a.D, N = NN ? NN : a.N, T = a.T, nj = a.nj, ndo = a.ndo, per = N * D, cw = a.cw;
  const int nkinds = nj < D ? 2 : 1;
  const BlendSmem L = blend_smem(T, D, N, ndo, nkinds, cw);
  const float* phi = reinterpret_cast<const float*>(smem + L.phi);
  const float* bl = reinterpret_cast<const float*>(smem + L.bl);
  const float* wlo = reinterpret_cast<const float*>(smem + L.wlo);
  const float* whi = reinterpret_cast<const float*>(smem + L.whi);
  const int* dst = reinterpret_cast<const int*>(smem + L.dst);
  const unsigned char* tokl = smem + L.tok;
  float* wimg = reinterpret_cast<float*>(smem + L.wimg);
  int* rel = reinterpret_cast<int*>(smem + L.rel);
  int* rows = reinterpret_cast<int*>(smem + L.rows);
  int* col2d = reinterpret_cast<int*>(smem + L.col2d);
  float* ob = reinterpret_cast<float*>(smem + L.out);
  const int tid = threadIdx.x;
  const float vm1 = (float)(a.vocab - 1);
  const int qn = a.vocab <= beast::EXACT_QUOTIENT_MAX ? beast::EXACT_QUOTIENT_MAX : 0;

  // ---- prologue: the constants HBM -> LDS, once per workgroup: by DMA, but for the basis, whose
  //      rows are laid out in chain order (slot chain_place(a.posq, n) holds basis function n)
  for (int i = tid; i < nkinds * T * N; i += NT) {
    const int row = i / N;
    reinterpret_cast<float*>(smem + L.phi)[row * N + chain_place(a.posq, i - row * N)] = a.basis[i];
  }
  dma4<NT>(smem + L.bl, a.blend, T);
  dma4<NT>(smem + L.wlo, a.w_min, per);
  dma4<NT>(smem + L.whi, a.w_max, per);
  dma4<NT>(smem + L.dst, a.dof_dst, D);
  // num_dof_out > D: the columns dof_dst does not name are zeros; the staged image is cleared once
  // (the tiles only ever write the named columns)
  if (L.stage && ndo > D)
    for (int i = tid; i < BL_S * ndo; i += NT) ob[i] = 0.0f;
  // the thread's elements: e = u * NT + tid -> row e / D of the tile, DoF e % D; an element past the
  // tile gets a row no window can own
  int ei[EPT], ew[EPT], ep[EPT], ec[EPT];   // row in the tile, W offset d * N, basis offset kind * T * N, output column
  for (int u = 0; u < EPT; ++u) {
    const int e = u * NT + tid, i = e / D, d = e - i * D;
    ei[u] = e < BL_S * D ? i : -(1 << 20);
    ew[u] = d * N;
    ep[u] = (d < nj ? 0 : 1) * T * N;
  }
  __syncthreads();   // the constants are in place
  for (int u = 0; u < EPT; ++u) ec[u] = min(max(dst[(u * NT + tid) % D], 0), ndo - 1);
  if (!L.stage) {   // output column -> DoF, for the zeros of the direct store
    for (int c = tid; c < ndo; c += NT) col2d[c] = -1;
    __syncthreads();
    if (tid < D) col2d[min(max(dst[tid], 0), ndo - 1)] = tid;
    __syncthreads();
  }

  for (int64_t tile = blockIdx.x; tile < a.ntiles; tile += gridDim.x) {
    const int64_t r0 = tile * BL_S;
    const int nr = (int)min<int64_t>(BL_S, a.R - r0);
    long long wa, wb;
    beast::blend_candidates(a.win_start, a.W, a.R, T, r0, r0 + nr, wa, wb);   // the same in every thread
    const int64_t ncand = wb - wa;
    const int64_t nchunks = (ncand + cw - 1) / cw;

    float num[EPT], den[EPT];
    int cnt[EPT];
    for (int u = 0; u < EPT; ++u) {
      num[u] = 0.0f;
      den[u] = 0.0f;
      cnt[u] = 0;
    }
    // the first chunk's tokens and table entries (the token image is read between a chunk's two
    // barriers only, so nothing of the last tile reads it any more)
    long long ts = 0, te = 0;
    if (ncand > 0) {
      stage_rows<NT>(smem + L.tok, a.tsrc, wb, a.esz, wa, per, cw);
      if (tid < min<int64_t>(cw, ncand)) {
        ts = a.win_start[wa + tid];
        te = a.win_end[wa + tid];
      }
    }
    for (int64_t c0 = 0; c0 < ncand; c0 += cw) {
      const int cn = (int)min<int64_t>(cw, ncand - c0);
      __syncthreads();   // the chunk's DMA has landed; the last chunk's chains are done with W and the table
      // ---- the chunk's windows relative to the tile, and W[j][d][n] from the (n d) tokens
      if (tid < cn) {
        long long s;
        const int rw = beast::blend_rows(ts, te, a.R, T, s);
        // row i of the tile is sample i - (s - r0); beyond [-T, BL_S] no row of the tile is owned either
        rel[tid] = (int)min<long long>(max<long long>(s - r0, -(long long)T), BL_S);
        rows[tid] = rw;
      }
      for (int e = tid; e < cn * per; e += NT) {
        const int j = (int)fdiv((uint32_t)e, a.fd_per), r = e - j * per;
        const int n = (int)fdiv((uint32_t)r, a.fd_D), d = r - n * D, k = d * N + n;
        const float lo = wlo[k], hi = whi[k];
        float w;
        if (a.esz == 4) {
          w = beast::denormalize_one(reinterpret_cast<const float*>(tokl)[e], lo, hi);
        } else {
          const long long t1[1] = {reinterpret_cast<const long long*>(tokl)[e] - a.tok_offset};
          float nrm[1];
          fma_quotients(t1, qn, vm1, a.rinv, nrm);
          w = beast::dequantize_quotient(nrm[0], lo, hi);
        }
        wimg[j * per + d * N + chain_place(a.posq, n)] = w;
      }
      __syncthreads();   // W and the table are in place; the token image is free
      if (c0 + cw < ncand) {   // the next chunk's DMA runs under this chunk's chains
        const int64_t w1 = wa + c0 + cw;
        stage_rows<NT>(smem + L.tok, a.tsrc, wb, a.esz, w1, per, cw);
        if (tid < min<int64_t>(cw, wb - w1)) {
          ts = a.win_start[w1 + tid];
          te = a.win_end[w1 + tid];
        }
      }
      // ---- windows j ascending: blend_member's test on the staged (s - r0, rows), weight 0 skipped
      for (int j = 0; j < cn; ++j) {
        const int rl = rel[j], rw = rows[j];
        const float* Wj = wimg + j * per;
#pragma unroll
        for (int u = 0; u < EPT; ++u) {
          const int t = ei[u] - rl;
          if ((unsigned)t < (unsigned)rw) {
            const float bw = bl[t];
            if (bw != 0.0f) {
              const float y = blend_chain<NN>(phi + ep[u] + t * N, Wj + ew[u], N);   // slot order = chain order
              num[u] = fmaf(bw, y, num[u]);
              den[u] = den[u] + bw;
              cnt[u] += 1;
            }
          }
        }
      }
    }
    if (tid == 0 && a.tile_counts != nullptr) {
      atomicAdd(a.tile_counts, (uint32_t)nchunks);
      if (nchunks > 1) atomicAdd(a.tile_counts + 1, 1u);
    }

    // ---- the tile's rows: out (staged and stored coalesced, or straight to memory), coverage, weight
#pragma unroll
    for (int u = 0; u < EPT; ++u) {
      const int i = ei[u];
      if (i >= 0 && i < nr) {
        const float v = cnt[u] > 0 ? __fdiv_rn(num[u], den[u]) : a.fill;
        if (L.stage) ob[i * ndo + ec[u]] = v;
        else a.out[(r0 + i) * a.out_sr + ec[u]] = v;
        if (ew[u] == 0) {   // DoF 0 of the row
          if (a.coverage != nullptr) a.coverage[r0 + i] = cnt[u];
          if (a.weight != nullptr) a.weight[r0 + i] = den[u];
        }
      }
    }
    if (L.stage) {
      __syncthreads();
      float* gout = a.out + r0 * a.out_sr;
      if (a.out_sr == ndo) {
        store_out<NT>(gout, ob, nr * ndo);
      } else {
        for (int e = tid; e < nr * ndo; e += NT) {
          const int i = e / ndo, c = e - i * ndo;
          gout[(int64_t)i * a.out_sr + c] = ob[e];
        }
      }
      __syncthreads();   // the image is rewritten by the next tile
    } else {
      for (int e = tid; e < nr * ndo; e += NT) {
        const int i = e / ndo, c = e - i * ndo;
        if (col2d[c] < 0) a.out[(r0 + i) * a.out_sr + c] = 0.0f;
      }
    }
  }
}

template <int EPT>
int launch_blend_t(const BlendArgs& a, int lds, const Queue& q) {
  const int64_t grid = grid_for(a.ntiles, lds, q.dev);
  if (a.N == 10) return launch<k_blend_windows<EPT, 10>>((unsigned)grid, NTHREADS, lds, q, "k_blend_windows", a);
  return launch<k_blend_windows<EPT, 0>>((unsigned)grid, NTHREADS, lds, q, "k_blend_windows", a);
}

}  // namespace

extern "C" int beast_blend_candidates_host(const int64_t* win_start, const int64_t* win_end, int64_t W, int64_t R,
                                           int T, int64_t r0, int64_t r1, int64_t* a_out, int64_t* b_out) {
  BEAST_REQUIRE(a_out && b_out, "beast_blend_candidates_host: null output pointer");
  BEAST_REQUIRE(W >= 0 && R >= 0 && T >= 1, "beast_blend_candidates_host: need W >= 0, R >= 0, T >= 1");
  BEAST_REQUIRE(W == 0 || (win_start && win_end), "beast_blend_candidates_host: null table");
  BEAST_REQUIRE(0 <= r0 && r0 <= r1 && r1 <= R, "beast_blend_candidates_host: need 0 <= r0 <= r1 <= R");
  long long a, b;
  beast::blend_candidates(reinterpret_cast<const long long*>(win_start), W, R, T, r0, r1, a, b);
  *a_out = a;
  *b_out = b;
  return BEAST_OK;
}

extern "C" int beast_blend_member_host(int64_t start, int64_t end, int64_t R, int T, int64_t r) {
  int t;
  return (R >= 1 && T >= 1 && beast::blend_member(start, end, R, T, r, t)) ? t : -1;
}

extern "C" int beast_reconstruct_windows_f32(const int64_t* tokens, const float* ntokens, int64_t W, int D,
                                             int n_joint, int N, int vocab, int64_t tok_offset, const float* w_min,
                                             const float* w_max, const float* basis, int T,
                                             const int64_t* win_start, const int64_t* win_end, int64_t R,
                                             const float* blend, float fill, const int32_t* dof_dst,
                                             int num_dof_out, float* frames_out, int64_t out_sr,
                                             int32_t* coverage_out, float* weight_out, uint32_t* tile_counts,
                                             void* stream) {
  const char* fn = "beast_reconstruct_windows_f32";
  BEAST_REQUIRE(w_min && w_max && basis && blend && dof_dst, "%s: null input pointer", fn);
  BEAST_REQUIRE(W >= 0 && R >= 0, "%s: need W >= 0 and R >= 0 (W=%lld R=%lld)", fn, (long long)W, (long long)R);
  BEAST_REQUIRE(win_start && win_end && frames_out, "%s: null window table or output pointer", fn);
  BEAST_REQUIRE((tokens != nullptr) != (ntokens != nullptr), "%s: exactly one of tokens / ntokens must be given", fn);
  BEAST_REQUIRE(T >= 1 && N >= 1, "%s: need T >= 1, N >= 1 (T=%d N=%d)", fn, T, N);
  BEAST_REQUIRE(D >= 1 && n_joint >= 0 && n_joint <= D, "%s: bad DoF split D=%d n_joint=%d", fn, D, n_joint);
  BEAST_REQUIRE(num_dof_out >= D, "%s: num_dof_out=%d < D=%d", fn, num_dof_out, D);
  BEAST_REQUIRE(out_sr >= num_dof_out, "%s: out_sr=%lld < num_dof_out=%d", fn, (long long)out_sr, num_dof_out);
  BEAST_REQUIRE(!tokens || vocab >= 2, "%s: tokens need vocab >= 2", fn);
  BEAST_REQUIRE_CODE(N <= BL_MAX_N && T <= BL_MAX_T && D <= BL_MAX_D && num_dof_out <= BL_MAX_NDO,
                     BEAST_E_UNSUPPORTED, "%s supports N <= %d, T <= %d, D <= %d, num_dof_out <= %d (N=%d T=%d D=%d "
                     "num_dof_out=%d)", fn, BL_MAX_N, BL_MAX_T, BL_MAX_D, BL_MAX_NDO, N, T, D, num_dof_out);
  if (R == 0) return BEAST_OK;
  BlendArgs a{};
  a.tsrc = ntokens ? static_cast<const void*>(ntokens) : static_cast<const void*>(tokens);
  a.esz = ntokens ? 4 : 8;
  a.W = W; a.R = R; a.ntiles = (R + BL_S - 1) / BL_S; a.tok_offset = tok_offset; a.out_sr = out_sr;
  a.D = D; a.nj = n_joint; a.N = N; a.T = T; a.ndo = num_dof_out; a.vocab = tokens ? vocab : 2;
  a.cw = blend_chunk(N * D);
  a.fd_per = make_fd((uint32_t)(N * D));
  a.fd_D = make_fd((uint32_t)D);
  const int lut_n = (tokens && vocab <= LUT_MAX) ? vocab : 0;   // as beast_reconstruct_f32 sizes its layout
  a.posq = blend_chain_places(N, rec_mfma_fits<8>(T, D, N, num_dof_out, lut_n));
  a.rinv = 1.0f / (float)(a.vocab - 1);
  a.fill = fill;
  a.w_min = w_min; a.w_max = w_max; a.basis = basis; a.blend = blend;
  a.win_start = reinterpret_cast<const long long*>(win_start);
  a.win_end = reinterpret_cast<const long long*>(win_end);
  a.dof_dst = dof_dst; a.out = frames_out; a.coverage = coverage_out; a.weight = weight_out;
  a.tile_counts = tile_counts;
  const int lds = blend_smem(T, D, N, num_dof_out, n_joint < D ? 2 : 1, a.cw).total;
  BEAST_REQUIRE_CODE(lds <= 160 * 1024, BEAST_E_UNSUPPORTED, "%s: a tile needs %d B of LDS", fn, lds);
  Queue q;
  BEAST_TRY(queue_of(stream, q, fn));
  if (BL_S * D <= 4 * NTHREADS) return launch_blend_t<4>(a, lds, q);
  if (BL_S * D <= 8 * NTHREADS) return launch_blend_t<8>(a, lds, q);
  return launch_blend_t<16>(a, lds, q);
}
