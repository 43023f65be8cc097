// k_reconstruct_derivs_stream (deriv.hip's second kernel): beast_reconstruct_derivs_f32 on a SHARED
// basis whose requested order slabs do not fit DV_BASIS_LDS -- a chunk decoded on a dense time grid
// (T_out 2000 for a 2 s chunk at 1 kHz), or a tokenizer with seq_len >= 342.  The slabs are not
// resident: they move through two LDS buffers in chunks of RC output rows, chunk c + 1 in flight by
// LDS-DMA while chunk c is multiplied.  A work item is (tile of trajectories, range of output rows):
// a batch whose tiles cannot fill the GPU is cut along the time axis as well, down to B = 1.
//
// The arithmetic is k_reconstruct_derivs': one fmaf chain over n = 0 .. NP - 1 from 0, the basis value
// first, on slabs zero-padded to NP = 4 ceil(N / 4) columns -- so an output row has the resident
// path's bits whatever the chunking (and an MFMA, whose order of summation differs, is ruled out).
//
// Included by deriv.hip after DerivArgs, small_div and the DV_* constants.
#pragma once

namespace {

// Threads of a workgroup.  Where tiles alone fill the GPU a workgroup walks whole time axes and asks
// for the whole LDS budget, so one fits a CU: 16 waves then hide the LDS latency that 8 do not
// (B 4,096, T_out 2,048: 376 against 485 us).  Where the time axis is cut into short ranges 8 waves
// start and drain sooner (B 64, T_out 512: 7.9 against 11.8 us).
constexpr int DS_THREADS_WHOLE = 1024, DS_THREADS_SPLIT = 512;
constexpr int DS_LDS = 160 * 1024;       // the one LDS budget: W image, both slab buffers, bounds, col2d
constexpr int DS_SLAB_ALIGN = 256;       // floats: a slab of a buffer ends on a whole 16-byte wave-instruction
constexpr int DS_MIN_ROWS = 8;           // output rows of a work item, at least
constexpr int DS_MAX_SLABS = 4;          // order 0 of both kinds, orders 1 and 2 of kind 0

typedef __attribute__((address_space(3))) void ds_lds_void;

// what a padding column's DMA lane reads
__device__ const float ds_zero[4] __attribute__((aligned(16))) = {0.0f, 0.0f, 0.0f, 0.0f};

struct DsArgs {
  int64_t nitems;                // tiles x row ranges
  int nsplit, rl;                // row ranges per tile; rows per range (a multiple of 4)
  int rc;                        // rows per chunk (a multiple of 4, <= the query's RC)
  int ns;                        // staged slabs
  int slab_src[DS_MAX_SLABS];    // float offset of staged slab k in a.basis
  int so[DV_ORDERS], sg;         // float offset in a buffer of order o's kind-0 slab / of order 0's kind-1 slab
  int sstride, bstride;          // floats per staged slab, per buffer
  int p16;                       // N == NP and a 16-byte aligned basis: DMA in 16-byte units
  float inv_ndo;
};

__host__ __device__ constexpr int ds_round_up(int x, int m) { return (x + m - 1) / m * m; }

// staged slabs of a request: bit o of mask = output o is wanted
inline int ds_slab_count(int D, int nj, int mask) {
  return ((mask & 1) ? (nj < D ? 2 : 1) : 0) + ((mask >> 1) & 1) + ((mask >> 2) & 1);
}

// The chunk length RC (beast_reconstruct_derivs_stream_rows): the rows of every staged slab, twice,
// that fit DS_LDS beside the W image of a 16-trajectory tile, the bounds and col2d.  It depends on
// T_out only through the 0: the resident path serves the shape, or the entry point rejects it.
inline int ds_rows(int Tout, int D, int nj, int N, int ndo, int mask) {
  if (N < 1 || N > DV_MAX_N || D < 1 || D > DV_MAX_D || nj < 0 || nj > D || Tout < 1 || Tout > DV_MAX_T || ndo < D ||
      ndo > DV_MAX_NDO || mask < 1 || mask > 7)
    return 0;
  const int NP = 4 * ((N + 3) / 4), ns = ds_slab_count(D, nj, mask);
  if ((int64_t)ns * Tout * NP * 4 <= DV_BASIS_LDS) return 0;
  const int fixed = DV_TILE * D * NP * 4 + ds_round_up(2 * N * D * 4, 16) + ds_round_up(ndo * 4, 16);
  return ((DS_LDS - fixed - 2 * ns * DS_SLAB_ALIGN * 4) / (2 * ns * NP * 4)) & ~3;
}

// the wave's own LDS-DMA and LDS stores retired, then the workgroup barrier.  The wait is spelled
// out: a release fence alone leaves it to the compiler's wait-count pass, which has dropped the
// vmcnt wait in front of a barrier in a loop that issues its DMA at the bottom (DESIGN.md §"Long
// horizons", list mode).
__device__ __forceinline__ void ds_sync() {
  __builtin_amdgcn_s_waitcnt(0);
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
  __builtin_amdgcn_s_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
}

// Rows r0 .. r0 + rc - 1 of every staged slab -> buf [slab][rc][NP] by LDS-DMA.  Every lane carries
// its own global address: a padding column (n >= N) reads ds_zero, a row past the grid's last
// repeats it (never multiplied), the surplus lanes of a slab's last wave-instruction repeat its last
// unit.  Units are 16 bytes where no column is padding and the basis is aligned (p16), else 4.
template <int NP, int NT>
__device__ __forceinline__ void ds_load_chunk(float* buf, const DerivArgs& a, const DsArgs& s, int r0) {
  const int tid = threadIdx.x, wb = tid & ~63, N = a.N, last = a.Tout - 1;
  const int n = s.rc * NP;
  for (int k = 0; k < s.ns; ++k) {
    const float* src = a.basis + s.slab_src[k];
    float* dst = buf + k * s.sstride;
    if (s.p16) {
      const int n4 = n >> 2;
      for (int base = 0; base < n4; base += NT) {
        if (base + wb < n4) {
          const int f = 4 * min(base + tid, n4 - 1), r = f / NP, c = f - r * NP;
          const float* g = src + min(r0 + r, last) * N + c;
          __builtin_amdgcn_global_load_lds(reinterpret_cast<const uint4*>(g),
                                           (ds_lds_void*)(reinterpret_cast<uint4*>(dst) + base + wb), 16, 0, 0);
        }
      }
    } else {
      for (int base = 0; base < n; base += NT) {
        if (base + wb < n) {
          const int f = min(base + tid, n - 1), r = f / NP, c = f - r * NP;
          const float* g = c < N ? src + min(r0 + r, last) * N + c : ds_zero;
          __builtin_amdgcn_global_load_lds(reinterpret_cast<const uint32_t*>(g),
                                           (ds_lds_void*)(reinterpret_cast<uint32_t*>(dst) + base + wb), 4, 0, 0);
        }
      }
    }
  }
}

// LDS: W [TB][D][NP] | slab buffers 0, 1: [ns][sstride] | w_min, w_max [D*N] | col2d [num_dof_out]
//
// A workgroup walks the work items it, it + grid, ..: item = tile * nsplit + range.  Per item it
// dequantises its tile's tokens into the W image (a few KB; k_reconstruct_derivs' code) while the
// range's first chunk lands, then walks the range in chunks of rc rows, one barrier per chunk.
// Chunks are numbered through the items (buffer = running count & 1).
//
// Within a chunk, trajectory j's outputs of one order are ONE contiguous run of rcv * num_dof_out
// floats.  A thread owns four consecutive elements on the 4-element grid of the TILE's output range
// (the tile starts on a 16-byte boundary where the output does), so its store is one 16-byte store
// per order; the groups that straddle a run's ends store their elements inside the run one by one,
// and the rest belongs to the neighbouring chunk or trajectory, which stores it the same way.
template <int KS, int TB, int DS_THREADS>
__global__ __launch_bounds__(DS_THREADS) void k_reconstruct_derivs_stream(DerivArgs a, DsArgs s) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  constexpr int NP = 4 * KS;
  const int D = a.D, N = a.N, nj = a.nj, per = N * D, Tout = a.Tout, ndo = a.ndo;
  float* W = reinterpret_cast<float*>(smem);                  // [TB][D][NP]
  float* phi = reinterpret_cast<float*>(smem + a.off_phi);    // two chunk buffers
  float* wlo = reinterpret_cast<float*>(smem + a.off_wlo);    // [per]
  float* whi = wlo + per;                                     // [per]
  int* col2d = reinterpret_cast<int*>(smem + a.off_col);      // [ndo] output column -> DoF
  const int tid = threadIdx.x;
  const float vm1 = (float)(a.vocab - 1);
  const bool grip = nj < D;

  for (int i = tid; i < per; i += DS_THREADS) {
    wlo[i] = a.w_min[i];
    whi[i] = a.w_max[i];
  }
  for (int i = tid; i < TB * D * NP; i += DS_THREADS) W[i] = 0.0f;   // the pad columns stay 0
  for (int c = tid; c < ndo; c += DS_THREADS) col2d[c] = -1;
  ds_sync();
  for (int d = tid; d < D; d += DS_THREADS) {
    const int dd = a.dof_dst[d];
    if (dd >= 0 && dd < ndo) col2d[dd] = d;
  }

  const int row = Tout * ndo;                                 // elements per trajectory and order
  int gc = 0;                                                 // chunks opened: chunk gc lies in buffer gc & 1
  for (int64_t it = blockIdx.x; it < s.nitems; it += gridDim.x) {
    const int64_t tile = it / s.nsplit;
    const int t0 = (int)(it - tile * s.nsplit) * s.rl, t1 = min(Tout, t0 + s.rl);
    const int nch = (t1 - t0 + s.rc - 1) / s.rc;
    const int64_t b0 = tile * TB;
    const int nb = (int)min<int64_t>(TB, a.B - b0);
    if (it != blockIdx.x) ds_sync();                          // the previous item's W is read out
    ds_load_chunk<NP, DS_THREADS>(phi + (gc & 1) * s.bstride, a, s, t0);
    // ---- (n d) tokens -> W[j][d][n], once for every order and chunk
    for (int e = tid; e < nb * per; e += DS_THREADS) {
      const int j = small_div(e, a.inv_per), r = e - j * per;
      const int n = small_div(r, a.inv_D), d = r - n * D, k = d * N + n;
      float w;
      if (a.init_p != nullptr && n == 0 && d < nj) w = a.init_p[(b0 + j) * a.init_p_sb + a.init_p_src[d]];
      else if (a.ntokens != nullptr) w = beast::denormalize_one(a.ntokens[b0 * per + e], wlo[k], whi[k]);
      else w = beast::dequantize_one(a.tokens[b0 * per + e] - a.tok_offset, wlo[k], whi[k], vm1);
      W[(j * D + d) * NP + n] = w;
    }
    const int64_t gbase = b0 * row;
    for (int c = 0; c < nch; ++c, ++gc) {
      const int r0 = t0 + c * s.rc, rcv = min(s.rc, t1 - r0);
      ds_sync();   // chunk gc has landed (and W, col2d are written); chunk gc - 1 is consumed
      if (c + 1 < nch) ds_load_chunk<NP, DS_THREADS>(phi + ((gc + 1) & 1) * s.bstride, a, s, r0 + s.rc);
      const float* Pb = phi + (gc & 1) * s.bstride;
      // ---- groups of four elements: gmax per trajectory cover its run from the 4-element grid
      // point at or below the run's first element on
      const int run = rcv * ndo, gmax = ((run + 3) >> 2) + 1, ngroups = nb * gmax;
      const int sj = DS_THREADS / gmax, sk = DS_THREADS - sj * gmax;
      int j = tid / gmax, k = tid - j * gmax;
      for (int i = tid; i < ngroups; i += DS_THREADS) {
        const int lo = j * row + r0 * ndo, hi = lo + run;     // the run, in elements of the tile (< 2^28)
        const int e0 = ((lo >> 2) + k) << 2;
        if (e0 < hi) {
          const int q_lo = max(lo - e0, 0), q_hi = min(hi - e0, 4);
          // (row of the chunk, column) of the first element: rel < 2^24 is exact in fp32 and the
          // quotient <= 2^12 is within 2^-11 of rel / ndo, so the floor is off by one at most
          const int rel = e0 + q_lo - lo;
          int tt = (int)((float)rel * s.inv_ndo), cc = rel - tt * ndo;
          if (cc < 0) { cc += ndo; --tt; }
          if (cc >= ndo) { cc -= ndo; ++tt; }
          float v[4][DV_ORDERS];
          float4 p[DV_ORDERS][KS] = {}, pg[KS] = {};          // basis rows of row tt of the chunk
          auto load_rows = [&](int ts) {
#pragma unroll
            for (int o = 0; o < DV_ORDERS; ++o) {
              if (a.out[o] == nullptr) continue;
              const float4* src = reinterpret_cast<const float4*>(Pb + s.so[o] + ts * NP);
#pragma unroll
              for (int kk = 0; kk < KS; ++kk) p[o][kk] = src[kk];
            }
            if (grip && a.out[0] != nullptr) {                // kind 1 (degree 0): positions only
              const float4* src = reinterpret_cast<const float4*>(Pb + s.sg + ts * NP);
#pragma unroll
              for (int kk = 0; kk < KS; ++kk) pg[kk] = src[kk];
            }
          };
          load_rows(tt);
#pragma unroll
          for (int q = 0; q < 4; ++q) {
            v[q][0] = v[q][1] = v[q][2] = 0.0f;
            if (q < q_lo || q >= q_hi) continue;
            const int d = col2d[cc];
            if (d >= 0) {                                     // else: a column dof_dst does not name
              const bool g1 = d >= nj;
              const float4* Wr = reinterpret_cast<const float4*>(W + (j * D + d) * NP);
              float4 w[KS];
#pragma unroll
              for (int kk = 0; kk < KS; ++kk) w[kk] = Wr[kk];
#pragma unroll
              for (int o = 0; o < DV_ORDERS; ++o) {
                if (a.out[o] == nullptr || (o > 0 && g1)) continue;   // gripper DoFs: derivatives 0
                float acc = 0.0f;
#pragma unroll
                for (int kk = 0; kk < KS; ++kk) {             // a sequential fma over n
                  const float4 b = (o == 0 && g1) ? pg[kk] : p[o][kk];
                  acc = fmaf(b.x, w[kk].x, acc);
                  acc = fmaf(b.y, w[kk].y, acc);
                  acc = fmaf(b.z, w[kk].z, acc);
                  acc = fmaf(b.w, w[kk].w, acc);
                }
                v[q][o] = acc;
              }
            }
            if (++cc == ndo) {                                // the output row wraps: next row of the chunk
              cc = 0;
              ++tt;
              if (q + 1 < q_hi) load_rows(tt);
            }
          }
#pragma unroll
          for (int o = 0; o < DV_ORDERS; ++o) {
            if (a.out[o] == nullptr) continue;
            float* g = a.out[o] + gbase + e0;
            if (a.vec4 && q_lo == 0 && q_hi == 4) {
              *reinterpret_cast<float4*>(g) = make_float4(v[0][o], v[1][o], v[2][o], v[3][o]);
            } else {
#pragma unroll
              for (int q = 0; q < 4; ++q)
                if (q >= q_lo && q < q_hi) g[q] = v[q][o];
            }
          }
        }
        k += sk;                                              // (j, k) += DS_THREADS groups: one carry
        j += sj;
        if (k >= gmax) { k -= gmax; ++j; }
      }
    }
  }
}

// The split: tiles of 16 from two per CU on, else of 4 (launch_derivs_ks' regimes).  Where the tiles
// are fewer than two per CU the time axis is cut into ranges of rl rows so that tiles x ranges
// reach that count; a range shorter than RC is one chunk, and the launch asks for its LDS only.
template <int KS>
int launch_derivs_stream(DerivArgs a, int rc, int mask, const Queue& q) {
  constexpr int NP = 4 * KS;
  const int cus = cu_count(q.dev);
  const bool bulk = (a.B + DV_TILE - 1) / DV_TILE >= 2 * (int64_t)cus;
  const int TB = bulk ? DV_TILE : DV_TILE_SMALL;
  a.ntiles = (a.B + TB - 1) / TB;
  DsArgs s{};
  s.nsplit = 1;
  s.rl = ds_round_up(a.Tout, 4);
  if (a.ntiles < 2 * (int64_t)cus) {
    const int want = (int)((2 * (int64_t)cus + a.ntiles - 1) / a.ntiles);
    s.rl = std::max(DS_MIN_ROWS, ds_round_up((a.Tout + want - 1) / want, 4));
    s.nsplit = (a.Tout + s.rl - 1) / s.rl;
  }
  s.nitems = a.ntiles * s.nsplit;
  s.rc = std::min(rc, s.rl);
  const bool grip = a.nj < a.D;
  s.sstride = ds_round_up(s.rc * NP, DS_SLAB_ALIGN);
  s.sg = 0;
  for (int o = 0; o < DV_ORDERS; ++o) {
    s.so[o] = 0;
    if (!(mask >> o & 1)) continue;
    s.so[o] = s.ns * s.sstride;
    s.slab_src[s.ns++] = o * 2 * a.Tout * a.N;
    if (o == 0 && grip) {
      s.sg = s.ns * s.sstride;
      s.slab_src[s.ns++] = a.Tout * a.N;
    }
  }
  s.bstride = s.ns * s.sstride;
  s.p16 = a.N == NP && (((uintptr_t)a.basis) & 15) == 0;
  s.inv_ndo = 1.0f / (float)a.ndo;
  a.off_phi = TB * a.D * NP * 4;
  a.off_wlo = a.off_phi + 2 * s.bstride * 4;
  a.off_col = a.off_wlo + ds_round_up(2 * a.N * a.D * 4, 16);
  const int lds = a.off_col + ds_round_up(a.ndo * 4, 16);
  BEAST_REQUIRE_CODE(lds <= DS_LDS, BEAST_E_UNSUPPORTED, "streamed reconstruct derivs needs %d B of LDS", lds);
  const int nt = s.nsplit == 1 ? DS_THREADS_WHOLE : DS_THREADS_SPLIT;
  const int per_cu = std::max(1, std::min(2048 / nt, DS_LDS / lds));   // resident workgroups only
  const unsigned grid = (unsigned)std::max<int64_t>(1, std::min<int64_t>(s.nitems, (int64_t)cus * per_cu));
  const char* what = "k_reconstruct_derivs_stream";
  if (s.nsplit > 1)   // only small batches are split: tiles of 4
    return launch<k_reconstruct_derivs_stream<KS, DV_TILE_SMALL, DS_THREADS_SPLIT>>(grid, nt, lds, q, what, a, s);
  if (bulk) return launch<k_reconstruct_derivs_stream<KS, DV_TILE, DS_THREADS_WHOLE>>(grid, nt, lds, q, what, a, s);
  return launch<k_reconstruct_derivs_stream<KS, DV_TILE_SMALL, DS_THREADS_WHOLE>>(grid, nt, lds, q, what, a, s);
}

}  // namespace
