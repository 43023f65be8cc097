// Encode action windows straight from an episode frame buffer: beast_encode_windows_f32.
//
// A window is (start, end) in rows of a flat [R][row_elems] frame buffer; its sample t is row
// min(start + t, end - 1) -- the next T actions, the episode's last frame repeated past its end.
// k_encode_windows is k_encode with another way of filling and addressing the LDS image: per tile
// of TBT consecutive windows it either stages the tile's row span ONCE (overlapping windows share
// their rows: at stride 1 a tile of 8 windows reads T + 7 rows, not 8 T) and points every
// window's B operand into that image, or -- scattered starts, whose span exceeds the image --
// gathers window by window into the [j][t][d] image k_encode's strided path builds.  The fit
// and the epilogue are codec_encode.h's enc_fit_tile / enc_store_tile: same products, same K
// order, same even / odd accumulators, same quantiser, so params and tokens are bitwise those of
// beast_encode_f32 on the gathered windows.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "common.h"
#include "launch.h"
#include "codec_device.h"
#include "codec_encode.h"

namespace {

constexpr int WIN_MAX_T = 256, WIN_MAX_N = 16, WIN_MAX_D = 64;

struct WinArgs {
  EncArgs e;                // traj = frames, B = W, st = the row stride sr, sd; sb unused
  int64_t R;
  const long long* win_start;
  const long long* win_end;
  uint32_t* tile_counts;    // nullable: [0] += 1 per shared-segment tile, [1] += 1 per gathered tile
  int Dl;                   // floats per row of the widest image: max(row_elems, D) when segments are possible
  int seg;                  // rows are contiguous floats (sd == 1) and TBT * T of them fit the image
  FastDiv fd_T;
};

struct WinSmem {
  EncSmem s;
  int ws, wv, total;        // per window of the tile: first row (int64), rows before the clamp (int)
};

// k_encode's layout with an image that holds TBT * T rows of Dl floats at any 16-byte phase, and
// the tile's window table behind it.
template <int TBT>
__host__ __device__ inline WinSmem win_smem(int T, int Tp, int Dl, int D, int N, int nkinds) {
  WinSmem w;
  EncSmem& s = w.s;
  int o = 0;
  s.P = o;    o += round_up(nkinds * 16 * Tp * 4 + 64 * ECH, 1024);
  // the image may start up to 12 bytes into the buffer (the source's offset inside its 16 bytes), and
  // the DMA then fills whole wave-instructions from byte 16: one more 16-byte unit than k_encode's
  s.Y = o;    o += round_up(TBT * T * Dl * 4, 1024) + 16;
  s.pb = o;   o += round_up(TBT * D * N * 4, 16);
  s.kq = o;   o += round_up(D * N * 16, 16);
  s.wlo = o;  o += round_up(D * N * 4, 256);
  s.whi = o;  o += round_up(D * N * 4, 256);
  s.lcol = o; o += round_up(D * 4, 256);
  s.total = o;
  w.ws = o;   o += TBT * 8;
  w.wv = o;   o += round_up(TBT * 4, 16);
  w.total = o;
  return w;
}

template <int TBT, class S>
__global__ __launch_bounds__(S::W * 64) void k_encode_windows(WinArgs w) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  constexpr int NW = S::W, NT = NW * 64;
  const EncArgs& a = w.e;
  const Geom& g = a.g;
  const Dims<S> m(g);
  const int D = m.D, N = m.N, T = m.T, Tp = m.Tp, DN = D * N;
  const int nkinds = (m.nj < D) ? 2 : 1;
  const WinSmem L = win_smem<TBT>(T, Tp, w.Dl, D, N, nkinds);
  float* P = reinterpret_cast<float*>(smem + L.s.P);
  float* Y = reinterpret_cast<float*>(smem + L.s.Y);
  float* pb = reinterpret_cast<float*>(smem + L.s.pb);
  float* wlo = reinterpret_cast<float*>(smem + L.s.wlo);
  float* whi = reinterpret_cast<float*>(smem + L.s.whi);
  float4* kq = reinterpret_cast<float4*>(smem + L.s.kq);
  int* lcol = reinterpret_cast<int*>(smem + L.s.lcol);
  long long* ws = reinterpret_cast<long long*>(smem + L.ws);
  int* wv = reinterpret_cast<int*>(smem + L.wv);
  const int tid = threadIdx.x;
  const bool quant = a.tokens_out != nullptr;
  const int re = a.row_elems;
  const int64_t sr = a.st;

  // ---- prologue: every constant HBM -> LDS by DMA (they land before the first tile's barrier)
  dma16<NT>(P, a.proj, nkinds * 4 * Tp);
  if (quant) {
    dma4<NT>(wlo, a.w_min, DN);
    dma4<NT>(whi, a.w_max, DN);
  }
  dma4<NT>(lcol, a.dof_src, D);

  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6), lane = tid & 63;
  const int lr = lane & 15, lk = lane >> 4;
  const float vm1 = (float)(a.vocab - 1);

  for (int64_t tile = blockIdx.x; tile < a.ntiles; tile += gridDim.x) {
    const int64_t b0 = tile * TBT;
    const int nb = (int)min<int64_t>(TBT, a.B - b0);

    // ---- the tile's windows, clamped: start into [0, R - 1], end into [start + 1, R], so every
    //      row below lies in [0, R) whatever the tables hold
    if (tid < nb) {
      const long long s = min(max(w.win_start[b0 + tid], 0ll), (long long)w.R - 1);
      const long long e = min(max(w.win_end[b0 + tid], s + 1), (long long)w.R);
      ws[tid] = s;
      wv[tid] = (int)min<long long>(e - s, T);   // rows the window owns: 1 .. T
    }
    __syncthreads();
    long long lo = ws[0], hi = ws[0] + wv[0];
    for (int j = 1; j < nb; ++j) {
      lo = min(lo, ws[j]);
      hi = max(hi, ws[j] + wv[j]);
    }
    // one decision per tile, the same in every thread: the span lo .. hi fits the image
    const bool seg = w.seg && hi - lo <= (long long)TBT * T;
    int shift = 0;   // floats between the image's first row and Y: the source's phase inside 16 bytes
    if (a.phases & 1) {
      if (seg) {
        const int rows = (int)(hi - lo);
        const float* src = a.traj + lo * sr;
        if (sr == re) {
          // one flat range of rows * re floats: whole wave-instructions of its 16-byte aligned middle
          // by 16-byte DMA into an image at the same phase; the floats before it (at most 3) and what
          // is left behind the last whole wave-instruction by plain loads.  No DMA lane is a padding
          // lane here: a padded tail would land, late, on the floats the plain loads store.
          const int nfl = rows * re;
          shift = (int)(((uintptr_t)src >> 2) & 3);
          const int head = min((4 - shift) & 3, nfl);
          const int n16 = ((nfl - head) >> 2) & ~63;
          float* img = Y + shift;
          dma16<NT>(img + head, src + head, n16);
          if (tid < head) img[tid] = src[tid];
          for (int i = head + 4 * n16 + tid; i < nfl; i += NT) img[i] = src[i];
        } else {
          // rows apart in memory: coalesced loads row by row
          for (int e = tid; e < rows * re; e += NT) {
            const int r = e / re, c = e - r * re;
            Y[e] = src[(int64_t)r * sr + c];
          }
        }
      } else {
        // [j][t][d], as k_encode's strided path builds it (the DoF map landed before the barrier above)
        for (int e = tid; e < nb * T * D; e += NT) {
          const int q = (int)div_by<S>((uint32_t)e, D, g.fd_D), d = e - q * D;
          const int j = (int)div_by<S>((uint32_t)q, T, w.fd_T), t = q - j * T;
          const int col = min(max(lcol[d], 0), re - 1);   // as the shared segment's columns: clamped into the row
          const int64_t row = ws[j] + min(t, wv[j] - 1);
          Y[e] = a.traj[row * sr + (int64_t)col * a.sd];
        }
      }
    }
    if (tid == 0 && w.tile_counts != nullptr) atomicAdd(w.tile_counts + (seg ? 0 : 1), 1u);
    __syncthreads();   // waits for the DMA (vmcnt) and the LDS stores
    if (quant && tile == blockIdx.x)   // bounds landed with the constants; read after the next barrier
      for (int i = tid; i < DN; i += NT)
        kq[i] = make_float4(wlo[i], whi[i], beast::quantize_scale(wlo[i], whi[i], vm1), 0.0f);

    // ---- fit: window j's sample t is row min(t, rows_j - 1) from its start inside the image
    if (a.phases & 2) {
      const int Dl = seg ? re : D;
      enc_fit_tile<TBT, S>(
          g, m, P, Y, pb, Dl, nb, wave, lr, lk, false,
          [&](int j, int& base, int& last) {
            const int jj = min(j, nb - 1);   // columns past the tile's last window are computed, never stored
            base = seg ? shift + (int)(ws[jj] - lo) * re : j * T * D;
            last = wv[jj] - 1;
          },
          [&](int d) { return seg ? min(max(lcol[d], 0), re - 1) : d; });
    }
    __syncthreads();

    // ---- epilogue: params (d n) and tokens (n d), both contiguous per tile
    enc_store_tile<S>(a, m, pb, kq, wlo, whi, b0, nb, vm1, false);
  }
}

template <int TBT>
int win_smem_total(int T, int Dl, int D, int N, int nkinds) {
  return win_smem<TBT>(T, round_up(T, 4), Dl, D, N, nkinds).total;
}
int win_smem_total(int tbt, int T, int Dl, int D, int N, int nkinds) {
  switch (tbt) {
    case 1: return win_smem_total<1>(T, Dl, D, N, nkinds);
    case 2: return win_smem_total<2>(T, Dl, D, N, nkinds);
    case 4: return win_smem_total<4>(T, Dl, D, N, nkinds);
    default: return win_smem_total<8>(T, Dl, D, N, nkinds);
  }
}

template <int TBT>
int launch_windows_t(WinArgs w, int T, int D, int nj, int N, const Queue& q) {
  w.e.g = make_geom<TBT>(D, nj, N, T);
  w.e.ntiles = (w.e.B + TBT - 1) / TBT;
  w.fd_T = make_fd((uint32_t)T);
  const int lds = win_smem<TBT>(T, w.e.g.Tp, w.Dl, D, N, nj < D ? 2 : 1).total;
  BEAST_REQUIRE_CODE(lds <= 160 * 1024, BEAST_E_UNSUPPORTED, "window tile needs %d B of LDS", lds);
  const int64_t grid = grid_for(w.e.ntiles, lds, q.dev);
  return launch<k_encode_windows<TBT, DynShape>>((unsigned)grid, DynShape::W * 64, lds, q, "k_encode_windows", w);
}

// The tile and its image, as launch_encode sizes them: the largest of 8/4/2/1 windows whose
// TBT * T rows fit 32 KB.  Rows that are no contiguous floats (sd != 1), or of which even T exceed
// 32 KB, are only ever gathered: the [j][t][d] image, the largest tile whose whole layout fits.
int launch_windows(WinArgs w, int T, int D, int nj, int N, const Queue& q) {
  const int nkinds = nj < D ? 2 : 1;
  w.seg = w.e.sd == 1 && (int64_t)T * std::max(w.e.row_elems, D) * 4 <= 32 * 1024;
  w.Dl = w.seg ? std::max(w.e.row_elems, D) : D;
  int tbt = 8;
  if (w.seg)
    while (tbt > 1 && (int64_t)tbt * T * w.Dl * 4 > 32 * 1024) tbt >>= 1;
  while (tbt > 1 && win_smem_total(tbt, T, w.Dl, D, N, nkinds) > 160 * 1024) tbt >>= 1;
  switch (tbt) {
    case 1: return launch_windows_t<1>(w, T, D, nj, N, q);
    case 2: return launch_windows_t<2>(w, T, D, nj, N, q);
    case 4: return launch_windows_t<4>(w, T, D, nj, N, q);
    default: return launch_windows_t<8>(w, T, D, nj, N, q);
  }
}

}  // namespace

extern "C" int beast_encode_windows_f32(const float* frames, int64_t R, int64_t sr, int64_t sd, int row_elems,
                                        const int64_t* win_start, const int64_t* win_end, int64_t W, int T, int D,
                                        int n_joint, const int32_t* dof_src, const float* proj, int N,
                                        const float* w_min, const float* w_max, int vocab, int64_t tok_offset,
                                        float* params_out, int64_t* tokens_out, uint32_t* tile_counts,
                                        void* stream) {
  BEAST_REQUIRE(frames && win_start && win_end && dof_src && proj, "beast_encode_windows_f32: null input pointer");
  BEAST_REQUIRE(params_out || tokens_out, "beast_encode_windows_f32: no output requested");
  BEAST_REQUIRE(W >= 0, "beast_encode_windows_f32: window count W=%lld must be >= 0", (long long)W);
  BEAST_REQUIRE(T >= 1 && N >= 1, "beast_encode_windows_f32: need T >= 1, N >= 1 (T=%d N=%d)", T, N);
  BEAST_REQUIRE(D >= 1 && n_joint >= 0 && n_joint <= D, "beast_encode_windows_f32: bad DoF split D=%d n_joint=%d", D,
                n_joint);
  BEAST_REQUIRE(row_elems >= 1, "beast_encode_windows_f32: row_elems must be >= 1");
  BEAST_REQUIRE(sr >= 0 && sd >= 0, "beast_encode_windows_f32: strides must be >= 0");
  BEAST_REQUIRE(R >= 1 || W == 0, "beast_encode_windows_f32: %lld windows over R=%lld frames", (long long)W,
                (long long)R);
  BEAST_REQUIRE(R <= 1 || sr >= (int64_t)(row_elems - 1) * sd + 1,
                "beast_encode_windows_f32: rows overlap (sr=%lld < (row_elems-1)*sd+1): a row must end before the next "
                "begins, so that every read stays below frames + R*sr", (long long)sr);
  BEAST_REQUIRE(!tokens_out || (w_min && w_max && vocab >= 2),
                "beast_encode_windows_f32: quantisation needs w_min/w_max and vocab >= 2");
  BEAST_REQUIRE_CODE(N <= WIN_MAX_N && T <= WIN_MAX_T && D <= WIN_MAX_D, BEAST_E_UNSUPPORTED,
                     "beast_encode_windows_f32 supports N <= %d, T <= %d, D <= %d (N=%d T=%d D=%d)", WIN_MAX_N,
                     WIN_MAX_T, WIN_MAX_D, N, T, D);
  if (W == 0) return BEAST_OK;
  WinArgs w{};
  EncArgs& a = w.e;
  a.traj = frames; a.B = W; a.sb = 0; a.st = sr; a.sd = sd; a.row_elems = row_elems; a.vocab = vocab;
  a.phases = debug_phases(); a.dof_src = dof_src; a.proj = proj; a.w_min = w_min; a.w_max = w_max;
  a.tok_offset = tok_offset; a.params_out = params_out; a.tokens_out = reinterpret_cast<long long*>(tokens_out);
  w.R = R;
  w.win_start = reinterpret_cast<const long long*>(win_start);
  w.win_end = reinterpret_cast<const long long*>(win_end);
  w.tile_counts = tile_counts;
  Queue q;
  BEAST_TRY(queue_of(stream, q, "beast_encode_windows_f32"));
  return launch_windows(w, T, D, n_joint, N, q);
}
