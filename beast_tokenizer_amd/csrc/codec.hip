// Fused BEAST encode / reconstruct kernels for gfx950: the host dispatch,
// the C-ABI entry points and the options.  One translation unit (the kernarg-preload flag, the
// -DBEAST_STAMPS device globals and the code-object comparison depend on that), in layers:
//
//   launch.h             host only, the whole library's launch layer: the stream's device, DeviceGuard,
//                        cu_count, grid_for, the debug knobs and the typed launch<kernel> (cached
//                        handles, dynamic-LDS grant)
//   codec_device.h       device primitives that know no argument block: FastDiv, LDS-DMA
//                        staging, st16 store policies, stamps, Geom / Shape / Dims, and the single
//                        definitions of the arithmetic the kernels must agree on bit for bit
//                        (wave_sync, lut_fill, lut_quotients, fma_quotients, slot_row / slot_values,
//                        wave_copy_out; the quantiser beast::quantize_bins, beast::dequantize_quotient
//                        and beast::exact_quotient are common.h's)
//   codec_encode.h       k_encode (4- / 7-wave tile walk: params = P . y on v_mfma_f32_16x16x4_f32,
//                        clamp / quantise / (d n)->(n d) / LLM-offset epilogue) and k_encode_v (one
//                        wave per trajectory, W trajectories per workgroup, no barrier after the
//                        prologue)
//   codec_reconstruct.h  k_reconstruct (tile walk: dequantise + init_p + Phi . W + scatter),
//                        k_reconstruct_v (one wave per trajectory) and k_reconstruct_rows (per-row
//                        basis and decode-only, VALU)
//   codec_roundtrip.h    k_roundtrip: encode -> reconstruct error statistics in one launch
//
// Which kernel a call gets is decided below (launch_encode, launch_reconstruct, the round-trip
// dispatch in beast_roundtrip_stats_f32) and reported through BEAST_OPT_LAST_CODEC_LAUNCH.
#include <hip/hip_runtime.h>

#include <atomic>

#include <algorithm>
#include <cstdlib>

#include "common.h"
#include "launch.h"
#include "codec_device.h"
#include "codec_encode.h"
#include "codec_reconstruct.h"
#include "codec_roundtrip.h"

namespace {

constexpr int MAX_T = 256;
constexpr int MAX_N = 16;
constexpr int MAX_D = 64;

// Diagnostic / test knob (beast_set_option): run the runtime-shape kernels even where a
// specialised one exists.
bool g_generic_only = false;

// Specialised 14-DoF kernels come in two widths.  A batch that gives every CU at most two
// tiles is latency-bound: 7 waves, one MFMA column tile each, shorten a workgroup's critical
// path.  Larger batches want more tiles in flight per CU: 4 waves (two column tiles each)
// fit 4 workgroups per CU where 7-wave ones fit 2.  beast_set_option(BEAST_OPT_BLOCK_WAVES,
// 4 | 7) forces one (tests, measurements); 0 = by batch size.
int g_block_waves = 0;
bool wide_blocks(int64_t ntiles, const Queue& q) {
  if (g_block_waves == 4 || g_block_waves == 7 || g_block_waves == 8) return g_block_waves != 4;
  return ntiles <= 2 * (int64_t)cu_count(q.dev);
}
// The per-trajectory kernels (k_encode_v, k_reconstruct_v) for the fixed shapes: encode at every
// batch size, reconstruct in the latency regime (its 4-wave kernel is as fast for bulk launches,
// profiles/r05/).  BEAST_OPT_BLOCK_WAVES 4 / 7 forces the 4- / 7-wave k_encode / k_reconstruct, 8
// the per-trajectory kernels at any batch size.
bool enc_v() { return g_block_waves == 0 || g_block_waves == 8; }

// The BEAST default shapes (T = 50, N = 10: the caller checks those) that have specialised
// kernels: 14 DoF with 0 or 2 gripper DoF and -- TILES, the tile-walking kernels -- 7 DoF and the
// 7-wave form of the 14-DoF shapes when `wide`.  Calls f with the Shape<> and returns true, or
// returns false for any other shape.
template <int NJ, bool TILES, class F>
int with_shape14(bool wide, F& f) {
  if constexpr (TILES) {
    if (wide) return f(Shape<14, NJ, 10, 50, 14, 7>{});
  }
  return f(Shape<14, NJ, 10, 50, 14>{});
}
template <bool TILES, class F>
bool with_fixed_shape(int D, int nj, bool wide, int& rc, F f) {
  if (D == 14 && nj == 14) rc = with_shape14<14, TILES>(wide, f);
  else if (D == 14 && nj == 12) rc = with_shape14<12, TILES>(wide, f);
  else if (TILES && D == 7 && nj == 7) {
    if constexpr (TILES) rc = f(Shape<7, 7, 10, 50, 7>{});
  } else return false;
  return true;
}

// BEAST_OPT_LAST_CODEC_LAUNCH (tests, tools): which kernel the last encode / reconstruct launch of
// this process chose, packed as include/beast_hip.h lays out.  Every launcher stores it once,
// relaxed, after its LDS check and before the launch; 0 until the first launch.
std::atomic<int> g_last_launch{0};
enum LaunchFamily {
  FAM_ENCODE_V = 1, FAM_ENCODE_SPEC = 2, FAM_ENCODE_DYN = 3, FAM_REC_V = 4, FAM_REC_SPEC = 5, FAM_REC_MFMA = 6,
  FAM_REC_ROWS = 7
};
constexpr int launch_mark(int family, int tile, int waves, int ks, bool fast, bool regs, bool staged, bool lat) {
  return family | tile << 4 | waves << 9 | ks << 14 | (fast ? 1 << 17 : 0) | (regs ? 1 << 18 : 0) |
         (staged ? 1 << 19 : 0) | (lat ? 1 << 20 : 0);
}
inline void mark_launch(int v) { g_last_launch.store(v, std::memory_order_relaxed); }

template <class S, int W, int SP>
int launch_encode_vw(EncArgs a, bool lat, const Queue& q) {
  constexpr EvSmem L = ev_smem<S, W>(S::NJ < S::D ? 2 : 1);
  static_assert(L.total <= (W <= 8 ? 80 : 160) * 1024, "k_encode_v LDS");
  a.g = make_geom<W>(S::D, S::NJ, S::N, S::T);
  a.ntiles = (a.B + W - 1) / W;
  mark_launch(launch_mark(FAM_ENCODE_V, W, W, 0, true, false, true, lat));
  return launch<k_encode_v<S, SP, W>>((unsigned)a.ntiles, W * 64, L.total, q, "k_encode_v", a.traj, a.B,
                                      EncVArgs{a.dof_src, a.proj, a.w_min, a.w_max, a.tokens_out, a.params_out,
                                               a.tok_offset, a.vocab, a.phases});
}

// write-through stores and RV_WE-wave tiles in the latency regime (at most one 16-trajectory tile
// per CU), write-back stores and 8-wave tiles for bulk launches
template <class S>
int launch_encode_v(EncArgs a, const Queue& q) {
  const bool lat = a.B <= 16 * (int64_t)cu_count(q.dev);
  return lat ? launch_encode_vw<S, RV_WE, LAT_SP>(a, true, q) : launch_encode_vw<S, RV_WE_BULK, 0>(a, false, q);
}

template <int TBT, class S>
int launch_encode_t(EncArgs a, int T, int D, int nj, int N, bool fast, const Queue& q) {
  a.g = make_geom<TBT>(D, nj, N, T);
  a.ntiles = (a.B + TBT - 1) / TBT;
  const int Dl = fast ? a.row_elems : D;
  const EncSmem L = enc_smem<TBT>(T, a.g.Tp, Dl, D, N, nj < D ? 2 : 1);
  BEAST_REQUIRE_CODE(L.total <= 160 * 1024, BEAST_E_UNSUPPORTED, "encode tile needs %d B of LDS", L.total);
  const int64_t grid = grid_for(a.ntiles, L.total, q.dev);
  mark_launch(launch_mark(S::fixed ? FAM_ENCODE_SPEC : FAM_ENCODE_DYN, TBT, S::W, 0, fast, false, true, S::W == 7));
  return fast ? launch<k_encode<TBT, true, S>>((unsigned)grid, S::W * 64, L.total, q, "k_encode", a)
              : launch<k_encode<TBT, false, S>>((unsigned)grid, S::W * 64, L.total, q, "k_encode", a);
}

int enc_smem_total(int tbt, int T, int Dl, int D, int N, int nkinds) {
  const int Tp = round_up(T, 4);
  switch (tbt) {
    case 1: return enc_smem<1>(T, Tp, Dl, D, N, nkinds).total;
    case 2: return enc_smem<2>(T, Tp, Dl, D, N, nkinds).total;
    case 4: return enc_smem<4>(T, Tp, Dl, D, N, nkinds).total;
    default: return enc_smem<8>(T, Tp, Dl, D, N, nkinds).total;
  }
}

// Tile size: the largest of 8/4/2/1 trajectories whose rows fit 32 KB of LDS
// (BEAST_ENC_TBT overrides, for measurements).  Rows the contiguous DMA path does not take
// (strided, misaligned, or one trajectory above 32 KB) are gathered into [T][D] images by the
// kernel: the largest tile whose whole LDS layout fits (one trajectory at T = 256, D = 64).
// The BEAST default shapes (T = 50, N = 10, D = 14 with 0 or 2 gripper DoF, D = 7) run fully
// specialised kernels.
int launch_encode(EncArgs a, int T, int D, int nj, int N, const Queue& q) {
  const int64_t traj_bytes = (int64_t)T * a.row_elems * 4;
  const bool contiguous = a.sd == 1 && a.st == a.row_elems && a.sb == (int64_t)T * a.row_elems &&
                          (((uintptr_t)a.traj) & 15) == 0 && ((int64_t)T * a.row_elems) % 4 == 0;
  static const int forced = [] {
    const char* e = getenv("BEAST_ENC_TBT");
    return e ? atoi(e) : 0;
  }();
  int tbt = 8;
  while (tbt > 1 && tbt * traj_bytes > 32 * 1024) tbt >>= 1;
  const bool fast = contiguous && tbt * traj_bytes <= 32 * 1024;
  if (!fast) {
    tbt = 8;
    while (tbt > 1 && enc_smem_total(tbt, T, D, D, N, nj < D ? 2 : 1) > 160 * 1024) tbt >>= 1;
  }
  if (forced == 1 || forced == 2 || forced == 4 || (forced == 8 && fast)) tbt = std::min(tbt, forced);
  // list mode: the contiguous DMA path only, tiles of one batch each
  BEAST_REQUIRE(!a.traj_list || (fast && a.list_rows % tbt == 0),
                "encode list: rows must be contiguous and rows per batch a multiple of %d", tbt);
  if (fast && tbt == 8 && !g_generic_only && T == 50 && N == 10 && a.row_elems == D) {
    int rc = 0;
    // k_encode_v stores its outputs with unconditional 16-byte stores: other alignments take k_encode
    const bool out16 = (((uintptr_t)a.params_out | (uintptr_t)a.tokens_out) & 15) == 0;
    if (!a.traj_list && enc_v() && out16 &&
        with_fixed_shape<false>(D, nj, false, rc, [&](auto sh) { return launch_encode_v<decltype(sh)>(a, q); }))
      return rc;
    if (with_fixed_shape<true>(D, nj, wide_blocks((a.B + 7) / 8, q), rc, [&](auto sh) {
          return launch_encode_t<8, decltype(sh)>(a, T, D, nj, N, true, q);
        }))
      return rc;
  }
  switch (tbt) {
    case 1: return launch_encode_t<1, DynShape>(a, T, D, nj, N, fast, q);
    case 2: return launch_encode_t<2, DynShape>(a, T, D, nj, N, fast, q);
    case 4: return launch_encode_t<4, DynShape>(a, T, D, nj, N, fast, q);
    default: return launch_encode_t<8, DynShape>(a, T, D, nj, N, fast, q);
  }
}

template <int TBT, int KS, int RT, class S = DynShape>
int launch_rec_ks(RecArgs a, int D, int nj, const Queue& q) {
  const RecSmem L = rec_smem<TBT, KS, RT>(a.Tout, D, a.g.N, a.ndo, nj < D ? 2 : 1, a.lut_n);
  BEAST_REQUIRE_CODE(L.total <= 160 * 1024, BEAST_E_UNSUPPORTED, "reconstruct tile needs %d B of LDS", L.total);
  const int64_t grid = grid_for(a.ntiles, L.total, q.dev);
  if constexpr (KS == 0) {
    mark_launch(launch_mark(FAM_REC_ROWS, TBT, NWAVES, 0, false, false, L.stage, false));
    return launch<k_reconstruct_rows<TBT>>((unsigned)grid, NTHREADS, L.total, q, "k_reconstruct_rows", a);
  } else {
    mark_launch(launch_mark(S::fixed ? FAM_REC_SPEC : FAM_REC_MFMA, TBT, S::W, KS, false, RT > 0, true, S::W == 7));
    return launch<k_reconstruct<TBT, KS, RT, S>>(
        (unsigned)grid, S::W * 64, L.total, q, "k_reconstruct",
        a.ntokens ? static_cast<const void*>(a.ntokens) : static_cast<const void*>(a.tokens), a.B, a.ntokens ? 4 : 8, a);
  }
}

template <int TBT, int RT>
int launch_rec_mfma(RecArgs a, int D, int nj, int N, const Queue& q) {
  switch ((N + 3) / 4) {
    case 1: return launch_rec_ks<TBT, 1, RT>(a, D, nj, q);
    case 2: return launch_rec_ks<TBT, 2, RT>(a, D, nj, q);
    case 3: return launch_rec_ks<TBT, 3, RT>(a, D, nj, q);
    default: return launch_rec_ks<TBT, 4, RT>(a, D, nj, q);
  }
}

// k_reconstruct_v takes the latency regime's fixed shapes unless BEAST_OPT_BLOCK_WAVES forces
// the 7-wave (or 4-wave) k_reconstruct; positions only (no params_out), int64 tokens, one tile
// per workgroup
bool rec_v(const RecArgs& a, const Queue& q) {
  return (g_block_waves == 8 || (g_block_waves == 0 && a.ntiles <= 2 * (int64_t)cu_count(q.dev))) &&
         a.params_out == nullptr && a.ntokens == nullptr && (((uintptr_t)a.pos_out) & 15) == 0;
}

template <class S>
int launch_rec_v(RecArgs a, const Queue& q) {
  constexpr int KS = (S::N + 3) / 4;
  constexpr RvSmem L = rv_smem<S>(S::NJ < S::D ? 2 : 1);
  static_assert(L.total <= (RV_WR <= 8 ? 64 : 160) * 1024, "k_reconstruct_v LDS");
  a.tbt = RV_WR;
  a.ntiles = (a.B + RV_WR - 1) / RV_WR;
  const bool lat = a.B <= 16 * (int64_t)cu_count(q.dev);   // at most one 16-trajectory tile per CU
  mark_launch(launch_mark(FAM_REC_V, RV_WR, RV_WR, KS, false, true, true, lat));
  const float vm1 = (float)(a.vocab - 1);   // the kernel's own conversion
  const RecVArgs v{a.w_min, a.w_max, a.basis, a.dof_dst, a.init_p, a.init_p_src, a.pos_out, a.tok_offset,
                   a.init_p_sb, a.vocab, 1.0f / vm1, a.phases};   // IEEE division: beast::exact_quotient's r
  const unsigned grid = (unsigned)a.ntiles;
  return lat ? launch<k_reconstruct_v<KS, S, LAT_SP>>(grid, RV_WR * 64, L.total, q, "k_reconstruct_v", a.tokens, a.B, 8, v)
             : launch<k_reconstruct_v<KS, S, 0>>(grid, RV_WR * 64, L.total, q, "k_reconstruct_v", a.tokens, a.B, 8, v);
}

template <int TBT>
int launch_reconstruct(RecArgs a, int D, int nj, int N, bool shared, const Queue& q) {
  a.g = make_geom<TBT>(D, nj, N, 1);
  a.ntiles = (a.B + TBT - 1) / TBT;
  a.tbt = TBT;
  a.fd_row = make_fd((uint32_t)(a.Tout * a.ndo));
  a.lut_n = (a.ntokens == nullptr && a.vocab <= LUT_MAX) ? a.vocab : 0;
  const bool pos = a.pos_out != nullptr;
  // MFMA path: shared basis, positions requested, the padded output tile fits LDS
  const bool mfma = shared && pos && rec_mfma_fits<TBT>(a.Tout, D, N, a.ndo, a.lut_n);
  if (!mfma) return launch_rec_ks<TBT, 0, 0>(a, D, nj, q);
  if (a.Tout <= 16 * RT_REG) {
    if (!g_generic_only && N == 10 && a.Tout == 50 && a.ndo == D) {
      int rc = 0;
      const bool wide = wide_blocks(a.ntiles, q);
      if (wide && rec_v(a, q) &&
          with_fixed_shape<false>(D, nj, false, rc, [&](auto sh) { return launch_rec_v<decltype(sh)>(a, q); }))
        return rc;
      if (with_fixed_shape<true>(D, nj, wide, rc, [&](auto sh) {
            return launch_rec_ks<TBT, 3, RT_REG, decltype(sh)>(a, D, nj, q);
          }))
        return rc;
    }
    return launch_rec_mfma<TBT, RT_REG>(a, D, nj, N, q);
  }
  return launch_rec_mfma<TBT, 0>(a, D, nj, N, q);
}

template <class S, int WF>
int launch_roundtrip(const float* traj, int64_t B, RtArgs a, int W, const Queue& q) {
  const RtSmem L = rt_smem(a.T, a.D, a.N, a.nj < a.D ? 2 : 1, W, a.lut_n);
  BEAST_REQUIRE_CODE(L.total <= 160 * 1024, BEAST_E_UNSUPPORTED, "round trip tile needs %d B of LDS", L.total);
  const int64_t grid = grid_for((B + W - 1) / W, L.total, q.dev);
  return launch<k_roundtrip<S, WF>>((unsigned)grid, (unsigned)(W * 64), (unsigned)L.total, q, "k_roundtrip", traj, B, a);
}

// 16-wave tiles while the batch gives every CU at most one, 8-wave tiles (three workgroups per CU
// overlap their prologues) for bulk launches, as k_encode_v
template <class S>
int launch_roundtrip_fixed(const float* traj, int64_t B, const RtArgs& a, const Queue& q) {
  return B <= RT_W * (int64_t)cu_count(q.dev) ? launch_roundtrip<S, RT_W>(traj, B, a, RT_W, q)
                                              : launch_roundtrip<S, RT_W_BULK>(traj, B, a, RT_W_BULK, q);
}

}  // namespace

// =================================================================== C-ABI ==
extern "C" int beast_encode_f32(const float* traj, int64_t B, int T, int64_t sb, int64_t st, int64_t sd,
                                int row_elems, int D, int n_joint, const int32_t* dof_src, const float* proj,
                                int N, const float* w_min, const float* w_max, int vocab, int64_t tok_offset,
                                float* params_out, int64_t* tokens_out, void* stream) {
  BEAST_REQUIRE(traj && dof_src && proj, "beast_encode_f32: null input pointer");
  BEAST_REQUIRE(params_out || tokens_out, "beast_encode_f32: no output requested");
  BEAST_REQUIRE(T >= 1 && T <= MAX_T, "seq_len T=%d outside [1, %d]", T, MAX_T);
  BEAST_REQUIRE(N >= 1 && N <= MAX_N, "num_basis N=%d outside [1, %d]", N, MAX_N);
  BEAST_REQUIRE(D >= 1 && D <= MAX_D && n_joint >= 0 && n_joint <= D, "bad DoF split D=%d n_joint=%d", D, n_joint);
  BEAST_REQUIRE(row_elems >= 1, "row_elems must be >= 1");
  BEAST_REQUIRE(!tokens_out || (w_min && w_max && vocab >= 2), "quantisation needs w_min/w_max and vocab >= 2");
  BEAST_REQUIRE(B >= 0, "batch size B=%lld must be >= 0", (long long)B);
  if (B == 0) return BEAST_OK;
  EncArgs a{};
  a.traj = traj; a.B = B; a.sb = sb; a.st = st; a.sd = sd; a.row_elems = row_elems; a.vocab = vocab;
  a.phases = debug_phases(); a.dof_src = dof_src; a.proj = proj; a.w_min = w_min; a.w_max = w_max;
  a.tok_offset = tok_offset; a.params_out = params_out; a.tokens_out = reinterpret_cast<long long*>(tokens_out);
  Queue q;
  if (const int rc = queue_of(stream, q, "beast_encode_f32")) return rc;
  return launch_encode(a, T, D, n_joint, N, q);
}

extern "C" int beast_encode_list_f32(const float* const* traj_list, int nbatch, int64_t rows_per_batch, int T,
                                     int row_elems, int D, int n_joint, const int32_t* dof_src, const float* proj,
                                     int N, float* params_out, void* stream) {
  BEAST_REQUIRE(traj_list && dof_src && proj && params_out, "beast_encode_list_f32: null pointer");
  BEAST_REQUIRE(nbatch >= 0 && rows_per_batch >= 0, "beast_encode_list_f32: negative sizes");
  BEAST_REQUIRE(rows_per_batch % 8 == 0, "rows_per_batch=%lld is not a multiple of 8", (long long)rows_per_batch);
  BEAST_REQUIRE(T >= 1 && T <= MAX_T, "seq_len T=%d outside [1, %d]", T, MAX_T);
  BEAST_REQUIRE(N >= 1 && N <= MAX_N, "num_basis N=%d outside [1, %d]", N, MAX_N);
  BEAST_REQUIRE(D >= 1 && D <= MAX_D && n_joint >= 0 && n_joint <= D, "bad DoF split D=%d n_joint=%d", D, n_joint);
  BEAST_REQUIRE(row_elems >= 1 && ((int64_t)T * row_elems) % 4 == 0,
                "beast_encode_list_f32: T*row_elems must be a multiple of 4");
  if (nbatch == 0 || rows_per_batch == 0) return BEAST_OK;
  EncArgs a{};
  a.traj = nullptr; a.traj_list = traj_list; a.list_rows = rows_per_batch;
  a.B = (int64_t)nbatch * rows_per_batch; a.sb = (int64_t)T * row_elems; a.st = row_elems; a.sd = 1;
  a.row_elems = row_elems; a.vocab = 0; a.phases = debug_phases(); a.dof_src = dof_src; a.proj = proj;
  a.params_out = params_out;
  Queue q;
  if (const int rc = queue_of(stream, q, "beast_encode_list_f32")) return rc;
  return launch_encode(a, T, D, n_joint, N, q);
}

extern "C" int beast_reconstruct_f32(const int64_t* tokens, int64_t B, int D, int n_joint, int N, int vocab,
                                     int64_t tok_offset, const float* w_min, const float* w_max,
                                     const float* basis, int64_t basis_sb, int T_out, const int32_t* dof_dst,
                                     int num_dof_out, const float* init_p, int64_t init_p_sb,
                                     const int32_t* init_p_src, float* params_out, float* pos_out,
                                     const float* ntokens, void* stream) {
  BEAST_REQUIRE((tokens || ntokens) && w_min && w_max, "beast_reconstruct_f32: null input pointer");
  BEAST_REQUIRE(params_out || pos_out, "beast_reconstruct_f32: no output requested");
  BEAST_REQUIRE(N >= 1 && N <= MAX_N, "num_basis N=%d outside [1, %d]", N, MAX_N);
  BEAST_REQUIRE(D >= 1 && D <= MAX_D && n_joint >= 0 && n_joint <= D, "bad DoF split D=%d n_joint=%d", D, n_joint);
  BEAST_REQUIRE(vocab >= 2 || ntokens, "vocab must be >= 2");
  BEAST_REQUIRE(!pos_out || (basis && dof_dst && T_out >= 1 && T_out <= 4096 && num_dof_out >= D &&
                             num_dof_out <= 4096),
                "reconstruct: need basis, dof_dst, 1 <= T_out <= 4096, D <= num_dof_out <= 4096");
  BEAST_REQUIRE(!init_p || init_p_src, "init_p needs init_p_src");
  BEAST_REQUIRE(B >= 0, "batch size B=%lld must be >= 0", (long long)B);
  if (B == 0) return BEAST_OK;
  RecArgs a{};
  a.tokens = reinterpret_cast<const long long*>(tokens); a.ntokens = ntokens; a.B = B; a.tok_offset = tok_offset;
  a.basis_sb = basis_sb; a.init_p_sb = init_p_sb; a.vocab = vocab; a.Tout = pos_out ? T_out : 1;
  a.ndo = pos_out ? num_dof_out : 1; a.phases = debug_phases(); a.w_min = w_min; a.w_max = w_max; a.basis = basis;
  a.dof_dst = dof_dst; a.init_p = init_p; a.init_p_src = init_p_src; a.params_out = params_out; a.pos_out = pos_out;
  const bool shared = (basis_sb == 0);
  Queue q;
  if (const int rc = queue_of(stream, q, "beast_reconstruct_f32")) return rc;
  return launch_reconstruct<8>(a, D, n_joint, N, shared, q);
}

extern "C" int beast_roundtrip_stats_f32(const float* traj, int64_t B, int T, int64_t sb, int64_t st, int64_t sd,
                                         int row_elems, int D, int n_joint, const int32_t* dof_src,
                                         const float* proj, const float* basis, int N, const float* w_min,
                                         const float* w_max, int vocab, int64_t tok_offset, int64_t* tokens_out,
                                         float* stats_out, uint32_t* clip_counts, void* stream) {
  BEAST_REQUIRE(traj && dof_src && proj && basis && w_min && w_max,
                "beast_roundtrip_stats_f32: null input pointer");
  BEAST_REQUIRE(stats_out, "beast_roundtrip_stats_f32: stats_out is required");
  BEAST_REQUIRE(T >= 1 && T <= MAX_T, "seq_len T=%d outside [1, %d]", T, MAX_T);
  BEAST_REQUIRE(N >= 1 && N <= MAX_N, "num_basis N=%d outside [1, %d]", N, MAX_N);
  BEAST_REQUIRE(D >= 1 && D <= MAX_D && n_joint >= 0 && n_joint <= D, "bad DoF split D=%d n_joint=%d", D, n_joint);
  BEAST_REQUIRE(row_elems >= 1, "row_elems must be >= 1");
  BEAST_REQUIRE(vocab >= 2, "vocab must be >= 2");
  BEAST_REQUIRE(B >= 0, "batch size B=%lld must be >= 0", (long long)B);
  if (B == 0) return BEAST_OK;
  RtArgs a{};
  a.sb = sb; a.st = st; a.sd = sd; a.tok_offset = tok_offset; a.dof_src = dof_src; a.proj = proj; a.basis = basis;
  a.w_min = w_min; a.w_max = w_max; a.tokens_out = reinterpret_cast<long long*>(tokens_out); a.stats_out = stats_out;
  a.clip = clip_counts; a.row_elems = row_elems; a.vocab = vocab; a.D = D; a.nj = n_joint; a.N = N; a.T = T;
  // the positions beast_reconstruct_f32 gives for these tokens (num_dof_out = D): MFMA order or the rows kernel's
  a.lut_n = vocab <= LUT_MAX ? vocab : 0;
  a.seq = rec_mfma_fits<8>(T, D, N, D, a.lut_n) ? 0 : 1;
  Queue q;
  int rc = queue_of(stream, q, "beast_roundtrip_stats_f32");
  if (rc) return rc;
  const bool contiguous = sd == 1 && st == row_elems && sb == (int64_t)T * row_elems && row_elems == D &&
                          (((uintptr_t)traj) & 15) == 0;
  if (contiguous && !g_generic_only && T == 50 && N == 10 &&
      with_fixed_shape<false>(D, n_joint, false, rc, [&](auto sh) {
        return launch_roundtrip_fixed<decltype(sh)>(traj, B, a, q);
      }))
    return rc;
  // runtime shape: the most trajectories per tile whose LDS layout fits (one at T = 256, D = 64, where
  // the dequantise LUT may have to go: its quotients are then divided on the spot)
  const int nkinds = n_joint < D ? 2 : 1;
  int W = 16;
  while (W > 1 && rt_smem(T, D, N, nkinds, W, a.lut_n).total > 160 * 1024) W >>= 1;
  if (rt_smem(T, D, N, nkinds, W, a.lut_n).total > 160 * 1024) a.lut_n = 0;
  return launch_roundtrip<DynShape, 0>(traj, B, a, W, q);
}

#ifdef BEAST_STAMPS
extern "C" int beast_stamps_read(unsigned long long* out) {   // [2][16][16]
  return hipMemcpyFromSymbol(out, HIP_SYMBOL(g_stamps), sizeof(g_stamps)) == hipSuccess ? 0 : -2;
}

extern "C" int beast_bstamps_read(unsigned long long* out) {   // [2][4096][4]
  return hipMemcpyFromSymbol(out, HIP_SYMBOL(g_bstamps), sizeof(g_bstamps)) == hipSuccess ? 0 : -2;
}
#endif

extern "C" int beast_set_option(int option, int value) {
  if (option == BEAST_OPT_GENERIC_KERNELS) {
    g_generic_only = value != 0;
    return BEAST_OK;
  }
  if (option == BEAST_OPT_BLOCK_WAVES) {
    BEAST_REQUIRE(value == 0 || value == 4 || value == 7 || value == 8,
                  "BEAST_OPT_BLOCK_WAVES: %d is not 0, 4, 7 or 8", value);
    g_block_waves = value;
    return BEAST_OK;
  }
  if (option == BEAST_OPT_MERGE_LDS_MIN) {
    BEAST_REQUIRE(value >= 0, "BEAST_OPT_MERGE_LDS_MIN: %d < 0", value);
    beast::g_merge_lds_min = value;
    return BEAST_OK;
  }
  if (option == BEAST_OPT_BPE_ENCODE_MODE) {
    BEAST_REQUIRE(value >= 0 && value <= 3, "BEAST_OPT_BPE_ENCODE_MODE: %d is not 0..3", value);
    beast::g_bpe_encode_mode = value;
    return BEAST_OK;
  }
  if (option == BEAST_OPT_BPE_DEDUP_KEY_BITS) {
    BEAST_REQUIRE(value >= 2 && value <= 64, "BEAST_OPT_BPE_DEDUP_KEY_BITS: %d is not 2..64", value);
    beast::g_bpe_dedup_key_bits = value;
    return BEAST_OK;
  }
  if (option == BEAST_OPT_BPE_TRAIN_HOST_LOOP) {
    BEAST_REQUIRE(value >= 0 && value <= 2, "BEAST_OPT_BPE_TRAIN_HOST_LOOP: %d is not 0..2", value);
    beast::g_bpe_train_host = value;
    return BEAST_OK;
  }
  BEAST_REQUIRE(option != BEAST_OPT_LAST_CODEC_LAUNCH, "BEAST_OPT_LAST_CODEC_LAUNCH is read-only");
  BEAST_REQUIRE(option != BEAST_OPT_LAST_LAUNCH_GRID, "BEAST_OPT_LAST_LAUNCH_GRID is read-only");
  BEAST_REQUIRE(false, "unknown option %d", option);
  return BEAST_E_INVALID;
}

extern "C" int beast_get_option(int option) {
  if (option == BEAST_OPT_GENERIC_KERNELS) return g_generic_only ? 1 : 0;
  if (option == BEAST_OPT_BLOCK_WAVES) return g_block_waves;
  if (option == BEAST_OPT_MERGE_LDS_MIN) return (int)beast::g_merge_lds_min;
  if (option == BEAST_OPT_BPE_ENCODE_MODE) return beast::g_bpe_encode_mode;
  if (option == BEAST_OPT_BPE_DEDUP_KEY_BITS) return beast::g_bpe_dedup_key_bits;
  if (option == BEAST_OPT_BPE_TRAIN_HOST_LOOP) return beast::g_bpe_train_host;
  if (option == BEAST_OPT_LAST_CODEC_LAUNCH) return g_last_launch.load(std::memory_order_relaxed);
  if (option == BEAST_OPT_LAST_LAUNCH_GRID) return (int)beast::g_last_launch_grid.load(std::memory_order_relaxed);
  beast::set_error("unknown option %d", option);
  return BEAST_E_INVALID;
}

