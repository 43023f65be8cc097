// Device primitives of the codec kernels (codec.hip's first layer): nothing here knows an argument
// block (EncArgs, RecArgs, ...).  Store policies and LDS-DMA staging, the cycle stamps, the problem
// geometry (Geom / Shape / Dims / VShape, tile_col), and the shared kernel arithmetic: helpers that
// are the one definition of what k_encode, k_encode_v, k_reconstruct, k_reconstruct_v,
// k_reconstruct_rows and k_roundtrip must compute identically.
#pragma once

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <type_traits>

#include "common.h"

namespace {

constexpr int NTHREADS = 256;
constexpr int NWAVES = NTHREADS / 64;

typedef float float4_t __attribute__((ext_vector_type(4)));

__host__ __device__ constexpr int round_up(int x, int m) { return (x + m - 1) / m * m; }

// x / d for x * d < 2^32 by multiply-high (d uniform, m = ceil(2^32 / d)).
struct FastDiv {
  uint32_t d, m;
};
inline FastDiv make_fd(uint32_t d) {
  FastDiv f;
  f.d = d;
  f.m = d <= 1 ? 0u : (uint32_t)((0x100000000ull + d - 1) / d);
  return f;
}
__device__ __forceinline__ uint32_t fdiv(uint32_t x, FastDiv f) { return f.d <= 1 ? x : __umulhi(x, f.m); }

// ------------------------------------------------------------- staging --
// 16-byte output store with a cache policy SP: 0 plain (write-back L2), 1 nt, 2 sc1
// (write-through).  A dependent kernel boundary pays for the bytes its predecessor leaves
// dirty in L2 (MI355X_MICROARCH.md, "boundary": + B / 6 TB/s); in the latency regime (a tile or
// two per CU, the bench's B = 4,096) write-through stores move that write-back inside the
// kernel, under the other waves' work: encode -> reconstruct step 12.2 -> 10.5 us.  Bulk
// launches keep write-back stores (write-through encode at B = 262,144: 227 -> 311 us).
// BEAST_LAT_SP overrides the latency-regime policy (measurements).
#ifndef BEAST_LAT_SP
#define BEAST_LAT_SP 2
#endif
constexpr int LAT_SP = BEAST_LAT_SP;
typedef unsigned u32x4_t __attribute__((ext_vector_type(4)));
template <int SP>
__device__ __forceinline__ void st16(void* p, u32x4_t v) {
  if constexpr (SP == 1) {
    __builtin_nontemporal_store(v, static_cast<u32x4_t*>(p));
  } else if constexpr (SP == 2) {
    // vector store, write-through to memory (vmcnt counts it like any store; s_nop 1 covers
    // the store-data hazard of an inline-asm 128-bit store)
    asm volatile("global_store_dwordx4 %0, %1, off sc1\n\ts_nop 1" ::"v"(p), "v"(v) : "memory");
  } else {
    *static_cast<u32x4_t*>(p) = v;
  }
}
template <int SP>
__device__ __forceinline__ void st16(void* p, float4 v) {
  st16<SP>(p, u32x4_t{__float_as_uint(v.x), __float_as_uint(v.y), __float_as_uint(v.z), __float_as_uint(v.w)});
}
template <int SP>
__device__ __forceinline__ void st16(void* p, long long a, long long b) {
  st16<SP>(p, u32x4_t{(unsigned)a, (unsigned)((unsigned long long)a >> 32), (unsigned)b,
                      (unsigned)((unsigned long long)b >> 32)});
}

// LDS -> global, float count
template <int NT = NTHREADS, int SP = 0>
__device__ __forceinline__ void store_out(float* __restrict__ dst, const float* __restrict__ src, int count) {
  if ((((uintptr_t)src | (uintptr_t)dst) & 15) == 0) {
    const int n4 = count >> 2;
    const float4* s4 = reinterpret_cast<const float4*>(src);
    float4* d4 = reinterpret_cast<float4*>(dst);
    for (int i = threadIdx.x; i < n4; i += NT) st16<SP>(d4 + i, s4[i]);
    for (int i = (n4 << 2) + threadIdx.x; i < count; i += NT) dst[i] = src[i];
  } else {
    for (int i = threadIdx.x; i < count; i += NT) dst[i] = src[i];
  }
}

// LDS-DMA (global_load_lds): HBM -> LDS with no VGPR round trip, so every load of a stage
// is in flight at once and one vmcnt wait (the next __syncthreads) retires them all.  A
// wave-instruction writes 64 consecutive slots from a wave-uniform base: destinations are
// padded to whole wave-instructions, sources past the end are clamped to the last element.
typedef __attribute__((address_space(3))) void lds_void;

template <int NT = NTHREADS>
__device__ __forceinline__ void dma16(void* lds, const void* g, int n16) {
  const int tid = threadIdx.x, wb = tid & ~63;
  for (int base = 0; base < n16; base += NT) {
    if (base + wb < n16)
      __builtin_amdgcn_global_load_lds(static_cast<const uint4*>(g) + min(base + tid, n16 - 1),
                                       (lds_void*)(static_cast<uint4*>(lds) + base + wb), 16, 0, 0);
  }
}

template <int NT = NTHREADS>
__device__ __forceinline__ void dma4(void* lds, const void* g, int n) {
  const int tid = threadIdx.x, wb = tid & ~63;
  for (int base = 0; base < n; base += NT) {
    if (base + wb < n)
      __builtin_amdgcn_global_load_lds(static_cast<const uint32_t*>(g) + min(base + tid, n - 1),
                                       (lds_void*)(static_cast<uint32_t*>(lds) + base + wb), 4, 0, 0);
  }
}

// Keeps a lane-only value that was computed before the tile barrier in its register: without it
// the compiler sinks the arithmetic back behind the barrier, next to its use.
template <class V>
__device__ __forceinline__ void pin(V& v) {
  asm volatile("" : "+v"(v));
}

// rows [b0, b0 + tbt) of a [B][per] array of esz-byte elements HBM -> LDS by DMA
template <int NT = NTHREADS>
__device__ __forceinline__ void stage_rows(void* lds, const void* base, int64_t B, int esz, int64_t b0, int per,
                                           int tbt) {
  const int nb = (int)min<int64_t>(B - b0, tbt);
  const char* src = static_cast<const char*>(base) + b0 * per * esz;
  const int bytes = nb * per * esz;
  if ((bytes & 15) == 0 && (((uintptr_t)src) & 15) == 0) dma16<NT>(lds, src, bytes >> 4);
  else dma4<NT>(lds, src, bytes >> 2);
}

// ------------------------------------------------- shared kernel arithmetic --
// The single definition of what the kernels must agree on bit for bit (tokens of k_roundtrip equal
// k_encode_v's equal k_encode's, positions likewise); the lane quantiser is beast::quantize_bins.

using beast::wave_sync;   // common.h: a wave's LDS writes become visible to its other lanes

// Dequantise LUT: lut[t] = t / (vocab - 1), IEEE-divided once per workgroup (nt threads).
__device__ __forceinline__ void lut_fill(float* lut, int lut_n, float vm1, int nt) {
  for (int t = threadIdx.x; t < lut_n; t += nt) lut[t] = __fdiv_rn((float)t, vm1);
}

// A token as ATen's .to(float) sees it.
__device__ __forceinline__ float tok_f32(long long t) { return (float)t; }

// The quotients t / (vocab - 1) of a lane's NQ slots (tokens, offset removed) through the
// LUT: every entry is requested before any is used (one LDS round trip); tokens outside
// [0, lut_n) (rare) take the IEEE division behind one branch for all slots.
// beast::dequantize_quotient turns a quotient into the coefficient.
template <int NQ, class Tok>
__device__ __forceinline__ void lut_quotients(const Tok (&t)[NQ], const float* lut, int lut_n, float vm1,
                                              float (&nrm)[NQ]) {
  using U = std::make_unsigned_t<Tok>;
  bool far = false;
#pragma unroll
  for (int u = 0; u < NQ; ++u) {
    const bool in = (U)t[u] < (U)lut_n;   // 0 <= t < lut_n
    far = far | !in;
    nrm[u] = lut[in ? (int)t[u] : 0];
  }
  if (far) {
#pragma unroll
    for (int u = 0; u < NQ; ++u)
      if (!((U)t[u] < (U)lut_n)) nrm[u] = __fdiv_rn(tok_f32(t[u]), vm1);
  }
}

// The same quotients without a table: beast::exact_quotient (three VALU) for tokens in [0, qn),
// where qn is beast::EXACT_QUOTIENT_MAX while vocab <= EXACT_QUOTIENT_MAX and 0 for larger
// vocabularies; r = RN(1 / vm1) comes from the host.  Every other token (negative, >= qn: tokens
// are user data) takes the IEEE division behind one branch for all slots, so the bits are
// lut_quotients' for every input.
template <int NQ, class Tok>
__device__ __forceinline__ void fma_quotients(const Tok (&t)[NQ], int qn, float vm1, float r, float (&nrm)[NQ]) {
  using U = std::make_unsigned_t<Tok>;
  bool far = false;
#pragma unroll
  for (int u = 0; u < NQ; ++u) {
    far = far | !((U)t[u] < (U)qn);   // 0 <= t < qn: the low dword is the token
    nrm[u] = beast::exact_quotient((float)(int)t[u], vm1, r);
  }
  if (far) {
#pragma unroll
    for (int u = 0; u < NQ; ++u)
      if (!((U)t[u] < (U)qn)) nrm[u] = __fdiv_rn(tok_f32(t[u]), vm1);
  }
}

// The accumulators of an MFMA lane (C/D map: rows n = 4 lk + r, r < 4) as quantiser slots: four,
// or three (Q3, N <= 10): rows 4 lk + 3 of lanes lk < 2 move into slot 2 of lanes lk >= 2 (one
// v_permlane32_swap), whose own rows there are padding, so 192 slots serve the 140 values.
template <bool Q3>
__device__ __forceinline__ int slot_row(int lk, int u) {   // the row n of slot u (u < 4, so | adds)
  return (!Q3 || u < 2 || lk < 2) ? (4 * lk | u) : 4 * (lk - 2) + 3;
}
template <bool Q3, int NQ>
__device__ __forceinline__ void slot_values(const float (&p4)[4], float (&p)[NQ]) {
  if constexpr (Q3) {   // slot 2: lanes lk < 2 keep their row 4 lk + 2, lanes lk >= 2 take row 4 (lk - 2) + 3 of lane - 32
    const auto sw = __builtin_amdgcn_permlane32_swap(__float_as_uint(p4[2]), __float_as_uint(p4[3]), false, false);
    p[0] = p4[0]; p[1] = p4[1]; p[2] = __uint_as_float(sw[0]);
  } else {
#pragma unroll
    for (int r = 0; r < 4; ++r) p[r] = p4[r];
  }
}

// A wave copies N16 16-byte units of its private LDS image (floats or int64) out, store policy SP.
template <int SP, int N16, class T>
__device__ __forceinline__ void wave_copy_out(T* g, const T* img, int lane) {
  constexpr int K = 16 / sizeof(T);
#pragma unroll
  for (int u = 0; u < (N16 + 63) / 64; ++u) {
    const int i = u * 64 + lane;
    if (i < N16) st16<SP>(g + K * i, *reinterpret_cast<const u32x4_t*>(img + K * i));
  }
}

// In-kernel cycle stamps (tools/stamps builds this file with -DBEAST_STAMPS; the product
// library compiles them out): s_memtime of lane 0 of every wave of workgroup 0 at the
// phase boundaries of its first tile.
#ifdef BEAST_STAMPS
__device__ unsigned long long g_stamps[2][16][16];   // [kernel][wave of a workgroup (<= 16)][stamp]
#define STAMP(k, i)                                                                              \
  do {                                                                                           \
    if (blockIdx.x == 0 && (threadIdx.x & 63) == 0) g_stamps[k][threadIdx.x >> 6][i] = __builtin_amdgcn_s_memtime(); \
  } while (0)
// Per-workgroup lifetime (first 4096 workgroups): s_memrealtime (100 MHz, chip-wide) at
// entry and after the drain, and HW_ID / XCC_ID of the wave.
__device__ unsigned long long g_bstamps[2][4096][4];
#define BSTAMP(k, i)                                                                             \
  do {                                                                                           \
    if (threadIdx.x == 0 && blockIdx.x < 4096) {                                                 \
      g_bstamps[k][blockIdx.x][i] = __builtin_amdgcn_s_memrealtime();                            \
      if (i == 0)                                                                                \
        g_bstamps[k][blockIdx.x][2] = ((unsigned long long)__builtin_amdgcn_s_getreg(0xF814) << 32) | \
                                      (unsigned)__builtin_amdgcn_s_getreg(0xF804);               \
    }                                                                                            \
  } while (0)
#else
#define STAMP(k, i) do { } while (0)
#define BSTAMP(k, i) do { } while (0)
#endif

// -------------------------------------------------------------- geometry --
struct Geom {
  int D, nj, N, T, Tp, per;   // per = N * D
  int nq0, nq;                // column tiles of kind 0, of both kinds
  FastDiv fd_nj, fd_ng, fd_per, fd_N, fd_D, fd_nq;
};

template <int TBT>
inline Geom make_geom(int D, int nj, int N, int T) {
  Geom g;
  g.D = D; g.nj = nj; g.N = N; g.T = T; g.Tp = round_up(T, 4); g.per = N * D;
  const int ng = D - nj;
  g.nq0 = (TBT * nj + 15) / 16;
  g.nq = g.nq0 + (TBT * ng + 15) / 16;
  g.fd_nj = make_fd(std::max(nj, 1));
  g.fd_ng = make_fd(std::max(ng, 1));
  g.fd_per = make_fd(g.per);
  g.fd_N = make_fd(N);
  g.fd_D = make_fd(D);
  g.fd_nq = make_fd(std::max(g.nq, 1));
  return g;
}

// Compile-time problem shape.  A zero field is read from the runtime Geom instead; the
// BEAST defaults (N = 10 basis functions, T = 50 steps, 7 or 14 DoF with or without the
// two gripper DoF) get fully specialised kernels in which every index is a constant.
template <int SD, int SNJ, int SN, int ST, int SDL, int SW = NWAVES>
struct Shape {
  static constexpr int D = SD, NJ = SNJ, N = SN, T = ST, DL = SDL;
  static constexpr int W = SW;   // waves per workgroup: one per MFMA column tile of a full tile
  static constexpr bool fixed = SD > 0;
};
using DynShape = Shape<0, 0, 0, 0, 0>;

template <class S>
struct Dims {   // the shape, constant-folded where S fixes it
  int D, nj, ng, N, T, Tp, per;
  __device__ __forceinline__ Dims(const Geom& g)
      : D(S::D ? S::D : g.D), nj(S::fixed ? S::NJ : g.nj), ng(D - nj), N(S::N ? S::N : g.N),
        T(S::T ? S::T : g.T), Tp(S::T ? round_up(S::T, 4) : g.Tp), per(N * D) {}
};

template <class S>
__device__ __forceinline__ uint32_t div_by(uint32_t x, int dconst, const FastDiv& f) {
  return S::fixed ? x / (uint32_t)dconst : fdiv(x, f);
}

// MFMA column (trajectory j, DoF d) of tile q (wave-uniform) for lane column lc; valid =
// inside the tile set.
template <int TBT, class S>
__device__ __forceinline__ void tile_col(const Geom& g, const Dims<S>& m, int q, int lc, int& j, int& d, int& kind,
                                         bool& valid) {
  const int nq0 = (TBT * m.nj + 15) / 16;
  const int k0 = q < nq0 ? 0 : 1;
  const int dk = k0 ? m.ng : m.nj;
  const int c = (q - (k0 ? nq0 : 0)) * 16 + lc;
  valid = c < TBT * dk;
  const uint32_t cc = valid ? c : TBT * dk - 1;
  const uint32_t jj = k0 ? div_by<S>(cc, m.ng > 0 ? m.ng : 1, g.fd_ng) : div_by<S>(cc, m.nj > 0 ? m.nj : 1, g.fd_nj);
  j = (int)jj;
  d = (int)(cc - jj * dk) + (k0 ? m.nj : 0);
  kind = k0;
}

template <int TBT, class S>
__device__ __forceinline__ int n_coltiles(const Dims<S>& m) {
  return (TBT * m.nj + 15) / 16 + (TBT * m.ng + 15) / 16;
}

// Fixed shapes of the per-trajectory kernels (k_encode_v): the MFMA K-steps over Tp.
template <class S>
struct VShape {
  static_assert(S::fixed && S::T > 0 && S::DL > 0 && ((S::T * S::DL) % 4) == 0, "per-trajectory encode: fixed shape");
  static constexpr int T = S::T, DL = S::DL, D = S::D, N = S::N, DN = S::D * S::N, Tp = round_up(S::T, 4);
  static constexpr int NST = Tp / 4;   // MFMA K-steps
};

}  // namespace
