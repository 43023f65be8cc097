// Byte-level BPE inference, first layer (bpe_codec.hip): what the encode and decode kernels
// share.  Constants, the per-row status codes, the merge maps and their probe, the encode argument
// block, the phase stamps of the tools builds, and the inference row pre-tokeniser.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

#include "common.h"
#include "pretok.h"

namespace {

constexpr uint32_t EMPTY_KEY = 0xFFFFFFFFu;
using beast_pt::CLS_OTHER;
using beast_pt::regex_word;
using beast_pt::wave_excl_scan;
using beast_pt::wave_sync;
using beast_pt::word_starts;
constexpr int WAVES = 4;            // rows in flight per workgroup (decode)
constexpr int ENC_MAX_WAVES = 16;   // encode: as many rows per workgroup as the LDS holds, up to 16
constexpr int BLOCK = 64 * WAVES;
constexpr int MAX_SPECIAL = 64, MAX_SPECIAL_LEN = 64;
constexpr int RM_PER = 8;           // symbol positions per lane of the round merge (rows <= 512 symbols)
constexpr int RM_NARROW = 6;        // ... in the narrow kernel (rows <= 384 symbols)
constexpr uint32_t RK_NONE = 0xFFFFFFFFu;
constexpr int LDS_MAP_MAX_LOG2 = 13;   // stage maps of <= 8192 slots (64 KiB + rank table)
constexpr size_t LDS_BUDGET = 160 * 1024;
constexpr size_t STATIC_LDS = 2048;         // k_bpe_encode's byte -> id table and LUT head   // gfx950: one workgroup may declare all 160 KiB

// encode status per row (host maps them to the reference's exceptions)
constexpr int ST_OK = 0, ST_BELOW_MIN = 1, ST_ABOVE_MAX = 2, ST_NOT_UNICODE = 3, ST_SURROGATE = 4,
              ST_NO_CLASS = 5, ST_TOO_LONG = 6;

#ifdef BPE_STAMPS
// tools/codec/bpe_encode_phases.py only (the product compiles these out): per row r < 4096,
// s_memrealtime (100 MHz) at each phase boundary [0, 7), then merge rounds, byte symbols, words
// and the workgroup's map-staging start / end -- plain stores by lane 0, one slot per row, so
// the stamps add no atomics and no shared address
constexpr int BPE_RS = 4096;
__device__ unsigned long long g_bpe_rs[BPE_RS][12];
// k_bpe_words' merge tasks per row wave: [0..3) time in mid / short / tiny tasks, [3..6) their counts
__device__ unsigned long long g_bpe_wt[BPE_RS][8];
#define BPE_STAMP(k)                                                                          \
  do {                                                                                        \
    if (lane == 0 && r < BPE_RS) g_bpe_rs[r][k] = __builtin_amdgcn_s_memrealtime();          \
  } while (0)
#else
#define BPE_STAMP(k) do { } while (0)
#endif

__host__ __device__ inline size_t al16(size_t x) { return (x + 15) & ~size_t(15); }

// ------------------------------------------------------------- merge map --
// layout: kv uint2[cap] (key a << 16 | b, EMPTY_KEY = free; value (rank + 1) << 16 | new_id, 0 =
// unset) | rank2new u16[n].  Key and value side by side: a probe is one 8-byte load.
struct MergeMap {
  const uint2* kv;
  const uint16_t* rank2new;
  int log2cap;
};

__device__ __forceinline__ uint32_t mm_hash(uint32_t key, int log2cap) {
  return (key * 0x9E3779B1u) >> (32 - log2cap);
}

// k_bpe_words' merge map: two-choice bucketed cuckoo hashing, 1 << log2b buckets of two (key,
// value) slots (16 bytes), every key in one of its two buckets -- a lookup is exactly two 16-byte
// reads, one LDS round trip, where a linear-probe chain is a loop whose longest lane sets the
// wave's pace.  Built on the host (beast_bpe_wordmap_build_host); same key / value encoding as
// the merge map above.
struct WordMap {
  const uint4* b;
  int log2b;
};
__host__ __device__ __forceinline__ uint32_t wm_h1(uint32_t key, int log2b) { return (key * 0x9E3779B1u) >> (32 - log2b); }
__host__ __device__ __forceinline__ uint32_t wm_h2(uint32_t key, int log2b) {
  return ((key ^ 0x5BD1E995u) * 0x85EBCA77u) >> (32 - log2b);
}

__global__ void k_mergemap_clear(uint2* __restrict__ kv, int cap) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < cap) kv[i] = make_uint2(EMPTY_KEY, 0u);
}

__global__ void k_mergemap_build(const int32_t* __restrict__ ma, const int32_t* __restrict__ mb,
                                 const int32_t* __restrict__ mnew, int n, uint2* __restrict__ kv,
                                 uint16_t* __restrict__ rank2new, int log2cap) {
  uint32_t* const w = reinterpret_cast<uint32_t*>(kv);   // slot h: key at 2h, value at 2h + 1
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const uint32_t key = ((uint32_t)ma[i] << 16) | (uint32_t)mb[i];
  const uint32_t mask = (1u << log2cap) - 1u;
  uint32_t h = mm_hash(key, log2cap);
  while (true) {
    const uint32_t prev = atomicCAS(&w[2 * h], EMPTY_KEY, key);
    if (prev == EMPTY_KEY || prev == key) break;
    h = (h + 1) & mask;
  }
  atomicMax(&w[2 * h + 1], ((uint32_t)(i + 1) << 16) | (uint32_t)mnew[i]);   // later rank wins
  rank2new[i] = (uint16_t)mnew[i];
}

// rank of pair (a, b), or -1; *new_id set when found
template <class Map>
__device__ __forceinline__ int mm_find(const Map& m, int a, int b, int& new_id) {
  const uint32_t key = ((uint32_t)a << 16) | (uint32_t)b;
  const uint32_t mask = (1u << m.log2cap) - 1u;
  uint32_t h = mm_hash(key, m.log2cap);
  while (true) {
    const uint2 e = m.kv[h];
    if (e.x == key) {
      new_id = (int)(e.y & 0xFFFFu);
      return (int)(e.y >> 16) - 1;
    }
    if (e.x == EMPTY_KEY) return -1;
    h = (h + 1) & mask;
  }
}

struct EncArgs {
  const long long* tok;
  const int64_t* row_off;
  int64_t n_rows;
  long long min_tok;
  long long max_span;         // largest allowed shifted value, < 0: unbounded
  const uint8_t* lut;
  int lut_n;
  const int32_t* byte2id;     // [256], -1: byte-level char not in the vocab
  MergeMap map;               // in HBM
  int n_merges;
  int map_in_lds;             // host choice: k_bpe_encode<true> stages the map
  int heap_merge;             // BEAST_OPT_BPE_ENCODE_MODE bit 0: HF's heap per word instead of rounds
  const int32_t* spec_cps;    // [n_spec][MAX_SPECIAL_LEN]
  const int32_t* spec_len;
  const int32_t* spec_id;
  int n_spec;
  int unk_id;                 // model unk token id, -1: unknown chars are dropped
  int fuse_unk;
  int Lc, S;
  int32_t* out_ids;
  int64_t out_stride;
  int32_t* out_len;
  int32_t* status;
};

// ------------------------------------------------------- row pre-tokeniser --
// The reference's range checks on a row's shifted values, one flag each, accumulated per lane by
// pretok_row's code-point functor and reported in the reference's order (:181-192: below-min first).
struct RangeFlags {
  int below = 0, above = 0, notuni = 0, surr = 0, nocls = 0;
};
__device__ __forceinline__ int range_status(const RangeFlags& f) {   // wave-uniform
  if (__any(f.below)) return ST_BELOW_MIN;
  if (__any(f.above)) return ST_ABOVE_MAX;
  if (__any(f.notuni)) return ST_NOT_UNICODE;
  if (__any(f.surr)) return ST_SURROGATE;
  if (__any(f.nocls)) return ST_NO_CLASS;
  return ST_OK;
}

// One row's pre-tokenisation into its LDS image L (one wave; EncLds of k_bpe_encode or DwRow of
// k_bpe_words), all by csrc/pretok.h:
//   1. code points, range checks, classes (code points < 256 from the workgroup's LDS copy of the
//      LUT) and UTF-8 symbol offsets -- stage_row, the first 256 loads in flight at once;
//   2. without special tokens, the regex word starts: L.wcp [n + 1], L.misc[0] = words.  L.wcp
//      is regex_ends' scratch until word_starts; L.e holds the word ends in between -- in EncLds
//      it is wcnt, which aliases the round merge's wmin, both live only later; L.wspec is
//      k_bpe_encode's per-word special-token id (set to -1) and null in k_bpe_words.  With special
//      tokens (k_bpe_encode only) the caller splits the row itself afterwards;
//   3. byte symbols as vocab ids in L.c: int32_t keeps a missing byte's -1, uint16_t narrows it
//      to SYM_NONE.
// ENDS: the word ends by regex_ends (k_bpe_words) or by regex_word from every position
// (k_bpe_encode: regex_ends there costs the kernel 16 to 24 more bytes of scratch, it is at its
// 128 VGPRs; DESIGN.md, "Where the BPE device code lives").
// Returns the row's status (wave-uniform; the image is complete only for ST_OK); n: its code points.
template <bool ENDS, class Row>
__device__ __forceinline__ int pretok_row(const EncArgs& a, const Row& L, int64_t r, int lane, const int32_t* s_b2i,
                                          const uint8_t* s_lut, int& n) {
  BPE_STAMP(0);
  const int64_t r0 = a.row_off[r];
  n = (int)(a.row_off[r + 1] - r0);
  if (n > a.Lc) return ST_TOO_LONG;
  RangeFlags f;
  const int nsym = beast_pt::stage_row<4>(a.tok + r0, n, lane, L.symoff, [&](int i, long long t) {
    const long long v = t - a.min_tok;
    f.below |= v < 0;
    f.above |= (a.max_span >= 0 && v > a.max_span);
    f.notuni |= v > 0x10FFFF;
    f.surr |= (v >= 0xD800 && v <= 0xDFFF);
    f.nocls |= v >= a.lut_n;
    const int cp = (int)((v < 0 || v > 0x10FFFF) ? 0 : v);
    L.cps[i] = cp;
    L.cls[i] = (uint8_t)beast_pt::class_of(cp, s_lut, a.lut, a.lut_n);
    return beast_pt::utf8_len(cp);
  });
  BPE_STAMP(1);
  const int st = range_status(f);
  if (st != ST_OK) return st;
  if (nsym > a.S) return ST_TOO_LONG;   // host sizes S from the code-point bound; guard anyway
  wave_sync();
  BPE_STAMP(2);
  if (a.n_spec == 0) {
    if constexpr (ENDS) {
      beast_pt::regex_ends(L.cps, L.cls, L.wcp, L.e, n, lane);
    } else {   // word_starts' first wave_sync publishes e
      for (int i = lane; i < n; i += 64) L.e[i] = regex_word(L.cps, L.cls, i, n);
    }
    word_starts(L.e, L.vis, L.wcp, L.wspec, L.misc, n, lane);
  }
  BPE_STAMP(3);
  for (int i = lane; i < n; i += 64) beast_pt::emit_utf8_ids(L.cps[i], s_b2i, L.c + L.symoff[i]);
  wave_sync();
  return ST_OK;
}

}  // namespace
