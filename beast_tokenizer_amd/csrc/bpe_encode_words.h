// Byte-level BPE inference, k_bpe_words (bpe_codec.hip): a workgroup's rows pre-tokenised, their
// distinct words merged once each, the rows' ids gathered from them.
#pragma once

#include "bpe_codec_device.h"

namespace {

// ------------------------------------------------------ encode, by words --
// (round 4) HF's BPE merges each pre-tokenised word on its own, so a row's ids are the
// concatenation of its words' ids, and a word's ids are a function of the word alone (its code
// points).  A batch of BEAST rows holds few distinct words (K5's codec sample: 302 k words,
// 77 k distinct, 5.9 byte symbols on average, 47 at most), so k_bpe_words (below) merges each
// distinct word of a workgroup's rows once instead of every word of every row.
constexpr int DW_TINY = 8;         // byte symbols of a tiny word: half a DPP row
constexpr int DW_SHORT = 16;       // ... of a short word: one 16-lane DPP row
constexpr int DW_MID = 64;         // ... of a mid word: one wave; longer -> ST_FALLBACK
constexpr int ST_FALLBACK = 7;     // the row needs k_bpe_encode
constexpr int DW_WAVES = 16;       // rows per k_bpe_words workgroup (at most)
constexpr uint32_t SYM_NONE = 0xFFFFu;

// per-row LDS of k_bpe_words
__host__ __device__ inline size_t dw_row_bytes(int Lc, int S) {
  return 3 * al16(sizeof(int32_t) * (Lc + 1)) + al16(sizeof(int32_t) * Lc) + al16(sizeof(uint16_t) * S) +
         2 * al16(Lc) + 16;
}
// the workgroup's word table (32-bit hash, first occurrence): more slots than the rows can hold words
__host__ __device__ inline int dw_ltab_log2(int Lc, int nwv) {
  int l = 4;
  while ((1ll << l) <= (long long)nwv * Lc) ++l;
  return l;
}
__host__ __device__ inline size_t dw_ltab_bytes(int Lc, int nwv) { return (size_t)8 << dw_ltab_log2(Lc, nwv); }

struct DwRow {
  int32_t* cps;      // [Lc]
  int32_t* symoff;   // [Lc + 1]
  int32_t* wcp;      // [Lc + 1]
  int32_t* e;        // [Lc]
  uint16_t* c;       // [S] byte symbols as vocab ids (SYM_NONE: not in the vocab)
  uint8_t* cls;      // [Lc]
  uint8_t* vis;      // [Lc]
  int32_t* misc;     // [4]
  static constexpr int32_t* wspec = nullptr;   // no special tokens (pretok_row, word_starts)
};

__device__ inline DwRow dw_carve(char* p, int Lc, int S) {
  DwRow R;
  auto take = [&](size_t bytes) { char* r = p; p += al16(bytes); return r; };
  R.cps = (int32_t*)take(sizeof(int32_t) * (Lc + 1));
  R.symoff = (int32_t*)take(sizeof(int32_t) * (Lc + 1));
  R.wcp = (int32_t*)take(sizeof(int32_t) * (Lc + 1));
  R.e = (int32_t*)take(sizeof(int32_t) * Lc);
  R.c = (uint16_t*)take(sizeof(uint16_t) * S);
  R.cls = (uint8_t*)take(Lc);
  R.vis = (uint8_t*)take(Lc);
  R.misc = (int32_t*)take(16);
  return R;
}

// One row's pre-tokenisation (pretok_row, bpe_codec_device.h: no special tokens here); a word of
// more than 64 byte symbols makes the row ST_FALLBACK.  st / nw: the row's status and word count.
__device__ __forceinline__ void dw_pretok_row(const EncArgs& a, const DwRow& L, int64_t r, int lane,
                                              const int32_t* s_b2i, const uint8_t* s_lut, int& st, int& nw) {
  int n;
  st = pretok_row<true>(a, L, r, lane, s_b2i, s_lut, n);
  if (st != ST_OK) return;
  nw = L.misc[0];
  bool fall = false;
  for (int k = lane; k < nw; k += 64) fall |= (L.symoff[L.wcp[k + 1]] - L.symoff[L.wcp[k]]) > DW_MID;
  if (__any(fall)) st = ST_FALLBACK;
}

// lane gl of a GW-lane group reads lane gl + 1 (down) / gl - 1 (up) of its group; `fill` past the ends
template <int GW>
__device__ __forceinline__ uint32_t grp_down1(uint32_t v, uint32_t fill) {
  if constexpr (GW == 8) {   // row_shl:1, and the last lane of each half-row takes the fill
    const uint32_t x = (uint32_t)__builtin_amdgcn_update_dpp((int)fill, (int)v, 0x101, 0xF, 0xF, false);
    return (threadIdx.x & 7) == 7 ? fill : x;
  }
  if constexpr (GW == 16) return (uint32_t)__builtin_amdgcn_update_dpp((int)fill, (int)v, 0x101, 0xF, 0xF, false);
  // wave_shl:1 (gfx9 DPP): lane 63 has no source and keeps `fill` -- no LDS permute on the round's chain
  else return (uint32_t)__builtin_amdgcn_update_dpp((int)fill, (int)v, 0x130, 0xF, 0xF, false);
}
template <int GW>
__device__ __forceinline__ uint32_t grp_up1(uint32_t v, uint32_t fill) {
  if constexpr (GW == 8) {   // row_shr:1, and the first lane of each half-row takes the fill
    const uint32_t x = (uint32_t)__builtin_amdgcn_update_dpp((int)fill, (int)v, 0x111, 0xF, 0xF, false);
    return (threadIdx.x & 7) == 0 ? fill : x;
  }
  if constexpr (GW == 16) return (uint32_t)__builtin_amdgcn_update_dpp((int)fill, (int)v, 0x111, 0xF, 0xF, false);
  else return (uint32_t)__builtin_amdgcn_update_dpp((int)fill, (int)v, 0x138, 0xF, 0xF, false);   // wave_shr:1
}
template <int GW>
__device__ __forceinline__ uint32_t grp_min(uint32_t v) {   // every lane of the group gets the group's min
  if constexpr (GW == 8) {   // half-row mirror (lane i with 7 - i), then the quad's xor 2 and xor 1
    v = min(v, (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x141, 0xF, 0xF, false));
    v = min(v, (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x4E, 0xF, 0xF, false));
    return min(v, (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0xB1, 0xF, 0xF, false));
  }
  if constexpr (GW == 64) {   // row_shr 1, 2, 4, 8 then row_bcast 15 / 31: lane 63 holds the min (DPP only)
    constexpr int MX = (int)0xFFFFFFFFu;
    v = min(v, (uint32_t)__builtin_amdgcn_update_dpp(MX, (int)v, 0x111, 0xF, 0xF, false));
    v = min(v, (uint32_t)__builtin_amdgcn_update_dpp(MX, (int)v, 0x112, 0xF, 0xF, false));
    v = min(v, (uint32_t)__builtin_amdgcn_update_dpp(MX, (int)v, 0x114, 0xF, 0xF, false));
    v = min(v, (uint32_t)__builtin_amdgcn_update_dpp(MX, (int)v, 0x118, 0xF, 0xF, false));
    v = min(v, (uint32_t)__builtin_amdgcn_update_dpp(MX, (int)v, 0x142, 0xA, 0xF, false));
    v = min(v, (uint32_t)__builtin_amdgcn_update_dpp(MX, (int)v, 0x143, 0xC, 0xF, false));
    return (uint32_t)__builtin_amdgcn_readlane((int)v, 63);
  }
  v = min(v, (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x128, 0xF, 0xF, false));   // row_ror:8
  v = min(v, (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x124, 0xF, 0xF, false));   // row_ror:4
  v = min(v, (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x122, 0xF, 0xF, false));   // row_ror:2
  v = min(v, (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x121, 0xF, 0xF, false));   // row_ror:1
  return v;
}

// The word's symbols move to the first n lanes of the group, in order (one forward permute).
template <int GW>
__device__ __forceinline__ uint32_t grp_compact(uint32_t sym, bool live, int gl, int gbase, int& n) {
  const unsigned long long bal = __ballot(live);
  const unsigned long long gm = GW == 64 ? bal : ((bal >> gbase) & ((1ull << GW) - 1ull));
  const unsigned long long below = gl == 0 ? 0ull : (gm & ((1ull << gl) - 1ull));
  n = __popcll(gm);
  const int dst = gbase + (live ? __popcll(below) : GW - 1);   // a dead lane only exists when n < GW
  const uint32_t got = (uint32_t)__builtin_amdgcn_ds_permute(dst * 4, (int)sym);
  return gl < n ? got : SYM_NONE;
}

// HF Word::merge_all of one word per GW-lane group: words of <= 16 byte symbols four to a wave
// (one 16-lane DPP row each), longer ones a wave each.  A round probes every adjacent pair's rank
// in the merge map, takes the word's lowest (DPP row rotations), merges its occurrences left to
// right (a self-pair run takes every other one) and compacts the word with one ds_permute.  For
// models whose merges only combine tokens made by earlier merges (the host checks) this is HF's
// merge_all.  raw: the lane's byte symbol
// (SYM_NONE: no vocab id), blen: the word's byte symbols (0: no word).  Returns the lane's final
// id (SYM_NONE past the end); n: the word's final length.
template <int GW>
__device__ __forceinline__ uint32_t dw_merge_word(const WordMap& mm, uint32_t raw, int blen, int unk_id, int fuse_unk,
                                                  int& n, int& rounds) {
  const int lane = threadIdx.x & 63, gl = lane & (GW - 1), gbase = lane - gl;
  // HF BPE::merge_word's unknown chars: unk_id (consecutive ones fused when fuse_unk), or dropped
  const bool in = gl < blen;
  const bool miss = in && raw == SYM_NONE;
  const bool pmiss = grp_up1<GW>(miss ? 1u : 0u, 0u) != 0u;
  const bool live = in && !(miss && (unk_id < 0 || (fuse_unk && pmiss)));
  const uint32_t id = miss ? (uint32_t)unk_id : raw;
  uint32_t sym = grp_compact<GW>(id, live, gl, gbase, n);
  for (int round = 0; round < DW_MID; ++round) {   // each round merges >= 1 pair: <= 63 rounds
    const uint32_t right = grp_down1<GW>(sym, SYM_NONE);
    const bool has = gl + 1 < n;
    uint32_t rk = RK_NONE;
    if (has) {
      const uint32_t key = (sym << 16) | right;
      const uint4 b1 = mm.b[wm_h1(key, mm.log2b)], b2 = mm.b[wm_h2(key, mm.log2b)];
      const uint32_t v = b1.x == key ? b1.y : b1.z == key ? b1.w : b2.x == key ? b2.y : b2.z == key ? b2.w : 0u;
      rk = v ? v - 0x10000u : RK_NONE;   // (rank + 1) << 16 | new_id -> rank << 16 | new_id
    }
    const uint32_t m = grp_min<GW>(rk);
    if (!__any(m != RK_NONE)) break;
    ++rounds;
    const bool match = has && m != RK_NONE && rk == m;
    const unsigned long long mb = __ballot(match);
    const unsigned long long M = GW == 64 ? mb : ((mb >> gbase) & ((1ull << GW) - 1ull));
    // a run of the same self-pair merges left to right: take a match when the matches right
    // before it are an even number (HF pops (rank, pos) in position order)
    const unsigned long long lowm = gl == 0 ? 0ull : ((1ull << gl) - 1ull);
    const unsigned long long z = ~M & lowm;
    const int hz = z ? 63 - __clzll(z) : -1;
    const bool take = match && !((gl - 1 - hz) & 1);
    const bool dies = grp_up1<GW>(take ? 1u : 0u, 0u) != 0u;
    if (take) sym = m & 0xFFFFu;
    sym = grp_compact<GW>(sym, gl < n && !dies, gl, gbase, n);
  }
  return sym;
}

// A word of <= ML byte symbols merged by ONE lane, in registers (round 5, the tiny words): HF's Word::merge_all
// exactly -- repeatedly the pair of lowest (rank, position) among the word's current pairs (the
// min-heap's order, without its stale entries), merged, and the two pairs it forms looked up --
// for any model (no rank-monotone requirement).  Every index into the register arrays is a
// compile-time one (select chains over the dynamic position), so nothing spills to scratch.  A
// wave merges 64 words at once: the cross-lane steps of dw_merge_word (DPP min, ballots, a
// ds_permute per round) are gone, and the map lookups of all lanes are in flight together.
// c: the word's byte symbols in the row image (SYM_NONE: no vocab id); the ids are written back
// over them.  Returns the word's final length.
__device__ __forceinline__ uint32_t wm_rank(const WordMap& mm, uint32_t a, uint32_t b) {   // rank << 16 | new id
  const uint32_t key = (a << 16) | b;
  const uint4 b1 = mm.b[wm_h1(key, mm.log2b)], b2 = mm.b[wm_h2(key, mm.log2b)];
  const uint32_t v = b1.x == key ? b1.y : b1.z == key ? b1.w : b2.x == key ? b2.y : b2.z == key ? b2.w : 0u;
  return v ? v - 0x10000u : RK_NONE;
}

template <int ML>
__device__ __forceinline__ int dw_merge_lane(const WordMap& mm, uint16_t* c, int blen, int unk_id, int fuse_unk,
                                             int& rounds) {
  uint32_t s[ML];
  bool miss_any = false;
#pragma unroll
  for (int i = 0; i < ML; ++i) {
    s[i] = i < blen ? (uint32_t)c[i] : SYM_NONE;
    miss_any |= i < blen && s[i] == SYM_NONE;
  }
  int n = blen;
  if (__any(miss_any)) {
    // HF BPE::merge_word's unknown chars (rare): unk_id, consecutive ones fused when fuse_unk, or
    // dropped without an unk token -- compacted by select chains
    uint32_t t[ML];
    bool pm = false;
    n = 0;
#pragma unroll
    for (int i = 0; i < ML; ++i) t[i] = SYM_NONE;
#pragma unroll
    for (int i = 0; i < ML; ++i) {
      if (i < blen) {
        const bool miss = s[i] == SYM_NONE;
        const bool live = !(miss && (unk_id < 0 || (fuse_unk && pm)));
        const uint32_t id = miss ? (uint32_t)unk_id : s[i];
#pragma unroll
        for (int k = 0; k <= i; ++k) t[k] = (live && k == n) ? id : t[k];
        n += live ? 1 : 0;
        pm = miss;
      }
    }
#pragma unroll
    for (int i = 0; i < ML; ++i) s[i] = t[i];
  }
  uint32_t rk[ML];   // rk[i]: the pair (s[i], s[i + 1]), RK_NONE when it is not a merge
#pragma unroll
  for (int i = 0; i < ML; ++i) rk[i] = i + 1 < n ? wm_rank(mm, s[i], s[i + 1]) : RK_NONE;
  for (int it = 0; it < ML - 1; ++it) {
    uint32_t best = 0xFFFFFFFFu;
#pragma unroll
    for (int i = 0; i + 1 < ML; ++i)
      best = min(best, rk[i] == RK_NONE ? 0xFFFFFFFFu : (((rk[i] >> 16) << 5) | (uint32_t)i));
    if (best == 0xFFFFFFFFu) break;
    ++rounds;
    const int p = (int)(best & 31u);
    uint32_t nid = 0, left = SYM_NONE, right = SYM_NONE;
#pragma unroll
    for (int i = 0; i < ML; ++i) {
      nid = i == p ? (rk[i] & 0xFFFFu) : nid;
      left = i + 1 == p ? s[i] : left;
      right = i == p + 2 ? s[i] : right;
    }
#pragma unroll
    for (int i = 0; i < ML; ++i) {   // s[p] <- the new id, the symbols after it move left by one
      const uint32_t nx = i + 1 < ML ? s[i + 1] : SYM_NONE;
      s[i] = i == p ? nid : (i > p ? nx : s[i]);
    }
    --n;
    const uint32_t rl = p > 0 ? wm_rank(mm, left, nid) : RK_NONE;
    const uint32_t rr = p + 1 < n ? wm_rank(mm, nid, right) : RK_NONE;
#pragma unroll
    for (int i = 0; i < ML; ++i) {
      const uint32_t nx = i + 1 < ML ? rk[i + 1] : RK_NONE;
      rk[i] = i + 1 == p ? rl : (i == p ? rr : (i > p ? nx : rk[i]));
    }
  }
#pragma unroll
  for (int i = 0; i < ML; ++i)
    if (i < n) c[i] = (uint16_t)s[i];
  return n;
}

// ------------------------------------------------------- encode by words, one launch --
// k_bpe_words: a workgroup takes nwv rows (one wave each) through the whole encode in LDS:
//   1. pre-tokenisation of each row (dw_pretok_row);
//   2. exact dedup of the workgroup's words: a table keyed by a 32-bit hash of the word's code
//      points, each entry (hash, first occurrence); a hash match is confirmed by comparing the
//      code points with the entry's occurrence, so equal hashes of different words only lengthen
//      the probe;
//   3. the distinct words counting-sorted by byte-symbol length, longest first, so the four
//      words of a 16-lane task have similar round counts;
//   4. every distinct word merged once (dw_merge_word), its ids written over its own byte
//      symbols in the row image, its id count beside it;
//   5. each row's ids gathered from its words' first occurrences.
// Nothing but the bins and the ids touches HBM (and the merge map when it is too large for LDS).
__device__ __forceinline__ uint32_t bw_hash(const int32_t* cps, int cs, int ce) {   // FNV-1a + murmur3 fmix
  uint32_t h = 0x811C9DC5u ^ (uint32_t)(ce - cs);
  for (int i = cs; i < ce; ++i) h = (h ^ (uint32_t)cps[i]) * 0x01000193u;
  h ^= h >> 16; h *= 0x85EBCA6Bu;
  h ^= h >> 13; h *= 0xC2B2AE35u;
  return h ^ (h >> 16);
}

__host__ __device__ inline size_t bw_lds_bytes(int Lc, int S, int nwv, int wm_log2b /* < 0: map in HBM */) {
  size_t b = wm_log2b >= 0 ? sizeof(uint4) << wm_log2b : 0;
  b += dw_ltab_bytes(Lc, nwv);
  b += 2 * al16(sizeof(uint32_t) * (size_t)nwv * Lc);
  return b + (size_t)nwv * dw_row_bytes(Lc, S);
}

template <bool MAP_LDS>
__global__ __launch_bounds__(64 * DW_WAVES) void k_bpe_words(EncArgs a, WordMap wm, int ltab_log2, int hash_shift) {
  extern __shared__ __align__(16) char lds_raw[];
  __shared__ int32_t s_b2i[256];
  __shared__ uint8_t s_lut[256];
  __shared__ int s_nd, s_next;
  __shared__ int s_hist[DW_MID + 1];   // distinct words per byte-symbol length, then sort cursors
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, nwv = blockDim.x >> 6;
  char* p = lds_raw;
  WordMap lm = wm;
  if constexpr (MAP_LDS) {
    uint4* kv = reinterpret_cast<uint4*>(p);
    for (int i = threadIdx.x; i < (1 << wm.log2b); i += blockDim.x) kv[i] = wm.b[i];
    lm.b = kv;
    p += sizeof(uint4) << wm.log2b;
  }
  const int lcap = 1 << ltab_log2;
  unsigned long long* ltab = reinterpret_cast<unsigned long long*>(p);
  p += sizeof(unsigned long long) * (size_t)lcap;
  const int capw = nwv * a.Lc;
  uint32_t* dl = reinterpret_cast<uint32_t*>(p);   // distinct words: wave << 22 | word << 7 | byte symbols
  p += al16(sizeof(uint32_t) * (size_t)capw);
  uint32_t* ds = reinterpret_cast<uint32_t*>(p);   // ... sorted, longest first
  p += al16(sizeof(uint32_t) * (size_t)capw);
  char* rows = p;
  const size_t rb = dw_row_bytes(a.Lc, a.S);
  for (int i = threadIdx.x; i < 256; i += blockDim.x) s_b2i[i] = a.byte2id[i];
  beast_pt::stage_lut256(s_lut, a.lut, a.lut_n);
  for (int i = threadIdx.x; i < lcap; i += blockDim.x) ltab[i] = 0ull;
  for (int i = threadIdx.x; i <= DW_MID; i += blockDim.x) s_hist[i] = 0;   // 65 bins: one wave is 64 threads
  if (threadIdx.x == 0) { s_nd = 0; s_next = nwv; }
  __syncthreads();
  const DwRow L = dw_carve(rows + (size_t)wave * rb, a.Lc, a.S);
  const int64_t r = (int64_t)blockIdx.x * nwv + wave;
#ifdef BPE_STAMPS
  if (lane == 0 && r < BPE_RS) g_bpe_rs[r][10] = __builtin_amdgcn_s_memrealtime();
#endif
  int st = ST_OK, nw = 0;
  if (r < a.n_rows) dw_pretok_row(a, L, r, lane, s_b2i, s_lut, st, nw);
  __syncthreads();   // every row's code points, word starts and symbols are readable workgroup-wide
  if (r < a.n_rows) BPE_STAMP(4);
  // 2. exact dedup; L.e[k] = the word's first occurrence (wave << 16 | word)
#ifdef BPE_WORDS_SKIP_DEDUP   // counter attribution only (wrong ids): no dedup, sort or merges
  if (r < a.n_rows && st == ST_OK)
    for (int k = lane; k < nw; k += 64) { L.e[k] = (int32_t)(((uint32_t)wave << 16) | (uint32_t)k); L.vis[k] = 0; }
  if (false) {
#else
  if (r < a.n_rows && st == ST_OK) {
#endif
    const uint32_t lmask = (uint32_t)lcap - 1u;
    for (int k = lane; k < nw; k += 64) {
      const int cs = L.wcp[k], ce = L.wcp[k + 1], len = ce - cs;
      const uint32_t hk = (bw_hash(L.cps, cs, ce) >> hash_shift) | 1u;
      const uint32_t me = ((uint32_t)wave << 16) | (uint32_t)k;
      const unsigned long long mine = ((unsigned long long)hk << 32) | me;
      uint32_t ls = (hk * 0x9E3779B1u) >> (32 - ltab_log2), rep = me;
      while (true) {
        unsigned long long e = ltab[ls];
        if (e == 0ull) {
          e = atomicCAS(&ltab[ls], 0ull, mine);
          if (e == 0ull) break;
        }
        if ((uint32_t)(e >> 32) == hk) {
          const uint32_t o = (uint32_t)e;
          const DwRow Ro = dw_carve(rows + (size_t)(o >> 16) * rb, a.Lc, a.S);
          const int ocs = Ro.wcp[o & 0xFFFF];
          bool same = Ro.wcp[(o & 0xFFFF) + 1] - ocs == len;
          for (int i = 0; same && i < len; ++i) same = Ro.cps[ocs + i] == L.cps[cs + i];
          if (same) { rep = o; break; }
        }
        ls = (ls + 1) & lmask;
      }
      L.e[k] = (int32_t)rep;
      if (rep == me) {
        const int blen = L.symoff[ce] - L.symoff[cs];   // 1..64 (longer words made the row ST_FALLBACK)
        dl[atomicAdd(&s_nd, 1)] = ((uint32_t)wave << 22) | ((uint32_t)k << 7) | (uint32_t)blen;
        atomicAdd(&s_hist[blen], 1);
      }
    }
  }
  __syncthreads();
  // 3. counting sort, longest first: lane l holds length 64 - l
  if (wave == 0) {
    int tot;
    const int ex = wave_excl_scan(s_hist[DW_MID - lane], lane, tot);
    s_hist[DW_MID - lane] = ex;
  }
  __syncthreads();
  const int nd = s_nd;
  for (int i = threadIdx.x; i < nd; i += blockDim.x) {
    const uint32_t v = dl[i];
    ds[atomicAdd(&s_hist[v & 127u], 1)] = v;
  }
  __syncthreads();
  if (r < a.n_rows) BPE_STAMP(5);
  // 4. merges: a mid word (17..64 byte symbols) per wave and words of 9..16 four to a wave (16-lane
  // rows) by dw_merge_word's cooperative rounds; words of <= 8 one per lane, 64 to a task
  // (dw_merge_lane: its select chains stay short, and the tiny words are most of them)
  // the cursor of length 17 has passed every longer word, that of length 9 every word of 9 or
  // more.  Cursors out of order would be a corrupt sort: the workgroup's rows then report
  // ST_FALLBACK (the host re-encodes them with the per-row kernel) and no task runs, instead of a
  // clamp quietly merging whatever the cursors point at (round 5)
  const int c17 = s_hist[DW_SHORT + 1], c9 = s_hist[DW_TINY + 1];
  const bool sane = 0 <= c17 && c17 <= c9 && c9 <= nd;
  if (!sane && st == ST_OK) st = ST_FALLBACK;
  const int nmid = sane ? c17 : 0;
  const int n9 = sane ? c9 : 0;
  const int t16 = nmid + (n9 - nmid + 3) / 4;
  const int tasks = sane ? t16 + (nd - n9 + 63) / 64 : 0;
  int nrounds = 0;
#if defined(BPE_WORDS_SKIP_MERGES) || defined(BPE_WORDS_SKIP_DEDUP)   // counter attribution only (wrong ids)
  if (r < a.n_rows && st == ST_OK)
    for (int k = lane; k < nw; k += 64) L.vis[k] = 0;
  for (int t = tasks; t < tasks;) {
#else
  // tasks longest first, each wave taking the next one when it is done (an LDS counter): the
  // workgroup waits for its slowest wave at the barrier below (29.8 vs 33.0 us with tasks dealt
  // round-robin, profiles/r04/ab/encode_words_variants_r04d.txt)
  for (int t = wave; t < tasks;) {
#endif
#ifdef BPE_STAMPS
    const unsigned long long t_task0 = __builtin_amdgcn_s_memrealtime();
    const int kind_task = t < nmid ? 0 : (t < t16 ? 1 : 2);
#endif
    if (t < nmid) {
      const uint32_t v = ds[t];
      const DwRow Rw = dw_carve(rows + (size_t)(v >> 22) * rb, a.Lc, a.S);
      const int k = (v >> 7) & 0x7FFF, blen = v & 127u;
      const int bs = Rw.symoff[Rw.wcp[k]];
      const uint32_t raw = lane < blen ? (uint32_t)Rw.c[bs + lane] : SYM_NONE;
      int n;
      const uint32_t id = dw_merge_word<DW_MID>(lm, raw, blen, a.unk_id, a.fuse_unk, n, nrounds);
      if (lane < n) Rw.c[bs + lane] = (uint16_t)id;
      if (lane == 0) Rw.vis[k] = (uint8_t)n;
    } else if (t < t16) {
      const int j = nmid + 4 * (t - nmid) + (lane >> 4), gl = lane & 15;
      const bool valid = j < n9;
      const uint32_t v = valid ? ds[j] : 0u;
      const DwRow Rw = dw_carve(rows + (size_t)(v >> 22) * rb, a.Lc, a.S);
      const int k = (v >> 7) & 0x7FFF, blen = valid ? (int)(v & 127u) : 0;
      const int bs = valid ? Rw.symoff[Rw.wcp[k]] : 0;
      const uint32_t raw = gl < blen ? (uint32_t)Rw.c[bs + gl] : SYM_NONE;
      int n;
      const uint32_t id = dw_merge_word<DW_SHORT>(lm, raw, blen, a.unk_id, a.fuse_unk, n, nrounds);
      if (valid && gl < n) Rw.c[bs + gl] = (uint16_t)id;
      if (valid && gl == 0) Rw.vis[k] = (uint8_t)n;
    } else {
      const int j = n9 + 64 * (t - t16) + lane;
      const bool valid = j < nd;
      const uint32_t v = valid ? ds[j] : 0u;
      const DwRow Rw = dw_carve(rows + (size_t)(v >> 22) * rb, a.Lc, a.S);
      const int k = (v >> 7) & 0x7FFF, blen = valid ? (int)(v & 127u) : 0;
      uint16_t* c = Rw.c + (valid ? Rw.symoff[Rw.wcp[k]] : 0);
      const int n = dw_merge_lane<DW_TINY>(lm, c, blen, a.unk_id, a.fuse_unk, nrounds);
      if (valid) Rw.vis[k] = (uint8_t)n;
    }
#ifdef BPE_STAMPS
    if (lane == 0 && r < BPE_RS) {
      g_bpe_wt[r][kind_task] += __builtin_amdgcn_s_memrealtime() - t_task0;
      g_bpe_wt[r][3 + kind_task] += 1;
    }
#endif
    int nt = 0;
    if (lane == 0) nt = atomicAdd(&s_next, 1);
    t = __builtin_amdgcn_readfirstlane(nt);
  }
  __syncthreads();
  if (r < a.n_rows) BPE_STAMP(6);
  // 5. the row's ids from its words' first occurrences
  if (r < a.n_rows) {
    if (st != ST_OK) {
      if (lane == 0) { a.out_len[r] = 0; a.status[r] = st; }
    } else {
      int32_t* out = a.out_ids + r * a.out_stride;
      int carry = 0;
      for (int base = 0; base < nw; base += 64) {
        const int k = base + lane;
        int cnt = 0;
        const uint16_t* src = nullptr;
        if (k < nw) {
          const uint32_t o = (uint32_t)L.e[k];
          const DwRow Ro = dw_carve(rows + (size_t)(o >> 16) * rb, a.Lc, a.S);
          const int ko = o & 0xFFFF;
          cnt = Ro.vis[ko];
          src = Ro.c + Ro.symoff[Ro.wcp[ko]];
        }
        int tot;
        const int off = carry + wave_excl_scan(cnt, lane, tot);
        for (int q = 0; q < cnt; ++q) out[off + q] = (int32_t)src[q];
        carry += tot;
      }
      if (lane == 0) { a.out_len[r] = carry; a.status[r] = ST_OK; }
    }
#ifdef BPE_STAMPS
    if (lane == 0 && r < BPE_RS) { g_bpe_rs[r][7] = __builtin_amdgcn_s_memrealtime(); g_bpe_rs[r][8] = nd; g_bpe_rs[r][9] = nw; }
    if (lane == 0 && r < BPE_RS) g_bpe_rs[r][11] = (unsigned long long)nrounds;
#endif
  }
  (void)nrounds;
}

}  // namespace
