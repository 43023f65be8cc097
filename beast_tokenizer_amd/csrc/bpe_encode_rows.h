// Byte-level BPE inference, k_bpe_encode (bpe_codec.hip): one wave per row, the row's words
// merged in LDS by rounds (or by HF's heap per word), special tokens included.
#pragma once

#include "bpe_codec_device.h"

namespace {

// ---------------------------------------------------------------- heap --
// min-heap of u32 keys (rank << 16 | pos) in LDS, one per word: HF's Merge order (rank, pos)
__device__ __forceinline__ void heap_push(uint32_t* h, int& n, uint32_t v) {
  int i = n++;
  while (i > 0) {
    const int p = (i - 1) >> 1;
    const uint32_t hp = h[p];
    if (hp <= v) break;
    h[i] = hp;
    i = p;
  }
  h[i] = v;
}

__device__ __forceinline__ uint32_t heap_pop(uint32_t* h, int& n) {
  const uint32_t top = h[0];
  const uint32_t v = h[--n];
  int i = 0;
  while (true) {
    int c = 2 * i + 1;
    if (c >= n) break;
    uint32_t hc = h[c];
    if (c + 1 < n) {
      const uint32_t h1 = h[c + 1];
      if (h1 < hc) { hc = h1; ++c; }
    }
    if (v <= hc) break;
    h[i] = hc;
    i = c;
  }
  if (n > 0) h[i] = v;
  return top;
}

// ------------------------------------------------------------- encode --
struct EncLds {
  uint32_t* heap;     // [3 S]
  int32_t* c;         // [S] symbol ids (-1: none)
  int32_t* cps;       // [Lc] shifted code points
  int32_t* symoff;    // [Lc + 1] first byte symbol of each code point
  int32_t* wcp;       // [Lc + 1] word boundaries (code point index)
  int32_t* wspec;     // [Lc] special-token id of a word, or -1
  int32_t* wcnt;      // [Lc] final symbols per word, then their output offsets
  int16_t* prv;       // [S]
  int16_t* nxt;       // [S]
  uint8_t* cls;       // [Lc]
  int32_t* misc;      // [4]: n_words
  uint32_t* rk;       // [S] round merge: (rank << 16 | new id) of the pair starting here, RK_NONE: none
  int16_t* wid;       // [S] word of each symbol
  uint8_t* cand;      // [S] this round's merge candidates
  uint8_t* dirty;     // [S] pair changed since its rank was read
  uint32_t* wmin;     // [Lc] this round's lowest pair per word
  int32_t* e;         // [Lc] pretok_row's regex word ends: wcnt (so wmin too), dead before step 4
  uint8_t* vis;       // [S] word_starts' marks: cand, dead before the round merge
};

// the heap (long rows, or heap mode) and the round merge's arrays (rows <= 64 * RM_PER symbols)
// share a region; a launch that never takes the heap path sizes it for the rounds only.  The
// per-word counts (wcnt, live in steps 2 and 5) alias the round merge's wmin (live in step 4).
__host__ __device__ inline bool enc_needs_heap(int S, int heap_merge) { return heap_merge || S > 64 * RM_PER; }
__host__ __device__ inline size_t enc_merge_bytes(int Lc, int S, bool heap) {
  const size_t rounds = al16(sizeof(uint32_t) * S) + al16(sizeof(uint32_t) * Lc) + 2 * al16(S);
  const size_t hp = heap ? al16(sizeof(uint32_t) * 3 * (size_t)S) : 0;
  return hp > rounds ? hp : rounds;
}
__host__ __device__ inline size_t enc_row_bytes(int Lc, int S, bool heap) {
  return enc_merge_bytes(Lc, S, heap) + al16(sizeof(int32_t) * S) + al16(sizeof(int32_t) * Lc) +
         2 * al16(sizeof(int32_t) * (Lc + 1)) + al16(sizeof(int32_t) * Lc) + 2 * al16(sizeof(int16_t) * S) +
         al16(Lc) + 16 + al16(sizeof(int16_t) * S);
}

__device__ inline EncLds enc_carve(char* p, int Lc, int S, bool heap) {
  EncLds L;
  auto take = [&](size_t bytes) { char* r = p; p += al16(bytes); return r; };
  char* merge = take(enc_merge_bytes(Lc, S, heap));   // heap, or rk | wmin | cand | dirty
  L.heap = (uint32_t*)merge;
  L.rk = (uint32_t*)merge;
  L.wmin = (uint32_t*)(merge + al16(sizeof(uint32_t) * S));
  L.cand = (uint8_t*)(merge + al16(sizeof(uint32_t) * S) + al16(sizeof(uint32_t) * Lc));
  L.dirty = L.cand + al16(S);
  L.c = (int32_t*)take(sizeof(int32_t) * S);
  L.cps = (int32_t*)take(sizeof(int32_t) * Lc);
  L.symoff = (int32_t*)take(sizeof(int32_t) * (Lc + 1));
  L.wcp = (int32_t*)take(sizeof(int32_t) * (Lc + 1));
  L.wspec = (int32_t*)take(sizeof(int32_t) * Lc);
  L.wcnt = (int32_t*)L.wmin;
  L.e = L.wcnt;
  L.vis = L.cand;
  L.prv = (int16_t*)take(sizeof(int16_t) * S);
  L.nxt = (int16_t*)take(sizeof(int16_t) * S);
  L.cls = (uint8_t*)take(Lc);
  L.misc = (int32_t*)take(16);
  L.wid = (int16_t*)take(sizeof(int16_t) * S);
  return L;
}

// bytes of the staged merge map (0 if it stays in HBM)
__host__ __device__ inline size_t map_lds_bytes(int log2cap, int n_merges) {
  if (log2cap > LDS_MAP_MAX_LOG2) return 0;
  return al16(sizeof(uint32_t) * 2 * ((size_t)1 << log2cap)) + al16(sizeof(uint16_t) * (size_t)n_merges);
}

// 4b. (see encode_row) the round merge of a row of <= 64 * RMP byte symbols
template <int RMP, class Map>
__device__ __forceinline__ void round_merge(const Map& mm, EncLds& L, int npos, int nw, int lane) {
    // Each step reads all of a lane's positions first (addresses clamped, loads in flight
    // together) and then acts on them, so a step costs one LDS round trip, not one per position.
    const int kmax = (npos + 63) >> 6;   // positions per lane in use (<= RMP)
    for (int k = 0; k < kmax; ++k) {
      const int s = lane + 64 * k;
      if (s < npos) { L.dirty[s] = 1; L.cand[s] = 0; }
    }
    wave_sync();
    const int last = npos > 0 ? npos - 1 : 0;
    // every round with a live pair merges at least one (each word's lowest pair has a head), so
    // npos rounds bound the loop: a broken invariant ends it instead of hanging the wave
    for (int round = 0; round < npos; ++round) {
#ifdef BPE_STAMPS
      if (lane == 0) L.misc[1] += 1;
#endif
      for (int w = lane; w < nw; w += 64) L.wmin[w] = RK_NONE;
      // (a) ranks of the pairs next to last round's merges
      int ck[RMP], nk[RMP], dk[RMP];
#pragma unroll
      for (int k = 0; k < RMP; ++k) {
        const int s = min(lane + 64 * k, last);
        dk[k] = k < kmax && lane + 64 * k < npos ? L.dirty[s] : 0;
        ck[k] = L.c[s];
        nk[k] = L.nxt[s];
      }
      int cn[RMP];
#pragma unroll
      for (int k = 0; k < RMP; ++k) cn[k] = L.c[max(nk[k], 0)];
      // the dirty pairs' first probes all in flight together (one 8-byte load each), then the
      // rare collision chains per position
      const uint32_t mmask = (1u << mm.log2cap) - 1u;
      constexpr int PG = RMP < 4 ? RMP : 4;   // positions probed together (registers)
#pragma unroll
      for (int k0 = 0; k0 < RMP; k0 += PG) {
        uint32_t key[PG], hs[PG];
        uint2 e[PG];
        bool q[PG];   // a live pair to look up (a dead symbol's key may equal EMPTY_KEY)
#pragma unroll
        for (int i = 0; i < PG; ++i) {
          const int k = min(k0 + i, RMP - 1);   // RMP need not be a multiple of PG
          q[i] = k0 + i < RMP && dk[k] && ck[k] >= 0 && nk[k] >= 0;
          key[i] = ((uint32_t)ck[k] << 16) | (uint32_t)cn[k];
          hs[i] = mm_hash(key[i], mm.log2cap);
          e[i] = q[i] ? mm.kv[hs[i]] : make_uint2(EMPTY_KEY, 0u);
        }
#pragma unroll
        for (int i = 0; i < PG; ++i) {
          const int k = min(k0 + i, RMP - 1);
          if (k0 + i >= RMP || !dk[k]) continue;
          while (q[i] && e[i].x != key[i] && e[i].x != EMPTY_KEY) {
            hs[i] = (hs[i] + 1) & mmask;
            e[i] = mm.kv[hs[i]];
          }
          // (rank + 1) << 16 | new_id  ->  rank << 16 | new_id
          L.rk[lane + 64 * k] = (q[i] && e[i].x == key[i]) ? e[i].y - 0x10000u : RK_NONE;
          L.dirty[lane + 64 * k] = 0;
        }
      }
      wave_sync();
      // (b) every word's lowest pair
      bool live = false;
      uint32_t rv[RMP];
      int wv[RMP];
#pragma unroll
      for (int k = 0; k < RMP; ++k) {
        const int s = min(lane + 64 * k, last);
        rv[k] = (k < kmax && lane + 64 * k < npos) ? L.rk[s] : RK_NONE;
        wv[k] = L.wid[s];
        ck[k] = L.c[s];
      }
#pragma unroll
      for (int k = 0; k < RMP; ++k)
        if (ck[k] >= 0 && rv[k] != RK_NONE) {
          atomicMin(&L.wmin[wv[k]], rv[k]);
          live = true;
        }
      if (!__any(live)) break;
      wave_sync();
      // (c) candidates: the pairs equal to their word's lowest
      uint32_t mv[RMP];
#pragma unroll
      for (int k = 0; k < RMP; ++k) mv[k] = L.wmin[wv[k]];
      bool cd[RMP];
#pragma unroll
      for (int k = 0; k < RMP; ++k) {
        cd[k] = ck[k] >= 0 && rv[k] != RK_NONE && rv[k] == mv[k];
        if (k < kmax && lane + 64 * k < npos) L.cand[lane + 64 * k] = cd[k];
      }
      // links only (d) changes, read in this step's round trip: each position's left neighbour
      // and the symbol after its pair (its right one, nk, is from (a): nxt is unchanged since)
      int pk[RMP], nnk[RMP];
#pragma unroll
      for (int k = 0; k < RMP; ++k) {
        pk[k] = L.prv[min(lane + 64 * k, last)];
        nnk[k] = L.nxt[max(nk[k], 0)];
      }
      wave_sync();
      // (d) each run's head applies its run (one merge unless a self-pair repeats).  The heads'
      // first merges read everything in one round trip before any write (no head writes what
      // another head's first merge reads: nxt / cand of its own pair only, prv of the symbol after
      // it -- read here only as the head's own left neighbour, which marks the same live pair
      // dirty either way), then the rare self-pair runs one step at a time
      int cf[RMP];   // cand of the left neighbour (bit 0), of the pair's right symbol (1), of the one after (2)
#pragma unroll
      for (int k = 0; k < RMP; ++k)
        cf[k] = (int)L.cand[max(pk[k], 0)] | ((int)L.cand[max(nk[k], 0)] << 1) | ((int)L.cand[max(nnk[k], 0)] << 2);
      bool hd[RMP];
#pragma unroll
      for (int k = 0; k < RMP; ++k) hd[k] = cd[k] && !(pk[k] >= 0 && (cf[k] & 1));
#pragma unroll
      for (int k = 0; k < RMP; ++k) {
        if (!hd[k]) continue;
        const int nid = (int)(rv[k] & 0xFFFFu);
        const int t = lane + 64 * k, u = nk[k], nn = nnk[k];
        L.c[t] = nid;
        L.c[u] = -1;
        L.nxt[t] = (int16_t)nn;
        if (nn >= 0) L.prv[nn] = (int16_t)t;
        L.dirty[t] = 1;
        if (pk[k] >= 0) L.dirty[pk[k]] = 1;
      }
#pragma unroll
      for (int k = 0; k < RMP; ++k) {
        if (!hd[k] || !(cf[k] & 2) || nnk[k] < 0 || !(cf[k] & 4)) continue;
        const int nid = (int)(rv[k] & 0xFFFFu);
        int t = nnk[k];   // the run of a self-pair goes on
        while (true) {
          const int u = L.nxt[t], nn = L.nxt[u];
          L.c[t] = nid;
          L.c[u] = -1;
          L.nxt[t] = (int16_t)nn;
          if (nn >= 0) L.prv[nn] = (int16_t)t;
          L.dirty[t] = 1;
          const int pv = L.prv[t];
          if (pv >= 0) L.dirty[pv] = 1;
          if (!L.cand[u] || nn < 0 || !L.cand[nn]) break;
          t = nn;
        }
      }
      wave_sync();
    }
}

// RMX: the widest round merge compiled in.  RM_NARROW (rows of <= 384 byte symbols, e.g. 140 bins
// of 2-byte code points) keeps the kernel at ~109 VGPRs with nothing spilled; the RM_PER form
// needs 128 and spills ~16 to scratch.  The host launches the narrow kernel whenever every row fits.
template <int RMX, class Map>
__device__ void encode_row(const EncArgs& a, const Map& mm, EncLds& L, int64_t r, int lane, const int32_t* b2i,
                           const uint8_t* lut256) {
#ifdef BPE_STAMPS
  if (lane == 0) L.misc[1] = 0;
#endif
  // 1.-3. code points, range checks, classes, UTF-8 symbol offsets, word boundaries (no special
  //       tokens), byte symbols as vocab ids: pretok_row (bpe_codec_device.h)
  int n;
  const int st = pretok_row<false>(a, L, r, lane, b2i, lut256, n);
  if (st != ST_OK) {
    if (lane == 0) { a.status[r] = st; a.out_len[r] = 0; }
    return;
  }
  // 2'. with special tokens the word boundaries are lane 0's: AddedVocabulary's split
  //     (leftmost-longest) and the regex walk per segment
  if (a.n_spec > 0 && lane == 0) {
    int nw = 0, seg = 0, i = 0;
    while (i <= n) {
      int mlen = 0, mid = -1;
      if (i < n) {
        for (int s = 0; s < a.n_spec; ++s) {
          const int sl = a.spec_len[s];
          if (sl <= mlen || i + sl > n) continue;
          const int32_t* sc = a.spec_cps + (size_t)s * MAX_SPECIAL_LEN;
          bool ok = true;
          for (int q = 0; q < sl && ok; ++q) ok = (L.cps[i + q] == sc[q]);
          if (ok) { mlen = sl; mid = a.spec_id[s]; }
        }
      }
      if (mlen > 0 || i == n) {
        int p = seg;
        while (p < i) {
          const int j = regex_word(L.cps, L.cls, p, i);
          L.wcp[nw] = p; L.wspec[nw] = -1; ++nw;
          p = j;
        }
        if (i == n) break;
        L.wcp[nw] = i; L.wspec[nw] = mid; ++nw;
        i += mlen;
        seg = i;
      } else {
        ++i;
      }
    }
    L.wcp[nw] = n;
    L.misc[0] = nw;
  }
  if (a.n_spec > 0) wave_sync();
  const int nw = L.misc[0];

  BPE_STAMP(4);
  // 4a. one word per lane: special words, unknown chars (HF's unk / fuse_unk), the symbol list
  const int npos = L.symoff[n];
  for (int w = lane; w < nw; w += 64) {
    const int sb = L.symoff[L.wcp[w]], se = L.symoff[L.wcp[w + 1]];
    for (int s = sb; s < se; ++s) L.wid[s] = (int16_t)w;
    if (L.wspec[w] >= 0) {
      L.c[sb] = L.wspec[w];
      L.nxt[sb] = -1;
      L.prv[sb] = -1;
      for (int s = sb + 1; s < se; ++s) L.c[s] = -1;
      continue;
    }
    bool pending_unk = false;
    int last = -1;
    for (int s = sb; s < se; ++s) {
      int id = L.c[s];
      if (id < 0) {
        if (a.unk_id >= 0 && !(a.fuse_unk && pending_unk)) { id = a.unk_id; pending_unk = true; }
        else id = -1;
      } else {
        pending_unk = false;
      }
      L.c[s] = id;
      if (id < 0) continue;
      L.prv[s] = (int16_t)last;
      L.nxt[s] = -1;
      if (last >= 0) L.nxt[last] = (int16_t)s;
      last = s;
    }
  }
  wave_sync();
#ifndef BPE_SKIP_MERGE
  if (npos <= 64 * RM_PER && !a.heap_merge) {
    // 4b. BPE::merge_word + Word::merge_all for every word of the row at once.  HF pops the
    //     lowest (rank, position) of the word's current pairs (stale heap entries skipped), so a
    //     word's result is: repeatedly merge its lowest-rank pair, leftmost first.  One round
    //     merges, in every word, all occurrences of that word's lowest pair (left to right in a
    //     run of a self-pair: each run's head walks it), so rounds = distinct ranks applied per
    //     word, and only pairs next to a merge are looked up again.
    if (npos <= 64 * 4) {
      round_merge<4>(mm, L, npos, nw, lane);
    } else {
      if constexpr (RMX == RM_NARROW) round_merge<RM_NARROW>(mm, L, npos, nw, lane);
      else round_merge<RM_PER>(mm, L, npos, nw, lane);
    }
  } else {
    // 4b'. long rows: one word per lane with HF's (rank, pos) min-heap
    for (int w = lane; w < nw; w += 64) {
      if (L.wspec[w] >= 0) continue;
      const int sb = L.symoff[L.wcp[w]], se = L.symoff[L.wcp[w + 1]];
      uint32_t* hp = L.heap + 3 * (size_t)sb;
      int hn = 0;
      for (int s = sb; s < se; ++s) {
        if (L.c[s] < 0 || L.nxt[s] < 0) continue;
        int nid;
        const int rk = mm_find(mm, L.c[s], L.c[L.nxt[s]], nid);
        if (rk >= 0) heap_push(hp, hn, ((uint32_t)rk << 16) | (uint32_t)(s - sb));
      }
      while (hn > 0) {
        const uint32_t top = heap_pop(hp, hn);
        const int pos = sb + (int)(top & 0xFFFFu);
        const int trank = (int)(top >> 16);
        if (L.c[pos] < 0) continue;             // merged into its left neighbour
        const int nx = L.nxt[pos];
        if (nx < 0) continue;                   // last symbol
        int new_id;
        const int rk = mm_find(mm, L.c[pos], L.c[nx], new_id);
        if (rk < 0) continue;
        if (rk != trank && mm.rank2new[trank] != new_id) continue;   // expired entry
        L.c[pos] = new_id;
        L.c[nx] = -1;
        const int nn = L.nxt[nx];
        L.nxt[pos] = (int16_t)nn;
        if (nn >= 0) L.prv[nn] = (int16_t)pos;
        const int pv = L.prv[pos];
        if (pv >= 0) {
          int nid;
          const int rp = mm_find(mm, L.c[pv], new_id, nid);
          if (rp >= 0) heap_push(hp, hn, ((uint32_t)rp << 16) | (uint32_t)(pv - sb));
        }
        if (nn >= 0) {
          int nid;
          const int rn = mm_find(mm, new_id, L.c[nn], nid);
          if (rn >= 0) heap_push(hp, hn, ((uint32_t)rn << 16) | (uint32_t)(pos - sb));
        }
      }
    }
    wave_sync();
  }
#endif
  // symbols left per word
  for (int w = lane; w < nw; w += 64) L.wcnt[w] = 0;
  wave_sync();
  for (int s = lane; s < npos; s += 64)
    if (L.c[s] >= 0) atomicAdd(&L.wcnt[L.wid[s]], 1);
  wave_sync();
  BPE_STAMP(5);
  // 5. word offsets (wave scan), ids in order
  int carry = 0;
  for (int base = 0; base < nw; base += 64) {
    const int w = base + lane;
    int tot;
    const int v = (w < nw) ? L.wcnt[w] : 0;
    const int ex = wave_excl_scan(v, lane, tot);
    if (w < nw) L.wcnt[w] = carry + ex;
    carry += tot;
  }
  wave_sync();
  int32_t* out = a.out_ids + r * a.out_stride;
  for (int w = lane; w < nw; w += 64) {
    const int sb = L.symoff[L.wcp[w]], se = L.symoff[L.wcp[w + 1]];
    int o = L.wcnt[w];
    for (int s = sb; s < se; ++s)
      if (L.c[s] >= 0) out[o++] = L.c[s];
  }
  if (lane == 0) { a.out_len[r] = carry; a.status[r] = ST_OK; }
  BPE_STAMP(6);
#ifdef BPE_STAMPS
  if (lane == 0 && r < BPE_RS) {
    g_bpe_rs[r][7] = (unsigned long long)L.misc[1];
    g_bpe_rs[r][8] = (unsigned long long)npos;
    g_bpe_rs[r][9] = (unsigned long long)nw;
  }
#endif
}

// the merge map staged in LDS: offsets from the dynamic LDS base, so every probe is a ds_read
struct LdsMap {
  const uint2* kv;
  const uint16_t* rank2new;
  int log2cap;
};

template <bool MAP_LDS, int RMX>
__global__ __launch_bounds__(64 * ENC_MAX_WAVES) void k_bpe_encode(EncArgs a) {
  extern __shared__ __align__(16) char lds_raw[];
  __shared__ int32_t s_b2i[256];    // byte -> vocab id
  __shared__ uint8_t s_lut[256];    // classes of code points < 256
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, nwv = blockDim.x >> 6;
#ifdef BPE_STAMPS
  const unsigned long long t_stage = __builtin_amdgcn_s_memrealtime();
#endif
  for (int i = threadIdx.x; i < 256; i += blockDim.x) s_b2i[i] = a.byte2id[i];
  beast_pt::stage_lut256(s_lut, a.lut, a.lut_n);
  if (!MAP_LDS) __syncthreads();
  size_t row_base = 0;
  LdsMap lm;
  if constexpr (MAP_LDS) {
    const int cap = 1 << a.map.log2cap;
    uint2* kv = reinterpret_cast<uint2*>(lds_raw);
    uint16_t* r2n = reinterpret_cast<uint16_t*>(lds_raw + al16(sizeof(uint32_t) * 2 * (size_t)cap));
    // 16-byte copies (cap >= 64 slots of 8 bytes, 16-byte aligned)
    const uint4* g = reinterpret_cast<const uint4*>(a.map.kv);
    for (int i = threadIdx.x; i < cap / 2; i += blockDim.x) reinterpret_cast<uint4*>(kv)[i] = g[i];
    for (int i = threadIdx.x; i < a.n_merges; i += blockDim.x) r2n[i] = a.map.rank2new[i];
    lm.kv = kv; lm.rank2new = r2n; lm.log2cap = a.map.log2cap;
    row_base = map_lds_bytes(a.map.log2cap, a.n_merges);
    __syncthreads();
  }
#ifdef BPE_STAMPS
  if (lane == 0) {
    const int64_t r0 = (int64_t)blockIdx.x * nwv + wave;
    if (r0 < BPE_RS) { g_bpe_rs[r0][10] = t_stage; g_bpe_rs[r0][11] = __builtin_amdgcn_s_memrealtime(); }
  }
#endif
  const bool heap = enc_needs_heap(a.S, a.heap_merge);
  EncLds L = enc_carve(lds_raw + row_base + (size_t)wave * enc_row_bytes(a.Lc, a.S, heap), a.Lc, a.S, heap);
  for (int64_t r = (int64_t)blockIdx.x * nwv + wave; r < a.n_rows; r += (int64_t)gridDim.x * nwv) {
    if constexpr (MAP_LDS) encode_row<RMX>(a, lm, L, r, lane, s_b2i, s_lut);
    else encode_row<RMX>(a, a.map, L, r, lane, s_b2i, s_lut);
    wave_sync();
  }
}

}  // namespace
