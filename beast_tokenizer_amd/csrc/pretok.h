// The ByteLevel row pre-tokeniser of every BPE kernel that stages a row (training: k_pretok_wave,
// k_pretok_dedup in bpe_setup.hip; inference: k_bpe_encode, k_bpe_words through bpe_codec_device.h's
// pretok_row), one wave per row.  Front half: class lookup, UTF-8 helpers and stage_row (code points,
// classes, UTF-8 symbol offsets in one pass); back half: regex_ends (the GPT-2 regex from every code
// point at once) and word_starts (the lane-parallel walk of its word chain).  The callers own
// their LDS layouts: nothing here declares an LDS array.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

#include "common.h"

namespace beast_pt {

using beast::wave_sync;

constexpr int CLS_OTHER = 0, CLS_LETTER = 1, CLS_NUMBER = 2, CLS_WS = 3;

// The first 256 entries of the class LUT into the workgroup's LDS (every BEAST bin of a 256
// vocab); the caller's __syncthreads follows.
template <class N>
__device__ __forceinline__ void stage_lut256(uint8_t* s_lut, const uint8_t* __restrict__ lut, N lut_n) {
  for (int i = threadIdx.x; i < 256; i += blockDim.x) s_lut[i] = i < lut_n ? lut[i] : (uint8_t)CLS_OTHER;
}

// class of a code point from the LUT in memory alone (pretok_serial: no LDS head)
template <class T, class N>
__device__ __forceinline__ int class_global(T cp, const uint8_t* __restrict__ lut, N lut_n) {
  return (cp >= 0 && cp < lut_n) ? lut[cp] : CLS_OTHER;
}

// class of a code point: the LDS head for cp < 256, the LUT in memory up to lut_n, CLS_OTHER past it
template <class T, class N>
__device__ __forceinline__ int class_of(T cp, const uint8_t* s_lut, const uint8_t* __restrict__ lut, N lut_n) {
  return (cp >= 0 && cp < 256) ? s_lut[cp] : class_global(cp, lut, lut_n);
}

template <class T>
__device__ __forceinline__ int utf8_len(T cp) { return cp < 0x80 ? 1 : cp < 0x800 ? 2 : cp < 0x10000 ? 3 : 4; }

// The UTF-8 bytes of a code point, first byte lowest: one register, no indexed array (which a
// kernel short of VGPRs would keep in scratch).
template <class T>
__device__ __forceinline__ uint32_t utf8_bytes(T cp) {
  const uint32_t c = (uint32_t)cp, t0 = 0x80u | (c & 0x3F), t1 = 0x80u | ((c >> 6) & 0x3F), t2 = 0x80u | ((c >> 12) & 0x3F);
  if (cp < 0x80) return c & 0xFFu;
  if (cp < 0x800) return ((0xC0u | (c >> 6)) & 0xFFu) | (t0 << 8);
  if (cp < 0x10000) return ((0xE0u | (c >> 12)) & 0xFFu) | (t1 << 8) | (t0 << 16);
  return ((0xF0u | (c >> 18)) & 0xFFu) | (t2 << 8) | (t1 << 16) | (t0 << 24);
}

// A code point's UTF-8 bytes as vocab ids through a byte -> id table, written to dst[0 .. len);
// returns len.  Id: uint16_t in training (global memory), int32_t in inference (LDS; -1 = the
// byte-level char is not in the vocab, kept by an int32_t dst and narrowed to 0xFFFF by a uint16_t one).
template <class T, class Id, class Out>
__device__ __forceinline__ int emit_utf8_ids(T cp, const Id* __restrict__ byte2id, Out* __restrict__ dst) {
  const int len = utf8_len(cp);
  uint32_t b = utf8_bytes(cp);
  for (int q = 0; q < len; ++q, b >>= 8) dst[q] = (Out)byte2id[b & 0xFFu];
  return len;
}

// GPT-2 regex from code point i of [.., n): returns the end of the word.
//   's|'t|'re|'ve|'m|'ll|'d| ?\p{L}+| ?\p{N}+| ?[^\s\p{L}\p{N}]+|\s+(?!\S)|\s+
__device__ __forceinline__ int regex_word(const int32_t* cps, const uint8_t* cls, int i, int n) {
  const int c = cps[i];
  if (c == '\'' && i + 1 < n) {
    const int c1 = cps[i + 1];
    if (c1 == 's' || c1 == 't' || c1 == 'm' || c1 == 'd') return i + 2;
    if (i + 2 < n) {
      const int c2 = cps[i + 2];
      if ((c1 == 'r' && c2 == 'e') || (c1 == 'v' && c2 == 'e') || (c1 == 'l' && c2 == 'l')) return i + 3;
    }
  }
  int k = cls[i], st = i;
  if (c == ' ' && i + 1 < n && cls[i + 1] != CLS_WS) { k = cls[i + 1]; st = i + 1; }
  int j;
  if (k != CLS_WS) {
    j = st + 1;
    while (j < n && cls[j] == k) ++j;
  } else {
    j = i + 1;
    while (j < n && cls[j] == CLS_WS) ++j;
    if (j < n && j - i >= 2) --j;  // \s+(?!\S): the last blank starts the next word
  }
  return j;
}

// Exclusive prefix sum over the wave (all 64 lanes active) by DPP: row_shr 1/2/4/8 inside each
// 16-lane row, then row_bcast:15 / row_bcast:31 carry the rows' totals -- no LDS round trip (a
// __shfl_up ladder is six ds_bpermute round trips).
__device__ __forceinline__ int wave_excl_scan(int v, int lane, int& total) {
  int x = v;
  x += __builtin_amdgcn_update_dpp(0, x, 0x111, 0xF, 0xF, false);   // row_shr:1
  x += __builtin_amdgcn_update_dpp(0, x, 0x112, 0xF, 0xF, false);   // row_shr:2
  x += __builtin_amdgcn_update_dpp(0, x, 0x114, 0xF, 0xF, false);   // row_shr:4
  x += __builtin_amdgcn_update_dpp(0, x, 0x118, 0xF, 0xF, false);   // row_shr:8
  x += __builtin_amdgcn_update_dpp(0, x, 0x142, 0xA, 0xF, false);   // row_bcast:15 -> rows 1, 3
  x += __builtin_amdgcn_update_dpp(0, x, 0x143, 0xC, 0xF, false);   // row_bcast:31 -> rows 2, 3
  total = __builtin_amdgcn_readlane(x, 63);
  (void)lane;
  return x - v;
}

// One wave stages a row of n code points (row[0 .. n), all 64 lanes call).  The first 64 * PF
// loads are issued before any is used.  code_point(i, token) is the caller's: it stores the code
// point and its class (class_of) in the caller's image, accumulates the caller's own validity
// flags and returns the code point's UTF-8 length.  The lengths are scanned in the same loop, from
// the register, into so[i] = the first byte symbol of code point i, so[n] = the row's byte
// symbols, which is also the return value.  Rows longer than 64 * PF go on chunk by chunk with
// direct loads (inference rows only: the training kernels skip rows of more than LC = 64 * PF code
// points before the call).  The caller's wave_sync follows.
template <int PF, class Off, class F>
__device__ __forceinline__ int stage_row(const long long* __restrict__ row, int n, int lane, Off* so, F&& code_point) {
  long long tv[PF];
#pragma unroll
  for (int k = 0; k < PF; ++k) tv[k] = (lane + 64 * k < n) ? row[lane + 64 * k] : 0;
  int carry = 0;
  auto chunk = [&](int i, long long t) {
    const int len = i < n ? code_point(i, t) : 0;
    int tot;
    const int ex = wave_excl_scan(len, lane, tot);
    if (i < n) so[i] = (Off)(carry + ex);
    carry += tot;
  };
#pragma unroll
  for (int k = 0; k < PF; ++k) {
    if (64 * k >= n) break;
    chunk(64 * k + lane, tv[k]);
  }
  for (int base = 64 * PF; base < n; base += 64) chunk(base + lane, base + lane < n ? row[base + lane] : 0);
  if (lane == 0) so[n] = (Off)carry;
  return carry;
}

// e[i] = regex_word(cps, cls, i, n) for every i, without the per-position class-run loops: the
// end of each class run comes from one ballot per 64 positions (run[p] = one past the last
// position of p's run; scratch [n]), so every lane's regex end is a few independent reads.
// Every caller passes its wcp array as run: wcp is scratch until word_starts fills it.
__device__ __forceinline__ void regex_ends(const int32_t* cps, const uint8_t* cls, int32_t* run, int32_t* e, int n,
                                           int lane) {
  int carry = n;   // one past the first run end in the chunks after the current one
  for (int base = (n - 1) & ~63; base >= 0; base -= 64) {
    const int p = base + lane;
    const bool in = p < n;
    const int c0 = in ? (int)cls[p] : -1;
    const int c1 = p + 1 < n ? (int)cls[p + 1] : -2;
    const unsigned long long m = __ballot(in && c0 != c1);   // p ends its run
    const unsigned long long rest = m >> lane;
    if (in) run[p] = rest ? p + __builtin_ctzll(rest) + 1 : carry;
    if (m) carry = base + __builtin_ctzll(m) + 1;
  }
  wave_sync();
  for (int i = lane; i < n; i += 64) {
    const int c = cps[i];
    const int c1 = i + 1 < n ? cps[i + 1] : -1, c2 = i + 2 < n ? cps[i + 2] : -1;
    const int k0 = cls[i], k1 = i + 1 < n ? (int)cls[i + 1] : CLS_WS;
    int j;
    if (c == '\'' && (c1 == 's' || c1 == 't' || c1 == 'm' || c1 == 'd')) {
      j = i + 2;
    } else if (c == '\'' && ((c1 == 'r' && c2 == 'e') || (c1 == 'v' && c2 == 'e') || (c1 == 'l' && c2 == 'l'))) {
      j = i + 3;
    } else if (c == ' ' && i + 1 < n && k1 != CLS_WS) {
      j = run[i + 1];                      // " ?" + the run of the next code point's class
    } else if (k0 != CLS_WS) {
      j = run[i];
    } else {
      j = run[i];                          // \s+, giving back the last blank before a non-blank
      if (j < n && j - i >= 2) --j;
    }
    e[i] = j;
  }
  wave_sync();
}

// The word starts of a row from e[i], the end of the regex word that would
// start at code point i: the chain 0 -> e[0] -> e[e[0]] -> ... < n.  Lane-parallel instead of one
// lane following ~n / 2 dependent links: lane s walks the chain from the start of its segment
// [s G, s G + G) (G = ceil(n / 64)), marking what it visits (vis, one byte per code point), and
// records where it leaves the segment.  The true chain enters segment s where it left segment
// s - 1; a marked entry means lane s's walk already is the true chain from there (the chain is a
// function of the position), an entry past the segment means the segment holds no start, and
// any other entry (rare: regex words self-synchronise within a word) makes the lane re-walk its
// segment from it -- repeated until no exit changes.  Starts = marked positions at or past
// their segment's entry, written in order by a wave scan.
// Invariant: the marks in [ws, se) are exactly the positions of the lane's latest walk, which
// started at ws and leaves the segment at wex.  The exit passed on, ex, is wex when the entry lies
// on that walk, or the entry itself when the chain jumps the segment.  A marked entry below ws is
// a mark of an older walk (e.g. "x!'tion": the walk from "'" marks "t" before the chain is known
// to enter at "t"), so only a marked entry at or past ws reuses the walk; anything else re-walks.
// wcp [n + 1] may have been regex_ends' run scratch (it is read no more once e is written).  wspec:
// the words' special-token ids, all set to -1 here -- k_bpe_encode passes its array, k_bpe_words
// and the training kernels have no special tokens and pass null.
__device__ __forceinline__ void word_starts(const int32_t* e, uint8_t* vis, int32_t* wcp, int32_t* wspec,
                                            int32_t* nw_out, int n, int lane) {
  const int G = (n + 63) >> 6;
  const int sb = min(lane * G, n), se = min(sb + G, n);
  for (int i = lane; i < n; i += 64) vis[i] = 0;
  wave_sync();
  int ex = sb;    // exit passed to the next lane: the first chain position >= se (n past the end)
  int ws = sb;    // start of the walk the marks in [ws, se) belong to
  int wex = sb;   // that walk's exit
  if (sb < se) {
    int p = sb;
    while (p < se) { vis[p] = 1; p = e[p]; }
    wex = ex = p;
  }
  int entry = 0;
  while (true) {
    const int prev = __shfl_up(ex, 1);
    const int en = lane == 0 ? 0 : prev;
    int nex = ex;
    bool changed = false;
    if (sb < se) {
      if (en >= se) {
        nex = en;                 // the chain jumps this segment
      } else if (en >= sb && en >= ws && vis[en]) {
        nex = wex;                // the entry lies on the latest walk
      } else if (en >= sb) {
        for (int i = en; i < se; ++i) vis[i] = 0;   // re-walk from the true entry
        int p = en;
        while (p < se) { vis[p] = 1; p = e[p]; }
        nex = wex = p;
        ws = en;
        changed = true;
      }
    } else {
      nex = en > sb ? en : sb;   // empty segment (past n): pass the exit on
    }
    changed |= nex != ex || en != entry;
    ex = nex;
    entry = en;
    if (!__any(changed)) break;
  }
  wave_sync();
  int cnt = 0;
  for (int i = max(sb, entry); i < se; ++i) cnt += vis[i];
  int tot;
  int o = wave_excl_scan(cnt, lane, tot);
  for (int i = max(sb, entry); i < se; ++i)
    if (vis[i]) {
      wcp[o] = i;
      if (wspec) wspec[o] = -1;
      ++o;
    }
  if (lane == 0) { wcp[tot] = n; *nw_out = tot; }
  wave_sync();
}

}  // namespace beast_pt
