// Byte-level BPE inference, k_bpe_decode (bpe_codec.hip): ids -> bytes -> code points, with
// Rust's lossy UTF-8 decoder for anything that is not valid UTF-8.
#pragma once

#include "bpe_codec_device.h"

namespace {

// ---------------------------------------------------------------- decode --
struct DecArgs {
  const int32_t* ids;
  const int64_t* row_off;
  int64_t n_rows;
  const int32_t* tok_off;     // [n_vocab + 1] byte ranges of each id's decoded bytes
  const uint8_t* tok_bytes;
  const uint8_t* tok_skip;    // [n_vocab] 1: special (skipped) or no such id
  int n_vocab;
  int unk_id;                 // id of "<unk>", -1: none
  long long min_tok;
  int L;                      // expected code points per row (output row width)
  int bcap;                   // LDS byte buffer per wave
  long long* out;             // [n_rows][L]
  int32_t* out_count;         // decoded code points per row
  int32_t* status;            // bit 0: the row holds the <unk> id; bit 1: an id < -1 (not a u32)
};

__device__ __forceinline__ bool cont(int b) { return (b & 0xC0) == 0x80; }

// One step of Rust's lossy UTF-8 decoder (core::str::lossy::Utf8Chunks) on b0 with the
// next bytes b1..b3 (0 past the end): code point (0xFFFD on error) and bytes consumed.
__device__ __forceinline__ int utf8_step(int b0, int b1, int b2, int b3, int& used) {
  if (b0 < 0x80) { used = 1; return b0; }
  if (b0 >= 0xC2 && b0 <= 0xDF) {
    if (cont(b1)) { used = 2; return ((b0 & 0x1F) << 6) | (b1 & 0x3F); }
    used = 1; return 0xFFFD;
  }
  if (b0 >= 0xE0 && b0 <= 0xEF) {
    const bool ok1 = (b0 == 0xE0) ? (b1 >= 0xA0 && b1 <= 0xBF) : (b0 == 0xED) ? (b1 >= 0x80 && b1 <= 0x9F)
                                                                              : (b1 >= 0x80 && b1 <= 0xBF);
    if (!ok1) { used = 1; return 0xFFFD; }
    if (!cont(b2)) { used = 2; return 0xFFFD; }
    used = 3; return ((b0 & 0x0F) << 12) | ((b1 & 0x3F) << 6) | (b2 & 0x3F);
  }
  if (b0 >= 0xF0 && b0 <= 0xF4) {
    const bool ok1 = (b0 == 0xF0) ? (b1 >= 0x90 && b1 <= 0xBF) : (b0 == 0xF4) ? (b1 >= 0x80 && b1 <= 0x8F)
                                                                              : (b1 >= 0x80 && b1 <= 0xBF);
    if (!ok1) { used = 1; return 0xFFFD; }
    if (!cont(b2)) { used = 2; return 0xFFFD; }
    if (!cont(b3)) { used = 3; return 0xFFFD; }
    used = 4; return ((b0 & 0x07) << 18) | ((b1 & 0x3F) << 12) | ((b2 & 0x3F) << 6) | (b3 & 0x3F);
  }
  used = 1; return 0xFFFD;
}

// serial lossy decode of a byte source (get(i) for i < nb); returns the code point count
template <class Get>
__device__ int decode_serial(Get get, int64_t nb, long long* out, int L, long long min_tok) {
  int cnt = 0;
  int64_t i = 0;
  while (i < nb) {
    const int b0 = get(i);
    const int b1 = i + 1 < nb ? get(i + 1) : 0, b2 = i + 2 < nb ? get(i + 2) : 0, b3 = i + 3 < nb ? get(i + 3) : 0;
    int used;
    const int cp = utf8_step(b0, b1, b2, b3, used);
    if (cnt < L) out[cnt] = (long long)cp + min_tok;
    ++cnt;
    i += used;
  }
  return cnt;
}

__device__ __forceinline__ int tok_len(const DecArgs& a, int id) {
  if (id < 0 || id >= a.n_vocab || a.tok_skip[id]) return 0;
  return a.tok_off[id + 1] - a.tok_off[id];
}

__device__ void decode_row(const DecArgs& a, uint8_t* buf, int64_t r, int lane) {
  const int64_t i0 = a.row_off[r], i1 = a.row_off[r + 1];
  const int n = (int)(i1 - i0);
  long long* out = a.out + r * (int64_t)a.L;
  int unk = 0, ovf = 0;
  // gather bytes into LDS at scanned offsets
  int64_t nb = 0;
  for (int base = 0; base < n; base += 64) {
    const int i = base + lane;
    const int id = (i < n) ? a.ids[i0 + i] : -1;
    unk |= (a.unk_id >= 0 && id == a.unk_id);
    ovf |= (id < -1);
    const int len = tok_len(a, id);
    int tot;
    const int ex = wave_excl_scan(len, lane, tot);
    const int64_t o = nb + ex;
    if (len > 0 && o + len <= a.bcap) {
      const uint8_t* src = a.tok_bytes + a.tok_off[id];
      for (int q = 0; q < len; ++q) buf[o + q] = src[q];
    }
    nb += tot;
  }
  const int flags = (__any(unk) ? 1 : 0) | (__any(ovf) ? 2 : 0);
  wave_sync();
  int cnt = -1;
  if (nb <= a.bcap) {
    // valid UTF-8 check and lane-parallel decode: every lead's sequence well-formed and
    // the continuation bytes exactly those the leads claim
    int bad = 0, claimed = 0, conts = 0;
    for (int i = lane; i < nb; i += 64) {
      const int b0 = buf[i];
      if (cont(b0)) { ++conts; continue; }
      const int b1 = i + 1 < nb ? buf[i + 1] : 0, b2 = i + 2 < nb ? buf[i + 2] : 0,
                b3 = i + 3 < nb ? buf[i + 3] : 0;
      int used;
      const int cp = utf8_step(b0, b1, b2, b3, used);
      bad |= (cp == 0xFFFD && !(b0 == 0xEF && b1 == 0xBF && b2 == 0xBD));   // a literal U+FFFD is valid
      claimed += used - 1;
    }
    for (int o = 32; o > 0; o >>= 1) {
      claimed += __shfl_xor(claimed, o);
      conts += __shfl_xor(conts, o);
    }
    if (!__any(bad) && claimed == conts) {
      int carry = 0;
      for (int base = 0; base < nb; base += 64) {
        const int i = base + lane;
        const bool lead = i < nb && !cont(buf[i]);
        int tot;
        const int ex = wave_excl_scan(lead ? 1 : 0, lane, tot);
        if (lead) {
          const int k = carry + ex;
          if (k < a.L) {
            const int b1 = i + 1 < nb ? buf[i + 1] : 0, b2 = i + 2 < nb ? buf[i + 2] : 0,
                      b3 = i + 3 < nb ? buf[i + 3] : 0;
            int used;
            out[k] = (long long)utf8_step(buf[i], b1, b2, b3, used) + a.min_tok;
          }
        }
        carry += tot;
      }
      cnt = carry;
    } else if (lane == 0) {
      cnt = decode_serial([&](int64_t i) { return (int)buf[i]; }, nb, out, a.L, a.min_tok);
    }
  } else if (lane == 0) {
    // more bytes than the LDS buffer holds (the row cannot decode to L code points anyway):
    // stream them from HBM to get HF's exact count for the error message
    const int32_t* ids = a.ids + i0;
    int64_t ti = 0;
    int32_t bo = 0, be = 0;
    auto next_byte = [&]() -> int {
      while (bo >= be) {
        if (ti >= n) return -1;
        const int id = ids[ti++];
        if (tok_len(a, id) == 0) continue;
        bo = a.tok_off[id];
        be = a.tok_off[id + 1];
      }
      return a.tok_bytes[bo++];
    };
    int bq[4], nq = 0, c = 0;
    while (true) {
      while (nq < 4) {
        const int b = next_byte();
        if (b < 0) break;
        bq[nq++] = b;
      }
      if (nq == 0) break;
      int used;
      const int cp = utf8_step(bq[0], nq > 1 ? bq[1] : 0, nq > 2 ? bq[2] : 0, nq > 3 ? bq[3] : 0, used);
      if (c < a.L) out[c] = (long long)cp + a.min_tok;
      ++c;
      for (int k = used; k < nq; ++k) bq[k - used] = bq[k];
      nq -= used;
    }
    cnt = c;
  }
  if (lane == 0) { a.out_count[r] = cnt; a.status[r] = flags; }
}

__global__ __launch_bounds__(BLOCK) void k_bpe_decode(DecArgs a) {
  extern __shared__ __align__(16) char lds_raw[];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  uint8_t* buf = (uint8_t*)lds_raw + (size_t)wave * al16(a.bcap);
  for (int64_t r = (int64_t)blockIdx.x * WAVES + wave; r < a.n_rows; r += (int64_t)gridDim.x * WAVES) {
    decode_row(a, buf, r, lane);
    wave_sync();
  }
}

}  // namespace
