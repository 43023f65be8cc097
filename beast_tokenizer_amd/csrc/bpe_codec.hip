// Byte-level BPE *inference* on gfx950: encode bin rows into BPE ids and decode BPE ids
// back into bins.  Replaces, per row,
//   tokenizer.encode("".join(map(chr, row - min)), add_special_tokens=False).ids
//   ord(c) + min for c in tokenizer.decode(ids, skip_special_tokens=True)
// of beast/beast_bspline_bpe_tokenizer.py:175-247 (HF tokenizers 0.22.2: AddedVocabulary
// split, ByteLevel pre-tokeniser, BPE::merge_word + Word::merge_all, ByteLevel decoder,
// String::from_utf8_lossy).
//
// One translation unit over layered headers -- bpe_codec_device.h (constants, status codes, merge
// maps, EncArgs, stamps, pretok_row over pretok.h's pre-tokeniser, which training shares),
// bpe_encode_rows.h (k_bpe_encode), bpe_encode_words.h (k_bpe_words), bpe_decode.h (k_bpe_decode);
// this file keeps the host side: map builders, workspace sizes, dispatch, the C-ABI.
//   k_mergemap_build   open-addressing (a, b) -> (rank, new_id) table + rank -> new_id;
//                      a pair listed twice keeps its LAST rank (HF collects the merges
//                      into a HashMap)
//   k_bpe_encode       one wave per row, 4 rows per workgroup in flight, grid-stride over
//                      rows; the merge map is staged once per workgroup into LDS when it
//                      fits (<= 8192 slots, <= 4096 merges), so every lookup of the merge loop is an LDS
//                      probe, not a dependent HBM/L2 round trip.  Per row, all in LDS:
//                        lanes: code points, range checks, classes, UTF-8 symbol offsets,
//                        GPT-2 regex word starts, byte -> vocab id (pretok_row)
//                        lane 0, special tokens only: their split (leftmost-longest) + regex walk
//                        one word per lane: HF's merge_all with
//                        its (rank, pos) min-heap (stale entries skipped exactly as HF
//                        does, so the result is HF's even when two merges share an id)
//                        lanes: scan of per-word counts, ids written to the padded output
//   k_bpe_decode       one wave per row: lanes gather their ids' bytes into LDS at
//                      scanned offsets; valid UTF-8 (the normal case) decodes lane-
//                      parallel (one lane per lead byte); anything else goes through
//                      Rust's lossy decoder (maximal-subpart U+FFFD) on lane 0
#include <hip/hip_runtime.h>

#include "common.h"
#include "launch.h"
#include "bpe_codec_device.h"
#include "bpe_encode_rows.h"
#include "bpe_encode_words.h"
#include "bpe_decode.h"

namespace {

inline int log2_ceil(int64_t x) {
  int l = 0;
  while ((int64_t(1) << l) < x) ++l;
  return l;
}

// k_bpe_encode, nwv rows (waves) per workgroup: at most the workgroups resident at once (each
// stages the merge map once and then loops over rows)
template <bool MAP, int RM>
int launch_bpe_encode(const EncArgs& a, int nwv, unsigned lds, const Queue& q) {
  const int per_cu = std::max(1, occupancy<k_bpe_encode<MAP, RM>>(64 * nwv, lds, q));
  const int64_t grid = std::min<int64_t>((a.n_rows + nwv - 1) / nwv, (int64_t)cu_count(q.dev) * per_cu);
  return launch<k_bpe_encode<MAP, RM>>((unsigned)grid, 64 * nwv, lds, q, "k_bpe_encode", a);
}

}  // namespace

#ifdef BPE_STAMPS
extern "C" int beast_debug_bpe_stamps(unsigned long long* host) {   // [4096][12]
  return hipMemcpyFromSymbol(host, HIP_SYMBOL(g_bpe_rs), sizeof(g_bpe_rs)) == hipSuccess ? 0 : -2;
}
extern "C" int beast_debug_bpe_task_times(unsigned long long* host, int clear) {   // [4096][8]
  if (clear) {
    static unsigned long long zero[BPE_RS][8];
    return hipMemcpyToSymbol(HIP_SYMBOL(g_bpe_wt), zero, sizeof(zero)) == hipSuccess ? 0 : -2;
  }
  return hipMemcpyFromSymbol(host, HIP_SYMBOL(g_bpe_wt), sizeof(g_bpe_wt)) == hipSuccess ? 0 : -2;
}
#endif

extern "C" int beast_bpe_mergemap_log2cap(int n_merges) {
  const int l = log2_ceil(2 * (int64_t)(n_merges > 0 ? n_merges : 1));
  return l < 6 ? 6 : l;
}

extern "C" size_t beast_bpe_mergemap_bytes(int n_merges) {
  const size_t cap = size_t(1) << beast_bpe_mergemap_log2cap(n_merges);
  return al16(cap * 2 * sizeof(uint32_t)) + al16((size_t)(n_merges > 0 ? n_merges : 1) * sizeof(uint16_t));
}

static MergeMap map_view(const void* map, int n_merges) {
  MergeMap m;
  m.log2cap = beast_bpe_mergemap_log2cap(n_merges);
  const size_t cap = size_t(1) << m.log2cap;
  m.kv = reinterpret_cast<const uint2*>(map);
  m.rank2new = reinterpret_cast<const uint16_t*>(reinterpret_cast<const char*>(map) + al16(cap * 2 * sizeof(uint32_t)));
  return m;
}

extern "C" int beast_bpe_mergemap_build(const int32_t* merge_a, const int32_t* merge_b, const int32_t* merge_new,
                                        int n_merges, void* map, size_t map_bytes, void* stream) {
  BEAST_REQUIRE(n_merges >= 0 && n_merges < 65536, "n_merges out of range (0..65535): %d", n_merges);
  BEAST_REQUIRE(map != nullptr, "mergemap buffer is null");
  BEAST_REQUIRE_CODE(map_bytes >= beast_bpe_mergemap_bytes(n_merges), BEAST_E_WORKSPACE,
                     "mergemap buffer too small: %zu < %zu", map_bytes, beast_bpe_mergemap_bytes(n_merges));
  BEAST_REQUIRE(n_merges == 0 || (merge_a && merge_b && merge_new), "merge arrays are null");
  const MergeMap m = map_view(map, n_merges);
  const int cap = 1 << m.log2cap;
  Queue q;
  BEAST_TRY(queue_of(stream, q, "beast_bpe_mergemap_build"));
  BEAST_TRY(launch<k_mergemap_clear>((cap + 255) / 256, 256, 0, q, "k_mergemap_clear", const_cast<uint2*>(m.kv), cap));
  if (n_merges > 0) {
    BEAST_TRY(launch<k_mergemap_build>((n_merges + 255) / 256, 256, 0, q, "k_mergemap_build", merge_a, merge_b,
                                       merge_new, n_merges, const_cast<uint2*>(m.kv), const_cast<uint16_t*>(m.rank2new),
                                       m.log2cap));
  }
  return BEAST_OK;
}

extern "C" size_t beast_bpe_encode_lds_bytes(int max_row_cps, int max_row_syms) {   // per row (wave)
  return enc_row_bytes(max_row_cps, max_row_syms, enc_needs_heap(max_row_syms, beast::g_bpe_encode_mode & 1));
}

extern "C" int beast_bpe_encode_rows(const int64_t* tok, const int64_t* row_off, int64_t n_rows, int64_t min_tok,
                                     int64_t max_span, const uint8_t* cls_lut, int64_t lut_n, const int32_t* byte2id,
                                     const void* map, int n_merges, const int32_t* spec_cps, const int32_t* spec_len,
                                     const int32_t* spec_id, int n_spec, int unk_id, int fuse_unk, int max_row_cps,
                                     int max_row_syms, int32_t* out_ids, int64_t out_stride, int32_t* out_len,
                                     int32_t* status, void* stream) {
  BEAST_REQUIRE(n_rows >= 0, "n_rows must be >= 0");
  if (n_rows == 0) return BEAST_OK;
  BEAST_REQUIRE(tok && row_off && cls_lut && byte2id && map && out_ids && out_len && status, "null pointer argument");
  BEAST_REQUIRE(lut_n > 0 && lut_n <= 65536, "class LUT size %lld out of range", (long long)lut_n);
  BEAST_REQUIRE(n_merges >= 0 && n_merges < 65536, "n_merges out of range (0..65535): %d", n_merges);
  BEAST_REQUIRE(max_row_cps >= 0 && max_row_cps < 32768, "max_row_cps %d out of range", max_row_cps);
  BEAST_REQUIRE_CODE(max_row_syms >= 0 && max_row_syms <= 16384, BEAST_E_UNSUPPORTED,
                     "rows of %d byte symbols exceed the encoder's per-row LDS budget (16384)", max_row_syms);
  BEAST_REQUIRE(out_stride >= max_row_syms, "out_stride %lld < max_row_syms %d", (long long)out_stride, max_row_syms);
  BEAST_REQUIRE(n_spec >= 0 && n_spec <= MAX_SPECIAL, "at most %d special tokens are supported", MAX_SPECIAL);
  BEAST_REQUIRE(n_spec == 0 || (spec_cps && spec_len && spec_id), "special-token arrays are null");
  const size_t row_b = enc_row_bytes(max_row_cps, max_row_syms, enc_needs_heap(max_row_syms, beast::g_bpe_encode_mode & 1));
  BEAST_REQUIRE_CODE(row_b + STATIC_LDS <= LDS_BUDGET, BEAST_E_UNSUPPORTED,
                     "rows of %d code points / %d byte symbols need %zu B of LDS (> 160 KiB)", max_row_cps,
                     max_row_syms, row_b);
  EncArgs a;
  a.tok = reinterpret_cast<const long long*>(tok);
  a.row_off = row_off; a.n_rows = n_rows; a.min_tok = min_tok; a.max_span = max_span;
  a.lut = cls_lut; a.lut_n = (int)lut_n; a.byte2id = byte2id;
  a.map = map_view(map, n_merges);
  a.n_merges = n_merges;
  // one workgroup per CU holding the merge map once and as many rows (waves) as fit beside it
  // (BEAST_OPT_BPE_ENCODE_MODE bit 1: four waves per workgroup, as many workgroups as fit)
  const size_t map_lds = map_lds_bytes(a.map.log2cap, n_merges);
  const int want_w = (beast::g_bpe_encode_mode & 2) ? WAVES : ENC_MAX_WAVES;
  a.map_in_lds = (map_lds > 0 && map_lds + row_b + STATIC_LDS <= LDS_BUDGET) ? 1 : 0;
  const size_t room = LDS_BUDGET - STATIC_LDS - (a.map_in_lds ? map_lds : 0);
  const int nwv = (int)std::max<size_t>(1, std::min<size_t>((size_t)want_w, room / row_b));
  const size_t rows_lds = (size_t)nwv * row_b;
  a.spec_cps = spec_cps; a.spec_len = spec_len; a.spec_id = spec_id; a.n_spec = n_spec;
  a.unk_id = unk_id; a.fuse_unk = fuse_unk;
  a.heap_merge = beast::g_bpe_encode_mode & 1;
  a.Lc = max_row_cps; a.S = max_row_syms;
  a.out_ids = out_ids; a.out_stride = out_stride; a.out_len = out_len; a.status = status;
  const size_t lds = rows_lds + (a.map_in_lds ? map_lds : 0);
  const bool narrow = max_row_syms <= 64 * RM_NARROW;   // every row fits the narrow kernel's round merge
  Queue q;
  BEAST_TRY(queue_of(stream, q, "beast_bpe_encode_rows"));
  if (a.map_in_lds)
    return narrow ? launch_bpe_encode<true, RM_NARROW>(a, nwv, lds, q) : launch_bpe_encode<true, RM_PER>(a, nwv, lds, q);
  return narrow ? launch_bpe_encode<false, RM_NARROW>(a, nwv, lds, q) : launch_bpe_encode<false, RM_PER>(a, nwv, lds, q);
}

// ---- k_bpe_words' merge map (host build) ----
extern "C" int beast_bpe_wordmap_log2buckets(int n_merges) {   // buckets >= merges: at most half the slots used
  return std::max(4, log2_ceil(std::max(1, n_merges)));
}
extern "C" size_t beast_bpe_wordmap_bytes(int n_merges) {   // room for one doubling if an insertion fails
  return sizeof(uint32_t) * 4 * ((size_t)2 << beast_bpe_wordmap_log2buckets(n_merges));
}
static bool wordmap_try(const int32_t* ma, const int32_t* mb, const int32_t* mn, int n, uint32_t* t, int lb) {
  const size_t nb = (size_t)1 << lb;
  for (size_t i = 0; i < 4 * nb; i += 2) { t[i] = EMPTY_KEY; t[i + 1] = 0u; }
  auto slot_of = [&](uint32_t key) -> uint32_t* {   // the key's slot, if present
    for (uint32_t bk : {wm_h1(key, lb), wm_h2(key, lb)})
      for (int q = 0; q < 2; ++q)
        if (t[4 * bk + 2 * q] == key) return &t[4 * bk + 2 * q];
    return nullptr;
  };
  uint32_t rng = 0x2545F491u;
  for (int i = 0; i < n; ++i) {
    uint32_t key = ((uint32_t)ma[i] << 16) | (uint32_t)mb[i];
    uint32_t val = ((uint32_t)(i + 1) << 16) | (uint32_t)mn[i];
    if (uint32_t* e = slot_of(key)) { e[1] = val; continue; }   // a pair listed twice keeps its last rank
    uint32_t bk = wm_h1(key, lb);
    bool placed = false;
    for (int kick = 0; kick < 512 && !placed; ++kick) {
      for (uint32_t c : {wm_h1(key, lb), wm_h2(key, lb)})
        for (int q = 0; q < 2 && !placed; ++q)
          if (t[4 * c + 2 * q] == EMPTY_KEY) { t[4 * c + 2 * q] = key; t[4 * c + 2 * q + 1] = val; placed = true; }
      if (placed) break;
      // evict a pseudo-random slot of the bucket not just left, carry its key on
      rng ^= rng << 13; rng ^= rng >> 17; rng ^= rng << 5;
      bk = (bk == wm_h1(key, lb)) ? wm_h2(key, lb) : wm_h1(key, lb);
      const int q = rng & 1;
      std::swap(key, t[4 * bk + 2 * q]);
      std::swap(val, t[4 * bk + 2 * q + 1]);
    }
    if (!placed) return false;
  }
  return true;
}
extern "C" int beast_bpe_wordmap_build_host(const int32_t* merge_a, const int32_t* merge_b, const int32_t* merge_new,
                                            int n_merges, void* host_out, size_t bytes, int* log2b_out) {
  BEAST_REQUIRE(n_merges >= 0 && n_merges < 65536, "n_merges out of range (0..65535): %d", n_merges);
  BEAST_REQUIRE(host_out && log2b_out && (n_merges == 0 || (merge_a && merge_b && merge_new)), "null pointer argument");
  BEAST_REQUIRE_CODE(bytes >= beast_bpe_wordmap_bytes(n_merges), BEAST_E_WORKSPACE, "word map buffer %zu < %zu", bytes,
                     beast_bpe_wordmap_bytes(n_merges));
  uint32_t* t = static_cast<uint32_t*>(host_out);
  const int lb0 = beast_bpe_wordmap_log2buckets(n_merges);
  for (int lb = lb0; lb <= lb0 + 1; ++lb)
    if (wordmap_try(merge_a, merge_b, merge_new, n_merges, t, lb)) {
      *log2b_out = lb;
      return BEAST_OK;
    }
  BEAST_REQUIRE_CODE(false, BEAST_E_UNSUPPORTED, "word map: cuckoo insertion failed");
  return BEAST_E_UNSUPPORTED;
}

extern "C" int beast_bpe_encode_rows_words(const int64_t* tok, const int64_t* row_off, int64_t n_rows,
                                           int64_t min_tok, int64_t max_span, const uint8_t* cls_lut, int64_t lut_n,
                                           const int32_t* byte2id, const void* wordmap, int wordmap_log2b, int unk_id,
                                           int fuse_unk, int max_row_cps, int max_row_syms, int32_t* out_ids,
                                           int64_t out_stride, int32_t* out_len, int32_t* status, void* stream) {
  BEAST_REQUIRE(n_rows >= 0, "n_rows must be >= 0");
  if (n_rows == 0) return BEAST_OK;
  BEAST_REQUIRE(tok && row_off && cls_lut && byte2id && wordmap && out_ids && out_len && status, "null pointer argument");
  BEAST_REQUIRE(lut_n > 0 && lut_n <= 65536, "class LUT size %lld out of range", (long long)lut_n);
  BEAST_REQUIRE(wordmap_log2b >= 4 && wordmap_log2b <= 20, "wordmap_log2b %d out of range (4..20)", wordmap_log2b);
  BEAST_REQUIRE(max_row_cps >= 0 && max_row_cps < 32768, "max_row_cps %d out of range", max_row_cps);
  BEAST_REQUIRE(max_row_syms >= 0 && max_row_syms <= 16384, "max_row_syms %d out of range", max_row_syms);
  BEAST_REQUIRE(out_stride >= max_row_syms, "out_stride %lld < max_row_syms %d", (long long)out_stride, max_row_syms);
  EncArgs a{};
  a.tok = reinterpret_cast<const long long*>(tok);
  a.row_off = row_off; a.n_rows = n_rows; a.min_tok = min_tok; a.max_span = max_span;
  a.lut = cls_lut; a.lut_n = (int)lut_n; a.byte2id = byte2id;
  a.unk_id = unk_id; a.fuse_unk = fuse_unk;
  a.Lc = max_row_cps; a.S = max_row_syms;
  a.out_ids = out_ids; a.out_stride = out_stride; a.out_len = out_len; a.status = status;
  const WordMap wm{static_cast<const uint4*>(wordmap), wordmap_log2b};
  // as many rows per workgroup as the LDS holds (<= 16), the merge map staged when it fits beside them
  const size_t room = LDS_BUDGET - STATIC_LDS;
  int map_log2 = wordmap_log2b <= 13 ? wordmap_log2b : -1, nwv = 0;
  for (int pass = 0; pass < 2 && nwv == 0; ++pass) {
    for (int nv = DW_WAVES; nv > 0 && nwv == 0; --nv)
      if (bw_lds_bytes(a.Lc, a.S, nv, map_log2) <= room) nwv = nv;
    if (nwv == 0) map_log2 = -1;
  }
  BEAST_REQUIRE_CODE(nwv > 0, BEAST_E_UNSUPPORTED, "rows of %d code points exceed k_bpe_words' LDS budget", max_row_cps);
  const int ltab_log2 = dw_ltab_log2(a.Lc, nwv);
  const int hash_shift = 32 - std::min(32, std::max(1, beast::g_bpe_dedup_key_bits));
  const size_t lds = bw_lds_bytes(a.Lc, a.S, nwv, map_log2);
  Queue q;
  BEAST_TRY(queue_of(stream, q, "beast_bpe_encode_rows_words"));
  const unsigned grid = (unsigned)((n_rows + nwv - 1) / nwv), block = 64 * nwv;
  return map_log2 >= 0 ? launch<k_bpe_words<true>>(grid, block, lds, q, "k_bpe_words", a, wm, ltab_log2, hash_shift)
                       : launch<k_bpe_words<false>>(grid, block, lds, q, "k_bpe_words", a, wm, ltab_log2, hash_shift);
}

extern "C" int beast_bpe_decode_rows(const int32_t* ids, const int64_t* row_off, int64_t n_rows,
                                     const int32_t* tok_off, const uint8_t* tok_bytes, const uint8_t* tok_skip,
                                     int n_vocab, int unk_id, int64_t min_tok, int L, int64_t* out,
                                     int32_t* out_count, int32_t* status, void* stream) {
  BEAST_REQUIRE(n_rows >= 0, "n_rows must be >= 0");
  if (n_rows == 0) return BEAST_OK;
  BEAST_REQUIRE(ids && row_off && tok_off && tok_bytes && tok_skip && out && out_count && status,
                "null pointer argument");
  BEAST_REQUIRE(n_vocab > 0 && L >= 0, "n_vocab must be > 0 and L >= 0");
  DecArgs a;
  a.ids = ids; a.row_off = row_off; a.n_rows = n_rows; a.tok_off = tok_off; a.tok_bytes = tok_bytes;
  a.tok_skip = tok_skip; a.n_vocab = n_vocab; a.unk_id = unk_id; a.min_tok = min_tok; a.L = L;
  // a row that decodes to L code points holds at most 4 L bytes; more -> streamed from HBM
  int64_t bcap = 4 * (int64_t)L + 16;
  if (bcap > (int64_t)(LDS_BUDGET / WAVES)) bcap = LDS_BUDGET / WAVES;
  a.bcap = (int)bcap;
  a.out = reinterpret_cast<long long*>(out); a.out_count = out_count; a.status = status;
  Queue q;
  BEAST_TRY(queue_of(stream, q, "beast_bpe_decode_rows"));
  const int64_t grid = std::min<int64_t>((n_rows + WAVES - 1) / WAVES, 4 * (int64_t)cu_count(q.dev));
  return launch<k_bpe_decode>((unsigned)grid, BLOCK, WAVES * al16(a.bcap), q, "k_bpe_decode", a);
}

