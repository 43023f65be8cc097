// beast_bpe_train: the whole byte-level BPE training in one C-ABI call (host code over the
// library's own entry points) -- what FIGBPE.fit_from_sequences does through HF
// (beast/beast_bpe_trainer.py:61-74, :76-98: BpeTrainer(vocab_size, min_frequency,
// special_tokens, initial_alphabet = chr(0 .. max - min), max_token_length) on the strings
// "".join(map(chr, seq - min))).  The same steps as beast_tokenizer_amd/bpe_train.py:train_bpe
// on one GPU: min / max, the code points present, the alphabet (special tokens, then byte-level
// chars by code point), pre-tokenisation (count, scan, emit), distinct words x counts, the
// length-ordered repack + word signatures, the pair table, then the device-driven batched
// merge loop with two chunks of passes in flight, and the host replay of its merge log against
// the real strings.  Vt <= 4,096 runs the batched loop; larger vocabularies (Vt <= 32,768, the
// dense pair table) the host-driven one (one merge per host round trip, bpe_train.py's loop
// below the device loop), as does a rerun after a 64-bit string-hash collision or a full merge
// log of the batched loop.  beast_bpe_train_comm is the same over several GPUs with the library's communicator
// (comm.hip): bpe_train.py's replicated form -- the range and presence all-reduced, the shards'
// distinct words all-gathered once, the loop run on the union on every rank.
//
// Everything that never touches the device (alphabet, token hashes, the merge step, the replay)
// is bpe_vocab.h.  Here, Trainer has one method per stage, and Trainer::run is the only place that
// issues collectives -- see the rule above it.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <optional>
#include <vector>

#include "bpe_vocab.h"
#include "common.h"
#include "launch.h"

namespace beast {
int g_bpe_train_host = 0;
}

namespace {

namespace bpe = beast::bpe;

// device allocations released on every return path
struct DevMem {
  std::vector<void*> ptrs;
  ~DevMem() {
    for (void* p : ptrs) (void)hipFree(p);
  }
  template <class T>
  T* get(size_t count) {
    void* p = nullptr;
    if (hipMalloc(&p, std::max<size_t>(count, 1) * sizeof(T)) != hipSuccess) return nullptr;
    ptrs.push_back(p);
    return static_cast<T*>(p);
  }
};

struct HostPinned {
  void* p = nullptr;
  ~HostPinned() {
    if (p) (void)hipHostFree(p);
  }
};

constexpr int KMAX = 8, CHUNK = 64;
constexpr int STATE_WORDS = 16;   // the int32 words of the loop state the host reads (BEAST_BPE_STATE_*)

// rank r's word starts index its own symbols: shift them by where its symbols land in the union
__global__ void k_offset_starts(uint32_t* __restrict__ w, int64_t n, uint32_t off) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) w[i] += off;
}

// the arguments of beast_bpe_train (include/beast_hip.h)
struct TrainArgs {
  const int64_t* tokens;
  const int64_t* seq_off;
  int64_t n_seq;
  const uint8_t* cls_lut;
  int64_t lut_n;
  int vocab_size, min_frequency, max_token_length;
  const char* const* special_tokens;
  int n_special;
  int64_t *out_min_token, *out_max_token;
  char* out_vocab_bytes;
  size_t vocab_bytes_cap;
  int64_t* out_vocab_off;
  int max_vocab;
  int* out_n_vocab;
  int32_t* out_merges;
  int max_merges_out;
  int* out_n_merges;
};

// the batched loop asks for the host-driven one (a 64-bit string-hash collision, or a full merge
// log): Trainer::run returns RERUN, the entry point destroys the trainer -- every device buffer of
// the attempt -- and trains again with host_loop set: the peak memory stays one training's
constexpr int RERUN = 1;

// distinct words x counts, length-ordered: n words, n_sym symbols with every span rounded up to 4
struct Words {
  uint16_t* sym = nullptr;
  uint32_t *start = nullptr, *len = nullptr, *count = nullptr;
  int64_t n = 0, n_sym = 0;
};

class Trainer {
 public:
  Trainer(const TrainArgs& args, beast_comm* comm, bool replicate, bool host_loop, const Queue& q)
      : a(args), comm(comm), replicated(comm != nullptr && replicate), sharded(comm != nullptr && !replicate),
        host_loop(host_loop), q(q), s(q.s), stream(q.s) {}
  int run();

 private:
  int agree(int rc) { return beast::comm_agree(comm, rc, s); }
  int allreduce(void* buf, int64_t n, int dtype, int op) {
    return beast_comm_allreduce(comm, buf, buf, n, dtype, op, stream);
  }
  template <class T>
  int alloc(T*& p, size_t n) {
    p = mem.get<T>(n);
    BEAST_REQUIRE_CODE(p != nullptr, BEAST_E_HIP, "beast_bpe_train: hipMalloc of %zu x %zu bytes failed", n, sizeof(T));
    return BEAST_OK;
  }
  int fetch(void* host, const void* dev, size_t bytes, const char* what) {   // a device value read, waited for
    BEAST_HIP(hipMemcpyAsync(host, dev, bytes, hipMemcpyDeviceToHost, s), what);
    BEAST_HIP(hipStreamSynchronize(s), "stream sync");
    return BEAST_OK;
  }
  bool host_done() const { return vocab->size() >= a.vocab_size || !frequent(key >> 32); }
  bool frequent(uint64_t count) const { return count >= 1 && count >= (uint64_t)std::max(a.min_frequency, 0); }

  const TrainArgs& a;
  beast_comm* const comm;
  const bool replicated;   // a communicator, and every rank runs the loop on the union of the words
  const bool sharded;      // a communicator, and every rank keeps its shard of the words
  const bool host_loop;    // the attempt after RERUN
  const Queue& q;
  const hipStream_t s;
  void* const stream;
  DevMem mem;
  HostPinned pinned;

  int64_t n_tok = 0, mn = 0, mx = 0, n_cp = 0;
  int64_t* red = nullptr;       // [2] on the device: what the token count and the range are all-reduced in,
                                //     then the count a dedup or a repack writes
  int64_t lo_nhi[2] = {0, 0};   // (min, -max): one MIN reduces both
  uint8_t* pr = nullptr;        // [n_cp] code points present
  std::optional<bpe::Vocab> vocab;
  int n_base = 0, Vt = 0, max_len = 0;
  Words w;
  // the union of the ranks' words: sizes [2 + 2 * world] on the device, then counts and
  // displacements of the words and of the symbols' bytes, the gathered arrays
  int world = 0;
  int64_t* sz = nullptr;
  int64_t mine[2] = {0, 0};
  std::vector<int64_t> wc, wd, bc, bd;
  int64_t NU = 0, NS = 0;
  uint16_t* gsym = nullptr;
  uint32_t *gw = nullptr, *gl = nullptr, *gc = nullptr;
  uint64_t* sig = nullptr;
  uint32_t* table = nullptr;
  // both loops
  bpe::TokenHashes th;
  uint64_t* hp_d = nullptr;
  uint32_t* tlen_d = nullptr;
  uint64_t* argws = nullptr;
  std::vector<int32_t> merge_ids;   // (a, b) per merge
  int n_log = 0;
  bool rerun = false;
  // host-driven loop
  int32_t* deltas = nullptr;
  uint64_t key = 0;           // the table's best pair: count << 32 | ~(a * Vt + b)
  int call = 0;
  int ma = 0, mb = 0, mnid = 0;   // the merge under way
  // batched loop
  int log_cap = 0;
  size_t bw_bytes = 0, nbd = 0;
  uint8_t *lws = nullptr, *bws = nullptr;
  int32_t* bdeltas = nullptr;   // sharded: each pass's pair-count changes, summed over the ranks
  const void* st_p = nullptr;
  const void* log_p = nullptr;

  // ---- the stages: local work only, each returns its status, except union_words, host_driven and
  // batch_sharded, which hold collectives and return an agreed one

  // ---- arguments, this shard's token count
  int arguments() {
    BEAST_REQUIRE(a.seq_off && a.cls_lut && a.out_min_token && a.out_max_token && a.out_vocab_bytes &&
                      a.out_vocab_off && a.out_n_vocab && a.out_merges && a.out_n_merges &&
                      (a.n_special == 0 || a.special_tokens),
                  "beast_bpe_train: null pointer argument");
    // with a communicator a rank may hold no sequences at all (its shard of the corpus is empty;
    // the total is checked after the sum); alone, the reference's "no non-empty sequences" rule applies
    BEAST_REQUIRE(a.n_seq >= (comm != nullptr ? 0 : 1) && a.vocab_size >= 1 && a.n_special >= 0,
                  "beast_bpe_train: bad sizes");
    BEAST_TRY(fetch(&n_tok, a.seq_off + a.n_seq, sizeof(int64_t), "seq_off read"));
    BEAST_REQUIRE(n_tok >= 0 && (n_tok == 0 || a.tokens != nullptr), "beast_bpe_train: null pointer argument");
    BEAST_TRY(alloc(red, 2));
    if (comm != nullptr) {
      BEAST_HIP(hipMemcpyAsync(red, &n_tok, sizeof(int64_t), hipMemcpyHostToDevice, s), "token count upload");
    } else {
      BEAST_REQUIRE(n_tok > 0, "No non-empty sequences provided for BPE training.");   // reference :84-85
    }
    return BEAST_OK;
  }

  // ---- min / max (reference :86-87); with a communicator the shards' token count, range and code
  // points are the corpus's
  int range() {
    if (comm != nullptr) {
      int64_t total = 0;
      BEAST_TRY(fetch(&total, red, sizeof(int64_t), "token count read"));
      BEAST_REQUIRE(total > 0, "No non-empty sequences provided for BPE training.");   // reference :84-85
    }
    constexpr int64_t NONE = int64_t(1) << 62;   // an empty shard's (min, -max)
    int64_t mmh[2] = {NONE, -NONE};
    if (n_tok > 0) {
      int64_t* mm = nullptr;
      BEAST_TRY(alloc(mm, 2));
      BEAST_TRY(beast_i64_minmax(a.tokens, n_tok, mm, stream));
      BEAST_TRY(fetch(mmh, mm, sizeof(mmh), "minmax read"));
    }
    mn = mmh[0], mx = mmh[1];
    if (comm != nullptr) {   // one MIN over (min, -max)
      lo_nhi[0] = mn, lo_nhi[1] = -mx;
      BEAST_HIP(hipMemcpyAsync(red, lo_nhi, sizeof(lo_nhi), hipMemcpyHostToDevice, s), "range upload");
    }
    return BEAST_OK;
  }

  // ---- the code points present
  int presence() {
    if (comm != nullptr) {
      BEAST_TRY(fetch(lo_nhi, red, sizeof(lo_nhi), "range read"));
      mn = lo_nhi[0], mx = -lo_nhi[1];
    }
    const int64_t K = mx - mn;
    n_cp = K + 1;
    BEAST_REQUIRE_CODE(K < 0xD800, BEAST_E_UNSUPPORTED,
                       "BPE alphabet reaches the UTF-16 surrogate range (max - min token >= 55296)");
    BEAST_REQUIRE(a.lut_n >= K + 1, "beast_bpe_train: class LUT covers %lld code points, the corpus needs %lld",
                  (long long)a.lut_n, (long long)(K + 1));
    BEAST_TRY(alloc(pr, n_cp));
    if (n_tok > 0) {
      BEAST_TRY(beast_bpe_cp_presence(a.tokens, n_tok, mn, pr, n_cp, stream));
    } else {
      BEAST_HIP(hipMemsetAsync(pr, 0, n_cp, s), "presence memset");
    }
    return BEAST_OK;
  }

  // ---- alphabet (HF BpeTrainer: special tokens, then compute_alphabet by code point), and the
  // output capacities against the sizes known so far
  int alphabet() {
    std::vector<uint8_t> present(n_cp);
    BEAST_TRY(fetch(present.data(), pr, n_cp, "presence read"));
    vocab.emplace(present.data(), n_cp, a.special_tokens, a.n_special);
    n_base = vocab->size();
    Vt = std::max(a.vocab_size, n_base);
    max_len = a.max_token_length > 0 ? a.max_token_length : 0x7FFFFFFF;
    BEAST_REQUIRE_CODE(Vt <= 32768, BEAST_E_UNSUPPORTED, "beast_bpe_train: Vt %d > 32768 (the dense pair table)", Vt);
    if (a.max_vocab < Vt || a.max_merges_out < std::max(a.vocab_size - n_base, 0)) {
      // the sizes a retry needs (upper bounds until the training has run)
      *a.out_n_vocab = Vt;
      *a.out_n_merges = std::max(a.vocab_size - n_base, 0);
      BEAST_REQUIRE_CODE(false, BEAST_E_WORKSPACE,
                         "beast_bpe_train: output capacity (vocab %d, merges %d) below the vocabulary size %d; the "
                         "required sizes are in *out_n_vocab, *out_n_merges",
                         a.max_vocab, a.max_merges_out, Vt);
    }
    return BEAST_OK;
  }

  // the length-ordered, contiguous copy of n words (start ow, length ol, count oc in sym, n_sym
  // symbols) that the loop scans: w
  int repack(const uint16_t* sym, const uint32_t* ow, const uint32_t* ol, const uint32_t* oc, int64_t n,
                      int64_t n_sym, const char* whose) {
    const size_t rp_bytes = beast_bpe_repack_workspace_bytes(n);
    uint8_t* rp_ws = nullptr;
    BEAST_TRY(alloc(rp_ws, rp_bytes));
    w.sym = mem.get<uint16_t>(n_sym + 3 * n);   // spans rounded up to 4
    w.start = mem.get<uint32_t>(n);
    w.len = mem.get<uint32_t>(n);
    w.count = mem.get<uint32_t>(n);
    BEAST_REQUIRE_CODE(w.sym && w.start && w.len && w.count, BEAST_E_HIP,
                       "beast_bpe_train: hipMalloc of the %s words failed", whose);
    BEAST_TRY(beast_bpe_repack_words(sym, ow, ol, oc, n, rp_ws, rp_bytes, w.sym, w.start, w.len, w.count, red, stream));
    BEAST_TRY(fetch(&w.n_sym, red, sizeof(int64_t), "symbol count read"));
    w.n = n;
    return BEAST_OK;
  }

  // ---- this shard's words: pre-tokenisation (count, scan, emit), the distinct words x counts (the
  // table grows 4x while it overflows) and their length-ordered repack
  int shard_words() {
    if (n_tok == 0) return BEAST_OK;
    const int64_t n_seq = a.n_seq;
    int64_t *wps = nullptr, *sps = nullptr, *woff = nullptr, *soff = nullptr;
    uint8_t* scan_ws = nullptr;
    BEAST_TRY(alloc(wps, n_seq));
    BEAST_TRY(alloc(sps, n_seq));
    BEAST_TRY(beast_bpe_pretok_count(a.tokens, a.seq_off, n_seq, mn, a.cls_lut, a.lut_n, wps, sps, stream));
    BEAST_TRY(alloc(scan_ws, beast_scan_workspace_bytes(n_seq)));
    BEAST_TRY(alloc(woff, n_seq + 1));
    BEAST_TRY(alloc(soff, n_seq + 1));
    BEAST_TRY(beast_exclusive_scan_i64(wps, woff, n_seq, scan_ws, stream));
    BEAST_TRY(beast_exclusive_scan_i64(sps, soff, n_seq, scan_ws, stream));
    int64_t nw = 0, ns = 0;
    BEAST_HIP(hipMemcpyAsync(&nw, woff + n_seq, sizeof(int64_t), hipMemcpyDeviceToHost, s), "word count read");
    BEAST_TRY(fetch(&ns, soff + n_seq, sizeof(int64_t), "symbol count read"));
    BEAST_REQUIRE_CODE(ns < (int64_t(1) << 32), BEAST_E_UNSUPPORTED,
                       "BPE corpus has >= 2^32 byte symbols on one GPU; shard it over more ranks");
    uint16_t *b2i_d = nullptr, *sym = nullptr;
    uint32_t *wstart = nullptr, *wlen = nullptr, *ow = nullptr, *ol = nullptr, *oc = nullptr;
    BEAST_TRY(alloc(b2i_d, 256));
    BEAST_HIP(hipMemcpyAsync(b2i_d, vocab->byte2id, sizeof(vocab->byte2id), hipMemcpyHostToDevice, s), "byte2id upload");
    BEAST_TRY(alloc(sym, ns));
    BEAST_TRY(alloc(wstart, nw));
    BEAST_TRY(alloc(wlen, nw));
    BEAST_TRY(beast_bpe_pretok_emit(a.tokens, a.seq_off, n_seq, mn, a.cls_lut, a.lut_n, woff, soff, b2i_d, sym, wstart,
                                    wlen, stream));
    BEAST_TRY(alloc(ow, nw));
    BEAST_TRY(alloc(ol, nw));
    BEAST_TRY(alloc(oc, nw));
    int64_t nu = -1;
    for (size_t nbytes = beast_bpe_dedup_workspace_bytes(nw); nu < 0; nbytes *= 4) {
      void* dws = nullptr;
      BEAST_HIP(hipMalloc(&dws, nbytes), "dedup workspace");
      int rc = beast_bpe_dedup_words(sym, wstart, wlen, nw, dws, nbytes, ow, ol, oc, red, stream);
      if (rc == BEAST_OK) rc = fetch(&nu, red, sizeof(int64_t), "distinct count read");
      (void)hipFree(dws);
      BEAST_TRY(rc);
    }
    return repack(sym, ow, ol, oc, nu, ns, "repacked");
  }

  // ---- with a communicator, replicated: every rank's distinct words x counts on every rank, in
  // rank order, repacked for the loop (bpe_train.py GpuBpeOps.gather_words): one all-gather of the
  // sizes, then one all-gather-v per array.  A word repeated across shards appears once per shard
  // with its shard count, which leaves every pair count (and so every merge) unchanged.
  int union_sizes() {
    BEAST_TRY(beast_comm_info(comm, &world, nullptr, nullptr));
    BEAST_TRY(alloc(sz, 2 + 2 * (size_t)world));
    mine[0] = w.n, mine[1] = w.n_sym;
    BEAST_HIP(hipMemcpyAsync(sz, mine, sizeof(mine), hipMemcpyHostToDevice, s), "size upload");
    return BEAST_OK;
  }

  int union_alloc() {
    std::vector<int64_t> all(2 * (size_t)world);
    BEAST_TRY(fetch(all.data(), sz + 2, sizeof(int64_t) * all.size(), "size read"));
    wc.resize(world), wd.resize(world), bc.resize(world), bd.resize(world);   // words; symbol bytes
    for (int r = 0; r < world; ++r) {
      wc[r] = all[2 * r];
      wd[r] = NU;
      bc[r] = 2 * all[2 * r + 1];
      bd[r] = 2 * NS;
      NU += all[2 * r];
      NS += all[2 * r + 1];
    }
    BEAST_REQUIRE_CODE(NS + 3 * NU < (int64_t(1) << 32), BEAST_E_UNSUPPORTED,
                       "beast_bpe_train: the shards' distinct words hold >= 2^32 symbols; the replicated loop keeps "
                       "them on every GPU");
    if (NU == 0) return BEAST_OK;
    BEAST_TRY(alloc(gsym, NS));
    BEAST_TRY(alloc(gw, NU));
    BEAST_TRY(alloc(gl, NU));
    BEAST_TRY(alloc(gc, NU));
    return BEAST_OK;
  }

  int union_repack() {
    for (int r = 0; r < world; ++r)
      if (wc[r] > 0 && bd[r] > 0) {
        BEAST_TRY(launch<k_offset_starts>((unsigned)((wc[r] + 255) / 256), 256, 0, q, "k_offset_starts", gw + wd[r],
                                          wc[r], (uint32_t)(bd[r] / 2)));
      }
    return repack(gsym, gw, gl, gc, NU, NS, "union's");
  }

  // on return the union's gathered words wait for union_repack, the next local stage, unless no
  // rank has a word (NU == 0, the same on every rank)
  int union_words() {
    BEAST_TRY(agree(union_sizes()));
    BEAST_TRY(beast_comm_allgather(comm, sz, sz + 2, 2, BEAST_DT_I64, stream));
    BEAST_TRY(agree(union_alloc()));
    if (NU == 0) {
      w = Words();
      return BEAST_OK;
    }
    BEAST_TRY(beast_comm_allgatherv(comm, w.sym, gsym, bc.data(), bd.data(), BEAST_DT_U8, stream));
    BEAST_TRY(beast_comm_allgatherv(comm, w.start, gw, wc.data(), wd.data(), BEAST_DT_U32, stream));
    BEAST_TRY(beast_comm_allgatherv(comm, w.len, gl, wc.data(), wd.data(), BEAST_DT_U32, stream));
    BEAST_TRY(beast_comm_allgatherv(comm, w.count, gc, wc.data(), wd.data(), BEAST_DT_U32, stream));
    return BEAST_OK;
  }

  // ---- the word signatures and the pair table
  int pair_table() {
    if (w.sym == nullptr) {   // no words anywhere: an empty table, the loop stops at once
      uint16_t* z16 = nullptr;
      uint32_t* z32 = nullptr;
      BEAST_TRY(alloc(z16, 4));
      BEAST_TRY(alloc(z32, 3));
      BEAST_HIP(hipMemsetAsync(z16, 0, 8, s), "empty words");
      BEAST_HIP(hipMemsetAsync(z32, 0, 12, s), "empty words");
      w.sym = z16, w.start = z32, w.len = z32 + 1, w.count = z32 + 2;
    }
    BEAST_TRY(alloc(sig, w.n));
    if (w.n > 0) BEAST_TRY(beast_bpe_word_signatures(w.sym, w.start, w.len, w.n, sig, stream));
    BEAST_TRY(alloc(table, (size_t)Vt * Vt));
    BEAST_HIP(hipMemsetAsync(table, 0, sizeof(uint32_t) * (size_t)Vt * Vt, s), "pair table memset");
    return beast_bpe_count_pairs(w.sym, w.start, w.len, w.count, w.n, table, Vt, n_base, stream);
  }

  // ---- what both loops start from: the tokens' hashes and lengths, the argmax workspace
  int loop_state() {
    th = bpe::token_hashes(*vocab);
    th.tlen.resize(Vt, 0u);
    BEAST_TRY(alloc(hp_d, th.hp.size()));
    BEAST_TRY(alloc(tlen_d, Vt));
    BEAST_HIP(hipMemcpyAsync(hp_d, th.hp.data(), sizeof(uint64_t) * th.hp.size(), hipMemcpyHostToDevice, s),
              "hash upload");
    BEAST_HIP(hipMemcpyAsync(tlen_d, th.tlen.data(), sizeof(uint32_t) * Vt, hipMemcpyHostToDevice, s), "tlen upload");
    const size_t aw_words = (beast_bpe_argmax_workspace_bytes(Vt) + 7) / 8;
    BEAST_TRY(alloc(argws, aw_words));
    BEAST_HIP(hipMemsetAsync(argws, 0, aw_words * 8, s), "argmax workspace memset");
    return BEAST_OK;
  }

  // ---- host-driven loop (bpe_train.py train_bpe below the device loop): argmax, merge in every
  // word, apply + next argmax; one host read of the decided pair per merge.  Its merges go straight
  // into the vocabulary.
  int host_setup() {
    BEAST_TRY(loop_state());
    BEAST_TRY(alloc(deltas, 4 * (size_t)Vt));
    BEAST_HIP(hipMemsetAsync(deltas, 0, sizeof(int32_t) * 4 * (size_t)Vt, s), "deltas memset");
    BEAST_HIP(hipHostMalloc(&pinned.p, 64, hipHostMallocDefault), "pinned key");
    BEAST_TRY(beast_bpe_argmax(table, Vt, n_base, argws, call, stream));
    BEAST_TRY(fetch(pinned.p, argws + 2 + (call++ & 1), sizeof(uint64_t), "argmax read"));
    key = *static_cast<uint64_t*>(pinned.p);
    return BEAST_OK;
  }

  // one merge, first half: the pair of `key` merged in this rank's words, the changes of the pair
  // counts left in deltas (sharded: summed over the ranks before host_apply)
  int host_merge() {
    const uint32_t idx = 0xFFFFFFFFu - (uint32_t)(key & 0xFFFFFFFFu);
    ma = (int)(idx / (uint32_t)Vt), mb = (int)(idx % (uint32_t)Vt);
    BEAST_REQUIRE_CODE(vocab->has(ma) && vocab->has(mb), BEAST_E_HIP,
                       "beast_bpe_train: argmax returned pair (%d, %d) outside the vocabulary", ma, mb);
    mnid = vocab->merge(ma, mb).nid;
    merge_ids.insert(merge_ids.end(), {ma, mb});
    ++n_log;
    return beast_bpe_merge(w.sym, w.start, w.len, w.count, w.n, ma, mb, mnid, tlen_d, max_len, deltas, Vt, sig,
                           (int64_t)(key >> 32), stream);
  }

  // second half: the table's update and the next pair's key; the last merge searches no more and
  // leaves the stream drained instead
  int host_apply() {
    const int k = call++;
    BEAST_TRY(beast_bpe_apply_argmax(table, deltas, Vt, vocab->size(), ma, mb, mnid, tlen_d, argws, k, stream));
    if (vocab->size() >= a.vocab_size) {
      BEAST_HIP(hipStreamSynchronize(s), "stream sync");
      return BEAST_OK;
    }
    BEAST_TRY(fetch(pinned.p, argws + 2 + (k & 1), sizeof(uint64_t), "argmax read"));
    key = *static_cast<uint64_t*>(pinned.p);
    return BEAST_OK;
  }

  // Sharded, every merge holds a collective, so its status is agreed before the next one's; the
  // replicated form and the single GPU run the loop alone, a failed step ends it, and one agreement
  // follows.
  int host_driven() {
    int rc = BEAST_OK;
    while (true) {
      if (sharded) BEAST_TRY(agree(rc));
      if (rc != BEAST_OK || host_done()) break;
      rc = host_merge();
      if (sharded) BEAST_TRY(allreduce(deltas, 4 * (int64_t)Vt, BEAST_DT_I32, BEAST_OP_SUM));
      if (rc == BEAST_OK) rc = host_apply();
    }
    return sharded ? rc : agree(rc);
  }

  // ---- batched loop (bpe_loop.hip): merges decided on the device, up to KMAX per pass
  int batch_setup() {
    BEAST_TRY(loop_state());
    log_cap = bpe::loop_log_capacity(a.vocab_size, n_base);
    const size_t lws_bytes = beast_bpe_loop_workspace_bytes(Vt, log_cap);
    bw_bytes = beast_bpe_batch_workspace_bytes(Vt);
    nbd = beast_bpe_batch_delta_count(Vt);
    BEAST_TRY(alloc(lws, lws_bytes));
    BEAST_TRY(beast_bpe_loop_init(lws, lws_bytes, Vt, log_cap, n_base, a.vocab_size, a.min_frequency, hp_d,
                                  hp_d + n_base, tlen_d, th.max_tlen, stream));
    BEAST_TRY(beast_bpe_loop_state(lws, Vt, log_cap, &st_p, &log_p));
    BEAST_TRY(alloc(bws, bw_bytes));
    if (sharded) {
      BEAST_TRY(alloc(bdeltas, nbd));
      BEAST_HIP(hipMemsetAsync(bdeltas, 0, sizeof(int32_t) * nbd, s), "pass deltas memset");
    }
    BEAST_HIP(hipHostMalloc(&pinned.p, 2 * sizeof(int32_t) * STATE_WORDS, hipHostMallocDefault), "pinned state");
    return BEAST_OK;
  }

  int batch_pass(int steps, int flags) {
    return beast_bpe_loop_batch(lws, Vt, log_cap, steps, KMAX, flags, w.sym, w.start, w.len, w.count, w.n, tlen_d,
                                max_len, sig, table, argws, bws, bw_bytes, a.vocab_size, bdeltas, nullptr, stream);
  }

  int batch_read_state(int32_t (&st)[STATE_WORDS]) { return fetch(st, st_p, sizeof(st), "loop state read"); }

  // Sharded: every rank holds the same table and takes the same decisions, so every rank runs the
  // same passes and collectives: merge on the shard, SUM of the pass's deltas, apply (bpe_train.py).
  // A launch that fails on one rank still joins every collective of its chunk; the chunk's end
  // agrees on the status of its launches and of the state's read.
  int batch_sharded() {
    int32_t st[STATE_WORDS] = {};
    st[BEAST_BPE_STATE_VCUR] = n_base;
    int rc = batch_pass(0, BEAST_BPE_BATCH_INIT);
    do {
      const int steps = std::max(1, std::min(CHUNK, (a.vocab_size - st[BEAST_BPE_STATE_VCUR] + 1) / 2));
      for (int i = 0; i < steps; ++i) {
        if (rc == BEAST_OK) rc = batch_pass(1, BEAST_BPE_BATCH_NO_APPLY);
        BEAST_TRY(allreduce(bdeltas, (int64_t)nbd, BEAST_DT_I32, BEAST_OP_SUM));
        if (rc == BEAST_OK) rc = batch_pass(1, BEAST_BPE_BATCH_NO_MERGE);
      }
      if (rc == BEAST_OK) rc = batch_read_state(st);
      BEAST_TRY(agree(rc));
    } while (st[BEAST_BPE_STATE_ACTIVE] && st[BEAST_BPE_STATE_VCUR] < a.vocab_size);
    return BEAST_OK;
  }

  // One GPU, or replicated: two chunks of passes in flight, the host reads the state the older one
  // left.  A pass takes at most KMAX merges, so ceil(remaining / KMAX) passes never overshoot the
  // vocabulary; the chunk still in flight is counted at 4 merges a pass.
  int batch_pipelined() {
    int32_t* st_host = static_cast<int32_t*>(pinned.p);
    struct Inflight {
      hipEvent_t ev;
      int slot, passes;
    };
    struct Flights {   // at most two, oldest first; their events destroyed on every way out
      std::vector<Inflight> v;
      ~Flights() {
        for (auto& f : v) (void)hipEventDestroy(f.ev);
      }
    } inflight;
    auto start = [&](int steps, int flags) -> int {
      BEAST_TRY(batch_pass(steps, flags));
      const int slot = inflight.v.empty() ? 0 : 1 - inflight.v.back().slot;
      BEAST_HIP(hipMemcpyAsync(st_host + STATE_WORDS * slot, st_p, sizeof(int32_t) * STATE_WORDS,
                               hipMemcpyDeviceToHost, s), "loop state copy");
      hipEvent_t ev;
      BEAST_HIP(hipEventCreateWithFlags(&ev, hipEventDisableTiming), "event");
      (void)hipEventRecord(ev, s);
      inflight.v.push_back({ev, slot, steps});
      return BEAST_OK;
    };
    int vcur = n_base;
    BEAST_TRY(start(std::max(1, std::min(CHUNK, (a.vocab_size - vcur + KMAX - 1) / KMAX)), BEAST_BPE_BATCH_INIT));
    while (true) {
      int queued = 0;
      for (auto& f : inflight.v) queued += f.passes;
      const int left = a.vocab_size - vcur - 4 * queued;
      if (left > 0) BEAST_TRY(start(std::min(CHUNK, (left + KMAX - 1) / KMAX), 0));
      const Inflight f = inflight.v.front();
      inflight.v.erase(inflight.v.begin());
      const hipError_t e = hipEventSynchronize(f.ev);
      (void)hipEventDestroy(f.ev);
      BEAST_HIP(e, "loop event");
      const int32_t* h = st_host + STATE_WORDS * f.slot;
      vcur = h[BEAST_BPE_STATE_VCUR];
      if (!h[BEAST_BPE_STATE_ACTIVE] || vcur >= a.vocab_size) return BEAST_OK;
      if (inflight.v.empty()) BEAST_TRY(start(1, 0));
    }
  }

  // ---- the loop's log, replayed against the real strings (bpe_train.py replay_log).  A full log,
  // or an entry that disagrees (a 64-bit string-hash collision), asks for the host-driven loop.
  int batch_replay(int rc) {
    BEAST_TRY(rc);
    int32_t st[STATE_WORDS];
    BEAST_TRY(batch_read_state(st));
    n_log = st[BEAST_BPE_STATE_NMERGES];
    if (n_log >= log_cap) return BEAST_OK;   // full: run() reruns
    std::vector<int32_t> log(4 * (size_t)std::max(n_log, 1));
    if (n_log > 0) BEAST_TRY(fetch(log.data(), log_p, sizeof(int32_t) * 4 * n_log, "log read"));
    if (beast::g_bpe_train_host == 2) return BEAST_OK;   // tests: run() reruns
    bpe::ReplayFault why;
    const int bad = bpe::replay(*vocab, log.data(), n_log, merge_ids, &why);
    BEAST_REQUIRE_CODE(why != bpe::ReplayFault::out_of_range, BEAST_E_UNSUPPORTED,
                       "beast_bpe_train: merge log entry %d out of range", bad);
    rerun = bad >= 0;
    return BEAST_OK;
  }

  // ---- outputs: the vocabulary's strings in id order, the merges, the token range.  Capacities
  // are checked against the finished training: when one is short, the required sizes come back
  // (*out_n_vocab, *out_n_merges, out_vocab_off[0] = vocabulary bytes) with BEAST_E_WORKSPACE
  int outputs() {
    const std::vector<std::string>& id2str = vocab->id2str;
    const int n_merges = (int)(merge_ids.size() / 2);
    size_t need_bytes = 0;
    for (const std::string& t : id2str) need_bytes += t.size();
    if ((int)id2str.size() > a.max_vocab || n_merges > a.max_merges_out || need_bytes > a.vocab_bytes_cap) {
      *a.out_n_vocab = (int)id2str.size();
      *a.out_n_merges = n_merges;
      a.out_vocab_off[0] = (int64_t)need_bytes;
      BEAST_REQUIRE_CODE(false, BEAST_E_WORKSPACE,
                         "beast_bpe_train: output capacity (vocab %d, merges %d, bytes %zu) below the result's (%zu, "
                         "%d, %zu); the required sizes are in *out_n_vocab, *out_n_merges, out_vocab_off[0]",
                         a.max_vocab, a.max_merges_out, a.vocab_bytes_cap, id2str.size(), n_merges, need_bytes);
    }
    std::memcpy(a.out_merges, merge_ids.data(), merge_ids.size() * sizeof(int32_t));
    size_t off = 0;
    for (size_t i = 0; i < id2str.size(); ++i) {
      a.out_vocab_off[i] = (int64_t)off;
      std::memcpy(a.out_vocab_bytes + off, id2str[i].data(), id2str[i].size());
      off += id2str[i].size();
    }
    a.out_vocab_off[id2str.size()] = (int64_t)off;
    *a.out_n_vocab = (int)id2str.size();
    *a.out_n_merges = n_merges;
    *a.out_min_token = mn;
    *a.out_max_token = mx;
    return BEAST_OK;
  }
};

// Every rank of a communicator must issue the same collectives in the same order, so a rank whose
// local work fails must not return alone: its peers would block in the next collective.  The rule
// is in this function's shape.  Every stretch of local work between two collectives is a stage
// (or a few, the first failure skipping the rest) that returns a status; the status passes through
// agree (the worst over the ranks, beast::comm_agree; the identity without a communicator) before
// the next collective, and only an agreed status or a collective's own failure -- the communicator
// is then past agreeing anything -- leaves, through BEAST_TRY.  union_words, host_driven and
// batch_sharded hold collectives of their own and keep the same shape.
int Trainer::run() {
  BEAST_TRY(agree(arguments()));
  if (comm != nullptr) BEAST_TRY(allreduce(red, 1, BEAST_DT_I64, BEAST_OP_SUM));
  BEAST_TRY(agree(range()));
  if (comm != nullptr) BEAST_TRY(allreduce(red, 2, BEAST_DT_I64, BEAST_OP_MIN));
  BEAST_TRY(agree(presence()));
  if (comm != nullptr) BEAST_TRY(allreduce(pr, n_cp, BEAST_DT_U8, BEAST_OP_MAX));
  int rc = alphabet();
  if (rc == BEAST_OK) rc = shard_words();
  BEAST_TRY(agree(rc));
  if (replicated) BEAST_TRY(union_words());
  rc = replicated && NU > 0 ? union_repack() : BEAST_OK;
  if (rc == BEAST_OK) rc = pair_table();
  BEAST_TRY(agree(rc));
  if (sharded) BEAST_TRY(allreduce(table, (int64_t)Vt * Vt, BEAST_DT_U32, BEAST_OP_SUM));
  if (host_loop || Vt > 4096 || beast::g_bpe_train_host == 1) {
    BEAST_TRY(agree(host_setup()));
    BEAST_TRY(host_driven());
    rerun = n_log >= bpe::loop_log_capacity(a.vocab_size, n_base) || beast::g_bpe_train_host == 2;
  } else {
    BEAST_TRY(agree(batch_setup()));
    rc = BEAST_OK;
    if (sharded) BEAST_TRY(batch_sharded());
    else rc = batch_pipelined();
    BEAST_TRY(agree(batch_replay(rc)));
    rerun = rerun || n_log >= log_cap || beast::g_bpe_train_host == 2;
  }
  if (!host_loop) {   // the batched attempt's rerun is decided by every rank together
    int any = rerun ? 1 : 0;
    BEAST_TRY(beast::comm_max_i32(comm, any, &any, s));
    if (any) return RERUN;
  }
  return outputs();
}

// the batched attempt, then (RERUN) the host-driven one with the first attempt's memory released
int bpe_train_entry(const TrainArgs& args, beast_comm* comm, bool replicate, void* stream) {
  // everything below -- the internal allocations, and the trainer's destructor (DevMem,
  // HostPinned) -- runs with the stream's device current; the caller's is restored on return
  Queue q;
  BEAST_TRY(queue_of(stream, q, "beast_bpe_train"));
  const DeviceGuard on(q.dev);
  BEAST_HIP(on.status(), "beast_bpe_train");
  int rc = RERUN;
  for (int attempt = 0; attempt < 2 && rc == RERUN; ++attempt)
    rc = Trainer(args, comm, replicate, attempt == 1, q).run();
  return rc;
}

}  // namespace

extern "C" int beast_bpe_train(const int64_t* tokens, const int64_t* seq_off, int64_t n_seq, const uint8_t* cls_lut,
                               int64_t lut_n, int vocab_size, int min_frequency, int max_token_length,
                               const char* const* special_tokens, int n_special, int64_t* out_min_token,
                               int64_t* out_max_token, char* out_vocab_bytes, size_t vocab_bytes_cap,
                               int64_t* out_vocab_off, int max_vocab, int* out_n_vocab, int32_t* out_merges,
                               int max_merges_out, int* out_n_merges, void* stream) {
  return bpe_train_entry({tokens, seq_off, n_seq, cls_lut, lut_n, vocab_size, min_frequency, max_token_length,
                          special_tokens, n_special, out_min_token, out_max_token, out_vocab_bytes, vocab_bytes_cap,
                          out_vocab_off, max_vocab, out_n_vocab, out_merges, max_merges_out, out_n_merges},
                         nullptr, true, stream);
}

extern "C" int beast_bpe_train_comm(const int64_t* tokens, const int64_t* seq_off, int64_t n_seq,
                                    const uint8_t* cls_lut, int64_t lut_n, int vocab_size, int min_frequency,
                                    int max_token_length, const char* const* special_tokens, int n_special,
                                    int64_t* out_min_token, int64_t* out_max_token, char* out_vocab_bytes,
                                    size_t vocab_bytes_cap, int64_t* out_vocab_off, int max_vocab, int* out_n_vocab,
                                    int32_t* out_merges, int max_merges_out, int* out_n_merges, beast_comm* comm,
                                    int replicate, void* stream) {
  return bpe_train_entry({tokens, seq_off, n_seq, cls_lut, lut_n, vocab_size, min_frequency, max_token_length,
                          special_tokens, n_special, out_min_token, out_max_token, out_vocab_bytes, vocab_bytes_cap,
                          out_vocab_off, max_vocab, out_n_vocab, out_merges, max_merges_out, out_n_merges},
                         comm, replicate != 0, stream);
}
