// The host-only vocabulary core of beast_bpe_train: the byte-level alphabet HF's BpeTrainer
// builds, the token-string hashes the device loop starts from, the one merge step (concatenate,
// re-use or allocate an id) and the replay of a merge log against the real strings.  Plain C++17,
// no HIP: it compiles with a host compiler alone (tests/host/bpe_vocab_check.cpp), and failures
// are plain values -- the caller words them.  The same steps in Python: bpe_train.py
// build_alphabet / token_hashes / replay_log.
#pragma once

#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <string>
#include <unordered_map>
#include <vector>

namespace beast {
namespace bpe {

// odd multiplier of the token-string hash: h(xy) = h(x) * P^len(y) + h(y)  (bpe_loop.hip's string
// table, _lib.py BPE_LOOP_P)
constexpr uint64_t LOOP_P = 0x9E3779B97F4A7C15ull;

// GPT-2 bytes_to_unicode: bytes 33-126, 161-172, 174-255 map to themselves, the other 68 to
// U+0100 + k in ascending byte order
inline void bytes_to_unicode(uint32_t (&b2u)[256]) {
  int k = 0;
  for (int b = 0; b < 256; ++b) {
    const bool keep = (b >= 33 && b <= 126) || (b >= 161 && b <= 172) || (b >= 174 && b <= 255);
    b2u[b] = keep ? (uint32_t)b : (uint32_t)(256 + k++);
  }
}

inline void append_utf8(std::string& s, uint32_t cp) {
  if (cp < 0x80) {
    s += (char)cp;
  } else if (cp < 0x800) {
    s += (char)(0xC0 | (cp >> 6));
    s += (char)(0x80 | (cp & 63));
  } else if (cp < 0x10000) {
    s += (char)(0xE0 | (cp >> 12));
    s += (char)(0x80 | ((cp >> 6) & 63));
    s += (char)(0x80 | (cp & 63));
  } else {
    s += (char)(0xF0 | (cp >> 18));
    s += (char)(0x80 | ((cp >> 12) & 63));
    s += (char)(0x80 | ((cp >> 6) & 63));
    s += (char)(0x80 | (cp & 63));
  }
}

inline size_t utf8_chars(const std::string& s) {   // HF counts token lengths in characters
  size_t n = 0;
  for (unsigned char c : s) n += (c & 0xC0) != 0x80;
  return n;
}

// log capacity of the batched device loop: a merge that re-uses an id does not grow the
// vocabulary, so the log may hold more than vocab_size - n_base entries
inline int loop_log_capacity(int vocab_size, int n_base) { return 4 * std::max(vocab_size - n_base, 0) + 1024; }

struct Vocab {
  std::vector<std::string> id2str;
  std::unordered_map<std::string, int> str2id;
  uint16_t byte2id[256];   // id of a byte's byte-level character, 0xFFFF for a byte the corpus lacks

  // HF BpeTrainer's alphabet for the code points present[0 .. n_cp): the special tokens (a
  // repeated one once), then the byte-level characters of the UTF-8 bytes seen plus the initial
  // alphabet chr(0 .. n_cp - 1), by code point
  Vocab(const uint8_t* present, int64_t n_cp, const char* const* special_tokens, int n_special) {
    uint32_t b2u[256];
    bytes_to_unicode(b2u);
    bool seen[256] = {};
    for (int64_t cp = 0; cp < n_cp; ++cp)
      if (present[cp]) {
        std::string u;
        append_utf8(u, (uint32_t)cp);
        for (unsigned char c : u) seen[c] = true;
      }
    std::vector<uint32_t> chars;
    for (int b = 0; b < 256; ++b)
      if (seen[b]) chars.push_back(b2u[b]);
    for (int64_t cp = 0; cp < n_cp; ++cp) chars.push_back((uint32_t)cp);
    std::sort(chars.begin(), chars.end());
    chars.erase(std::unique(chars.begin(), chars.end()), chars.end());
    for (int i = 0; i < n_special; ++i) find_or_add(special_tokens[i]);
    for (uint32_t c : chars) {
      std::string u;
      append_utf8(u, c);
      find_or_add(std::move(u));
    }
    for (int b = 0; b < 256; ++b) {
      std::string u;
      append_utf8(u, b2u[b]);
      byte2id[b] = seen[b] ? (uint16_t)str2id.at(u) : (uint16_t)0xFFFF;
    }
  }

  int size() const { return (int)id2str.size(); }
  bool has(int id) const { return id >= 0 && id < size(); }

  // the merge step: the string of a then b, its id when the vocabulary has it (HF re-uses it),
  // else the next id
  struct Merged {
    int nid;
    bool reused;
  };
  Merged merge(int a, int b) { return find_or_add(id2str[a] + id2str[b]); }

 private:
  Merged find_or_add(std::string t) {
    const auto ins = str2id.emplace(t, size());
    if (ins.second) id2str.push_back(std::move(t));
    return {ins.first->second, !ins.second};
  }
};

// what the device loop starts from, per token: hp[i] the hash of its UTF-8 bytes and hp[n + i]
// P^bytes (mod 2^64), tlen its length in HF's unit (characters), max_tlen the largest
struct TokenHashes {
  std::vector<uint64_t> hp;
  std::vector<uint32_t> tlen;
  int max_tlen = 0;
};
inline TokenHashes token_hashes(const Vocab& v) {
  const size_t n = v.id2str.size();
  TokenHashes t;
  t.hp.resize(2 * n);
  t.tlen.resize(n);
  for (size_t i = 0; i < n; ++i) {
    uint64_t h = 0, pw = 1;
    for (unsigned char c : v.id2str[i]) {
      h = h * LOOP_P + c;
      pw *= LOOP_P;
    }
    t.hp[i] = h;
    t.hp[n + i] = pw;
    t.tlen[i] = (uint32_t)utf8_chars(v.id2str[i]);
    t.max_tlen = std::max(t.max_tlen, (int)t.tlen[i]);
  }
  return t;
}

// Replays the merge log [n][4] {a, b, nid, reused} of the device loop against the real strings: an
// id the device re-used must be the string's, a new one the next id.  Returns -1 with v extended
// and (a, b) of every entry appended to merges, or the index of the first entry that does not
// hold -- `why` then says which way -- with v and merges as the entries before it left them.
enum class ReplayFault { none, out_of_range, disagrees };
inline int replay(Vocab& v, const int32_t* log, int n, std::vector<int32_t>& merges, ReplayFault* why = nullptr) {
  ReplayFault fault = ReplayFault::none;
  int i = 0;
  for (; i < n; ++i) {
    const int a = log[4 * i], b = log[4 * i + 1], nid = log[4 * i + 2], reused = log[4 * i + 3];
    if (!v.has(a) || !v.has(b)) {
      fault = ReplayFault::out_of_range;
      break;
    }
    const Vocab::Merged m = v.merge(a, b);
    if (m.nid != nid || m.reused != (reused != 0)) {
      if (!m.reused) {   // take the string back
        v.str2id.erase(v.id2str.back());
        v.id2str.pop_back();
      }
      fault = ReplayFault::disagrees;
      break;
    }
    merges.push_back(a);
    merges.push_back(b);
  }
  if (why) *why = fault;
  return fault == ReplayFault::none ? -1 : i;
}

}  // namespace bpe
}  // namespace beast
