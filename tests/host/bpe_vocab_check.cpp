// Stand-alone driver of csrc/bpe_vocab.h for tests/test_bpe_vocab_host.py (host compiler only).
// Reads one case from the file named on the command line:
//     n_cp / present as n_cp characters '0' '1' / n_special / one special token per line, hex /
//     n_log / "a b nid reused" per line
// and prints the alphabet with its hashes, byte2id, the replay's verdict, and the vocabulary and
// merges the replay left.  Strings travel as hex: the alphabet holds NUL and newline.
#include <cstdio>
#include <cstdint>
#include <fstream>
#include <string>
#include <vector>

#include "bpe_vocab.h"

namespace bpe = beast::bpe;

static std::string unhex(const std::string& h) {
  std::string s;
  for (size_t i = 0; i + 1 < h.size(); i += 2) s += (char)std::stoi(h.substr(i, 2), nullptr, 16);
  return s;
}

static void print_hex(const std::string& s) {
  if (s.empty()) std::printf("-");
  for (unsigned char c : s) std::printf("%02x", c);
}

int main(int argc, char** argv) {
  if (argc != 2) return 2;
  std::ifstream in(argv[1]);
  long long n_cp = 0;
  int n_special = 0, n_log = 0;
  std::string bits;
  in >> n_cp >> bits >> n_special;
  if (!in || (long long)bits.size() != n_cp) return 2;
  std::vector<uint8_t> present(n_cp);
  for (long long i = 0; i < n_cp; ++i) present[i] = bits[i] == '1';
  std::vector<std::string> specials(n_special);
  std::vector<const char*> special_ptrs;
  for (std::string& t : specials) {
    in >> t;
    t = unhex(t);
  }
  for (const std::string& t : specials) special_ptrs.push_back(t.c_str());
  in >> n_log;
  std::vector<int32_t> log(4 * (size_t)n_log);
  for (int32_t& v : log) in >> v;
  if (!in) return 2;

  bpe::Vocab vocab(present.data(), n_cp, special_ptrs.data(), n_special);
  const bpe::TokenHashes th = bpe::token_hashes(vocab);
  const int n = vocab.size();
  std::printf("tokens %d\n", n);
  for (int i = 0; i < n; ++i) {
    print_hex(vocab.id2str[i]);
    std::printf(" %llu %llu %u\n", (unsigned long long)th.hp[i], (unsigned long long)th.hp[n + i], th.tlen[i]);
  }
  std::printf("max_tlen %d\nbyte2id", th.max_tlen);
  for (int b = 0; b < 256; ++b) std::printf(" %d", (int)vocab.byte2id[b]);
  std::printf("\ncapacity %d\n", bpe::loop_log_capacity(n + n_log, n));

  std::vector<int32_t> merges;
  bpe::ReplayFault why;
  const int bad = bpe::replay(vocab, log.data(), n_log, merges, &why);
  std::printf("replay %d %d\n", bad, (int)why);
  std::printf("vocab %d\n", vocab.size());
  for (const std::string& t : vocab.id2str) {
    print_hex(t);
    std::printf("\n");
  }
  for (int i = 0; i < vocab.size(); ++i)
    if (vocab.str2id.at(vocab.id2str[i]) != i) return 3;   // the two maps agree
  if ((int)vocab.str2id.size() != vocab.size()) return 3;
  std::printf("merges %zu\n", merges.size() / 2);
  for (size_t m = 0; m < merges.size(); m += 2) std::printf("%d %d\n", merges[m], merges[m + 1]);
  return 0;
}
