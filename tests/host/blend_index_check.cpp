// Stand-alone host check of csrc/blend_index.h, meant to be built with the host compiler's address
// and undefined-behaviour sanitizers (tests/test_blend_oracle.py does): the tables are heap arrays
// of exactly W entries, so a table read outside [0, W) is reported, not just wrong.
//
//   blend_index_check <seed> <rounds>
//
// Per round a table of a random kind (sorted in range, sorted out of range, duplicate-heavy,
// shuffled, arbitrary 64-bit values) and random row ranges.  Checked on every table: 0 <= a <= b <= W
// and, for every window and a few rows, blend_member against a restatement, with t in [0, T).
// Checked on tables with non-decreasing starts: a and b are the counts the definition gives, and no
// window outside [a, b) owns a row of [r0, r1).  Prints "ok <tables> <ranges>" and returns 0.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <memory>
#include <random>

#include "blend_index.h"

static int fail(const char* what, long long x, long long y) {
  std::printf("FAIL %s %lld %lld\n", what, x, y);
  return 1;
}

int main(int argc, char** argv) {
  const unsigned seed = argc > 1 ? (unsigned)std::atoi(argv[1]) : 1u;
  const int rounds = argc > 2 ? std::atoi(argv[2]) : 200;
  std::mt19937_64 rng(seed);
  auto uni = [&](long long lo, long long hi) { return std::uniform_int_distribution<long long>(lo, hi)(rng); };
  long long n_ranges = 0;
  for (int round = 0; round < rounds; ++round) {
    const long long W = round % 7 == 0 ? 0 : uni(1, 300), R = uni(1, 400);
    const int T = (int)uni(1, 256), kind = (int)uni(0, 4);
    std::unique_ptr<long long[]> s(new long long[W]), e(new long long[W]);   // exactly W entries each
    for (long long w = 0; w < W; ++w) {
      switch (kind) {
        case 0: s[w] = uni(0, R - 1); e[w] = s[w] + uni(1, 2 * T); break;
        case 1: s[w] = uni(-3 * R, 4 * R); e[w] = uni(-3 * R, 4 * R); break;
        case 2: s[w] = uni(0, 3) * (R / 4); e[w] = R; break;
        case 3: s[w] = uni(0, R - 1); e[w] = uni(0, R); break;
        default: s[w] = (long long)rng(); e[w] = (long long)rng(); break;
      }
    }
    const bool sorted = kind <= 2;
    if (sorted) std::sort(s.get(), s.get() + W);
    for (int q = 0; q < 24; ++q) {
      long long r0 = uni(0, R), r1 = uni(r0, R);
      if (q == 0) { r0 = 0; r1 = R; }
      if (q == 1) r1 = std::min(R, r0 + 64);
      long long a = -1, b = -1;
      beast::blend_candidates(s.get(), W, R, T, r0, r1, a, b);
      ++n_ranges;
      if (!(0 <= a && a <= b && b <= W)) return fail("range", a, b);
      if (!sorted) continue;
      long long ca = 0, cb = 0;
      for (long long w = 0; w < W; ++w) {
        const long long cs = std::min(std::max(s[w], 0ll), R - 1);
        ca += cs <= r0 - T;
        cb += cs < r1;
      }
      if (a != ca || b != std::max(ca, cb)) return fail("definition", a, b);
      for (long long w = 0; w < W; ++w) {
        if (w >= a && w < b) continue;
        for (long long r = r0; r < r1; ++r) {
          int t;
          if (beast::blend_member(s[w], e[w], R, T, r, t)) return fail("a contributor outside [a, b)", w, r);
        }
      }
    }
    for (long long w = 0; w < W; ++w) {
      const long long cs = std::min(std::max(s[w], 0ll), R - 1);
      const long long ce = std::min(std::max(e[w], cs + 1), R);
      const long long rows = std::min<long long>(T, ce - cs);
      for (long long r : {0ll, cs, cs + rows - 1, cs + rows, R - 1, uni(0, R - 1)}) {
        if (r < 0 || r >= R) continue;
        int t = -7;
        const bool in = beast::blend_member(s[w], e[w], R, T, r, t);
        if (in != (cs <= r && r < cs + rows)) return fail("member", w, r);
        if (t < 0 || t >= T || (in && t != r - cs)) return fail("sample index", w, t);
      }
    }
  }
  std::printf("ok %d %lld\n", rounds, n_ranges);
  return 0;
}
