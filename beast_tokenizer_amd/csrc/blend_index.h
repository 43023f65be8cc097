// Index logic of beast_reconstruct_windows_f32 (blend.hip), in plain integer C++ for the host and
// the device: which windows of a (start, end) table can cover a range of output rows, and whether
// a window covers one row.  A table entry is never trusted: both functions see a window through
// the clamps of windows.hip -- start into [0, R - 1], end into [start + 1, R], rows = min(T, end -
// start) -- so whatever a table holds, every table index read lies in [0, W), every sample index
// returned in [0, T), and a bad table gives wrong numbers, never a fault.
// beast_blend_candidates_host runs blend_candidates over host arrays (tests/test_blend_oracle.py
// holds it to brute force, garbage tables included, on a machine without a GPU).
#pragma once

#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define BEAST_HD __host__ __device__
#else
#define BEAST_HD
#endif

namespace beast {

// windows.hip's clamp of a start: into [0, R - 1] (R >= 1)
BEAST_HD inline long long blend_clamp_start(long long start, long long R) {
  return start < 0 ? 0 : (start > R - 1 ? R - 1 : start);
}

// The first w in [0, W] whose clamped start exceeds `key`, by binary search: exact on a table
// with non-decreasing starts (the clamp is monotone, so such a table stays sorted under it); on
// any other table still some index in [0, W] after at most 64 reads, each inside [0, W).
BEAST_HD inline long long blend_first_above(const long long* win_start, long long W, long long R, long long key) {
  long long lo = 0, hi = W;
  while (lo < hi) {
    const long long mid = lo + (hi - lo) / 2;   // lo <= mid < hi <= W
    if (blend_clamp_start(win_start[mid], R) > key) hi = mid;
    else lo = mid + 1;
  }
  return lo;
}

// The windows that can cover a row of [r0, r1), 0 <= r0 <= r1 <= R, 1 <= T: the half-open range
// [a, b) with a the first w whose start exceeds r0 - T (an earlier window ends at or before r0) and
// b the first w whose start is >= r1.  0 <= a <= b <= W whatever the table holds.
BEAST_HD inline void blend_candidates(const long long* win_start, long long W, long long R, int T, long long r0,
                                      long long r1, long long& a, long long& b) {
  if (W <= 0 || R <= 0) {
    a = b = 0;
    return;
  }
  a = blend_first_above(win_start, W, R, r0 - T);
  b = blend_first_above(win_start, W, R, r1 - 1);
  if (b < a) b = a;   // only an unsorted table gets here
}

// The window (start, end) as the kernels use it (R >= 1): its first row s in [0, R - 1] and, returned,
// the rows it owns, min(T, end - s) in [1, T] after end is clamped into [s + 1, R].
BEAST_HD inline int blend_rows(long long start, long long end, long long R, int T, long long& s) {
  s = blend_clamp_start(start, R);
  long long e = end < s + 1 ? s + 1 : end;
  e = e > R ? R : e;
  return (int)(e - s < T ? e - s : T);
}

// Does the window (start, end) own row r, and as which sample?  The sample index t = r - s lies in
// [0, rows): samples at or past `rows` are edge padding and own no row.  t is 0 where it does not.
BEAST_HD inline bool blend_member(long long start, long long end, long long R, int T, long long r, int& t) {
  long long s;
  const int rows = blend_rows(start, end, R, T, s);
  const bool in = s <= r && r < s + rows;
  t = in ? (int)(r - s) : 0;
  return in;
}

}  // namespace beast
