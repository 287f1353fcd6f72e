// The host-only parts of the G2 MSM (msm_g2.hip): the window rule, the shifts, the Horner fold of the window sums and the cut of a
// bucket into chunks.  Plain C++ over g2.hpp's host arithmetic: tests/host/g2_msm_host.cpp compiles the same text with g++.
#pragma once
#include "g2.hpp"

namespace sonic {

// No thread of k_g2_bucket_accum adds more than this many entries in a row.  A longer bucket is cut into chunks that other threads walk, and
// k_g2_bucket_combine adds a bucket's partial sums.  Scalars that are all equal put n entries into one bucket per window, and the top
// window of a plan whose W c overshoots `bits` holds few buckets with many entries each (129 bits at c = 15: 9 bits, 256 buckets of
// n / 256): the bound is what keeps the accumulation's critical path at G2_WALK_MAX additions whatever the scalars are.  256 is four times
// the mean walk of a 2^19-term slab (2^19 / 2^14 = 32 entries per bucket at c = 15), so buckets of ordinary length are never cut, and it
// leaves at most n W / 256 extra partial sums, an eighth of the buckets' own memory there.  A smaller bound would shorten the tail of the
// accumulation over such a top window and lengthen the chain of k_g2_bucket_combine, which adds a bucket's partial sums in one thread
// (at most n / G2_WALK_MAX of them); neither direction has been measured.
constexpr int G2_WALK_MAX = 256;
// terms per chain: a longer sum runs as one chain per slab on the same workspace and the host adds the slab results (the constant of
// g2_weighted_sum and srs_scale_g2)
constexpr long G2_MSM_SLAB = 1L << 19;

// Window width from the number of terms: msm_plan's rule, c = floor(log2 n) - 4 clamped to [4, 16].  By operation count a c-bit window
// costs n mixed additions and 2^(c-1) (2 + ~1.5 c / K) full additions of the reduction per window, K = 8, so the rule keeps the reduction
// near a third of the accumulation.  Measured under this rule (profiles/r18_g2_msm.txt, one MI355X): the structure check at d = 2^21
// 364.9 ms against 1225.9 for the walk, 244 ms of it accumulation and 59 ms reduction; an MSM of 2^20 full-width terms 34.1 ms.  No other
// c has been measured, so the rule has not been moved.
HD int g2_msm_window_bits(long n) {
  int lg = 0;
  while ((1L << (lg + 1)) <= n) lg++;
  const int c = lg - 4;
  return c < 4 ? 4 : (c > 16 ? 16 : c);
}
// `bits`: the scalars are below 2^(bits - 1), so that the signed recoding's carry never leaves the top window -- 256 for any canonical Fr
// (r < 2^255), 255 for folded ones (<= (r - 1) / 2 < 2^254), 129 for the 128-bit randomizers of the structure check
HD int g2_msm_windows(int bits, int c) { return (bits + c - 1) / c; }
HD int g2_msm_shift(int c, int w) { return c * w; }

// chunks of a bucket of len entries, and entries [beg, end) of chunk j of a bucket that starts at entry `first`
HD uint32_t g2_chunks(uint32_t len) { return (len + (uint32_t)G2_WALK_MAX - 1) / (uint32_t)G2_WALK_MAX; }
struct G2ChunkRange { uint32_t beg, end; };
HD G2ChunkRange g2_chunk_range(uint32_t first, uint32_t len, uint32_t j) {
  G2ChunkRange r;
  r.beg = first + j * (uint32_t)G2_WALK_MAX;
  const uint32_t stop = first + len;
  r.end = stop - r.beg > (uint32_t)G2_WALK_MAX ? r.beg + (uint32_t)G2_WALK_MAX : stop;
  return r;
}

// sum_w 2^(c w) S_w by Horner from the top window: c doublings and one addition per window
inline G2Jac g2_msm_fold_windows(const G2Jac* S, int W, int c) {
  G2Jac acc = G2Jac::inf();
  for (int w = W - 1; w >= 0; w--) {
    const int up = w + 1 < W ? g2_msm_shift(c, w + 1) - g2_msm_shift(c, w) : 0;
    for (int b = 0; b < up; b++) acc = g2_dbl(acc);
    acc = g2_add(acc, S[w]);
  }
  return acc;
}

}  // namespace sonic
