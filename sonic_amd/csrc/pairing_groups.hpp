// The segmented product behind sonic_pairing_check and the per-proof fold of verify_batch (pairing.hip): n values of Fq12 cut into G groups
// by group_end[] -- group g is [group_end[g-1], group_end[g]) -- become one value per group, the group's product (1 for an empty group), in
// passes.  A pass cuts every group into chunks of at most GT_CHUNK values, counted from the group's own start; one thread multiplies one
// chunk; the chunk products, in group order, are the next pass's values.  A group of at most GT_CHUNK values (an empty one included) is one
// chunk, so after gt_passes(n) passes every group holds exactly one value and value g belongs to group g.
//
// Written once for the host and the device: k_gt_plan / k_gt_group_product run these functions, and tests/host/pairing_host.cpp compiles
// the same text with g++ and compares the passes with a straight loop.
#pragma once
#include "pairing.hpp"

namespace sonic {
namespace pairing {

constexpr int GT_CHUNK = 16;

HD long gt_chunks_of(long len) { return len <= GT_CHUNK ? 1 : (len + GT_CHUNK - 1) / GT_CHUNK; }
// the passes that n values need, whatever their grouping is (at least one: it is the pass that gives an empty group its 1)
inline int gt_passes(long n) {
  int p = 1;
  for (long m = gt_chunks_of(n); m > 1; m = gt_chunks_of(m)) p++;
  return p;
}
// an upper bound of a pass's output count from one of its input count: a group of len values has at most len / GT_CHUNK + 1 chunks
inline long gt_out_bound(long in_bound, long G) { return in_bound / GT_CHUNK + G; }

// the plan of a pass, out_end[g] = chunks of the groups 0 .. g, as two walks over a slice [g0, g1) of the groups: the slice's chunk count,
// and -- given the chunks before the slice -- its entries of out_end
HD long gt_plan_count(const int64_t* in_end, long g0, long g1) {
  long c = 0;
  for (long g = g0; g < g1; g++) c += gt_chunks_of((long)(in_end[g] - (g ? in_end[g - 1] : 0)));
  return c;
}
HD void gt_plan_write(const int64_t* in_end, long g0, long g1, long before, int64_t* out_end) {
  for (long g = g0; g < g1; g++) {
    before += gt_chunks_of((long)(in_end[g] - (g ? in_end[g - 1] : 0)));
    out_end[g] = before;
  }
}
// the group of output value t: the first g with out_end[g] > t (t < out_end[G - 1])
HD long gt_group_of(const int64_t* out_end, long G, long t) {
  long lo = 0, hi = G - 1;
  while (lo < hi) {
    const long mid = lo + (hi - lo) / 2;
    if (out_end[mid] > t) hi = mid; else lo = mid + 1;
  }
  return lo;
}
// output value t of a pass; false when the pass has fewer than t + 1 outputs
PHD bool gt_chunk_product(const F12* in, const int64_t* in_end, const int64_t* out_end, long G, long t, F12& out) {
  if (G <= 0 || t >= (long)out_end[G - 1]) return false;
  const long g = gt_group_of(out_end, G, t);
  const long j = t - (g ? (long)out_end[g - 1] : 0);
  const long s = (g ? (long)in_end[g - 1] : 0) + j * GT_CHUNK, ge = (long)in_end[g];
  const long e = s + GT_CHUNK < ge ? s + GT_CHUNK : ge;
  if (s >= e) { out = F12::one(); return true; }
  F12 acc = in[s];
#pragma unroll 1
  for (long i = s + 1; i < e; i++) acc = f12_mul(acc, in[i]);
  out = acc;
  return true;
}

}  // namespace pairing
}  // namespace sonic
