// k(y) = sum_q cs[q] y^{n+1+q} over many blocks (poly.hip: k_k_of_y_partials, k_k_of_y_finish): how the Q terms are cut into contiguous
// spans, one per block.  No HIP in here: the kernels, their launcher and a host test program (tests/host/k_of_y_host.cpp) compile this
// one text.  Block b sums the terms [b * span, min((b + 1) * span, Q)) -- its thread t the terms b * span + t, + 256, ... -- and writes
// one partial; one block then sums the `blocks` partials.  Every q < Q lies in exactly one span and no block is empty.
#pragma once

#if defined(__HIPCC__)
#define K_OF_Y_HD __host__ __device__ inline
#else
#define K_OF_Y_HD inline
#endif

namespace sonic {

constexpr int K_OF_Y_BLOCK = 256;             // threads per block of both stages
constexpr long K_OF_Y_SPAN_DEFAULT = 2048;    // terms per block: eight products per thread (SONIC_K_OF_Y_SPAN=<q per block>)

struct KOfYPlan {
  long blocks = 0;      // 0: one block over all of Q (k_sub_k_of_y, the form below the threshold)
  long span = 0;
};

// Q terms in spans of `span` (>= 1) each: ceil(Q / span) blocks, the last one shorter when span does not divide Q
K_OF_Y_HD KOfYPlan k_of_y_plan(long Q, long span) {
  KOfYPlan p;
  p.span = span < 1 ? 1 : span;
  p.blocks = Q < 1 ? 0 : (Q + p.span - 1) / p.span;
  return p;
}
// the terms of block b: [*lo, *hi)
K_OF_Y_HD void k_of_y_span(const KOfYPlan& p, long Q, long b, long* lo, long* hi) {
  *lo = b * p.span;
  const long end = *lo + p.span;
  *hi = end < Q ? end : Q;
}

}  // namespace sonic
