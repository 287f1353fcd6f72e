// What the bulk kernels of an MSM leave behind (MsmSlot) and the host tail that folds it (msm_finish_host).  No HIP in here: g1.hpp
// compiles for both sides, so the tail is also built and run by a plain host compiler (tests/host/slot_form_host.cpp).
#pragma once
#include <string.h>
#include "g1.hpp"
#include "endo.hpp"

namespace sonic {

constexpr int MSM_MAX_WINDOWS = 64;
constexpr int MSM_ENDO_SLOT_OFFSET = 32;      // where the second half of an endomorphism pair sits in MsmSlot::win

// Per-MSM hand-off between the bulk kernels and the (deferred, batched) tail: the per-window sums.
// Two forms: W window sums of a c-bit Horner walk (per-window bucket sets; pad1 == 0), or -- shared bucket sets reduced by the
// bit-sum butterfly, pad1 == 1 -- win[j] = sum of the buckets whose index has bit j set (j < W), win[W] = the sum of all buckets
// and pad0 = its weight: the MSM is sum_j 2^j win[j] + pad0 win[W].  pad1 == 2: an endomorphism pair -- the same form twice, the
// second at win[32 ..], result = first + phi(second).  pad1 == 3: shared bucket sets reduced by running sums over K-bucket segments
// (k_bucket_segments<true>), pad0 = K, a power of two -- win[j] = the bit sums of the segments' runs (j < W, by the butterfly),
// win[W] = the sum of the segments' local totals (k_window_sum, which also writes the header): the MSM is
// K sum_j 2^j win[j] + win[W].  msm_finish_host folds all of them.
struct MsmSlot {
  int W, c, pad0, pad1;
  G1XYZZ win[MSM_MAX_WINDOWS];
};

// What is left of an MSM after the bulk kernels is W <= 64 window sums: Horner over the windows
// (255 dependent doublings) and one Fq inversion for the canonical affine form.  That is ~2600
// strictly sequential Fq products -- ~10 ms on one GPU lane (measured), ~0.5 ms on a host core --
// so the host layer finishes it, with the same limb code (g1.hpp compiles for both sides).
inline G1XYZZ msm_finish_host(const MsmSlot& s) {
  // slots usually sit in pinned host memory, which the CPU reads uncached: limb-by-limb arithmetic straight out of it cost
  // ~20 us per window sum (0.3 ms per proof), so every window sum is copied out once before it is used
  const int W = s.W, c = s.c;
  G1XYZZ acc = G1XYZZ::inf();
  if (s.pad1 >= 1 && s.pad1 <= 3) {
    // bit-sum form (k_bucket_tree_levels): sum_j 2^j win[off + j] + pad0 * win[off + W]
    auto bitsum = [&](int off) {
      G1XYZZ a = G1XYZZ::inf();
      for (int w = W - 1; w >= 0; w--) {
        G1XYZZ win;
        memcpy(&win, &s.win[off + w], sizeof win);
        a = g1_add(g1_dbl(a), win);
      }
      G1XYZZ tot;
      memcpy(&tot, &s.win[off + W], sizeof tot);
      const uint32_t mul = (uint32_t)s.pad0;
      return g1_add(a, mul == 1 ? tot : g1_mul_small(tot, mul));
    };
    if (s.pad1 == 1) return bitsum(0);
    if (s.pad1 == 3) {
      // two-level running sums (k_bucket_segments<true>): pad0 = K, win[j < W] = the bit sums of the segments' runs, win[W] = the sum of
      // the segments' local totals: K * sum_j 2^j win[j] + win[W]
      G1XYZZ a = G1XYZZ::inf();
      for (int w = W - 1; w >= 0; w--) {
        G1XYZZ win;
        memcpy(&win, &s.win[w], sizeof win);
        a = g1_add(g1_dbl(a), win);
      }
      for (uint32_t k = (uint32_t)s.pad0; k > 1; k >>= 1) a = g1_dbl(a);
      G1XYZZ tot;
      memcpy(&tot, &s.win[W], sizeof tot);
      return g1_add(a, tot);
    }
    return g1_add(bitsum(0), g1_endo(bitsum(MSM_ENDO_SLOT_OFFSET)));         // endomorphism pair: sum(s1 P) + phi(sum(s2 P))
  }
  for (int w = W - 1; w >= 0; w--) {
    G1XYZZ win;
    memcpy(&win, &s.win[w], sizeof win);
    if (w == W - 1) { acc = win; continue; }
    for (int j = 0; j < c; j++) acc = g1_dbl(acc);
    acc = g1_add(acc, win);
  }
  return acc;
}

}  // namespace sonic
