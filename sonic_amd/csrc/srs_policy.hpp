// How an SRS handle is sized (srs_alloc, srs_api.hip): the window width of its tables by d, full versus endomorphism versus no tables by
// the free device memory, and whether the running sums and the symmetric sums of the alpha basis are held.  Pure host arithmetic -- no HIP
// -- so that the rule runs on a CPU (tests/host/srs_policy_host.cpp, tests/test_srs_policy_host.py); srs_alloc asks it three times, with
// the free memory read again before each question.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <stdlib.h>
#include "endo.hpp"        // ENDO_BITS (and, through g1.hpp, SONIC_SRS_POINT_BYTES)

namespace sonic {

// the environment knobs of the rule as atoi reads them; -1: not set (no knob gives a negative value a meaning)
struct SrsKnobs {
  int tables = -1;         // SONIC_MSM_TABLES: 0 switches the window tables off
  int table_c = -1;        // SONIC_MSM_TABLE_C: a window width in 9 .. 22 instead of the one chosen by d; anything else is ignored
  int endo = -1;           // SONIC_MSM_ENDO: 1 asks for the endomorphism tables, 0 forbids them
  int prefix = -1;         // SONIC_SRS_PREFIX: 0 drops the running sums of the alpha basis
  int sym = -1;            // SONIC_SRS_SYM: 0 drops the symmetric sums of the alpha basis
};
inline SrsKnobs srs_knobs_from_env() {
  auto knob = [](const char* name) { const char* v = getenv(name); return v ? atoi(v) : -1; };
  return SrsKnobs{knob("SONIC_MSM_TABLES"), knob("SONIC_MSM_TABLE_C"), knob("SONIC_MSM_ENDO"), knob("SONIC_SRS_PREFIX"), knob("SONIC_SRS_SYM")};
}

// c = 0, W = 1: no window tables
struct SrsWindows { int c, W; bool endo; };

// Window tables trade HBM capacity (288 GB) for work: W x the SRS size buys one shared bucket set per MSM.
// c grows with d (MSM sizes are a fraction of d); off with SONIC_MSM_TABLES=0 or when memory is short.
// (d decides the width; npts, the points a table holds, is what the memory questions are asked with: 2d + 1 for a whole string, fewer
// for a circuit-sized view of one, srs_view.hpp)
inline SrsWindows srs_window_policy(int64_t d, size_t npts, size_t free_bytes, const SrsKnobs& k) {
  const size_t n = npts;
  int lg = 0;
  while ((2L << lg) <= d) lg++;                 // floor(log2 d)
  // measured (prove at n = d/8, profiles/r05_table_c_ab.txt): up to d = 2^19 the MSMs (0.4 d .. 0.9 d terms) run best with ~2^16
  // bucket walks (c = 17: one to two waves per SIMD, short reduction); from d = 2^20 the two windows saved by c = 20 win (prove at
  // n = 2^17 20.2 -> 19.2 ms; a stand-alone MSM of 0.9 d terms 5.7 -> 2.9 ms: 2^16 walks of 210 entries are one wave per SIMD).
  int c = lg >= 20 ? 20 : (lg > 17 ? 17 : lg);
  // round 6, d = 2^16, 2^17: c = 16.  A proof's MSMs over such an SRS run as ONE chain (prove.hip, fused) whose accumulation is 45 n W
  // additions and whose butterfly costs ~2.8 additions' worth per bucket of 15 bucket sets: at n = d/8 = 2^14 the 2^16-bucket plan (c = 17)
  // spent 0.82 ms reducing beside 1.75 ms accumulating (profiles/r06_small_proofs.txt).  Measured at n = 2^14, ms per proof streamed / one
  // at a time: c = 17 4.09-4.18 / 4.27-4.54, c = 16 3.91-3.98 / 4.23-4.33, c = 15 4.09-4.11 / 4.44-4.51, c = 14 8.5 / 9.0 (15 x 2^13 bucket
  // walks are less than one round of the chip's wave slots and 350-800 entries long); at n = 2^16 c = 16 11.1 against 10.5-10.7 at 17
  // (profiles/r06_ab_small.txt).
  if (lg >= 15 && lg <= 17) c = lg == 15 ? 15 : 16;
  if (c < 9) c = 9;
  if (k.table_c >= 9 && k.table_c <= 22) c = k.table_c;
  // W windows of even width (msm.hpp): the widest is ceil(255 / W) <= c
  int W = (255 + c - 1) / c;
  const int c_full = (255 + W - 1) / W;
  const size_t per_table = 2 * n * (size_t)SONIC_SRS_POINT_BYTES;
  // endomorphism tables: windows over 130 bits -- half as many -- when the full set does not fit half of the free memory (or on
  // request: SONIC_MSM_ENDO=1, tests); one more addition per term and window-pair than the full tables, no tables at all costs 2.5x
  const int W_endo = (ENDO_BITS + c - 1) / c;
  bool endo = false;
  const bool fits_full = per_table * (size_t)W <= free_bytes / 2, fits_endo = per_table * (size_t)W_endo <= free_bytes / 2;
  const bool endo_forced = k.endo == 1, endo_off = k.endo == 0;
  if (k.tables == 0) { c = 0; W = 1; }
  else if ((endo_forced || (!fits_full && !endo_off)) && fits_endo) { endo = true; W = W_endo; c = (ENDO_BITS + W - 1) / W; }
  else if (fits_full && !endo_forced) c = c_full;
  else { c = 0; W = 1; }
  return SrsWindows{c, W, endo};
}
inline SrsWindows srs_window_policy(int64_t d, size_t free_bytes, const SrsKnobs& k) { return srs_window_policy(d, (size_t)(2 * d + 1), free_bytes, k); }

// the running sums of the alpha basis: one more table, where 1/13 of what the window tables took is still to be had
inline size_t srs_prefix_bytes_of(size_t npts) { return (size_t)SONIC_SRS_POINT_BYTES * npts; }
inline size_t srs_prefix_bytes(int64_t d) { return srs_prefix_bytes_of((size_t)(2 * d + 1)); }
inline bool srs_holds_prefix_of(size_t npts, size_t free_bytes, const SrsKnobs& k) { return k.prefix != 0 && srs_prefix_bytes_of(npts) <= free_bytes / 4; }
inline bool srs_holds_prefix(int64_t d, size_t free_bytes, const SrsKnobs& k) { return srs_holds_prefix_of((size_t)(2 * d + 1), free_bytes, k); }

// the symmetric sums of the alpha basis with window tables of their own: half of what the two bases took, where a quarter of the rest holds it
// (only with the full tables: the job over them shares a batched chain with jobs over the bases)
// (round 6: d + 1 slots per window -- exponents 0 .. d -- instead of a whole basis of 2d + 1)
// (sym_n: the slots of one table, exponents 0 .. sym_n - 1; d + 1 for a whole string)
inline size_t srs_sym_bytes_of(size_t sym_n, int W) { return (size_t)SONIC_SRS_POINT_BYTES * sym_n * (size_t)W; }
inline size_t srs_sym_bytes(int64_t d, int W) { return srs_sym_bytes_of((size_t)(d + 1), W); }
inline bool srs_holds_sym_of(size_t sym_n, int W, bool endo, size_t free_bytes, const SrsKnobs& k) {
  return k.sym != 0 && W > 1 && !endo && srs_sym_bytes_of(sym_n, W) <= free_bytes / 4;
}
inline bool srs_holds_sym(int64_t d, int W, bool endo, size_t free_bytes, const SrsKnobs& k) { return srs_holds_sym_of((size_t)(d + 1), W, endo, free_bytes, k); }

}  // namespace sonic
