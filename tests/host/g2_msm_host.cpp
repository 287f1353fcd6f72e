// Host driver of the G2 MSM's host-only parts (sonic_amd/csrc/msm_g2_host.hpp) for tests/test_g2_msm_host.py: the window rule and the
// shifts, the chunk cut, and the Horner fold of window sums over g2.hpp's host arithmetic.  Reads one case per line from stdin, prints
// one line each.
//   walkmax                    -> G2_WALK_MAX and G2_MSM_SLAB
//   rule n                     -> c               g2_msm_window_bits
//   win bits c                 -> W shift_0 .. shift_{W-1}
//   cut first len              -> nchunks beg:end ..      every chunk of a bucket of len entries that starts at entry `first`
//   fold c W k_0 .. k_{W-1}    -> point           g2_msm_fold_windows over S_w = k_w h (k_w < 2^64; 0: infinity), 192 canonical bytes in hex
#include <stdio.h>
#include <stdlib.h>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>
#include "../../sonic_amd/csrc/compress.hpp"
#include "../../sonic_amd/csrc/srs_scale.hpp"
#include "../../sonic_amd/csrc/msm_g2_host.hpp"

using namespace sonic;

static G2Affine generator() {
  constexpr uint32_t x0[12] = G2_GEN_X0_MONT, x1[12] = G2_GEN_X1_MONT, y0[12] = G2_GEN_Y0_MONT, y1[12] = G2_GEN_Y1_MONT;
  G2Affine g;
  for (int i = 0; i < 12; i++) { g.x.c0.l[i] = x0[i]; g.x.c1.l[i] = x1[i]; g.y.c0.l[i] = y0[i]; g.y.c1.l[i] = y1[i]; }
  return g;
}

int main() {
  std::string line;
  while (std::getline(std::cin, line)) {
    std::istringstream in(line);
    std::string op;
    in >> op;
    if (op == "walkmax") {
      printf("%d %ld\n", G2_WALK_MAX, G2_MSM_SLAB);
    } else if (op == "rule") {
      long n = 0;
      in >> n;
      printf("%d\n", g2_msm_window_bits(n));
    } else if (op == "win") {
      int bits = 0, c = 0;
      in >> bits >> c;
      if (c < 1) { fprintf(stderr, "g2_msm_host: c = %d\n", c); return 2; }
      const int W = g2_msm_windows(bits, c);
      printf("%d", W);
      for (int w = 0; w < W; w++) printf(" %d", g2_msm_shift(c, w));
      printf("\n");
    } else if (op == "cut") {
      unsigned long first = 0, len = 0;
      in >> first >> len;
      const uint32_t k = g2_chunks((uint32_t)len);
      printf("%u", k);
      for (uint32_t j = 0; j < k; j++) { const G2ChunkRange r = g2_chunk_range((uint32_t)first, (uint32_t)len, j); printf(" %u:%u", r.beg, r.end); }
      printf("\n");
    } else if (op == "fold") {
      int c = 0, W = 0;
      in >> c >> W;
      if (W < 1 || W > 64) { fprintf(stderr, "g2_msm_host: W = %d\n", W); return 2; }
      std::vector<G2Jac> S((size_t)W);
      const G2Affine h = generator();
      for (int w = 0; w < W; w++) {
        unsigned long long k = 0;
        in >> k;
        Fr s = Fr::zero();
        s.l[0] = (uint32_t)k; s.l[1] = (uint32_t)(k >> 32);
        S[(size_t)w] = g2_scale(h, s, 2);
      }
      uint32_t out[48];
      g2_canonical_words(g2_to_affine(g2_msm_fold_windows(S.data(), W, c)), out);
      const uint8_t* b = reinterpret_cast<const uint8_t*>(out);
      for (int i = 0; i < 192; i++) printf("%02x", b[i]);
      printf("\n");
    } else if (!op.empty()) {
      fprintf(stderr, "g2_msm_host: unknown case '%s'\n", op.c_str());
      return 2;
    }
  }
  printf("g2_msm_host ok\n");
  return 0;
}
