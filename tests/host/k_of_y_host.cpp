// Host driver of k(y) over many blocks (sonic_amd/csrc/k_of_y_plan.hpp; kernels: poly.hip, k_k_of_y_partials / k_k_of_y_finish) for
// tests/test_k_of_y_host.py, built plain and under ASan / UBSan (k_of_y.mk).  The span plan is the text the kernels compile; the field
// product is field.hpp's as the host compiles it.  Reads one case per line from stdin, prints one line each:
//   plan Q span   -> "blocks first_len last_len covered min_cover max_cover empty"
//       the spans of k_of_y_plan(Q, span) walked block by block over an exactly-sized heap array of Q counters: how many q were covered,
//       the least and the greatest number of times, and how many blocks had no term
//   sum Q span seed -> "one_pass one_block two_stage" (three times 64 hex digits, Montgomery limbs as they are)
//       cs and the powers: Q pseudo-random elements below 2^254 each (seed); one_pass = sum_q cs[q] ypow[q] in order; one_block = the sum
//       as k_sub_k_of_y forms it (256 strided accumulators, a tree over them); two_stage = the partials of every block formed the same
//       way over its span, then 256 strided accumulators over the partials and the tree
#include <stdio.h>
#include <stdlib.h>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>
#include "../../sonic_amd/csrc/field.hpp"
#include "../../sonic_amd/csrc/k_of_y_plan.hpp"

using namespace sonic;

static uint64_t rng_state;
static uint64_t next64() {      // splitmix64
  uint64_t z = (rng_state += 0x9e3779b97f4a7c15ull);
  z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull;
  z = (z ^ (z >> 27)) * 0x94d049bb133111ebull;
  return z ^ (z >> 31);
}
static Fr random_fr() {         // below 2^254 < r: a reduced element
  Fr a;
  for (int i = 0; i < 8; i += 2) { const uint64_t v = next64(); a.l[i] = (uint32_t)v; a.l[i + 1] = (uint32_t)(v >> 32); }
  a.l[7] &= 0x3fffffffu;
  return a;
}
static std::string hex_of(const Fr& a) {
  std::string s;
  char t[9];
  for (int i = 7; i >= 0; i--) { snprintf(t, 9, "%08x", a.l[i]); s += t; }
  return s;
}
// what one block of K_OF_Y_BLOCK threads leaves in sh[0]: thread t accumulates term(lo + t), term(lo + t + 256), .., then the tree
template <class Term>
static Fr block_sum(long lo, long hi, Term term) {
  std::vector<Fr> sh((size_t)K_OF_Y_BLOCK, Fr::zero());
  for (long t = 0; t < K_OF_Y_BLOCK; t++)
    for (long q = lo + t; q < hi; q += K_OF_Y_BLOCK) sh[(size_t)t] = fp_add(sh[(size_t)t], term(q));
  for (int o = K_OF_Y_BLOCK / 2; o >= 1; o >>= 1)
    for (int t = 0; t < o; t++) sh[(size_t)t] = fp_add(sh[(size_t)t], sh[(size_t)(t + o)]);
  return sh[0];
}

int main() {
  std::string line;
  while (std::getline(std::cin, line)) {
    std::istringstream in(line);
    std::string op;
    in >> op;
    if (op == "plan") {
      long Q, span;
      in >> Q >> span;
      const KOfYPlan p = k_of_y_plan(Q, span);
      std::vector<uint32_t> cover((size_t)Q, 0);      // exactly Q counters: a span that leaves [0, Q) is the sanitizer's to find
      long empty = 0, first_len = 0, last_len = 0;
      for (long b = 0; b < p.blocks; b++) {
        long lo, hi;
        k_of_y_span(p, Q, b, &lo, &hi);
        if (hi <= lo) empty++;
        if (b == 0) first_len = hi - lo;
        if (b == p.blocks - 1) last_len = hi - lo;
        for (long q = lo; q < hi; q++) cover[(size_t)q]++;
      }
      long covered = 0;
      uint32_t mn = ~0u, mx = 0;
      for (long q = 0; q < Q; q++) { covered += cover[(size_t)q] > 0; mn = cover[(size_t)q] < mn ? cover[(size_t)q] : mn; mx = cover[(size_t)q] > mx ? cover[(size_t)q] : mx; }
      printf("%ld %ld %ld %ld %u %u %ld\n", p.blocks, first_len, last_len, covered, mn, mx, empty);
    } else if (op == "sum") {
      long Q, span;
      unsigned long long seed;
      in >> Q >> span >> seed;
      rng_state = seed;
      std::vector<Fr> cs((size_t)Q), yp((size_t)Q);
      for (long q = 0; q < Q; q++) { cs[(size_t)q] = random_fr(); yp[(size_t)q] = random_fr(); }
      auto term = [&](long q) { return fp_mul(cs[(size_t)q], yp[(size_t)q]); };
      Fr one_pass = Fr::zero();
      for (long q = 0; q < Q; q++) one_pass = fp_add(one_pass, term(q));
      const Fr one_block = block_sum(0, Q, term);
      const KOfYPlan p = k_of_y_plan(Q, span);
      std::vector<Fr> partial((size_t)p.blocks);
      for (long b = 0; b < p.blocks; b++) {
        long lo, hi;
        k_of_y_span(p, Q, b, &lo, &hi);
        partial[(size_t)b] = block_sum(lo, hi, term);
      }
      const Fr two_stage = block_sum(0, p.blocks, [&](long b) { return partial[(size_t)b]; });
      printf("%s %s %s\n", hex_of(fp_canonical(one_pass)).c_str(), hex_of(fp_canonical(one_block)).c_str(), hex_of(fp_canonical(two_stage)).c_str());
    } else if (!op.empty()) {
      printf("unknown op %s\n", op.c_str());
      return 2;
    }
  }
  printf("k_of_y_host ok\n");
  return 0;
}
