// Host driver of the subgroup tests for tests/test_subgroup_host.py: g1_in_subgroup / g1_in_subgroup_walk (g1.hpp) and g2_in_subgroup /
// g2_in_subgroup_walk (g2.hpp) as the host compiles them, and the constants they use.  Reads one case per line from stdin, prints one line
// each.  Points are the canonical little-endian encodings of the C ABI in hex; they must be finite and on the curve / twist (the
// precondition of all four functions), which is checked here: anything else ends the run with status 2.
//   consts            -> "beta cx.c0 cx.c1 cy.c0 cy.c1"     standard form, hex
//   g1 hex96          -> "endo walk"                          0 | 1 each
//   g2 hex192         -> "endo walk"
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>
#include "../../sonic_amd/csrc/g2.hpp"

using namespace sonic;

static std::string hex_of_fq(const Fq& a) {
  char buf[97];
  for (int k = 0; k < 12; k++) snprintf(buf + 8 * k, 9, "%08x", a.l[11 - k]);
  return buf;
}
static bool bytes_of_hex(const std::string& h, size_t want, std::vector<uint8_t>& b) {
  if (h.size() != 2 * want) return false;
  b.resize(want);
  for (size_t i = 0; i < want; i++) b[i] = (uint8_t)strtoul(h.substr(2 * i, 2).c_str(), nullptr, 16);
  return true;
}
static Fq fq_of_bytes(const uint8_t* b) {         // canonical standard form -> Montgomery
  Fq r;
  memcpy(r.l, b, 48);
  return fp_to_mont(r);
}

int main() {
  std::string line;
  while (std::getline(std::cin, line)) {
    std::istringstream in(line);
    std::string op, a;
    in >> op;
    if (op == "consts") {
      G2Affine one;                                // psi(1, 1) = (c_x, c_y)
      one.x = Fq2::one(); one.y = Fq2::one();
      const G2Affine c = g2_psi(one);
      printf("%s %s %s %s %s\n", hex_of_fq(fp_from_mont(g1_endo_beta())).c_str(), hex_of_fq(fp_from_mont(c.x.c0)).c_str(),
             hex_of_fq(fp_from_mont(c.x.c1)).c_str(), hex_of_fq(fp_from_mont(c.y.c0)).c_str(), hex_of_fq(fp_from_mont(c.y.c1)).c_str());
    } else if (op == "g1") {
      in >> a;
      std::vector<uint8_t> e;
      if (!bytes_of_hex(a, 96, e)) { fprintf(stderr, "subgroup_host: a G1 point is 96 bytes\n"); return 2; }
      G1Affine p;
      p.x = fq_of_bytes(e.data()); p.y = fq_of_bytes(e.data() + 48);
      const Fq four = fp_dbl(fp_dbl(Fq::one()));
      if (p.is_inf() || fp_sqr(p.y) != fp_add(fp_mul(fp_sqr(p.x), p.x), four)) { fprintf(stderr, "subgroup_host: not a finite point of the curve\n"); return 2; }
      printf("%d %d\n", g1_in_subgroup(p) ? 1 : 0, g1_in_subgroup_walk(p) ? 1 : 0);
    } else if (op == "g2") {
      in >> a;
      std::vector<uint8_t> e;
      if (!bytes_of_hex(a, 192, e)) { fprintf(stderr, "subgroup_host: a G2 point is 192 bytes\n"); return 2; }
      G2Affine p;
      p.x.c0 = fq_of_bytes(e.data()); p.x.c1 = fq_of_bytes(e.data() + 48); p.y.c0 = fq_of_bytes(e.data() + 96); p.y.c1 = fq_of_bytes(e.data() + 144);
      if (p.is_inf() || !(f2_sqr(p.y) == g2_curve_rhs(p.x))) { fprintf(stderr, "subgroup_host: not a finite point of the twist\n"); return 2; }
      printf("%d %d\n", g2_in_subgroup(p) ? 1 : 0, g2_in_subgroup_walk(p) ? 1 : 0);
    } else if (!op.empty()) {
      fprintf(stderr, "subgroup_host: unknown case '%s'\n", op.c_str());
      return 2;
    }
  }
  printf("subgroup_host ok\n");
  return 0;
}
