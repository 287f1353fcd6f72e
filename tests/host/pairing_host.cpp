// Host driver of the pairing as the device also compiles it, for tests/test_pairing_groups_host.py: pairing.hpp (one copy of the formulas)
// and pairing_groups.hpp (the segmented product of k_gt_plan / k_gt_group_product).  Reads one case per line from stdin, prints one line
// each.  Points and values are the canonical little-endian encodings of the C ABI in hex; points must be finite or all zeros, on the curve /
// twist (not checked: the callers of miller_loop validate).
//   consts                      -> ten field elements, gamma_1 .. gamma_5 of constants.hpp as c0 c1 each (standard form, hex); the program
//                                  has compared them with xi^(i (q - 1) / 6) computed at run time, status 3 when they differ
//   segments s0 s1 ...          -> "ok passes=P values=N": groups of these sizes over values made from a counter, through the passes of
//                                  pairing_groups.hpp (the plan walked in 1, 3 and 256 slices), against a straight loop; status 3 on a difference
//   gt hex576                   -> the 576 bytes after f12_from_words and f12_to_words ("bad" for a coordinate that is not below q)
//   pairs hexP hexQ [hexP hexQ ...]  -> the 576 bytes of final_exponentiation(prod miller_loop(P_i, Q_i))
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <algorithm>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>
#include "../../sonic_amd/csrc/pairing_groups.hpp"

using namespace sonic;
using namespace sonic::pairing;

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
static std::string hex_of_f12(const F12& v) {
  uint32_t w[144];
  f12_to_words(v, w);
  uint8_t b[576];
  memcpy(b, w, 576);
  std::string s(1152, '0');
  for (int i = 0; i < 576; i++) snprintf(&s[2 * i], 3, "%02x", b[i]);
  s.resize(1152);
  return s;
}

// gamma_i = xi^(i (q - 1) / 6) by a square-and-multiply over the bits of (q - 1) / 6: what constants.hpp's tables must hold
static void gammas_at_run_time(Fq2 gamma[6]) {
  constexpr uint32_t q[12] = FQ_P;
  uint32_t e[12];
  uint64_t rem = 0;
  for (int i = 11; i >= 0; i--) {                         // (q - 1) / 6; q - 1 only clears bit 0 of the odd q
    const uint64_t cur = (rem << 32) | (i == 0 ? q[0] - 1 : q[i]);
    e[i] = (uint32_t)(cur / 6);
    rem = cur % 6;
  }
  Fq2 xi; xi.c0 = Fq::one(); xi.c1 = Fq::one();
  Fq2 g = Fq2::one();
  for (int i = 12 * 32 - 1; i >= 0; i--) {
    g = f2_sqr(g);
    if ((e[i >> 5] >> (i & 31)) & 1) g = f2_mul(g, xi);
  }
  gamma[0] = Fq2::one();
  for (int i = 1; i < 6; i++) gamma[i] = f2_mul(gamma[i - 1], g);
}

// a value of Fq12 from a counter: twelve small, distinct, non-zero coordinates
static F12 value_of(long i) {
  F12 v;
  Fq2* cs[6] = {&v.c0.a0, &v.c0.a1, &v.c0.a2, &v.c1.a0, &v.c1.a1, &v.c1.a2};
  for (int j = 0; j < 6; j++) {
    Fq a = Fq::zero(), b = Fq::zero();
    a.l[0] = (uint32_t)(1 + 12 * i + 2 * j); a.l[1] = (uint32_t)(i * 2654435761u);
    b.l[0] = (uint32_t)(2 + 12 * i + 2 * j); b.l[2] = (uint32_t)(j + 1);
    cs[j]->c0 = fp_to_mont(a); cs[j]->c1 = fp_to_mont(b);
  }
  return v;
}

// the passes as pairing_groups_device strings them, the plan of each walked in `slices` slices; false on a difference from the loop
static bool run_segments(const std::vector<long>& sizes, int slices, int* passes_out, long* n_out) {
  const long G = (long)sizes.size();
  std::vector<int64_t> end((size_t)G);
  long n = 0;
  for (long g = 0; g < G; g++) { n += sizes[(size_t)g]; end[(size_t)g] = n; }
  std::vector<F12> val((size_t)n);
  for (long i = 0; i < n; i++) val[(size_t)i] = value_of(i);
  std::vector<F12> want((size_t)G, F12::one());
  for (long g = 0; g < G; g++)
    for (long i = g ? end[(size_t)g - 1] : 0; i < end[(size_t)g]; i++) want[(size_t)g] = f12_mul(want[(size_t)g], val[(size_t)i]);
  const int passes = gt_passes(n);
  long bound = n;
  std::vector<F12> in = val;
  std::vector<int64_t> in_end = end;
  for (int p = 0; p < passes; p++) {
    bound = gt_out_bound(bound, G);
    std::vector<int64_t> out_end((size_t)G, -1);
    const long per = (G + slices - 1) / slices;
    std::vector<long> cnt((size_t)slices);
    for (int t = 0; t < slices; t++) { const long g0 = std::min<long>(t * per, G), g1 = std::min<long>(g0 + per, G); cnt[(size_t)t] = gt_plan_count(in_end.data(), g0, g1); }
    long before = 0;
    for (int t = 0; t < slices; t++) {
      const long g0 = std::min<long>(t * per, G), g1 = std::min<long>(g0 + per, G);
      gt_plan_write(in_end.data(), g0, g1, before, out_end.data());
      before += cnt[(size_t)t];
    }
    if (out_end[(size_t)G - 1] > bound) return false;         // the launch bound holds
    // the device's buffers hold b1 values, the first pass's bound, in every pass: no pass may produce a value beyond them
    const long b1 = gt_out_bound(n, G);
    std::vector<F12> out((size_t)b1);
    long made = 0;
    for (long t = 0; t < bound; t++) {
      F12 v;
      if (!gt_chunk_product(in.data(), in_end.data(), out_end.data(), G, t, v)) continue;
      if (t >= b1) return false;
      out[(size_t)t] = v;
      made++;
    }
    if (made != out_end[(size_t)G - 1]) return false;
    out.resize((size_t)made);
    in.swap(out); in_end.swap(out_end);
  }
  if ((long)in.size() != G) return false;
  for (long g = 0; g < G; g++) if (in_end[(size_t)g] != g + 1 || !(in[(size_t)g] == want[(size_t)g])) return false;
  *passes_out = passes; *n_out = n;
  return true;
}

int main() {
  std::string line;
  while (std::getline(std::cin, line)) {
    std::istringstream in(line);
    std::string op, a, b;
    in >> op;
    if (op == "consts") {
      Fq2 rt[6];
      gammas_at_run_time(rt);
      const Fq2 gen[6] = {Fq2::one(), frobenius_gamma<1>(), frobenius_gamma<2>(), frobenius_gamma<3>(), frobenius_gamma<4>(), frobenius_gamma<5>()};
      std::string out;
      for (int i = 1; i < 6; i++) {
        if (!(gen[i] == rt[i])) { fprintf(stderr, "pairing_host: gamma_%d of constants.hpp is not xi^(%d (q - 1) / 6)\n", i, i); return 3; }
        out += hex_of_fq(fp_from_mont(gen[i].c0)) + " " + hex_of_fq(fp_from_mont(gen[i].c1)) + (i < 5 ? " " : "");
      }
      printf("%s\n", out.c_str());
    } else if (op == "segments") {
      std::vector<long> sizes;
      long s;
      while (in >> s) sizes.push_back(s);
      if (sizes.empty()) { fprintf(stderr, "pairing_host: segments needs sizes\n"); return 2; }
      int passes = 0;
      long n = 0;
      for (int slices : {1, 3, 256})
        if (!run_segments(sizes, slices, &passes, &n)) { fprintf(stderr, "pairing_host: the segmented product differs from the loop (%d slices)\n", slices); return 3; }
      printf("ok passes=%d values=%ld\n", passes, n);
    } else if (op == "gt") {
      in >> a;
      std::vector<uint8_t> e;
      if (!bytes_of_hex(a, 576, e)) { fprintf(stderr, "pairing_host: a value is 576 bytes\n"); return 2; }
      uint32_t w[144];
      memcpy(w, e.data(), 576);
      F12 v;
      if (!f12_from_words(w, v)) printf("bad\n");
      else printf("%s\n", hex_of_f12(v).c_str());
    } else if (op == "pairs") {
      F12 prod = F12::one();
      int count = 0;
      while (in >> a >> b) {
        std::vector<uint8_t> e1, e2;
        if (!bytes_of_hex(a, 96, e1) || !bytes_of_hex(b, 192, e2)) { fprintf(stderr, "pairing_host: a pair is 96 and 192 bytes\n"); return 2; }
        G1Affine p = G1Affine::inf();
        G2Affine q = G2Affine::inf();
        bool z1 = true, z2 = true;
        for (uint8_t x : e1) z1 = z1 && x == 0;
        for (uint8_t x : e2) z2 = z2 && x == 0;
        if (!z1) { p.x = fq_of_bytes(e1.data()); p.y = fq_of_bytes(e1.data() + 48); }
        if (!z2) { q.x.c0 = fq_of_bytes(e2.data()); q.x.c1 = fq_of_bytes(e2.data() + 48); q.y.c0 = fq_of_bytes(e2.data() + 96); q.y.c1 = fq_of_bytes(e2.data() + 144); }
        prod = f12_mul(prod, miller_loop(p, q));
        count++;
      }
      if (!count) { fprintf(stderr, "pairing_host: pairs needs pairs\n"); return 2; }
      printf("%s\n", hex_of_f12(final_exponentiation(prod)).c_str());
    } else if (!op.empty()) {
      fprintf(stderr, "pairing_host: unknown case '%s'\n", op.c_str());
      return 2;
    }
  }
  printf("pairing_host ok\n");
  return 0;
}
