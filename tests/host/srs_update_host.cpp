// Host driver of the updatable SRS for tests/test_srs_update_host.py: the HD scaling functions (srs_scale.hpp), the G2 addition (g2.hpp),
// the randomizers of the structure check and the proof of a contribution (srs_update.hpp) as the host compiles them.  Reads one case per
// line from stdin, prints one line each.  Every value is the hex of its canonical bytes (scalars 32, G1 96, G2 192, little-endian).
//   g1s point scalar limbs   -> point       g1_scale over the low 32 * limbs bits
//   g2s point scalar limbs   -> point       g2_scale
//   g2a point point          -> point       g2_add of the two as Jacobian points
//   rho seed index           -> hex16       srs_check_rho
//   chal d id points384      -> scalar      srs_update::challenge
//   nonce seed x1 a1 id i    -> scalar      srs_update::seeded_nonce
//   make d id x1 a1 kx ka    -> proof       srs_update::make_proof
//   schnorr d id proof       -> "0" | "1 X A"     srs_update::schnorr_ok
//   peq g1 g2 g1 g2          -> "0|1"       srs_update::pairs_equal
#include <stdio.h>
#include <stdlib.h>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>
#include "../../sonic_amd/csrc/compress.hpp"
#include "../../sonic_amd/csrc/srs_update.hpp"

using namespace sonic;

static std::vector<uint8_t> bytes_of_hex(const std::string& h) {
  std::vector<uint8_t> b(h.size() / 2);
  for (size_t i = 0; i < b.size(); i++) b[i] = (uint8_t)strtoul(h.substr(2 * i, 2).c_str(), nullptr, 16);
  return b;
}
static std::string hex_of_bytes(const uint8_t* b, size_t n) {
  std::string s;
  char t[3];
  for (size_t i = 0; i < n; i++) { snprintf(t, 3, "%02x", b[i]); s += t; }
  return s;
}
static bool sized(const std::vector<uint8_t>& b, size_t n) {
  if (b.size() == n) return true;
  fprintf(stderr, "srs_update_host: a value of %zu bytes where %zu are expected\n", b.size(), n);
  exit(2);
}
static G1Affine g1_of(const std::vector<uint8_t>& e) {
  sized(e, 96);
  G1Affine p;
  memcpy(p.x.l, e.data(), 48); memcpy(p.y.l, e.data() + 48, 48);
  if (!p.is_inf()) { p.x = fp_to_mont(p.x); p.y = fp_to_mont(p.y); }
  return p;
}
static G2Affine g2_of(const std::vector<uint8_t>& e) {
  sized(e, 192);
  G2Affine p;
  memcpy(p.x.c0.l, e.data(), 48); memcpy(p.x.c1.l, e.data() + 48, 48); memcpy(p.y.c0.l, e.data() + 96, 48); memcpy(p.y.c1.l, e.data() + 144, 48);
  if (!p.is_inf()) { p.x.c0 = fp_to_mont(p.x.c0); p.x.c1 = fp_to_mont(p.x.c1); p.y.c0 = fp_to_mont(p.y.c0); p.y.c1 = fp_to_mont(p.y.c1); }
  return p;
}
static Fr fr_of(const std::vector<uint8_t>& e) { sized(e, 32); Fr k; memcpy(k.l, e.data(), 32); return k; }
static std::string hex_of_g1(const G1Affine& p) { uint32_t w[24]; g1_canonical_words(p, w); return hex_of_bytes(reinterpret_cast<const uint8_t*>(w), 96); }
static std::string hex_of_g2(const G2Affine& p) { uint32_t w[48]; g2_canonical_words(p, w); return hex_of_bytes(reinterpret_cast<const uint8_t*>(w), 192); }
static G2Jac jac_of(const G2Affine& p) {
  if (p.is_inf()) return G2Jac::inf();
  G2Jac r; r.x = p.x; r.y = p.y; r.z = Fq2::one();
  return r;
}

int main() {
  std::string line;
  while (std::getline(std::cin, line)) {
    std::istringstream in(line);
    std::string op, a, b, c, e, f, g;
    in >> op;
    if (op == "g1s" || op == "g2s") {
      int limbs = 8;
      in >> a >> b >> limbs;
      if (limbs < 1 || limbs > 8) { fprintf(stderr, "srs_update_host: limbs = %d\n", limbs); return 2; }
      const Fr k = fr_of(bytes_of_hex(b));
      if (op == "g1s") printf("%s\n", hex_of_g1(g1_to_affine(g1_scale(g1_of(bytes_of_hex(a)), k, limbs))).c_str());
      else printf("%s\n", hex_of_g2(g2_to_affine(g2_scale(g2_of(bytes_of_hex(a)), k, limbs))).c_str());
    } else if (op == "g2a") {
      in >> a >> b;
      // the second operand in a non-trivial Jacobian form: (4x, 8y, 2) is the same point
      G2Jac q = jac_of(g2_of(bytes_of_hex(b)));
      if (!q.is_inf()) { q.x = f2_dbl(f2_dbl(q.x)); q.y = f2_dbl(f2_dbl(f2_dbl(q.y))); q.z = f2_dbl(q.z); }
      printf("%s\n", hex_of_g2(g2_to_affine(g2_add(jac_of(g2_of(bytes_of_hex(a))), q))).c_str());
    } else if (op == "rho") {
      unsigned long long index = 0;
      in >> a >> index;
      const std::vector<uint8_t> s = bytes_of_hex(a);
      sized(s, 32);
      uint32_t be[8], out[4];
      for (int k = 0; k < 8; k++) be[k] = (uint32_t)s[4 * k] << 24 | (uint32_t)s[4 * k + 1] << 16 | (uint32_t)s[4 * k + 2] << 8 | s[4 * k + 3];
      srs_check_rho(be, index, out);
      printf("%s\n", hex_of_bytes(reinterpret_cast<const uint8_t*>(out), 16).c_str());
    } else if (op == "chal") {
      long long d = 0;
      in >> d >> a >> b;
      const std::vector<uint8_t> id = bytes_of_hex(a), pts = bytes_of_hex(b);
      sized(id, 32); sized(pts, 384);
      uint8_t out[32];
      srs_update::challenge(d, id.data(), pts.data(), out);
      printf("%s\n", hex_of_bytes(out, 32).c_str());
    } else if (op == "nonce") {
      unsigned i = 0;
      in >> a >> b >> c >> e >> i;
      const std::vector<uint8_t> seed = bytes_of_hex(a), x1 = bytes_of_hex(b), a1 = bytes_of_hex(c), id = bytes_of_hex(e);
      sized(seed, 32); sized(x1, 32); sized(a1, 32); sized(id, 32);
      uint8_t out[32];
      srs_update::seeded_nonce(seed.data(), x1.data(), a1.data(), id.data(), i, out);
      printf("%s\n", hex_of_bytes(out, 32).c_str());
    } else if (op == "make") {
      long long d = 0;
      in >> d >> a >> b >> c >> e >> f;
      const std::vector<uint8_t> id = bytes_of_hex(a), x1 = bytes_of_hex(b), a1 = bytes_of_hex(c), kx = bytes_of_hex(e), ka = bytes_of_hex(f);
      sized(id, 32); sized(x1, 32); sized(a1, 32); sized(kx, 32); sized(ka, 32);
      uint8_t proof[srs_update::PROOF_BYTES];
      srs_update::make_proof(d, id.data(), x1.data(), a1.data(), kx.data(), ka.data(), proof);
      printf("%s\n", hex_of_bytes(proof, sizeof proof).c_str());
    } else if (op == "schnorr") {
      long long d = 0;
      in >> d >> a >> b;
      const std::vector<uint8_t> id = bytes_of_hex(a), proof = bytes_of_hex(b);
      sized(id, 32); sized(proof, srs_update::PROOF_BYTES);
      G1Affine X, A;
      if (srs_update::schnorr_ok(d, id.data(), proof.data(), X, A)) printf("1 %s %s\n", hex_of_g1(X).c_str(), hex_of_g1(A).c_str());
      else printf("0\n");
    } else if (op == "peq") {
      in >> a >> b >> c >> e;
      printf("%d\n", srs_update::pairs_equal(g1_of(bytes_of_hex(a)), g2_of(bytes_of_hex(b)), g1_of(bytes_of_hex(c)), g2_of(bytes_of_hex(e))) ? 1 : 0);
    } else if (!op.empty()) {
      fprintf(stderr, "srs_update_host: unknown case '%s'\n", op.c_str());
      return 2;
    }
  }
  printf("srs_update_host ok\n");
  return 0;
}
