// Host driver of the compressed encodings for tests/test_compress_host.py: the HD functions of field.hpp / g2.hpp / compress.hpp as the
// host compiles them, and the compressed SRS container's reader (srs_file.hpp).  Reads one case per line from stdin, prints one line each:
//   sqrt a            -> "ok root"          fq_sqrt (values: hex integers, standard form)
//   sqrt2 a0 a1       -> "ok r0 r1"         fq2_sqrt
//   high y            -> "0|1"              fq_is_high
//   high2 c0 c1       -> "0|1"              fq2_is_high
//   g1d hex48 sub     -> "verdict hex96"    g1_decompress_point (+ g1_in_subgroup when sub = 1), canonical bytes
//   g1c hex96         -> "hex48"            g1_compress_point
//   g2d hex96 sub     -> "verdict hex192"
//   g2c hex192        -> "hex96"
//   zfile path        -> "rc version flags d |g0| |g1| |h0| |h1|"      srs_zfile_read
//   sfile path        -> "rc"                                           srs_file_read (must refuse the compressed magic)
#include <stdio.h>
#include <stdlib.h>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>
#include "../../sonic_amd/csrc/compress.hpp"
#include "../../sonic_amd/csrc/srs_file.hpp"

using namespace sonic;

static Fq fq_of_hex(const std::string& h) {      // standard form, as given (not reduced)
  Fq r = Fq::zero();
  int nib = 0;
  for (int i = (int)h.size() - 1; i >= 0 && nib < 96; i--, nib++) {
    const char c = h[(size_t)i];
    const uint32_t v = c >= 'a' ? c - 'a' + 10 : c >= 'A' ? c - 'A' + 10 : c - '0';
    r.l[nib / 8] |= v << (4 * (nib % 8));
  }
  return r;
}
static std::string hex_of_fq(const Fq& a) {
  char buf[97];
  for (int k = 0; k < 12; k++) snprintf(buf + 8 * k, 9, "%08x", a.l[11 - k]);
  return buf;
}
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

int main() {
  std::string line;
  while (std::getline(std::cin, line)) {
    std::istringstream in(line);
    std::string op, a, b;
    in >> op;
    if (op == "sqrt") {
      in >> a;
      bool ok;
      const Fq r = fq_sqrt(fp_to_mont(fq_of_hex(a)), &ok);
      printf("%d %s\n", ok ? 1 : 0, hex_of_fq(fp_from_mont(r)).c_str());
    } else if (op == "sqrt2") {
      in >> a >> b;
      Fq2 x; x.c0 = fp_to_mont(fq_of_hex(a)); x.c1 = fp_to_mont(fq_of_hex(b));
      bool ok;
      const Fq2 r = fq2_sqrt(x, &ok);
      printf("%d %s %s\n", ok ? 1 : 0, hex_of_fq(fp_from_mont(r.c0)).c_str(), hex_of_fq(fp_from_mont(r.c1)).c_str());
    } else if (op == "high") {
      in >> a;
      printf("%d\n", fq_is_high(fq_of_hex(a)) ? 1 : 0);
    } else if (op == "high2") {
      in >> a >> b;
      printf("%d\n", fq2_is_high(fq_of_hex(a), fq_of_hex(b)) ? 1 : 0);
    } else if (op == "g1d") {
      int sub = 0;
      in >> a >> sub;
      const std::vector<uint8_t> z = bytes_of_hex(a);
      G1Affine p;
      uint8_t v = g1_decompress_point(z.data(), p);
      if (!v && sub && !p.is_inf() && !g1_in_subgroup(p)) { v = Z_OUTSIDE_SUBGROUP; p = G1Affine::inf(); }
      uint32_t w[24];
      g1_canonical_words(p, w);
      printf("%d %s\n", v, hex_of_bytes(reinterpret_cast<const uint8_t*>(w), 96).c_str());
    } else if (op == "g1c") {
      in >> a;
      const std::vector<uint8_t> e = bytes_of_hex(a);
      G1Affine p;
      memcpy(p.x.l, e.data(), 48); memcpy(p.y.l, e.data() + 48, 48);
      if (!p.is_inf()) { p.x = fp_to_mont(p.x); p.y = fp_to_mont(p.y); }
      uint8_t z[48];
      g1_compress_point(p, z);
      printf("%s\n", hex_of_bytes(z, 48).c_str());
    } else if (op == "g2d") {
      int sub = 0;
      in >> a >> sub;
      const std::vector<uint8_t> z = bytes_of_hex(a);
      G2Affine p;
      uint8_t v = g2_decompress_point(z.data(), p);
      if (!v && sub && !p.is_inf() && !g2_in_subgroup(p)) { v = Z_OUTSIDE_SUBGROUP; p = G2Affine::inf(); }
      uint32_t w[48];
      g2_canonical_words(p, w);
      printf("%d %s\n", v, hex_of_bytes(reinterpret_cast<const uint8_t*>(w), 192).c_str());
    } else if (op == "g2c") {
      in >> a;
      const std::vector<uint8_t> e = bytes_of_hex(a);
      G2Affine p;
      memcpy(p.x.c0.l, e.data(), 48); memcpy(p.x.c1.l, e.data() + 48, 48); memcpy(p.y.c0.l, e.data() + 96, 48); memcpy(p.y.c1.l, e.data() + 144, 48);
      if (!p.is_inf()) { p.x.c0 = fp_to_mont(p.x.c0); p.x.c1 = fp_to_mont(p.x.c1); p.y.c0 = fp_to_mont(p.y.c0); p.y.c1 = fp_to_mont(p.y.c1); }
      uint8_t z[96];
      g2_compress_point(p, z);
      printf("%s\n", hex_of_bytes(z, 96).c_str());
    } else if (op == "zfile" || op == "sfile") {
      in >> a;
      SrsFile f;
      std::string why;
      const int rc = op == "zfile" ? srs_zfile_read(a.c_str(), f, why) : srs_file_read(a.c_str(), f, why);
      printf("%d %u %u %lld %zu %zu %zu %zu\n", rc, f.version, f.flags, (long long)f.d, f.g0.size(), f.g1.size(), f.h0.size(), f.h1.size());
    } else if (!op.empty()) {
      fprintf(stderr, "compress_host: unknown case '%s'\n", op.c_str());
      return 2;
    }
  }
  printf("compress_host ok\n");
  return 0;
}
