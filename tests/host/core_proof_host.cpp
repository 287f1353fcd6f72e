// Host driver of the core-proof pieces that need no GPU (sonic_amd/csrc/proof_layout.hpp, fs.hpp) for tests/test_core_proof_host.py,
// built plain and under ASan / UBSan (core_proof.mk).  Reads one case per line from stdin, prints for each (hex without separators):
//   layout Q                                  -> "count ..." lines, then "field <offset> <G|F> <index>" for every field core_proof_layout
//                                                writes, "head <offset> <G|F> <index>" for the first 576 bytes of proof_layout(Q), and
//                                                "z <offset> <G|F> <index>" for the 96 -> 48 repack
//   chal n Q d digest srsid proof             -> y || z of fs_core_challenges_of_proof
//   bdigest n Q d digest srsid K proofs yz cs -> D of fs_core_batch_digest
#include <stdio.h>
#include <stdlib.h>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>
#include "../../sonic_amd/csrc/fs.hpp"
#include "../../sonic_amd/csrc/proof_layout.hpp"

using namespace sonic;

static std::vector<uint8_t> bytes_of_hex(const std::string& h) {
  if (h == "-") return {};
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
    std::string op;
    in >> op;
    if (op == "layout") {
      long Q;
      in >> Q;
      const ProofLayout L{Q};
      printf("count core_K %ld\ncount core_F %ld\ncount core_transcript_len %ld\ncount core_proof_bytes %zu\ncount core_proof_bytes_compressed %zu\n", L.core_K, L.core_F,
             L.core_transcript_len, L.core_proof_bytes(), L.core_proof_bytes_compressed());
      // every input block carries its kind and index; the output is then walked field by field
      std::vector<uint8_t> pts(96 * (size_t)L.K(), 0), frs(32 * (size_t)L.F(), 0), tr(32 * (size_t)L.transcript_len(), 0), full(L.proof_bytes(), 0);
      for (long i = 0; i < L.K(); i++) { pts[96 * i] = 'G'; pts[96 * i + 1] = (uint8_t)i; }
      for (long i = 0; i < L.F(); i++) { frs[32 * i] = 'F'; frs[32 * i + 1] = (uint8_t)i; }
      std::vector<uint8_t> core(L.core_proof_bytes(), 0), z(L.core_proof_bytes_compressed(), 0), back(L.core_proof_bytes(), 0);
      core_proof_layout(pts.data(), frs.data(), core.data());
      proof_layout(Q, pts.data(), frs.data(), tr.data(), full.data());
      for (size_t at = 0; at < core.size(); at += core[at] == 'G' ? 96 : 32) printf("field %zu %c %d\n", at, core[at], (int)core[at + 1]);
      for (size_t at = 0; at < core.size(); at += full[at] == 'G' ? 96 : 32) printf("head %zu %c %d\n", at, full[at], (int)full[at + 1]);
      const bool ok = core_proof_repack(core.data(), 96, z.data(), 48, [](const uint8_t* i, uint8_t* o) { memcpy(o, i, 48); return true; });
      for (size_t at = 0; at < z.size(); at += z[at] == 'G' ? 48 : 32) printf("z %zu %c %d\n", at, z[at], (int)z[at + 1]);
      // and back: a refused point makes the result false while the walk goes on
      int seen = 0;
      const bool ok2 = core_proof_repack(z.data(), 48, back.data(), 96, [&](const uint8_t* i, uint8_t* o) { memcpy(o, i, 48); return ++seen != 2; });
      printf("repack %d %d %d %d\n", (int)ok, (int)ok2, seen, (int)(memcmp(back.data() + 544, core.data() + 544, 32) == 0));
    } else if (op == "chal") {
      long n, Q, d;
      std::string dg, sid, pf;
      in >> n >> Q >> d >> dg >> sid >> pf;
      const std::vector<uint8_t> D = bytes_of_hex(dg), S = bytes_of_hex(sid), P = bytes_of_hex(pf);
      if (D.size() != 32 || S.size() != 32 || P.size() != 576) { printf("bad sizes\n"); return 2; }
      uint8_t yz[64];
      fs_core_challenges_of_proof(n, Q, d, D.data(), S.data(), P.data(), yz);
      printf("%s\n", hex_of_bytes(yz, 64).c_str());
    } else if (op == "bdigest") {
      long n, Q, d, K;
      std::string dg, sid, pf, yz, cs;
      in >> n >> Q >> d >> dg >> sid >> K >> pf >> yz >> cs;
      const std::vector<uint8_t> D = bytes_of_hex(dg), S = bytes_of_hex(sid), P = bytes_of_hex(pf), Y = bytes_of_hex(yz), Cs = bytes_of_hex(cs);
      if (D.size() != 32 || S.size() != 32 || P.size() != (size_t)(576 * K) || Y.size() != (size_t)(64 * K) || Cs.size() != (size_t)(32 * Q * K)) { printf("bad sizes\n"); return 2; }
      uint8_t out[32];
      fs_core_batch_digest(n, Q, d, D.data(), S.data(), K, P.data(), Y.data(), Cs.data(), out);
      printf("%s\n", hex_of_bytes(out, 32).c_str());
    } else if (!op.empty()) {
      printf("unknown op %s\n", op.c_str());
      return 2;
    }
  }
  printf("core_proof_host ok\n");
  return 0;
}
