// Host driver of the two-halved circuit digest and the batch digest v2 (sonic_amd/csrc/fs.hpp) for tests/test_statements_host.py: the
// functions as the host compiles them, built plain and under ASan / UBSan (statements.mk).  Reads one case per line from stdin, prints one
// line each (hex without separators; "-" stands for an empty list):
//   dense n Q hexW hexcs                       -> "midstate resumed whole"     hexW = wL || wR || wO; whole = SHA-256 over the one string
//   csr n Q rowptr cols hexval hexcs           -> "midstate resumed"           rowptr, cols: comma-separated integers
//   resume hexmid hexcs                        -> "rc digest"                  fs_circuit_digest_resume's status (0, 1, 2)
//   d2 n Q d K hexdigest hexsrsid hexproofs hexchal hexcs   -> "D"             fs_batch_digest_v2
#include <stdio.h>
#include <stdlib.h>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>
#include "../../sonic_amd/csrc/fs.hpp"

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
static std::vector<int64_t> ints_of(const std::string& s) {
  std::vector<int64_t> v;
  if (s == "-") return v;
  std::istringstream in(s);
  std::string tok;
  while (std::getline(in, tok, ',')) v.push_back(strtoll(tok.c_str(), nullptr, 10));
  return v;
}

int main() {
  std::string line;
  while (std::getline(std::cin, line)) {
    std::istringstream in(line);
    std::string op;
    in >> op;
    if (op == "dense") {
      int64_t n, Q;
      std::string hw, hc;
      in >> n >> Q >> hw >> hc;
      const std::vector<uint8_t> W = bytes_of_hex(hw), cs = bytes_of_hex(hc);
      if (W.size() != (size_t)(96 * Q * n) || cs.size() != (size_t)(32 * Q)) { printf("bad sizes\n"); return 2; }
      const size_t m = (size_t)(32 * Q * n);
      Sha256 h;
      fs_circuit_begin(h, n, Q);
      fs_circuit_absorb_dense(h, n, Q, W.data(), W.data() + m, W.data() + 2 * m);
      uint8_t mid[FS_MIDSTATE_SIZE], resumed[32], whole[32];
      fs_midstate_save(h, Q, mid);
      if (fs_circuit_digest_resume(mid, cs.data(), resumed) != 0) { printf("resume refused\n"); return 2; }
      Sha256 w;
      fs_circuit_begin(w, n, Q);
      w.update(W.data(), W.size());
      w.update(cs.data(), cs.size());
      w.finish(whole);
      printf("%s %s %s\n", hex_of_bytes(mid, sizeof mid).c_str(), hex_of_bytes(resumed, 32).c_str(), hex_of_bytes(whole, 32).c_str());
    } else if (op == "csr") {
      int64_t n, Q;
      std::string rp, cl, hv, hc;
      in >> n >> Q >> rp >> cl >> hv >> hc;
      const std::vector<int64_t> row_ptr = ints_of(rp), col = ints_of(cl);
      const std::vector<uint8_t> val = bytes_of_hex(hv), cs = bytes_of_hex(hc);
      if (row_ptr.size() != (size_t)(3 * Q + 1) || val.size() != 32 * col.size() || cs.size() != (size_t)(32 * Q)) { printf("bad sizes\n"); return 2; }
      Sha256 h;
      fs_circuit_begin(h, n, Q);
      fs_circuit_absorb_csr(h, n, Q, row_ptr.data(), col.data(), val.data());
      uint8_t mid[FS_MIDSTATE_SIZE], resumed[32];
      fs_midstate_save(h, Q, mid);
      if (fs_circuit_digest_resume(mid, cs.data(), resumed) != 0) { printf("resume refused\n"); return 2; }
      printf("%s %s\n", hex_of_bytes(mid, sizeof mid).c_str(), hex_of_bytes(resumed, 32).c_str());
    } else if (op == "resume") {
      std::string hm, hc;
      in >> hm >> hc;
      const std::vector<uint8_t> mid = bytes_of_hex(hm), cs = bytes_of_hex(hc);
      if (mid.size() != FS_MIDSTATE_SIZE) { printf("bad sizes\n"); return 2; }
      // (a refused midstate never reads cs; an accepted one reads 32 Q bytes of it: the test sends that many)
      const int64_t Q = fs_midstate_Q(mid.data());
      if (Q > 0 && cs.size() != (size_t)(32 * Q)) { printf("bad sizes\n"); return 2; }
      uint8_t out[32] = {0};
      const int rc = fs_circuit_digest_resume(mid.data(), cs.data(), out);
      printf("%d %s\n", rc, hex_of_bytes(out, 32).c_str());
    } else if (op == "d2") {
      int64_t n, Q, d, K;
      std::string hd, hs, hp, hch, hc;
      in >> n >> Q >> d >> K >> hd >> hs >> hp >> hch >> hc;
      const std::vector<uint8_t> dg = bytes_of_hex(hd), id = bytes_of_hex(hs), proofs = bytes_of_hex(hp), chal = bytes_of_hex(hch), cs = bytes_of_hex(hc);
      const size_t psz = (size_t)((7 + 4 * Q) * 96 + (5 + 2 * Q) * 32);
      if (dg.size() != 32 || id.size() != 32 || proofs.size() != psz * (size_t)K || chal.size() != (size_t)(32 * (2 + 2 * Q) * K) || cs.size() != (size_t)(32 * Q * K)) { printf("bad sizes\n"); return 2; }
      uint8_t D[32];
      fs_batch_digest_v2(n, Q, d, dg.data(), id.data(), K, proofs.data(), psz, chal.data(), cs.data(), D);
      printf("%s\n", hex_of_bytes(D, 32).c_str());
    } else if (!op.empty()) {
      printf("unknown op %s\n", op.c_str());
      return 2;
    }
  }
  printf("statements_host ok\n");
  return 0;
}
