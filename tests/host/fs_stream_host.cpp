// Host driver of witness digest v2 (sonic_amd/csrc/witness_tree.hpp, fs.hpp) for tests/test_fs_stream_host.py: the functions the kernels
// of witness.hip are made of, as the host compiles them, built plain and under ASan / UBSan (fs_stream.mk).  Reads one case per line
// from stdin, prints one line each (hex without separators):
//   tree n hexB                 -> "root digest blinder0"     hexB = the canonical bytes of aL || aR || aO (96 n bytes); blinder0 =
//                                                             fs_blinder(seed = 32 x 0x07, circuit digest = 32 x 0x01, srs id = 32 x 0x02, digest, 0)
//   sha hexmsg                  -> "ours sha256.hpp"          wt_compress over the padded message, and Sha256 of the same bytes ("-": empty)
#include <stdio.h>
#include <stdlib.h>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>
#include "../../sonic_amd/csrc/fs.hpp"
#include "../../sonic_amd/csrc/witness_tree.hpp"

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

// SHA-256 of any message through wt_compress alone: FIPS 180-4 padding, big-endian words
static void sha_by_compress(const std::vector<uint8_t>& msg, uint8_t out[32]) {
  std::vector<uint8_t> m = msg;
  m.push_back(0x80);
  while (m.size() % 64 != 56) m.push_back(0);
  const uint64_t bits = 8 * (uint64_t)msg.size();
  for (int i = 0; i < 8; i++) m.push_back((uint8_t)(bits >> (56 - 8 * i)));
  uint32_t s[8], w[16];
  wt_iv(s);
  for (size_t at = 0; at < m.size(); at += 64) {
    for (int k = 0; k < 16; k++) w[k] = (uint32_t)m[at + 4 * k] << 24 | (uint32_t)m[at + 4 * k + 1] << 16 | (uint32_t)m[at + 4 * k + 2] << 8 | m[at + 4 * k + 3];
    wt_compress(s, w);
  }
  wt_digest_bytes(s, out);
}

int main() {
  std::string line;
  while (std::getline(std::cin, line)) {
    std::istringstream in(line);
    std::string op;
    in >> op;
    if (op == "tree") {
      long n;
      std::string hb;
      in >> n >> hb;
      const std::vector<uint8_t> B = bytes_of_hex(hb);
      if (n < 1 || B.size() != (size_t)(96 * n)) { printf("bad sizes\n"); return 2; }
      // the handle keeps the assignment in Montgomery form, in three arrays: so does this
      std::vector<Fr> a((size_t)(3 * n));
      for (long e = 0; e < 3 * n; e++) { Fr v; memcpy(v.l, &B[32 * (size_t)e], 32); a[(size_t)e] = fp_to_mont(v); }
      const std::vector<Fr> aL(a.begin(), a.begin() + n), aR(a.begin() + n, a.begin() + 2 * n), aO(a.begin() + 2 * n, a.end());
      std::vector<uint32_t> tree(8 * (size_t)wt_tree_digests(n));
      uint8_t root[32], digest[32], blinder[32], seed[32], cd[32], sid[32];
      wt_tree_host(aL.data(), aR.data(), aO.data(), n, tree.data(), root);
      fs_witness_digest_v2(n, root, digest);
      memset(seed, 7, 32); memset(cd, 1, 32); memset(sid, 2, 32);
      fs_blinder(seed, cd, sid, digest, 0, blinder);
      printf("%s %s %s\n", hex_of_bytes(root, 32).c_str(), hex_of_bytes(digest, 32).c_str(), hex_of_bytes(blinder, 32).c_str());
    } else if (op == "sha") {
      std::string hm;
      in >> hm;
      const std::vector<uint8_t> msg = bytes_of_hex(hm);
      uint8_t ours[32], theirs[32];
      sha_by_compress(msg, ours);
      Sha256 h;
      h.update(msg.data(), msg.size());
      h.finish(theirs);
      printf("%s %s\n", hex_of_bytes(ours, 32).c_str(), hex_of_bytes(theirs, 32).c_str());
    } else if (!op.empty()) {
      printf("unknown op %s\n", op.c_str());
      return 2;
    }
  }
  printf("fs_stream_host ok\n");
  return 0;
}
