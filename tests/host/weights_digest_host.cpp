// Host driver of weights digest v2 (sonic_amd/csrc/weights_tree.hpp, fs.hpp) for tests/test_weights_digest_host.py: the functions the kernels
// of weights_digest.hip are made of, as the host compiles them, built plain and under ASan / UBSan (weights_digest.mk).  Reads one case per
// line from stdin, prints one line each (hex without separators):
//   csr n Q rp0,rp1,..,rp3Q cols hexval hexcs   -> "root wd2 wd2m cd2"
//       cols = c0,c1,.. or "-" (no entries); hexval = the canonical bytes of the values (32 nnz bytes, or "-"); hexcs = Q x 32 bytes.
//       root and wd2 come from the ABI's form (int64 indices, canonical bytes: wd_tree_host<int64_t, false>); wd2m from the form the
//       handles keep (int32 indices, Montgomery values, converted per item: wd_tree_host<int32_t, true>, what the kernels instantiate);
//       cd2 = circuit digest v2 of (wd2, cs).
#include <stdio.h>
#include <stdlib.h>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>
#include "../../sonic_amd/csrc/fs.hpp"
#include "../../sonic_amd/csrc/weights_tree.hpp"

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
static std::vector<int64_t> ints_of_list(const std::string& s) {
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
    if (op == "csr") {
      long n, Q;
      std::string srp, scol, hval, hcs;
      in >> n >> Q >> srp >> scol >> hval >> hcs;
      const std::vector<int64_t> rp = ints_of_list(srp), col = ints_of_list(scol);
      const std::vector<uint8_t> val = bytes_of_hex(hval), cs = bytes_of_hex(hcs);
      const long R = 3 * Q;
      if (n < 1 || Q < 1 || (long)rp.size() != R + 1 || rp[0] != 0 || rp[(size_t)R] != (int64_t)col.size() || val.size() != 32 * col.size() || cs.size() != 32 * (size_t)Q) {
        printf("bad sizes\n");
        return 2;
      }
      const long nnz = (long)col.size();
      // exactly-sized heap copies, so that a read past either end is the sanitizer's to find
      std::vector<uint32_t> tree(8 * (size_t)wd_tree_digests(nnz));
      uint8_t root[32], rootm[32], wd[32], wdm[32], cd[32];
      wd_tree_host<int64_t, false>(rp.data(), col.data(), val.data(), R, tree.data(), root);
      fs_weights_digest_v2(n, Q, nnz, root, wd);
      std::vector<int32_t> rp32(rp.begin(), rp.end()), col32(col.begin(), col.end());
      std::vector<Fr> vm((size_t)nnz);
      for (long k = 0; k < nnz; k++) { Fr v; memcpy(v.l, &val[32 * (size_t)k], 32); vm[(size_t)k] = fp_to_mont(v); }
      std::vector<uint32_t> tree2(8 * (size_t)wd_tree_digests(nnz));
      wd_tree_host<int32_t, true>(rp32.data(), col32.data(), vm.data(), R, tree2.data(), rootm);
      fs_weights_digest_v2(n, Q, nnz, rootm, wdm);
      int64_t bad = -1;
      if (fs_circuit_digest_v2(wd, Q, cs.data(), cd, &bad) != 0) { printf("cs %lld not canonical\n", (long long)bad); return 2; }
      printf("%s %s %s %s\n", hex_of_bytes(root, 32).c_str(), hex_of_bytes(wd, 32).c_str(), hex_of_bytes(wdm, 32).c_str(), hex_of_bytes(cd, 32).c_str());
    } else if (!op.empty()) {
      printf("unknown op %s\n", op.c_str());
      return 2;
    }
  }
  printf("weights_digest_host ok\n");
  return 0;
}
