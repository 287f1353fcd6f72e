// Host driver of witness_src.hpp (sonic_amd/csrc) for tests/test_witness_src_host.py: the int64 -> Fr conversion the kernel of
// witness_src.hip is made of and the checks of a sonic_witness_src_t that need no device, as the host compiles them, built plain and
// under ASan / UBSan (witness_src.mk).  Reads one case per line from stdin, prints one line each:
//   i64 v                                   -> the 32 canonical bytes of v (hex), and the same after a round trip through Montgomery form
//   src kind on_device aL aR aO stride stream n B   -> "0 kind on_device stride" for an accepted description (the resolved stride), else
//                                              "7 message"; aL, aR, aO, stream: addresses as decimal integers (never dereferenced), 0 = NULL
//   null                                    -> the verdict on a NULL description
#include <inttypes.h>
#include <stdio.h>
#include <stdlib.h>
#include <iostream>
#include <sstream>
#include <string>
#include "../../sonic_amd/csrc/witness_src.hpp"

using namespace sonic;

static std::string hex_of_fr(const Fr& v) {
  std::string s;
  char t[3];
  for (int i = 0; i < 32; i++) { snprintf(t, 3, "%02x", (unsigned)((v.l[i >> 2] >> (8 * (i & 3))) & 0xff)); s += t; }
  return s;
}

int main() {
  std::string line;
  while (std::getline(std::cin, line)) {
    std::istringstream in(line);
    std::string op;
    in >> op;
    if (op == "i64") {
      long long v;
      in >> v;
      const Fr f = wit_i64_to_fr((int64_t)v);
      if (!fp_is_canonical(f)) { printf("not canonical\n"); return 2; }
      printf("%s %s\n", hex_of_fr(f).c_str(), hex_of_fr(fp_from_mont(fp_to_mont(f))).c_str());
    } else if (op == "src" || op == "null") {
      sonic_witness_src_t s;
      long long kind = 0, dev = 0, stride = 0, n = 1, B = 1;
      unsigned long long aL = 0, aR = 0, aO = 0, stream = 0;
      if (op == "src") in >> kind >> dev >> aL >> aR >> aO >> stride >> stream >> n >> B;
      s.aL = (const void*)(uintptr_t)aL; s.aR = (const void*)(uintptr_t)aR; s.aO = (const void*)(uintptr_t)aO;
      s.kind = (int32_t)kind; s.on_device = (int32_t)dev; s.stride = (int64_t)stride; s.hip_stream = (void*)(uintptr_t)stream;
      WitnessView v;
      char msg[256] = "";
      const int rc = wit_view_checked(op == "null" ? nullptr : &s, (int64_t)n, (int64_t)B, &v, msg, sizeof msg);
      if (rc) printf("%d %s\n", rc, msg);
      else {
        // the view carries the description over, the stride resolved, and block b starts b strides in
        const WitnessView b1 = v.block(1);
        if (v.aL != s.aL || v.aR != s.aR || v.aO != s.aO || b1.aL != v.aL + v.stride || (v.aO ? b1.aO != v.aO + v.stride : b1.aO != nullptr)) { printf("view differs\n"); return 2; }
        printf("0 %d %d %" PRId64 "\n", v.kind, (int)v.on_device, v.stride);
      }
    } else if (!op.empty()) {
      printf("unknown op %s\n", op.c_str());
      return 2;
    }
  }
  printf("witness_src_host ok\n");
  return 0;
}
