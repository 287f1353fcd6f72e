// Host driver of r1cs.hpp (sonic_amd/csrc) for tests/test_r1cs_host.py: the validation of three CSR matrices and the layouts made of them
// (the Sonic CSR of layout 1, the constants, the split of the rows into the kernels' two classes), as the host compiles them, built plain
// and under ASan / UBSan (r1cs.mk).  Reads cases from the file named on the command line and prints, per case, what the test compares
// byte for byte with the Python-integer model (tests/r1cs_ref.py).  A case is
//   case m N n_pub   then for each of A, B, C:   <count> row_ptr...   <count> col...   <count> val (64 hex digits each, little-endian bytes)...
// and its answer "refused <status> <message>" or
//   ok n Q nnz g / row_ptr ... / col ... / val ... / cs ... / short ... / long ...
#include <inttypes.h>
#include <stdio.h>
#include <stdlib.h>
#include <fstream>
#include <string>
#include <vector>
#include "../../sonic_amd/csrc/r1cs.hpp"

using namespace sonic;

static void print_hex(const uint8_t* p, size_t count) {
  for (size_t k = 0; k < count; k++) {
    putchar(' ');
    for (int i = 0; i < 32; i++) printf("%02x", (unsigned)p[32 * k + i]);
  }
  putchar('\n');
}

int main(int argc, char** argv) {
  if (argc < 2) { fprintf(stderr, "usage: r1cs_host <cases file>\n"); return 2; }
  std::ifstream in(argv[1]);
  if (!in) { fprintf(stderr, "cannot read %s\n", argv[1]); return 2; }
  printf("chunk %d\n", R1CS_ROW_CHUNK);
  std::string op;
  while (in >> op) {
    if (op != "case") { printf("unknown op %s\n", op.c_str()); return 2; }
    long long m, N, l;
    in >> m >> N >> l;
    std::vector<int64_t> rp[3], cl[3];
    std::vector<uint8_t> vl[3];
    for (int k = 0; k < 3; k++) {
      size_t cnt;
      in >> cnt;
      rp[k].resize(cnt);
      for (auto& x : rp[k]) { long long t; in >> t; x = t; }
      in >> cnt;
      cl[k].resize(cnt);
      for (auto& x : cl[k]) { long long t; in >> t; x = t; }
      in >> cnt;
      vl[k].resize(32 * cnt);
      for (size_t e = 0; e < cnt; e++) {
        std::string h;
        in >> h;
        if (h.size() != 64) { printf("bad value %s\n", h.c_str()); return 2; }
        for (int i = 0; i < 32; i++) vl[k][32 * e + i] = (uint8_t)strtoul(h.substr(2 * i, 2).c_str(), nullptr, 16);
      }
    }
    if (!in) { printf("truncated case\n"); return 2; }
    R1csView v;
    v.m = m; v.N = N; v.n_pub = l;
    for (int k = 0; k < 3; k++) v.M[k] = sonic_r1cs_matrix_t{rp[k].data(), cl[k].data(), vl[k].data()};
    char msg[256] = "";
    const int rc = r1cs_validate(v, msg, sizeof msg);
    if (rc) { printf("refused %d %s\n", rc, msg); continue; }
    const R1csShape s = r1cs_shape(v);
    printf("ok %" PRId64 " %" PRId64 " %" PRId64 " %" PRId64 "\n", s.n, s.Q, s.nnz, s.g);
    // exactly the sizes the header promises: the sanitizer build sees a write past any of them
    std::vector<int64_t> row_ptr(3 * (size_t)s.Q + 1), col((size_t)s.nnz);
    std::vector<uint8_t> val(32 * (size_t)s.nnz), cs(32 * (size_t)s.Q);
    r1cs_compile(v, row_ptr.data(), col.data(), val.data(), cs.data());
    printf("row_ptr");
    for (int64_t x : row_ptr) printf(" %" PRId64, x);
    printf("\ncol");
    for (int64_t x : col) printf(" %" PRId64, x);
    printf("\nval");
    print_hex(val.data(), (size_t)s.nnz);
    printf("cs");
    print_hex(cs.data(), (size_t)s.Q);
    R1csDeviceLayout L;
    r1cs_device_layout(v, L);
    // the stacked rows are the caller's, in order
    size_t at = 0;
    for (int k = 0; k < 3; k++)
      for (int64_t r = 0; r < m; r++) {
        if (L.row_ptr[(size_t)(k * m + r)] != (int32_t)at) { printf("device layout: row_ptr differs\n"); return 2; }
        for (int64_t e = rp[k][(size_t)r]; e < rp[k][(size_t)r + 1]; e++, at++)
          if (L.col[at] != (int32_t)cl[k][(size_t)e] || memcmp(&L.val[32 * at], &vl[k][32 * (size_t)e], 32)) { printf("device layout: entry differs\n"); return 2; }
      }
    if (L.row_ptr[3 * (size_t)m] != (int32_t)at) { printf("device layout: row_ptr differs\n"); return 2; }
    printf("short");
    for (int32_t x : L.short_rows) printf(" %d", x);
    printf("\nlong");
    for (int32_t x : L.long_rows) printf(" %d", x);
    printf("\n");
  }
  printf("r1cs_host ok\n");
  return 0;
}
