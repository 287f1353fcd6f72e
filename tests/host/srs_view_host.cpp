// Prints what sonic_amd/csrc/srs_view.hpp computes, for tests/test_srs_view_host.py.  Plain g++, no HIP.
//   stdin, one command per line; stdout, one line per command:
//     geo n Q d              ->  lo0 hi0 lo1 hi1 npts centre sym_n full          (n = 0: the whole string of d)
//     need n d               ->  the d a circuit of n needs when d is below it, else 0
//     slots n Q d            ->  e:slot for every exponent in [-d, d] (slot -1: not held), in exponent order
//     contains n Q d e0 cnt  ->  0 | 1
//     width n                ->  c W of the view's rule, then c W of srs_window_policy(8n), both with no memory limit and the environment's knobs
//     ranges z g2 n Q d      ->  file_bytes, then vector:e0:count:offset:bytes for every range a view reads (z: compressed container)
//     read path n Q          ->  rc, then on success: z g2 d npts, then per G1 basis the first u32 of every point read, then of every G2 point
#include <stdio.h>
#include <string.h>
#include <sstream>
#include <string>
#include "../../sonic_amd/csrc/srs_view.hpp"

using namespace sonic;

static SrsGeometry geo_of(long long n, long long Q, long long d) { return n ? srs_view_geometry(d, n, Q) : srs_full_geometry(d); }
static uint32_t u32_at(const std::vector<uint8_t>& v, size_t off) { uint32_t x; memcpy(&x, &v[off], 4); return x; }

int main() {
  char line[1024];
  while (fgets(line, sizeof line, stdin)) {
    std::istringstream in(line);
    std::string cmd;
    if (!(in >> cmd)) continue;
    long long n = 0, Q = 0, d = 0;
    if (cmd == "geo" && in >> n >> Q >> d) {
      const SrsGeometry g = geo_of(n, Q, d);
      printf("%lld %lld %lld %lld %lld %lld %lld %d\n", (long long)g.lo0, (long long)g.hi0, (long long)g.lo1, (long long)g.hi1, (long long)g.npts(),
             (long long)g.centre(), (long long)g.sym_n(), g.full() ? 1 : 0);
    } else if (cmd == "need" && in >> n >> d) {
      printf("%lld\n", (long long)srs_view_d_needed(d, n));
    } else if (cmd == "slots" && in >> n >> Q >> d) {
      const SrsGeometry g = geo_of(n, Q, d);
      for (long long e = -d; e <= d; e++) printf("%lld:%lld ", e, g.holds(e) ? (long long)g.slot(e) : -1LL);
      printf("\n");
    } else if (cmd == "contains") {
      long long e0 = 0, cnt = 0;
      if (!(in >> n >> Q >> d >> e0 >> cnt)) { printf("bad line\n"); return 2; }
      printf("%d\n", geo_of(n, Q, d).contains(e0, cnt) ? 1 : 0);
    } else if (cmd == "width" && in >> n) {
      const SrsKnobs k = srs_knobs_from_env();
      const SrsWindows v = srs_view_window_policy(n, 7 * n + 1, SIZE_MAX, k), w = srs_window_policy(8 * n, SIZE_MAX, k);
      printf("%d %d %d %d\n", v.c, v.W, w.c, w.W);
    } else if (cmd == "ranges") {
      int z = 0, g2 = 0;
      if (!(in >> z >> g2 >> n >> Q >> d)) { printf("bad line\n"); return 2; }
      SrsFileHead h;
      h.compressed = z != 0; h.version = z ? 1 : 2; h.flags = g2 ? 1u : 0u; h.d = d;
      printf("%llu", (unsigned long long)srs_file_bytes(h));
      for (const SrsFileRange& r : srs_view_file_ranges(h, srs_view_geometry(d, n, Q), n))
        printf(" %d:%lld:%lld:%llu:%llu", r.vector, (long long)r.e0, (long long)r.count, (unsigned long long)r.offset, (unsigned long long)r.bytes);
      printf("\n");
    } else if (cmd == "read") {
      std::string path;
      if (!(in >> path >> n >> Q)) { printf("bad line\n"); return 2; }
      SrsViewFile f;
      std::string err;
      const int rc = srs_view_file_read(path.c_str(), n, Q, f, err);
      printf("%d", rc);
      if (!rc) {
        printf(" %d %d %lld %lld", f.head.compressed ? 1 : 0, f.head.has_g2() ? 1 : 0, (long long)f.head.d, (long long)f.geo.npts());
        const size_t p1 = (size_t)srs_file_g1_point_bytes(f.head), p2 = (size_t)srs_file_g2_point_bytes(f.head);
        for (int b = 0; b < 2; b++)
          for (size_t i = 0; i < (size_t)f.geo.npts(); i++) printf(" %u", u32_at(f.g[b], i * p1));
        for (size_t i = 0; i * p2 < f.g2.size(); i++) printf(" %u", u32_at(f.g2, i * p2));
      }
      printf("\n");
    } else {
      printf("bad line\n");
      return 2;
    }
  }
  return 0;
}
