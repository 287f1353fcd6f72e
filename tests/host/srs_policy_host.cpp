// Prints what sonic_amd/csrc/srs_policy.hpp decides, for tests/test_srs_policy_host.py.  Plain g++, no HIP.
//   stdin, one case per line:  d free_w free_p free_s [SONIC_...=value ...]
//       the free memory before each of srs_alloc's three questions -- windows, running sums, symmetric sums -- as a decimal number of
//       bytes, or "max" for no limit
//   stdout, one line per case: c W endo prefix sym
// The knobs of a line go into the environment and are read back by srs_knobs_from_env, as srs_alloc reads them.
#include <stdio.h>
#include <string.h>
#include <sstream>
#include <string>
#include <vector>
#include "../../sonic_amd/csrc/srs_policy.hpp"

using namespace sonic;

int main() {
  char line[512];
  while (fgets(line, sizeof line, stdin)) {
    std::istringstream in(line);
    long long d;
    std::string fr[3], kv;
    if (!(in >> d >> fr[0] >> fr[1] >> fr[2])) continue;
    size_t free_b[3];
    for (int i = 0; i < 3; i++) free_b[i] = fr[i] == "max" ? SIZE_MAX : (size_t)strtoull(fr[i].c_str(), nullptr, 10);
    std::vector<std::string> names;
    while (in >> kv) {
      const size_t eq = kv.find('=');
      if (eq == std::string::npos) { printf("bad knob %s\n", kv.c_str()); return 2; }
      names.push_back(kv.substr(0, eq));
      setenv(names.back().c_str(), kv.c_str() + eq + 1, 1);
    }
    const SrsKnobs k = srs_knobs_from_env();
    for (const std::string& n : names) unsetenv(n.c_str());
    const SrsWindows w = srs_window_policy(d, free_b[0], k);
    printf("%d %d %d %d %d\n", w.c, w.W, w.endo ? 1 : 0, srs_holds_prefix(d, free_b[1], k) ? 1 : 0, srs_holds_sym(d, w.W, w.endo, free_b[2], k) ? 1 : 0);
  }
  return 0;
}
