// msm_finish_host (sonic_amd/csrc/msm_slot.hpp) on the slot form of the two-level running sums (pad1 == 3): built by
// tests/test_slot_form_host.py with g++ -fsanitize=address,undefined.  A slot is filled as the kernels fill it -- from nseg = 2^L runs
// run_sg = r_sg G (small multiples of the generator, some of them infinity) win[j] = the sum of the runs whose index has bit j set, and
// win[L] = T = t G -- and the fold must give K sum_sg sg run_sg + T = (K sum_sg sg r_sg + t) G, the directly weighted sum.  Also the
// butterfly's own form (pad1 == 1) with a weight on the total, which shares the function.  Prints one line per case and "slot_form_host ok".
#include <stdio.h>
#include <stdint.h>
#include <vector>
#include "../../sonic_amd/csrc/msm_slot.hpp"
#include "../../sonic_amd/csrc/g1_host.hpp"
using namespace sonic;

#define CHECK(c, ...) do { if (!(c)) { printf("FAILED (line %d): ", __LINE__); printf(__VA_ARGS__); printf("\n"); return 1; } } while (0)

static uint64_t st_ = 0x9e3779b97f4a7c15ull;
static uint64_t rnd64() { st_ ^= st_ << 13; st_ ^= st_ >> 7; st_ ^= st_ << 17; return st_; }

static G1Affine generator() {
  G1Affine g;
  const uint32_t gx[12] = G1_GEN_X_MONT, gy[12] = G1_GEN_Y_MONT;
  memcpy(g.x.l, gx, 48); memcpy(g.y.l, gy, 48);
  return g;
}
// k G by the literal double-and-add
static G1XYZZ mul_gen(uint64_t k) {
  const G1Affine g = generator();
  G1XYZZ acc = G1XYZZ::inf();
  for (int i = k ? 63 - __builtin_clzll(k) : -1; i >= 0; i--) {
    acc = g1_dbl(acc);
    if ((k >> i) & 1) acc = g1_add_mixed(acc, g);
  }
  return acc;
}
static bool same_point(const G1XYZZ& a, const G1XYZZ& b) {
  uint8_t x[96], y[96];
  g1_canonical_bytes_host(a, x);
  g1_canonical_bytes_host(b, y);
  return memcmp(x, y, 96) == 0;
}

enum Runs { RANDOM, ALL_INFINITY, ALL_EQUAL, SPARSE };

// the runs of one bucket set as the butterfly leaves them: their bit sums, and the two sums of their multipliers the checks need
struct RunSums { int L; std::vector<G1XYZZ> win; uint64_t weighted, plain; };
static RunSums make_runs(int L, Runs kind) {
  RunSums rs{L, std::vector<G1XYZZ>((size_t)L, G1XYZZ::inf()), 0, 0};
  for (int sg = 0; sg < (1 << L); sg++) {
    uint64_t r = 0;
    switch (kind) {
      case RANDOM: r = rnd64() % 5 == 0 ? 0 : rnd64() & 0xffff; break;
      case ALL_INFINITY: break;
      case ALL_EQUAL: r = 7; break;                                     // P + P in every sum
      case SPARSE: r = rnd64() % 64 == 0 ? (rnd64() & 0xff) + 1 : 0; break;   // nearly every run is infinity
    }
    rs.weighted += (uint64_t)sg * r;
    rs.plain += r;
    if (!r) continue;
    const G1XYZZ run = mul_gen(r);
    for (int j = 0; j < L; j++) if ((sg >> j) & 1) rs.win[(size_t)j] = g1_add(rs.win[(size_t)j], run);
  }
  return rs;
}

// one slot of form 3 (K > 0), or of form 1 (K == 0: run sg weighs sg + tot_mul, that is, the total weighs `tot_mul`)
static int one_case(const RunSums& rs, int K, Runs kind, bool zero_tot, uint32_t tot_mul) {
  const int L = rs.L;
  std::vector<MsmSlot> mem(1);
  MsmSlot& s = mem[0];
  memset(&s, 0xa5, sizeof s);              // whatever an earlier MSM left in the entries this form does not use
  for (int j = 0; j < L; j++) s.win[j] = rs.win[(size_t)j];
  s.W = L; s.c = 1;
  uint64_t want;
  if (K > 0) {
    const uint64_t t = zero_tot ? 0 : (rnd64() & 0xffffffffu) + 1;
    s.win[L] = mul_gen(t);
    s.pad0 = K; s.pad1 = 3;
    want = (uint64_t)K * rs.weighted + t;
  } else {
    s.win[L] = mul_gen(rs.plain);
    s.pad0 = (int)tot_mul; s.pad1 = 1;
    want = rs.weighted + (uint64_t)tot_mul * rs.plain;
  }
  const G1XYZZ got = msm_finish_host(s);
  CHECK(same_point(got, mul_gen(want)), "L = %d, K = %d, runs %d, zero total %d, weight %u", L, K, (int)kind, (int)zero_tot, tot_mul);
  if (want == 0) CHECK(got.is_inf(), "an empty sum is infinity (L = %d, K = %d)", L, K);
  printf("L=%d K=%d runs=%d zero_tot=%d mul=%u ok\n", L, K, (int)kind, (int)zero_tot, tot_mul);
  return 0;
}

int main() {
  for (int L : {2, 12, 13})
    for (Runs kind : {RANDOM, ALL_INFINITY, ALL_EQUAL, SPARSE}) {
      const RunSums rs = make_runs(L, kind);
      for (int K : {8, 64})
        for (bool zero_tot : {false, true})
          if (one_case(rs, K, kind, zero_tot, 0)) return 1;
      // K = 1: no doubling between the bit sums and the total
      if (L == 2 && one_case(rs, 1, kind, false, 0)) return 1;
      // the butterfly's form through the same function: total weighted 1 and (a bucket range of a sharded MSM) base + 1
      if (L == 12 && (kind == RANDOM || kind == ALL_INFINITY))
        for (uint32_t mul : {1u, 16385u})
          if (one_case(rs, 0, kind, false, mul)) return 1;
    }
  printf("slot_form_host ok\n");
  return 0;
}
