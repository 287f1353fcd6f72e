// Stand-alone check of sonic_amd/csrc/stream_pool.hpp (tests/test_stream_pool_host.py builds it plain and under ASan / UBSan): the three
// mapping rules for every pool size, the parsing of the two environment variables, and a small simulation of two proofs queued in one
// global order on P in-order streams.  Prints the mapping (one line per P) and, last, "stream_pool_host ok"; the first failed check is
// printed and the exit status is 1.
#include <stdio.h>
#include <functional>
#include <string>
#include <vector>
#include "../../sonic_amd/csrc/stream_pool.hpp"

using namespace sonic;

namespace {

constexpr int N_GROUPS = 6, N_CHAINS = 2;      // more roles than a proof has streams for: the round-robin must wrap
using Mapping = std::function<int(PoolRole, int, int)>;

int fails = 0;
void fail(const std::string& what) { printf("FAIL %s\n", what.c_str()); fails++; }
std::string at(const char* what, int P) { return std::string(what) + " at P = " + std::to_string(P); }

// the three rules of stream_pool.hpp and "every role maps below P"; returns whether `m` keeps them at P
bool rules_hold(const Mapping& m, int P, bool say) {
  bool ok = true;
  auto bad = [&](const char* what) { ok = false; if (say) fail(at(what, P)); };
  const int head = m(PoolRole::HEAD, 0, P), ntt = m(PoolRole::NTT, 0, P), tail = m(PoolRole::TAIL, 0, P), tg = m(PoolRole::T_GROUP, 0, P);
  std::vector<int> groups, chains, body;      // the streams of GROUP(k), of CHAIN(c), of both
  for (int k = 0; k < N_GROUPS; k++) groups.push_back(m(PoolRole::GROUP, k, P));
  for (int c = 0; c < N_CHAINS; c++) chains.push_back(m(PoolRole::CHAIN, c, P));
  body = groups;
  body.insert(body.end(), chains.begin(), chains.end());
  for (int s : {head, ntt, tail, tg}) if (s < 0 || s >= P) bad("a role maps outside the pool");
  for (int s : body) if (s < 0 || s >= P) bad("a group or chain maps outside the pool");
  // 1. TAIL never with HEAD or NTT
  if (tail == head) bad("TAIL shares HEAD's stream");
  if (tail == ntt) bad("TAIL shares NTT's stream");
  // 2. TAIL only with the body that is queued last -- T_GROUP, and the chains below P = 6 -- and with no GROUP, except at P = 2, where nothing
  //    else is left
  if (tail != tg) bad("TAIL is not on T_GROUP's stream");
  if (P > 2) for (int s : groups) if (s == tail) bad("a GROUP shares TAIL's stream");
  if (P >= 6) for (int s : chains) if (s == tail) bad("a CHAIN shares TAIL's stream although the pool has a stream for the chains");
  //    (and no group on a chain's stream: the next proof's preparation would wait for the chain)
  if (P > 2) for (int g : groups) for (int c : chains) if (g == c) bad("a GROUP shares a CHAIN's stream");
  // 3. HEAD with no GROUP, T_GROUP or CHAIN; with NTT only at the smallest P
  if (tg == head) bad("HEAD shares T_GROUP's stream");
  for (int s : body) if (s == head) bad("HEAD shares a GROUP's or CHAIN's stream");
  if (P > 2 && ntt == head) bad("HEAD shares NTT's stream above P = 2");
  return ok;
}

// ---- simulation: ops on in-order streams, each waiting for ops queued before it ----
struct Op { int stream; std::vector<int> deps; };
struct Proof { int head_last, ntt, last_body, tail; };      // indices of the ops the checks look at

// one proof as enqueue_proof queues it (prove.hip): HEAD a (r(X,1)), HEAD b (s(X,y)), NTT, HEAD c (s(X,y_j), s(u,Y)), GROUP(0) behind
// r(X,1), GROUP(1..3) behind HEAD c, T_GROUP behind the product, [fused: CHAIN(0) behind every lane], HEAD d (the side MSMs, behind a
// lane's masked copy), TAIL behind everything
Proof enqueue(std::vector<Op>& ops, const Mapping& m, int P, bool fused) {
  auto push = [&](PoolRole r, int k, std::vector<int> deps) { ops.push_back(Op{m(r, k, P), deps}); return (int)ops.size() - 1; };
  const int ha = push(PoolRole::HEAD, 0, {});
  const int hb = push(PoolRole::HEAD, 0, {ha});
  const int ntt = push(PoolRole::NTT, 0, {hb});
  const int hc = push(PoolRole::HEAD, 0, {hb});
  std::vector<int> lanes;
  lanes.push_back(push(PoolRole::GROUP, 0, {ha}));
  for (int k = 1; k < 4; k++) lanes.push_back(push(PoolRole::GROUP, k, {hc}));
  // (a fused proof's t lane only prepares openings, as a GROUP: prove.hip)
  const int tg = fused ? push(PoolRole::GROUP, 4, {ntt, hb}) : push(PoolRole::T_GROUP, 0, {ntt, hb});
  lanes.push_back(tg);
  int last_body = tg;
  if (fused) last_body = push(PoolRole::CHAIN, 0, lanes);
  const int hd = push(PoolRole::HEAD, 0, {hc, lanes[1]});
  std::vector<int> all = lanes;
  all.push_back(hd); all.push_back(ntt); all.push_back(last_body);
  const int tail = push(PoolRole::TAIL, 0, all);
  return Proof{hc, ntt, last_body, tail};
}

// runs the streams until nothing moves; `held` (or -1) never finishes.  Returns which ops finished.
std::vector<char> run(const std::vector<Op>& ops, int P, int held) {
  std::vector<std::vector<int>> q((size_t)P);
  for (int i = 0; i < (int)ops.size(); i++) q[(size_t)ops[(size_t)i].stream].push_back(i);
  std::vector<size_t> at((size_t)P, 0);
  std::vector<char> done(ops.size(), 0);
  for (bool moved = true; moved;) {
    moved = false;
    for (int s = 0; s < P; s++) {
      while (at[(size_t)s] < q[(size_t)s].size()) {
        const int i = q[(size_t)s][at[(size_t)s]];
        bool ready = i != held;
        for (int d : ops[(size_t)i].deps) ready = ready && done[(size_t)d];
        if (!ready) break;
        done[(size_t)i] = 1; at[(size_t)s]++; moved = true;
      }
    }
  }
  return done;
}

// two proofs in one global order: everything drains, and while the first proof's last body op is still running the second proof's head
// and product go through (what the pool is for).  Returns whether both hold.
bool simulate(const Mapping& m, int P, bool fused, bool check_overlap, bool say) {
  std::vector<Op> ops;
  const Proof a = enqueue(ops, m, P, fused), b = enqueue(ops, m, P, fused);
  bool ok = true;
  for (const Op& o : ops) if (o.stream < 0 || o.stream >= P) { if (say) fail(at("simulation: a stream outside the pool", P)); return false; }
  const std::vector<char> all = run(ops, P, -1);
  for (char d : all) if (!d) { ok = false; if (say) fail(at(fused ? "simulation (fused): does not drain" : "simulation: does not drain", P)); break; }
  if (check_overlap) {
    const std::vector<char> part = run(ops, P, a.last_body);
    if (part[(size_t)a.tail]) { ok = false; if (say) fail(at("simulation: a tail finished before its proof's body", P)); }
    if (!part[(size_t)b.head_last] || !part[(size_t)b.ntt]) { ok = false; if (say) fail(at("simulation: the second proof's head waits for the first proof's body", P)); }
  }
  return ok;
}

void expect_eq(const char* what, int got, int want) {
  if (got != want) fail(std::string(what) + ": got " + std::to_string(got) + ", want " + std::to_string(want));
}

}  // namespace

int main() {
  const Mapping ours = [](PoolRole r, int k, int P) { return pool_stream_of(r, k, P); };
  for (int P = POOL_MIN; P <= POOL_MAX; P++) {
    rules_hold(ours, P, true);
    simulate(ours, P, /*fused=*/false, /*check_overlap=*/true, true);
    simulate(ours, P, /*fused=*/true, /*check_overlap=*/true, true);
    printf("P %d head %d ntt %d groups", P, ours(PoolRole::HEAD, 0, P), ours(PoolRole::NTT, 0, P));
    for (int k = 0; k < N_GROUPS; k++) printf(" %d", ours(PoolRole::GROUP, k, P));
    printf(" t %d chains %d %d tail %d\n", ours(PoolRole::T_GROUP, 0, P), ours(PoolRole::CHAIN, 0, P), ours(PoolRole::CHAIN, 1, P), ours(PoolRole::TAIL, 0, P));
    // the groups spread over every stream that is left to them
    std::vector<char> used((size_t)P, 0);
    for (int k = 0; k < POOL_MAX; k++) used[(size_t)ours(PoolRole::GROUP, k, P)] = 1;
    int n_used = 0;
    for (char u : used) n_used += u;
    const int left = P == 2 ? 1 : P - 2 - (P >= 5 ? 1 : 0) - (P >= 6 ? 1 : 0);
    expect_eq(at("streams the groups use", P).c_str(), n_used, left);
  }
  // a mapping that puts TAIL on HEAD's stream: refused by the rules, and by the simulation (the second head waits for the first proof)
  const Mapping tail_on_head = [](PoolRole r, int k, int P) { return r == PoolRole::TAIL ? pool_stream_of(PoolRole::HEAD, 0, P) : pool_stream_of(r, k, P); };
  for (int P : {2, 4, 8}) {
    if (rules_hold(tail_on_head, P, false)) fail(at("the rules accept TAIL on HEAD's stream", P));
    if (simulate(tail_on_head, P, false, true, false)) fail(at("the simulation accepts TAIL on HEAD's stream", P));
  }
  // GPU_MAX_HW_QUEUES: unset, "4", "8", "0", "99", "x"
  expect_eq("queues unset", pool_queues_of_env(nullptr), 4);
  expect_eq("queues \"\"", pool_queues_of_env(""), 4);
  expect_eq("queues 4", pool_queues_of_env("4"), 4);
  expect_eq("queues 8", pool_queues_of_env("8"), 8);
  expect_eq("queues 0", pool_queues_of_env("0"), POOL_MIN);
  expect_eq("queues 99", pool_queues_of_env("99"), POOL_MAX);
  expect_eq("queues x", pool_queues_of_env("x"), 4);
  expect_eq("queues 8x", pool_queues_of_env("8x"), 4);
  // the pool's size: min(queues, 8) when the pool is on by default, the knob first
  expect_eq("size unset / on", pool_size_of_env(nullptr, nullptr, true), 4);
  expect_eq("size 8 / on", pool_size_of_env("8", nullptr, true), 8);
  expect_eq("size 32 / on", pool_size_of_env("32", nullptr, true), POOL_CAP);
  expect_eq("size 0 / on", pool_size_of_env("0", nullptr, true), 2);
  expect_eq("size x / on", pool_size_of_env("x", nullptr, true), 4);
  expect_eq("size unset / off", pool_size_of_env("8", nullptr, false), 0);
  expect_eq("knob 0", pool_size_of_env("8", "0", true), 0);
  expect_eq("knob 2", pool_size_of_env("8", "2", false), 2);
  expect_eq("knob 1", pool_size_of_env("8", "1", false), POOL_MIN);
  expect_eq("knob 8 over 4 queues", pool_size_of_env("4", "8", false), 8);
  expect_eq("knob 64", pool_size_of_env(nullptr, "64", false), POOL_MAX);
  expect_eq("knob x / on", pool_size_of_env("8", "x", true), 8);
  expect_eq("knob x / off", pool_size_of_env("8", "x", false), 0);
  if (fails) return 1;
  printf("stream_pool_host ok\n");
  return 0;
}
