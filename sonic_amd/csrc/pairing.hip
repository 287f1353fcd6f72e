// Pairings on the device (include/sonic_hip.h, "Pairing"): products of pairings checked in groups.  The formulas are pairing.hpp's, the
// same text the host verifier compiles, so the device and the host compute the same field elements.
//
//   k_miller_loops       one thread per pair, blocks of 64: f_{|x|, Q}(P), 1 where either point is infinity
//   k_gt_plan            the chunk counts of one pass of the segmented product as a running sum (pairing_groups.hpp), one block
//   k_gt_group_product   one thread per chunk of a group; repeated until one value per group is left
//   k_final_exp          one thread per group: the final exponentiation, is_one, and the value's 576 bytes where asked for
//
// pairing_groups_device strings them together for sonic_pairing_check (below) and for the per-proof fold of the batched verifier
// (verify_batch.hip).  Nothing here waits on another block: every dependency is a kernel boundary on one stream.
#include <string.h>
#include <stdlib.h>
#include <algorithm>
#include <system_error>
#include "internal.hpp"
#include "pairing_groups.hpp"
#include "pairing_device.hpp"

namespace sonic {
namespace {

using namespace pairing;

__global__ __launch_bounds__(64) void k_miller_loops(const G1Affine* __restrict__ P, const G2Affine* __restrict__ Q, long n, F12* __restrict__ out) {
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  out[i] = miller_loop(P[i], Q[i]);
}

constexpr int PLAN_BLOCK = 256;
__global__ __launch_bounds__(PLAN_BLOCK) void k_gt_plan(const int64_t* __restrict__ in_end, long G, int64_t* __restrict__ out_end) {
  __shared__ long cnt[PLAN_BLOCK];
  const long per = (G + PLAN_BLOCK - 1) / PLAN_BLOCK;
  const long g0 = min((long)threadIdx.x * per, G), g1 = min(g0 + per, G);
  cnt[threadIdx.x] = gt_plan_count(in_end, g0, g1);
  __syncthreads();
  long before = 0;
  for (int t = 0; t < (int)threadIdx.x; t++) before += cnt[t];
  gt_plan_write(in_end, g0, g1, before, out_end);
}
__global__ __launch_bounds__(64) void k_gt_group_product(const F12* __restrict__ in, const int64_t* __restrict__ in_end, const int64_t* __restrict__ out_end, long G,
                                                         long bound, F12* __restrict__ out) {
  const long t = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= bound) return;
  F12 v;
  if (gt_chunk_product(in, in_end, out_end, G, t, v)) out[t] = v;
}
__global__ __launch_bounds__(64) void k_final_exp(const F12* __restrict__ val, long G, uint8_t* __restrict__ is_one, uint8_t* __restrict__ gt) {
  const long g = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (g >= G) return;
  const F12 v = final_exponentiation(val[g]);
  is_one[g] = v.is_one() ? 1 : 0;
  if (gt) f12_to_words(v, reinterpret_cast<uint32_t*>(gt + 576 * g));
}

// sonic_pairing_check on the device: the pairs whose encodings the validators accepted (flag 0) as Montgomery points; a refused pair
// enters as (O, O) and its group's verdict is made of the flags
__global__ __launch_bounds__(256) void k_pairing_points(const uint8_t* __restrict__ g1, const uint8_t* __restrict__ g2, const uint8_t* __restrict__ f1,
                                                        const uint8_t* __restrict__ f2, long n, G1Affine* __restrict__ P, G2Affine* __restrict__ Q) {
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  G1Affine p = G1Affine::inf();
  G2Affine q = G2Affine::inf();
  if (!(f1[i] | f2[i])) {
    const uint32_t* a = reinterpret_cast<const uint32_t*>(g1 + 96 * i);
    const uint32_t* b = reinterpret_cast<const uint32_t*>(g2 + 192 * i);
    for (int k = 0; k < 12; k++) { p.x.l[k] = a[k]; p.y.l[k] = a[12 + k]; }
    for (int k = 0; k < 12; k++) { q.x.c0.l[k] = b[k]; q.x.c1.l[k] = b[12 + k]; q.y.c0.l[k] = b[24 + k]; q.y.c1.l[k] = b[36 + k]; }
    if (!p.is_inf()) { p.x = fp_to_mont(p.x); p.y = fp_to_mont(p.y); }
    if (!q.is_inf()) { q.x.c0 = fp_to_mont(q.x.c0); q.x.c1 = fp_to_mont(q.x.c1); q.y.c0 = fp_to_mont(q.y.c0); q.y.c1 = fp_to_mont(q.y.c1); }
  }
  P[i] = p; Q[i] = q;
}
// one thread per group: the validators' bits (1 non-canonical, 2 off the curve, 4 outside the subgroup) of the group's points, ORed and
// doubled, are the verdict of a group with a bad point and its value is zeros; else 0 / 1 from is_one
__global__ __launch_bounds__(256) void k_pairing_verdicts(const uint8_t* __restrict__ f1, const uint8_t* __restrict__ f2, const int64_t* __restrict__ group_end, long G,
                                                          const uint8_t* __restrict__ is_one, uint8_t* __restrict__ verdict, uint8_t* __restrict__ gt) {
  const long g = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (g >= G) return;
  uint32_t bad = 0;
  for (long i = g ? (long)group_end[g - 1] : 0; i < (long)group_end[g]; i++) bad |= f1[i] | f2[i];
  verdict[g] = bad ? (uint8_t)(bad << 1) : (is_one[g] ? 0 : 1);
  if (bad && gt) {
    uint32_t* o = reinterpret_cast<uint32_t*>(gt + 576 * g);
    for (int k = 0; k < 144; k++) o[k] = 0;
  }
}

}  // namespace

void pairing_groups_device(hipStream_t st, const G1Affine* dP, const G2Affine* dQ, long n, const int64_t* d_group_end, long G, uint8_t* d_is_one, uint8_t* d_gt) {
  if (G <= 0) return;
  // The passes come from n, not from the largest group: only the device knows the groups.  A pass over groups that are down to one value
  // each copies them.  `bound`, what a pass launches, is an upper bound from upper bounds and can exceed a buffer's size from the third
  // pass on; what a pass WRITES is its true chunk count, out_end[G - 1] (gt_chunk_product refuses every t beyond it), and after the first
  // pass -- where an empty group becomes one value -- a group's count never grows: count c -> max(1, ceil(c / 16)) <= c.  So every pass
  // writes at most the first pass's count, which is at most b1, the size of both buffers.
  const int passes = gt_passes(n);
  const long b1 = gt_out_bound(n, G);
  DevBuf f(sizeof(F12) * (size_t)std::max<long>(n, 1)), va(sizeof(F12) * (size_t)b1), vb(sizeof(F12) * (size_t)b1);
  DevBuf ea(sizeof(int64_t) * (size_t)G), eb(sizeof(int64_t) * (size_t)G);
  if (n > 0) LAUNCH(k_miller_loops, ceil_div(n, 64), 64, 0, st, dP, dQ, n, f.as<F12>());
  const F12* in = f.as<F12>();
  const int64_t* in_end = d_group_end;
  long bound = n;
  for (int p = 0; p < passes; p++) {
    F12* out = (p & 1 ? vb : va).as<F12>();
    int64_t* out_end = (p & 1 ? eb : ea).as<int64_t>();
    bound = gt_out_bound(bound, G);
    LAUNCH(k_gt_plan, 1, PLAN_BLOCK, 0, st, in_end, G, out_end);
    LAUNCH(k_gt_group_product, ceil_div(bound, 64), 64, 0, st, in, in_end, (const int64_t*)out_end, G, bound, out);
    in = out; in_end = out_end;
  }
  LAUNCH(k_final_exp, ceil_div(G, 64), 64, 0, st, in, G, d_is_one, d_gt);
  HIP_OK(hipStreamSynchronize(st));               // the intermediate values live in this call's buffers
}

// SONIC_PAIRING_GPU, read per call: 0 never, 1 always, anything else (or unset) the measured rule
int pairing_gpu_knob() {
  const char* e = getenv("SONIC_PAIRING_GPU");
  if (!e || !*e) return -1;
  return strcmp(e, "0") == 0 ? 0 : strcmp(e, "1") == 0 ? 1 : -1;
}

namespace {

// the host validators with the verdict bits of sonic_pairing_check: 2 non-canonical, 4 off the curve / twist, 8 outside the subgroup
uint8_t host_load_g1(const uint8_t* b, G1Affine& p) {
  memcpy(p.x.l, b, 48); memcpy(p.y.l, b + 48, 48);
  if (p.is_inf()) return 0;
  if (!fp_is_canonical(p.x) || !fp_is_canonical(p.y)) return 2;
  p.x = fp_to_mont(p.x); p.y = fp_to_mont(p.y);
  const Fq four = fp_dbl(fp_dbl(Fq::one()));
  if (fp_sqr(p.y) != fp_add(fp_mul(fp_sqr(p.x), p.x), four)) return 4;
  return g1_in_subgroup(p) ? 0 : 8;
}
uint8_t host_load_g2(const uint8_t* b, G2Affine& p) {
  memcpy(p.x.c0.l, b, 48); memcpy(p.x.c1.l, b + 48, 48); memcpy(p.y.c0.l, b + 96, 48); memcpy(p.y.c1.l, b + 144, 48);
  if (p.is_inf()) return 0;
  if (!fp_is_canonical(p.x.c0) || !fp_is_canonical(p.x.c1) || !fp_is_canonical(p.y.c0) || !fp_is_canonical(p.y.c1)) return 2;
  p.x.c0 = fp_to_mont(p.x.c0); p.x.c1 = fp_to_mont(p.x.c1); p.y.c0 = fp_to_mont(p.y.c0); p.y.c1 = fp_to_mont(p.y.c1);
  if (!(f2_sqr(p.y) == g2_curve_rhs(p.x))) return 4;
  return g2_in_subgroup(p) ? 0 : 8;
}

// work(i) for i < count on up to 16 host threads (the calling one among them)
template <class F>
void parallel_for(long count, F&& work) {
  const int nt = (int)std::min<long>(count, std::min<long>(16, std::max(1u, std::thread::hardware_concurrency())));
  auto run = [&](int w) { for (long i = w; i < count; i += nt) work(i); };
  ThreadGroup th;
  int started = 1;
  try {
    for (; started < nt; started++) th.emplace_back(run, started);
  } catch (const std::system_error&) {}          // thread limit of the host process: the calling thread takes the rest
  if (nt > 0) run(0);
  for (int w = started; w < nt; w++) run(w);
  th.join();
}

void pairing_check_host(const uint8_t* g1, const uint8_t* g2, long n, const int64_t* group_end, long G, uint8_t* verdict, uint8_t* gt) {
  std::vector<F12> f((size_t)n);
  std::vector<uint8_t> bad((size_t)n);
  parallel_for(n, [&](long i) {
    G1Affine p; G2Affine q;
    bad[(size_t)i] = host_load_g1(g1 + 96 * (size_t)i, p) | host_load_g2(g2 + 192 * (size_t)i, q);
    f[(size_t)i] = bad[(size_t)i] ? F12::one() : miller_loop(p, q);
  });
  parallel_for(G, [&](long g) {
    const long s = g ? (long)group_end[g - 1] : 0, e = (long)group_end[g];
    uint8_t b = 0;
    for (long i = s; i < e; i++) b |= bad[(size_t)i];
    if (b) { verdict[g] = b; if (gt) memset(gt + 576 * (size_t)g, 0, 576); return; }
    F12 prod = F12::one();
    for (long i = s; i < e; i++) prod = i == s ? f[(size_t)i] : f12_mul(prod, f[(size_t)i]);
    const F12 v = final_exponentiation(prod);
    verdict[g] = v.is_one() ? 0 : 1;
    if (gt) { uint32_t w[144]; f12_to_words(v, w); memcpy(gt + 576 * (size_t)g, w, 576); }
  });
}

void pairing_check_device(const uint8_t* g1, const uint8_t* g2, long n, const int64_t* group_end, long G, uint8_t* verdict, uint8_t* gt) {
  CallLease lease;
  hipStream_t st = lease.st();
  const size_t n1 = (size_t)std::max<long>(n, 1);
  DevBuf r1(96 * n1), r2(192 * n1), f1(n1), f2(n1), P(sizeof(G1Affine) * n1), Q(sizeof(G2Affine) * n1);
  DevBuf ge(sizeof(int64_t) * (size_t)G), one((size_t)G), vd((size_t)G), dgt(gt ? 576 * (size_t)G : 0);
  if (n > 0) {
    HIP_OK(hipMemcpyAsync(r1.p, g1, 96 * (size_t)n, hipMemcpyHostToDevice, st));
    HIP_OK(hipMemcpyAsync(r2.p, g2, 192 * (size_t)n, hipMemcpyHostToDevice, st));
  }
  HIP_OK(hipMemcpyAsync(ge.p, group_end, sizeof(int64_t) * (size_t)G, hipMemcpyHostToDevice, st));
  g1_subgroup_enqueue(st, r1.as<uint8_t>(), f1.as<uint8_t>(), n, SONIC_SUBGROUP_DEFAULT);
  g2_subgroup_enqueue(st, r2.as<uint8_t>(), f2.as<uint8_t>(), n, SONIC_SUBGROUP_DEFAULT);
  if (n > 0) LAUNCH(k_pairing_points, ceil_div(n, 256), 256, 0, st, (const uint8_t*)r1.as<uint8_t>(), (const uint8_t*)r2.as<uint8_t>(), (const uint8_t*)f1.as<uint8_t>(),
                    (const uint8_t*)f2.as<uint8_t>(), n, P.as<G1Affine>(), Q.as<G2Affine>());
  uint8_t* d_gt = gt ? dgt.as<uint8_t>() : nullptr;
  pairing_groups_device(st, P.as<G1Affine>(), Q.as<G2Affine>(), n, ge.as<int64_t>(), G, one.as<uint8_t>(), d_gt);
  LAUNCH(k_pairing_verdicts, ceil_div(G, 256), 256, 0, st, (const uint8_t*)f1.as<uint8_t>(), (const uint8_t*)f2.as<uint8_t>(), (const int64_t*)ge.as<int64_t>(), G,
         (const uint8_t*)one.as<uint8_t>(), vd.as<uint8_t>(), d_gt);
  HIP_OK(hipMemcpyAsync(verdict, vd.p, (size_t)G, hipMemcpyDeviceToHost, st));
  if (gt) HIP_OK(hipMemcpyAsync(gt, dgt.p, 576 * (size_t)G, hipMemcpyDeviceToHost, st));
  HIP_OK(hipStreamSynchronize(st));
}

int pairing_args_ok(const uint8_t* g1, const uint8_t* g2, int64_t n, const int64_t* group_end, int64_t G, int where, const uint8_t* verdict) {
  const char* why = nullptr;
  if (n < 0 || n > MSM_TABLE_MAX_TERMS || G < 0 || G > MSM_TABLE_MAX_TERMS) why = "n_pairs and n_groups are 0 .. 2^26";
  else if (n > 0 && (!g1 || !g2)) why = "a point array is NULL";
  else if (G > 0 && (!group_end || !verdict)) why = "group_end or verdict is NULL";
  else if (where != SONIC_PAIRING_AUTO && where != SONIC_PAIRING_HOST && where != SONIC_PAIRING_GPU) why = "where is none of SONIC_PAIRING_AUTO, _HOST, _GPU";
  else if (G == 0 && n != 0) why = "pairs without a group";
  else {
    int64_t prev = 0;
    for (int64_t g = 0; g < G && !why; g++) { if (group_end[g] < prev) why = "group_end decreases (or starts below 0)"; prev = group_end[g]; }
    if (!why && G > 0 && group_end[G - 1] != n) why = "the last entry of group_end is not n_pairs";
  }
  if (!why) return SONIC_OK;
  set_error("sonic_pairing_check: bad argument: %s (n_pairs = %lld, n_groups = %lld, where = %d)", why, (long long)n, (long long)G, where);
  return SONIC_ERR_INVALID_ARG;
}

}  // namespace
}  // namespace sonic

using namespace sonic;

extern "C" int sonic_pairing_check(const uint8_t* g1, const uint8_t* g2, int64_t n_pairs, const int64_t* group_end, int64_t n_groups, int where, uint8_t* verdict,
                                   uint8_t* gt) {
  if (int rc = pairing_args_ok(g1, g2, n_pairs, group_end, n_groups, where, verdict)) return rc;
  if (n_groups == 0) return SONIC_OK;
  if (where == SONIC_PAIRING_AUTO) {
    const int knob = pairing_gpu_knob();
    where = knob == 1 || (knob < 0 && n_groups >= PAIRING_GPU_MIN_GROUPS) ? SONIC_PAIRING_GPU : SONIC_PAIRING_HOST;
  }
  if (where == SONIC_PAIRING_HOST) {
    API_HOST_BEGIN
    pairing_check_host(g1, g2, (long)n_pairs, group_end, (long)n_groups, verdict, gt);
    API_END
  }
  API_BEGIN
  pairing_check_device(g1, g2, (long)n_pairs, group_end, (long)n_groups, verdict, gt);
  API_END
}
