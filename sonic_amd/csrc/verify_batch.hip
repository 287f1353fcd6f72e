// The batched verifier: K proofs for ONE circuit folded into one pairing product (Sonic's "helped"/batched setting).
//
// A pcV check i = (max_i, F_i, z_i, v_i, W_i) holds iff e(W_i, h^{alpha x}) e(g^{v_i} W_i^{-z_i}, h^alpha) = e(F_i, h^{x^{max_i - d}}).  With
// non-zero 128-bit randomizers rho_i the fold accepts iff
//
//     e(sum rho_i W_i, h^{alpha x}) . e((sum rho_i v_i) g - sum (rho_i z_i) W_i, h^alpha) . prod_m e(- sum_{max_i = m} rho_i F_i, h^{x^{m-d}}) = 1
//
// over all checks of all proofs: 2 + (distinct m) Miller loops -- 4 for `verify`, m in {n, d} -- and ONE final exponentiation, whatever K
// and Q are.  What grows with K runs on the device:
//   k_g1_validate      K (4Q + 7) proof points: canonical, on the curve, r P = O -- exactly what load_g1 accepts (verify_host.hpp)
//   k_s_of_uv_batch    s(u_k, v_k) for K pairs over the handle's resident circuit (device CSR), O(K (nnz + n)), no K x n table
//   the G1 sums        the variable-base MSM of msm.hip over the validated points, on the handle's own stream and workspace
// and the host keeps the list of checks (proof_checks: the same function sonic_verify uses), the scalars rho_i, rho_i z_i (K (3Q + 4) Fr
// products) and the pairing tail.
//
// rho_i = the first 128 bits (little-endian) of SHA-256("sonic-hip/batch/v1" || seed || D || le64 i), 0 replaced by 1, with
// D = SHA-256("sonic-hip/batch-digest/v1" || le64 n || le64 Q || le64 d || circuit digest || srs id || le64 K || K x (proof bytes || its
// 2 + 2Q challenges)) and i = k (3Q + 4) + (index of the check in proof_checks' order).  D binds everything the verdict depends on, so even
// a fixed public seed leaves a cheating prover no rho to aim at.
#include <string.h>
#include <stdlib.h>
#include <sys/random.h>
#include <algorithm>
#include <chrono>
#include <memory>
#include <system_error>
#include "verify_host.hpp"
#include "srs_handle.hpp"
#include "proof_layout.hpp"
#include "srs_scale.hpp"
#include "pairing_device.hpp"
#include "weights_tree.hpp"

namespace sonic {
namespace {

// ---- kernels --------------------------------------------------------------------------------------------------------------------

// M points from their 96-byte encodings -> affine Montgomery points for the MSM and one flag per point: 1 = what load_g1 accepts (both
// coordinates canonical; the encoding of infinity, or on the curve and in the order-r subgroup by the endomorphism test, g1_in_subgroup).
// A refused point is written as infinity, so that nothing downstream ever adds a point outside the subgroup.
__global__ __launch_bounds__(256) void k_g1_validate(const uint8_t* __restrict__ in, G1Affine* __restrict__ out, uint8_t* __restrict__ flags, long n) {
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const uint32_t* w = reinterpret_cast<const uint32_t*>(in + 96 * i);
  G1Affine p;
  for (int k = 0; k < 12; k++) { p.x.l[k] = w[k]; p.y.l[k] = w[12 + k]; }
  if (p.is_inf()) { out[i] = p; flags[i] = 1; return; }
  bool ok = fp_is_canonical(p.x) && fp_is_canonical(p.y);
  if (ok) {
    p.x = fp_to_mont(p.x); p.y = fp_to_mont(p.y);
    const Fq four = fp_dbl(fp_dbl(Fq::one()));
    ok = fp_sqr(p.y) == fp_add(fp_mul(fp_sqr(p.x), p.x), four);
  }
  ok = ok && g1_in_subgroup(p);
  out[i] = ok ? p : G1Affine::inf();
  flags[i] = ok ? 1 : 0;
}
// sonic_g1_subgroup_check: the same tests with the loaders' bits as the verdict (0 accepted, infinity included; 1 non-canonical, 2 off the
// curve, 4 outside the subgroup) and the membership test named by METHOD: the endomorphism test every loader runs, or the definition.
template <int METHOD>
__global__ __launch_bounds__(256) void k_g1_subgroup(const uint8_t* __restrict__ in, uint8_t* __restrict__ flags, long n) {
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const uint32_t* w = reinterpret_cast<const uint32_t*>(in + 96 * i);
  G1Affine p;
  for (int k = 0; k < 12; k++) { p.x.l[k] = w[k]; p.y.l[k] = w[12 + k]; }
  if (p.is_inf()) { flags[i] = 0; return; }
  if (!fp_is_canonical(p.x) || !fp_is_canonical(p.y)) { flags[i] = 1; return; }
  p.x = fp_to_mont(p.x); p.y = fp_to_mont(p.y);
  const Fq four = fp_dbl(fp_dbl(Fq::one()));
  if (fp_sqr(p.y) != fp_add(fp_mul(fp_sqr(p.x), p.x), four)) { flags[i] = 2; return; }
  flags[i] = (METHOD == SONIC_SUBGROUP_WALK ? g1_in_subgroup_walk(p) : g1_in_subgroup(p)) ? 0 : 4;
}

// The resident circuit: the 3Q rows as CSR (values Montgomery) and the work items the s-kernel's threads take -- at most S_ITEM entries of
// one row each, then S_ITEM consecutive gates of the diagonal each.
constexpr int S_ITEM = 32;
constexpr int S_BLOCK = 256;
struct CircuitDev {
  long n, Q, nnz;
  long row_items, items, nblk;                  // items = row_items + ceil(n / S_ITEM); nblk = ceil(items / S_BLOCK)
  const int32_t *row_ptr, *col, *item_row, *item_begin;
  const Fr* val;
};
struct UvPair { Fr u, uinv, v, vinv; };          // Montgomery; the inverses of a zero are zero (the proof is refused)

__device__ __forceinline__ Fr block_sum(Fr acc, Fr* sh) {
  sh[threadIdx.x] = acc;
  __syncthreads();
  for (int s = S_BLOCK / 2; s > 0; s >>= 1) {
    if ((int)threadIdx.x < s) sh[threadIdx.x] = fp_add(sh[threadIdx.x], sh[threadIdx.x + s]);
    __syncthreads();
  }
  return sh[0];
}

// s(u_k, v_k) = sum_q v^{n+q+1} sum_{entries of rows q, Q+q, 2Q+q} val u^{-i | i | i+n}  -  sum_i u^{i+n} (v^i + v^-i), the sum of s_of_uv
// (verify_host.hpp).  Grid = (proof, block of S_BLOCK items); a thread gets the power at the start of its item by one exponentiation and
// steps from there (column gaps inside a sparse row by a short exponentiation); the block's partial sums are reduced in LDS and written
// to partial[k * nblk + block]; k_s_of_uv_finish adds them per proof.
__global__ __launch_bounds__(S_BLOCK) void k_s_of_uv_batch(CircuitDev c, const UvPair* __restrict__ uv, long K, Fr* __restrict__ partial) {
  __shared__ Fr sh[S_BLOCK];
  const long k = (long)blockIdx.x / c.nblk, blk = (long)blockIdx.x % c.nblk;
  const UvPair p = uv[k];
  if (p.u.is_zero() || p.v.is_zero()) return;                  // refused per proof (block-uniform): k_s_of_uv_finish flags it
  const long t = blk * S_BLOCK + threadIdx.x;
  Fr acc = Fr::zero();
  if (t < c.row_items) {
    const long r = c.item_row[t], b = c.item_begin[t];
    const long rend = c.row_ptr[r + 1], e = b + S_ITEM < rend ? b + S_ITEM : rend;
    const int mat = (int)(r / c.Q);
    const long q = r % c.Q;
    const Fr base = mat == 0 ? p.uinv : p.u;
    long iprev = 0;
    Fr pw = Fr::one();
    for (long x = b; x < e; x++) {
      const long i = c.col[x] + 1;
      const long gap = x == b ? (mat == 2 ? i + c.n : i) : i - iprev;
      pw = gap == 1 ? fp_mul(pw, base) : fp_mul(pw, fp_pow_u64(base, (uint64_t)gap));
      iprev = i;
      acc = fp_add(acc, fp_mul(c.val[x], pw));
    }
    acc = fp_mul(acc, fp_pow_u64(p.v, (uint64_t)(c.n + q + 1)));
  } else if (t < c.items) {
    const long i0 = 1 + (t - c.row_items) * S_ITEM, i1 = i0 + S_ITEM - 1 < c.n ? i0 + S_ITEM - 1 : c.n;
    Fr a = fp_pow_u64(p.u, (uint64_t)(i0 + c.n)), vp = fp_pow_u64(p.v, (uint64_t)i0), vm = fp_pow_u64(p.vinv, (uint64_t)i0);
    for (long i = i0; i <= i1; i++) {
      acc = fp_sub(acc, fp_mul(a, fp_add(vp, vm)));
      a = fp_mul(a, p.u); vp = fp_mul(vp, p.v); vm = fp_mul(vm, p.vinv);
    }
  }
  const Fr sum = block_sum(acc, sh);
  if (threadIdx.x == 0) partial[k * c.nblk + blk] = sum;
}
// one block per proof: out[k] = sum of its nblk partial sums (Montgomery), ok[k] = 0 for a refused pair (u = 0 or v = 0; out[k] = 0)
__global__ __launch_bounds__(S_BLOCK) void k_s_of_uv_finish(const Fr* __restrict__ partial, long nblk, const UvPair* __restrict__ uv, Fr* __restrict__ out,
                                                            uint8_t* __restrict__ ok) {
  __shared__ Fr sh[S_BLOCK];
  const long k = blockIdx.x;
  const bool refused = uv[k].u.is_zero() || uv[k].v.is_zero();
  Fr acc = Fr::zero();
  if (!refused) for (long j = threadIdx.x; j < nblk; j += S_BLOCK) acc = fp_add(acc, partial[k * nblk + j]);
  const Fr sum = block_sum(acc, sh);
  if (threadIdx.x == 0) { out[k] = sum; ok[k] = refused ? 0 : 1; }
}

// ---- the per-proof fold on the device (`each` after a failed fold; fold_each_device below) ----
// Proof k's sums are sum_j scal(s)[k NP + j] * pts[k NP + j] for the S = 2 + (classes of max) scalar arrays s, the very sums fold_sums
// takes from range_msm one proof at a time.  Here every term is a thread: a double-and-add of its scalar (g1_scale, the walk of
// k_g1_scale_each), infinity at once for a zero scalar.  Slot NP of array 1 is the generator's term gv_k * g.  good[i] is the proof of group i.
__global__ __launch_bounds__(256) void k_each_terms(const G1Affine* __restrict__ pts, const Fr* __restrict__ scalars, const Fr* __restrict__ gv, const int32_t* __restrict__ good,
                                                    long groups, int S, long NP, long N, G1Affine gen, G1XYZZ* __restrict__ terms) {
  const long t = (long)blockIdx.x * blockDim.x + threadIdx.x, T = NP + 1;
  if (t >= groups * S * T) return;
  const long i = t / (S * T), j = t % T;
  const int s = (int)((t / T) % S);
  const long k = good[i];
  G1XYZZ r = G1XYZZ::inf();
  if (j < NP) {
    const Fr sc = scalars[(size_t)s * (size_t)N + (size_t)(k * NP + j)];
    if (!sc.is_zero()) r = g1_scale(pts[k * NP + j], sc);
  } else if (s == 1) {
    r = g1_scale(gen, gv[k]);
  }
  terms[t] = r;
}
// one thread per (proof, sum): the terms added, negated where fold_sums negates -- A = sum_0, B = gv g - sum_1, C_c = -sum_{2+c} -- and
// made affine, beside the G2 element it is paired with (h2: h^{alpha x}, h^alpha, h^{x^{m-d}} per class)
__global__ __launch_bounds__(64) void k_each_sums(const G1XYZZ* __restrict__ terms, long groups, int S, long NP, const G2Affine* __restrict__ h2,
                                                  G1Affine* __restrict__ P, G2Affine* __restrict__ Qo) {
  const long t = (long)blockIdx.x * blockDim.x + threadIdx.x, T = NP + 1;
  if (t >= groups * S) return;
  const int s = (int)(t % S);
  const G1XYZZ* mine = terms + t * T;
  G1XYZZ acc = G1XYZZ::inf();
#pragma unroll 1
  for (long j = 0; j < NP; j++) acc = g1_add(acc, mine[j]);
  if (s == 1) acc = g1_add(mine[NP], g1_neg(acc));
  G1Affine a = g1_to_affine(acc);
  if (s >= 2 && !a.is_inf()) a = g1_neg(a);
  P[t] = a;
  Qo[t] = h2[s];
}

}  // namespace
void g1_validate_enqueue(hipStream_t st, const uint8_t* d_in96, G1Affine* out, uint8_t* d_flags, long n) {
  if (n > 0) LAUNCH(k_g1_validate, ceil_div(n, 256), 256, 0, st, d_in96, out, d_flags, n);
}
void g1_subgroup_enqueue(hipStream_t st, const uint8_t* d_in96, uint8_t* d_flags, long n, int method) {
  if (n <= 0) return;
  if (method == SONIC_SUBGROUP_WALK) LAUNCH(k_g1_subgroup<SONIC_SUBGROUP_WALK>, ceil_div(n, 256), 256, 0, st, d_in96, d_flags, n);
  else LAUNCH(k_g1_subgroup<SONIC_SUBGROUP_DEFAULT>, ceil_div(n, 256), 256, 0, st, d_in96, d_flags, n);
}
namespace {

double now_ms() { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count(); }
// host phases of a batch, in the kernel profiler's table (sonic_profile_get) under names no kernel has
void host_phase(const char* name, double ms) {
  if (!profiler().on) return;
  std::lock_guard<std::mutex> g(profiler().mu);
  auto& t = profiler().totals[name];
  t.first += ms; t.second += 1;
}

void le64(Sha256& h, int64_t v) { FsTranscript::le64(h, v); }

}  // namespace

// rho_i for i in [i0, i0 + count): 16 bytes each, little-endian
void batch_randomizers(const uint8_t seed[32], const uint8_t D[32], int64_t i0, int64_t count, uint8_t* out) {
  for (int64_t i = 0; i < count; i++) {
    Sha256 h;
    uint8_t dg[32];
    h.update("sonic-hip/batch/v1", 18); h.update(seed, 32); h.update(D, 32); le64(h, i0 + i);
    h.finish(dg);
    bool zero = true;
    for (int b = 0; b < 16; b++) zero = zero && dg[b] == 0;
    if (zero) dg[0] = 1;
    memcpy(out + 16 * i, dg, 16);
  }
}

}  // namespace sonic

using namespace sonic;

struct sonic_verifier {
  const sonic_srs* srs = nullptr;
  int device = 0;
  long n = 0, Q = 0;
  int64_t d = 0;
  VerifierKey vk;
  std::vector<int64_t> ms;              // the distinct max of a proof's checks: n and d (one entry when n == d)
  std::vector<G2Affine> hm;             // h^{x^{m - d}} for them
  uint8_t digest[32], srs_id[32];
  uint8_t midstate[FS_MIDSTATE_SIZE];   // the circuit digest before the constants (fs.hpp): each statement's digest from it (the `_cs` calls)
  std::vector<uint8_t> cs;
  uint8_t weights_digest[32];           // of the midstate (fs.hpp, "helped verification"): made by the first helped call, not when the handle is
  bool have_weights_digest = false;
  // Which circuit digest the handle's Fiat-Shamir calls derive (sonic_verifier_new_digest): 1 = circuit digest v1 over the dense bytes the
  // weights stand for (midstate + resume, O(Q n) hashing when the handle is made); 2 = circuit digest v2 over the CSR entries (fs.hpp):
  // the GPU hashes the resident CSR into weights digest v2 when the handle is made -- `weights_digest`, have_weights_digest true from the
  // start -- no dense byte is hashed and `midstate` is never filled.  Everything below the digests takes the 32 bytes it is given.
  int digest_kind = 1;
  DevBuf wdtree;                        // the tree of weights digest v2 (weights_digest.hip), all levels
  bool have_wd2 = false;                // kind 1: weights digest v2 is made by the first sonic_verifier_weights_digest_v2, into wd2
  uint8_t wd2[32];
  std::mutex mu;                        // one call at a time per handle
  hipStream_t st = nullptr;
  MsmWorkspace ws;
  CircuitDev cd;
  DevBuf row_ptr, col, val, item_row, item_begin;
  // per call, grown on demand: K (4Q + 7) encodings, points and flags; K pairs, s-values and flags; K nblk partial sums; the scalars
  DevBuf raw, zraw, pts, flags, uv, sv, sok, partial, scalars;      // (zraw: the compressed encodings of the `_z` calls)
  // the per-proof fold on the device (fold_each_device): h^{alpha x}, h^alpha, hm[] uploaded by the first such call; per call the terms,
  // the pairs, the generator's scalars, the proofs of the groups, the groups' ends and verdicts
  DevBuf each_g2, each_terms, each_P, each_Q, each_gv, each_good, each_end, each_one;
  bool have_each_g2 = false;
};

namespace {

struct Sums { G1Affine A, B; std::vector<G1Affine> C; };

// one batch in flight
struct Batch {
  sonic_verifier* v;
  long K, NP, NC;                       // points and checks per proof
  std::vector<char> good;               // well-formed and not refused (u, v != 0)
  std::vector<Fr> gv;                   // per proof: sum rho_i v_i (Montgomery)
  size_t N() const { return (size_t)K * (size_t)NP; }
  const Fr* scal(int which) const { return v->scalars.as<Fr>() + (size_t)which * N(); }     // 0: rho (on W), 1: rho z (on W), 2 + c: rho on the F's of class c
};

// sum_{k0 <= k < k1} of one scalar array over the proofs' points
G1XYZZ range_msm(const Batch& b, int which, long k0, long k1) {
  sonic_verifier* v = b.v;
  const long n = (k1 - k0) * b.NP;
  uint8_t part[192];
  msm_blocking(v->st, v->ws, msm_plan(n), PointArray::packed(v->pts.as<G1Affine>() + k0 * b.NP), b.scal(which) + k0 * b.NP, n, false, nullptr, part);
  G1XYZZ s;
  memcpy(&s, part, sizeof s);
  return s;
}
// the G1 side of the fold over proofs [k0, k1)
Sums fold_sums(const Batch& b, long k0, long k1) {
  Sums s;
  s.A = g1_to_affine(range_msm(b, 0, k0, k1));
  Fr g = Fr::zero();
  for (long k = k0; k < k1; k++) if (b.good[(size_t)k]) g = fp_add(g, b.gv[(size_t)k]);
  s.B = g1_to_affine(g1_add(g1_mul_fr(g1_gen_host(), fp_from_mont(g)), g1_neg(range_msm(b, 1, k0, k1))));
  for (size_t c = 0; c < b.v->ms.size(); c++) s.C.push_back(g1_neg(g1_to_affine(range_msm(b, 2 + (int)c, k0, k1))));
  return s;
}
// the pairing side: 2 + (distinct m) Miller loops, on host threads when `threads`, one product, one final exponentiation
bool fold_accepts(const sonic_verifier* v, const Sums& s, bool threads) {
  using namespace pairing;
  const size_t L = 2 + s.C.size();
  std::vector<F12> f(L);
  auto work = [&](size_t i) { f[i] = i == 0 ? miller_loop(s.A, v->vk.h_alpha_x) : i == 1 ? miller_loop(s.B, v->vk.h_alpha) : miller_loop(s.C[i - 2], v->hm[i - 2]); };
  {
    ThreadGroup th;
    size_t started = 1;
    if (threads) {
      try {
        for (; started < L; started++) th.emplace_back(work, started);
      } catch (const std::system_error&) {}      // thread limit of the host process: the calling thread takes the rest
    } else started = L;
    work(0);
    if (!threads) for (size_t i = 1; i < L; i++) work(i);
    else for (size_t i = started; i < L; i++) work(i);
    th.join();
  }
  F12 prod = f[0];
  for (size_t i = 1; i < L; i++) prod = f12_mul(prod, f[i]);
  return final_exponentiation(prod).is_one();
}

// `each` after a failed fold, on the device: every well-formed proof folded on its own -- k_each_terms, k_each_sums, then one group of
// 2 + (classes) pairs per proof through pairing_groups_device.  The sums are fold_sums' sums (the same group elements, so the same affine
// coordinates) and the pairing is fold_accepts' pairing (one copy of the formulas), so each[k] is what the host form gives.
void fold_each_device(const Batch& b, uint8_t* each) {
  sonic_verifier* v = b.v;
  hipStream_t st = v->st;
  const int S = 2 + (int)v->ms.size();
  const long NP = b.NP, T = NP + 1;
  std::vector<int32_t> good;
  for (long k = 0; k < b.K; k++) if (b.good[(size_t)k]) good.push_back((int32_t)k);
  const long groups = (long)good.size();
  if (groups == 0) return;
  if (!v->have_each_g2) {
    std::vector<G2Affine> h2{v->vk.h_alpha_x, v->vk.h_alpha};
    h2.insert(h2.end(), v->hm.begin(), v->hm.end());
    v->each_g2.ensure(sizeof(G2Affine) * h2.size());
    HIP_OK(hipMemcpyAsync(v->each_g2.p, h2.data(), sizeof(G2Affine) * h2.size(), hipMemcpyHostToDevice, st));
    HIP_OK(hipStreamSynchronize(st));
    v->have_each_g2 = true;
  }
  std::vector<Fr> gv((size_t)b.K);
  for (long k = 0; k < b.K; k++) gv[(size_t)k] = fp_from_mont(b.gv[(size_t)k]);
  // in slices of proofs whose terms fit EACH_TERMS_BYTES: the handle keeps its buffers, and a batch of any size must not pin more than that
  constexpr size_t EACH_TERMS_BYTES = (size_t)64 << 20;
  long slice = std::max<long>(1, (long)(EACH_TERMS_BYTES / (sizeof(G1XYZZ) * (size_t)S * (size_t)T)));
  if (const char* e = getenv("SONIC_EACH_SLICE")) { const long want = atol(e); if (want >= 1 && want < slice) slice = want; }      // (tests: several slices at a small K)
  slice = std::min(slice, groups);
  std::vector<int64_t> ends((size_t)slice);
  for (long i = 0; i < slice; i++) ends[(size_t)i] = (i + 1) * S;
  const size_t cap = (size_t)slice * (size_t)S;
  v->each_terms.ensure(sizeof(G1XYZZ) * cap * (size_t)T);
  v->each_P.ensure(sizeof(G1Affine) * cap); v->each_Q.ensure(sizeof(G2Affine) * cap);
  v->each_gv.ensure(sizeof(Fr) * gv.size()); v->each_good.ensure(sizeof(int32_t) * good.size());
  v->each_end.ensure(sizeof(int64_t) * ends.size()); v->each_one.ensure((size_t)slice);
  HIP_OK(hipMemcpyAsync(v->each_gv.p, gv.data(), sizeof(Fr) * gv.size(), hipMemcpyHostToDevice, st));
  HIP_OK(hipMemcpyAsync(v->each_good.p, good.data(), sizeof(int32_t) * good.size(), hipMemcpyHostToDevice, st));
  HIP_OK(hipMemcpyAsync(v->each_end.p, ends.data(), sizeof(int64_t) * ends.size(), hipMemcpyHostToDevice, st));
  std::vector<uint8_t> one((size_t)slice);
  for (long g0 = 0; g0 < groups; g0 += slice) {
    const long m = std::min(slice, groups - g0), pairs = m * S;          // the first m entries of ends are this slice's
    LAUNCH(k_each_terms, ceil_div(pairs * T, 256), 256, 0, st, (const G1Affine*)v->pts.as<G1Affine>(), (const Fr*)v->scalars.as<Fr>(), (const Fr*)v->each_gv.as<Fr>(),
           (const int32_t*)v->each_good.as<int32_t>() + g0, m, S, NP, (long)b.N(), g1_gen_host(), v->each_terms.as<G1XYZZ>());
    LAUNCH(k_each_sums, ceil_div(pairs, 64), 64, 0, st, (const G1XYZZ*)v->each_terms.as<G1XYZZ>(), m, S, NP, (const G2Affine*)v->each_g2.as<G2Affine>(),
           v->each_P.as<G1Affine>(), v->each_Q.as<G2Affine>());
    pairing_groups_device(st, v->each_P.as<G1Affine>(), v->each_Q.as<G2Affine>(), pairs, v->each_end.as<int64_t>(), m, v->each_one.as<uint8_t>(), nullptr);
    HIP_OK(hipMemcpyAsync(one.data(), v->each_one.p, (size_t)m, hipMemcpyDeviceToHost, st));
    HIP_OK(hipStreamSynchronize(st));
    for (long i = 0; i < m; i++) each[good[(size_t)(g0 + i)]] = one[(size_t)i] ? 1 : 0;
  }
}

// s(u_k, v_k) for K pairs (standard-form pairs on the host, canonical) on the handle's stream: Montgomery values and per-pair flags
void eval_s_device(sonic_verifier* v, long K, const std::vector<Fr>& us, const std::vector<Fr>& vs, std::vector<Fr>& out, std::vector<uint8_t>& ok) {
  // inverses by Montgomery's trick: one inversion for the batch (zeros are left out and keep a zero inverse)
  std::vector<UvPair> h((size_t)K);
  std::vector<Fr> pre((size_t)(2 * K));
  Fr run = Fr::one();
  for (long i = 0; i < 2 * K; i++) {
    const Fr& x = i & 1 ? vs[(size_t)(i >> 1)] : us[(size_t)(i >> 1)];
    pre[(size_t)i] = run;
    if (!x.is_zero()) run = fp_mul(run, x);
  }
  Fr inv = fp_inv(run);
  for (long i = 2 * K - 1; i >= 0; i--) {
    const Fr& x = i & 1 ? vs[(size_t)(i >> 1)] : us[(size_t)(i >> 1)];
    Fr xi = Fr::zero();
    if (!x.is_zero()) { xi = fp_mul(inv, pre[(size_t)i]); inv = fp_mul(inv, x); }
    UvPair& p = h[(size_t)(i >> 1)];
    if (i & 1) { p.v = x; p.vinv = xi; } else { p.u = x; p.uinv = xi; }
  }
  v->uv.ensure(sizeof(UvPair) * (size_t)K);
  v->sv.ensure(sizeof(Fr) * (size_t)K);
  v->sok.ensure((size_t)K);
  v->partial.ensure(sizeof(Fr) * (size_t)K * (size_t)v->cd.nblk);
  hipStream_t st = v->st;
  HIP_OK(hipMemcpyAsync(v->uv.p, h.data(), sizeof(UvPair) * (size_t)K, hipMemcpyHostToDevice, st));
  LAUNCH(k_s_of_uv_batch, (unsigned)(K * v->cd.nblk), S_BLOCK, 0, st, v->cd, (const UvPair*)v->uv.as<UvPair>(), K, v->partial.as<Fr>());
  LAUNCH(k_s_of_uv_finish, (unsigned)K, S_BLOCK, 0, st, (const Fr*)v->partial.as<Fr>(), v->cd.nblk, (const UvPair*)v->uv.as<UvPair>(), v->sv.as<Fr>(), v->sok.as<uint8_t>());
  out.resize((size_t)K); ok.resize((size_t)K);
  HIP_OK(hipMemcpyAsync(out.data(), v->sv.p, sizeof(Fr) * (size_t)K, hipMemcpyDeviceToHost, st));
  HIP_OK(hipMemcpyAsync(ok.data(), v->sok.p, (size_t)K, hipMemcpyDeviceToHost, st));
  HIP_OK(hipStreamSynchronize(st));
}

// points from encodings on the handle's stream: validated points stay in v->pts, the flags come back
void validate_device(sonic_verifier* v, const uint8_t* enc, long M, std::vector<uint8_t>& flags) {
  v->raw.ensure(96 * (size_t)M); v->pts.ensure(sizeof(G1Affine) * (size_t)M); v->flags.ensure((size_t)M);
  hipStream_t st = v->st;
  HIP_OK(hipMemcpyAsync(v->raw.p, enc, 96 * (size_t)M, hipMemcpyHostToDevice, st));
  g1_validate_enqueue(st, v->raw.as<uint8_t>(), v->pts.as<G1Affine>(), v->flags.as<uint8_t>(), M);
  flags.resize((size_t)M);
  HIP_OK(hipMemcpyAsync(flags.data(), v->flags.p, (size_t)M, hipMemcpyDeviceToHost, st));
  HIP_OK(hipStreamSynchronize(st));
}

// K compressed proofs (the `_z` entry points): k_g1_decompress is the validation stage -- the affine points stay in v->pts for the MSMs as
// after validate_device, and the canonical 96-byte encodings come back, from which the host rebuilds the uncompressed proof bytes: those
// are what the batch digest, the Fiat-Shamir challenges and proof_checks read, so a compressed proof is the same proof.  accepted[i] = 1
// as k_g1_validate's flags; a refused point stands in the rebuilt proof as infinity and rejects its proof through accepted.
void decompress_device(sonic_verifier* v, long K, const uint8_t* proofs_z, std::vector<uint8_t>& proofs, std::vector<uint8_t>& accepted) {
  const long Q = v->Q, NP = 4 * Q + 7;
  const size_t psz = sonic_proof_size(Q), zsz = sonic_proof_size_compressed(Q), M = (size_t)K * (size_t)NP;
  std::vector<uint8_t> stage(48 * M), canon(96 * M);
  proofs.resize(psz * (size_t)K);
  uint8_t* s = stage.data();
  for (long k = 0; k < K; k++)
    proof_repack(Q, proofs_z + zsz * (size_t)k, 48, &proofs[psz * (size_t)k], 96, [&](const uint8_t* in, uint8_t*) { memcpy(s, in, 48); s += 48; return true; });
  v->raw.ensure(96 * M); v->zraw.ensure(48 * M); v->pts.ensure(sizeof(G1Affine) * M); v->flags.ensure(M);
  hipStream_t st = v->st;
  HIP_OK(hipMemcpyAsync(v->zraw.p, stage.data(), 48 * M, hipMemcpyHostToDevice, st));
  g1_decompress_enqueue(st, v->zraw.as<uint8_t>(), PointArrayMut{v->pts.as<char>(), (uint32_t)sizeof(G1Affine)}, v->raw.as<uint8_t>(), v->flags.as<uint8_t>(), (long)M, true);
  accepted.resize(M);
  HIP_OK(hipMemcpyAsync(canon.data(), v->raw.p, 96 * M, hipMemcpyDeviceToHost, st));
  HIP_OK(hipMemcpyAsync(accepted.data(), v->flags.p, M, hipMemcpyDeviceToHost, st));
  HIP_OK(hipStreamSynchronize(st));
  for (auto& f : accepted) f = f ? 0 : 1;                       // the kernel's verdict is 0 = accepted
  const uint8_t* c = canon.data();
  for (long k = 0; k < K; k++)
    proof_repack(Q, proofs_z + zsz * (size_t)k, 48, &proofs[psz * (size_t)k], 96, [&](const uint8_t*, uint8_t* out) { memcpy(out, c, 96); c += 96; return true; });
}

// The end of every batch, whatever its proofs are: the scalars of the fold (host) -- rho on W, rho z on W, rho on F by class of max, from
// checks_of(k), the NC checks of the well-formed proof k with points as indices into its NP points, and the randomizers rho_{k NC + i}
// of (seed, D) -- then the fold over every well-formed proof (a malformed one contributes zero scalars) and, where `each` is asked for and
// the fold fails, every proof folded on its own.  t0: when the host began with the digest (the profiler's host_scalars phase).
template <class ChecksOf>
int fold_batch(Batch& b, const uint8_t seed[32], const uint8_t D[32], bool any_bad, double t0, ChecksOf&& checks_of, int* all_accepted, uint8_t* each) {
  sonic_verifier* v = b.v;
  const long K = b.K, NP = b.NP, NC = b.NC;
  const size_t N = b.N();
  const size_t nclass = v->ms.size();
  std::vector<Fr> sc((2 + nclass) * N, Fr::zero());          // Montgomery while they are summed
  std::vector<uint8_t> rho((size_t)(16 * NC));
  long good_count = 0;
  for (long k = 0; k < K; k++) {
    if (!b.good[(size_t)k]) continue;
    good_count++;
    const auto checks = checks_of(k);
    batch_randomizers(seed, D, (int64_t)k * NC, NC, rho.data());
    const size_t base = (size_t)(k * NP);
    for (long i = 0; i < NC; i++) {
      const auto& c = checks[(size_t)i];
      Fr r = Fr::zero();
      memcpy(r.l, &rho[(size_t)(16 * i)], 16);
      r = fp_to_mont(r);
      sc[base + (size_t)c.W] = fp_add(sc[base + (size_t)c.W], r);
      sc[N + base + (size_t)c.W] = fp_add(sc[N + base + (size_t)c.W], fp_mul(r, c.z));
      b.gv[(size_t)k] = fp_add(b.gv[(size_t)k], fp_mul(r, c.val));
      size_t cls = 0;
      while (v->ms[cls] != c.maxm) cls++;
      sc[(2 + cls) * N + base + (size_t)c.F] = fp_add(sc[(2 + cls) * N + base + (size_t)c.F], r);
    }
  }
  for (auto& x : sc) x = fp_from_mont(x);
  v->scalars.ensure(sizeof(Fr) * sc.size());
  HIP_OK(hipMemcpyAsync(v->scalars.p, sc.data(), sizeof(Fr) * sc.size(), hipMemcpyHostToDevice, v->st));
  HIP_OK(hipStreamSynchronize(v->st));
  host_phase("verify_batch:host_scalars", now_ms() - t0);

  // 5. the fold over every well-formed proof (a malformed one contributes zero scalars)
  bool fold_ok = false;
  if (good_count > 0) {
    t0 = now_ms();
    const Sums s = fold_sums(b, 0, K);
    host_phase("verify_batch:msm", now_ms() - t0);
    t0 = now_ms();
    fold_ok = fold_accepts(v, s, true);
    host_phase("verify_batch:host_pairing", now_ms() - t0);
  }
  *all_accepted = (fold_ok && !any_bad) ? 1 : 0;
  if (!each) return SONIC_OK;
  // the fold of the well-formed proofs held: each of them is accepted (the soundness of the fold); else every one is folded on its own
  for (long k = 0; k < K; k++) each[k] = (fold_ok && b.good[(size_t)k]) ? 1 : 0;
  if (fold_ok || good_count == 0) return SONIC_OK;
  t0 = now_ms();
  // the device form from the measured size upward (pairing_device.hpp); SONIC_PAIRING_GPU = 0 / 1: never / always
  const int knob = pairing_gpu_knob();
  if (knob == 1 || (knob < 0 && K >= EACH_GPU_MIN_PROOFS)) {
    fold_each_device(b, each);
    host_phase("verify_batch:each_gpu", now_ms() - t0);
    return SONIC_OK;
  }
  std::vector<Sums> sums((size_t)K);
  for (long k = 0; k < K; k++) if (b.good[(size_t)k]) sums[(size_t)k] = fold_sums(b, k, k + 1);
  const int nt = (int)std::min<long>(K, 16);
  auto work = [&](int w) { for (long k = w; k < K; k += nt) if (b.good[(size_t)k]) each[k] = fold_accepts(v, sums[(size_t)k], false) ? 1 : 0; };
  {
    ThreadGroup th;
    int started = 1;
    try {
      for (; started < nt; started++) th.emplace_back(work, started);
    } catch (const std::system_error&) {}
    work(0);
    for (int w = started; w < nt; w++) work(w);
    th.join();
  }
  host_phase("verify_batch:each", now_ms() - t0);
  return SONIC_OK;
}

// challenges: K blocks of (2 + 2Q) x 32 bytes (y, z, then the pairs).  accepted: null, or the per-point flags of a batch that decompress_device
// has already validated into v->pts.  cs_each: null -- every proof is checked against the handle's constants, batch digest v1 -- or K x Q
// constants, proof k's own: k(y) of proof k is summed over cs_k (Q more field products per proof, on the host beside the K (3Q + 4) of the
// scalars), a non-canonical cs_k makes proof k malformed, and the batch digest is v2, which hashes cs_k behind proof k's challenges.
int verify_batch_core(sonic_verifier* v, long K, const uint8_t* proofs, const uint8_t* challenges, const uint8_t* seed_in, int* all_accepted, uint8_t* each,
                      const std::vector<uint8_t>* accepted = nullptr, const uint8_t* cs_each = nullptr) {
  const long Q = v->Q, NP = 4 * Q + 7, NC = 3 * Q + 4;
  const size_t psz = sonic_proof_size(Q), csz = 32 * (size_t)(2 + 2 * Q);
  const size_t N = (size_t)K * (size_t)NP;
  uint8_t seed[32];
  if (seed_in) memcpy(seed, seed_in, 32);
  else if (getrandom(seed, 32, 0) != 32) { set_error("sonic_verifier_verify_batch: the operating system gave no random bytes for the seed"); return SONIC_ERR_INVALID_ARG; }
  double t0 = now_ms();

  // 1. decode: field elements on the host, point encodings into a staging buffer in proof order (index = position in the proof)
  Batch b{v, K, NP, NC, std::vector<char>((size_t)K, 0), std::vector<Fr>((size_t)K, Fr::zero())};
  std::vector<ProofViewT<int32_t>> views((size_t)K);
  std::vector<Fr> yms((size_t)K), zms((size_t)K);
  std::vector<uint8_t> stage(accepted ? 0 : 96 * N, 0);
  long first_bad = -1;
  for (long k = 0; k < K; k++) {
    int32_t idx = 0;
    uint8_t* dst = accepted ? nullptr : &stage[96 * (size_t)(k * NP)];
    auto take = [&](const uint8_t* enc, int32_t& o) { o = idx++; if (!accepted) memcpy(dst + 96 * (size_t)o, enc, 96); return true; };
    const uint8_t* ch = challenges + csz * (size_t)k;
    b.good[(size_t)k] = parse_proof(proofs + psz * (size_t)k, Q, ch, ch + 32, ch + 64, views[(size_t)k], yms[(size_t)k], zms[(size_t)k], take) ? 1 : 0;
    for (long q = 0; cs_each && q < Q && b.good[(size_t)k]; q++) { Fr c; if (!load_fr(cs_each + 32 * (size_t)(k * Q + q), c)) b.good[(size_t)k] = 0; }
    if (!b.good[(size_t)k] && first_bad < 0) first_bad = k;
  }
  host_phase("verify_batch:host_decode", now_ms() - t0);

  // 2. the points: canonical, on the curve, in the subgroup (device)
  std::vector<uint8_t> flags;
  if (accepted) flags = *accepted;
  else validate_device(v, stage.data(), (long)N, flags);
  for (long k = 0; k < K; k++) {
    bool ok = true;
    for (long j = 0; j < NP; j++) ok = ok && flags[(size_t)(k * NP + j)];
    if (!ok) { b.good[(size_t)k] = 0; if (first_bad < 0 || k < first_bad) first_bad = k; }
  }
  const bool any_malformed = first_bad >= 0;
  if (any_malformed) set_error("verify_batch: proof %ld is malformed (non-canonical field element%s, or point off the curve or outside the order-r subgroup)", first_bad,
                               cs_each ? " in the proof or its constants" : "");

  // 3. s(u_k, v_k) (device); a malformed proof rides along as the pair (1, 1)
  std::vector<Fr> us((size_t)K), vs((size_t)K), svs;
  std::vector<uint8_t> sok;
  for (long k = 0; k < K; k++) {
    us[(size_t)k] = b.good[(size_t)k] ? views[(size_t)k].h.u : Fr::one();
    vs[(size_t)k] = b.good[(size_t)k] ? views[(size_t)k].h.v : Fr::one();
  }
  eval_s_device(v, K, us, vs, svs, sok);
  long first_refused = -1;
  for (long k = 0; k < K; k++) if (b.good[(size_t)k] && !sok[(size_t)k]) { b.good[(size_t)k] = 0; if (first_refused < 0) first_refused = k; }
  if (first_refused >= 0 && !any_malformed) set_error("verify_batch: proof %ld has u or v zero", first_refused);
  const bool any_bad = any_malformed || first_refused >= 0;

  // 4. the randomizers and the scalars of the fold (host): rho on W, rho z on W, rho on F by class of max
  t0 = now_ms();
  uint8_t D[32];
  if (cs_each) fs_batch_digest_v2(v->n, Q, v->d, v->digest, v->srs_id, K, proofs, psz, challenges, cs_each, D);
  else {
    Sha256 h;
    h.update("sonic-hip/batch-digest/v1", 25);
    le64(h, v->n); le64(h, Q); le64(h, v->d);
    h.update(v->digest, 32); h.update(v->srs_id, 32);
    le64(h, K);
    for (long k = 0; k < K; k++) { h.update(proofs + psz * (size_t)k, psz); h.update(challenges + csz * (size_t)k, csz); }
    h.finish(D);
  }
  CircuitView cview{v->n, Q, v->cs.data(), true, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
  return fold_batch(b, seed, D, any_bad, t0, [&](long k) {
    Fr t;
    if (cs_each) cview.cs = cs_each + 32 * (size_t)(k * Q);
    proof_t(cview, views[(size_t)k], yms[(size_t)k], t);      // (cs was checked when the handle was made, cs_k in step 1)
    return proof_checks<int32_t>(v->n, v->d, views[(size_t)k], yms[(size_t)k], zms[(size_t)k], t, svs[(size_t)k]);
  }, all_accepted, each);
}

// the digest of one statement of the handle's circuit, of the handle's kind: v1 resumes the midstate, v2 hashes the constants behind
// weights digest v2 (fs.hpp).  Non-zero: cs is not canonical (dk is left alone)
int statement_digest(const sonic_verifier* v, const uint8_t* cs, uint8_t dk[32]) {
  if (v->digest_kind == 2) return fs_circuit_digest_v2(v->weights_digest, v->Q, cs, dk);
  return fs_circuit_digest_resume(v->midstate, cs, dk);
}

// the Fiat-Shamir form: the challenges each proof determines (fs.hpp), in sonic_verify's order; a proof whose own u, v are not its
// transcript's is rejected
// cs_each (the `_cs` form): proof k's transcript starts from the digest of ITS statement, resume(midstate, cs_k); a cs_k that is not canonical has
// no digest -- the proof rides along under the handle's and verify_batch_core refuses it as malformed
int verify_fs_batch_core(sonic_verifier* v, long K, const uint8_t* proofs, const uint8_t* seed, int* all_accepted, uint8_t* each, const std::vector<uint8_t>* accepted,
                         const uint8_t* cs_each = nullptr) {
  const long Q = v->Q;
  const size_t psz = sonic_proof_size(Q), csz = 32 * (size_t)(2 + 2 * Q);
  std::vector<uint8_t> chal(csz * (size_t)K), ch(32 * (size_t)(4 + 2 * Q)), mine((size_t)K, 1);
  bool all_mine = true;
  for (int64_t k = 0; k < K; k++) {
    const uint8_t* proof = proofs + psz * (size_t)k;
    uint8_t dk[32];
    memcpy(dk, v->digest, 32);
    if (cs_each && statement_digest(v, cs_each + 32 * (size_t)(k * Q), dk) != 0) memcpy(dk, v->digest, 32);
    fs_challenges_of_proof(v->n, Q, v->d, dk, v->srs_id, proof, ch.data());
    if (memcmp(proof + psz - 64, &ch[32 * (size_t)(2 + 2 * Q)], 64) != 0) { mine[(size_t)k] = 0; all_mine = false; }
    uint8_t* o = &chal[csz * (size_t)k];
    memcpy(o, &ch[0], 64);
    for (long j = 0; j < Q; j++) { memcpy(o + 64 + 64 * j, &ch[32 * (size_t)(2 + j)], 32); memcpy(o + 96 + 64 * j, &ch[32 * (size_t)(2 + Q + j)], 32); }
  }
  if (!all_mine && !each) return SONIC_OK;                      // rejected, and nobody asked which
  const int rc = verify_batch_core(v, K, proofs, chal.data(), seed, all_accepted, each, accepted, cs_each);
  if (rc) return rc;
  if (!all_mine) {
    *all_accepted = 0;
    for (int64_t k = 0; k < K; k++) if (!mine[(size_t)k]) each[k] = 0;
  }
  return SONIC_OK;
}

// ---- core proofs (include/sonic_hip.h, "Core proofs"): K x (R, T, a, W_a, b, W_b, W_t, s) ------------------------------------------------
// No signature vouches for a core proof's s: the verifier evaluates s(z_k, y_k) itself -- k_s_of_uv_batch at (u, v) = (z_k, y_k), what the
// full batch spends on s(u_k, v_k) -- and a proof whose s differs is REJECTED, like a malformed one: it rides along with zero scalars and
// the others' verdicts stand.  The 3K checks of the heads (core_checks) fold into the same four Miller loops.
// K compressed core proofs: decompress_device's steps over the 5K points
void decompress_core_device(sonic_verifier* v, long K, const uint8_t* proofs_z, std::vector<uint8_t>& proofs, std::vector<uint8_t>& accepted) {
  const long NP = ProofLayout::core_K;
  const size_t psz = ProofLayout::core_proof_bytes(), zsz = ProofLayout::core_proof_bytes_compressed(), M = (size_t)K * (size_t)NP;
  std::vector<uint8_t> stage(48 * M), canon(96 * M);
  proofs.resize(psz * (size_t)K);
  uint8_t* s = stage.data();
  for (long k = 0; k < K; k++)
    core_proof_repack(proofs_z + zsz * (size_t)k, 48, &proofs[psz * (size_t)k], 96, [&](const uint8_t* in, uint8_t*) { memcpy(s, in, 48); s += 48; return true; });
  v->raw.ensure(96 * M); v->zraw.ensure(48 * M); v->pts.ensure(sizeof(G1Affine) * M); v->flags.ensure(M);
  hipStream_t st = v->st;
  HIP_OK(hipMemcpyAsync(v->zraw.p, stage.data(), 48 * M, hipMemcpyHostToDevice, st));
  g1_decompress_enqueue(st, v->zraw.as<uint8_t>(), PointArrayMut{v->pts.as<char>(), (uint32_t)sizeof(G1Affine)}, v->raw.as<uint8_t>(), v->flags.as<uint8_t>(), (long)M, true);
  accepted.resize(M);
  HIP_OK(hipMemcpyAsync(canon.data(), v->raw.p, 96 * M, hipMemcpyDeviceToHost, st));
  HIP_OK(hipMemcpyAsync(accepted.data(), v->flags.p, M, hipMemcpyDeviceToHost, st));
  HIP_OK(hipStreamSynchronize(st));
  for (auto& f : accepted) f = f ? 0 : 1;                       // the kernel's verdict is 0 = accepted
  const uint8_t* c = canon.data();
  for (long k = 0; k < K; k++)
    core_proof_repack(proofs_z + zsz * (size_t)k, 48, &proofs[psz * (size_t)k], 96, [&](const uint8_t*, uint8_t* out) { memcpy(out, c, 96); c += 96; return true; });
}

// proofs: K x 576 bytes; yz: K x (y_k, z_k); cs_each: K x Q constants or null (the handle's, for every proof); accepted: as verify_batch_core's
int verify_core_proofs_batch(sonic_verifier* v, long K, const uint8_t* proofs, const uint8_t* yz, const uint8_t* cs_each, const uint8_t* seed_in, int* all_accepted,
                             uint8_t* each, const std::vector<uint8_t>* accepted = nullptr) {
  const long Q = v->Q, NP = ProofLayout::core_K, NC = 3;
  const size_t psz = ProofLayout::core_proof_bytes(), N = (size_t)K * (size_t)NP;
  uint8_t seed[32];
  if (seed_in) memcpy(seed, seed_in, 32);
  else if (getrandom(seed, 32, 0) != 32) { set_error("sonic_verifier_verify_core_batch: the operating system gave no random bytes for the seed"); return SONIC_ERR_INVALID_ARG; }
  double t0 = now_ms();

  // 1. decode, as the full batch does
  Batch b{v, K, NP, NC, std::vector<char>((size_t)K, 0), std::vector<Fr>((size_t)K, Fr::zero())};
  std::vector<ProofViewT<int32_t>> views((size_t)K);
  std::vector<Fr> yms((size_t)K), zms((size_t)K);
  std::vector<uint8_t> stage(accepted ? 0 : 96 * N, 0);
  long first_bad = -1;
  for (long k = 0; k < K; k++) {
    int32_t idx = 0;
    uint8_t* dst = accepted ? nullptr : &stage[96 * (size_t)(k * NP)];
    auto take = [&](const uint8_t* enc, int32_t& o) { o = idx++; if (!accepted) memcpy(dst + 96 * (size_t)o, enc, 96); return true; };
    b.good[(size_t)k] = parse_core_proof(proofs + psz * (size_t)k, yz + 64 * (size_t)k, yz + 64 * (size_t)k + 32, views[(size_t)k], yms[(size_t)k], zms[(size_t)k], take) ? 1 : 0;
    for (long q = 0; cs_each && q < Q && b.good[(size_t)k]; q++) { Fr c; if (!load_fr(cs_each + 32 * (size_t)(k * Q + q), c)) b.good[(size_t)k] = 0; }
    if (!b.good[(size_t)k] && first_bad < 0) first_bad = k;
  }
  host_phase("verify_core_batch:host_decode", now_ms() - t0);

  // 2. the 5K points (device)
  std::vector<uint8_t> flags;
  if (accepted) flags = *accepted;
  else validate_device(v, stage.data(), (long)N, flags);
  for (long k = 0; k < K; k++) {
    bool ok = true;
    for (long j = 0; j < NP; j++) ok = ok && flags[(size_t)(k * NP + j)];
    if (!ok) { b.good[(size_t)k] = 0; if (first_bad < 0 || k < first_bad) first_bad = k; }
  }
  const bool any_malformed = first_bad >= 0;
  if (any_malformed) set_error("verify_core_batch: proof %ld is malformed (non-canonical field element in the proof, its challenges or its constants, or point off the curve or "
                               "outside the order-r subgroup)", first_bad);

  // 3. s(z_k, y_k) (device), held against the proof's own s; a malformed proof rides along as the pair (1, 1)
  std::vector<Fr> us((size_t)K), vs((size_t)K), svs;
  std::vector<uint8_t> sok;
  for (long k = 0; k < K; k++) {
    us[(size_t)k] = b.good[(size_t)k] ? zms[(size_t)k] : Fr::one();
    vs[(size_t)k] = b.good[(size_t)k] ? yms[(size_t)k] : Fr::one();
  }
  eval_s_device(v, K, us, vs, svs, sok);
  long first_refused = -1, first_unbound = -1;
  for (long k = 0; k < K; k++) {
    if (!b.good[(size_t)k]) continue;
    if (!sok[(size_t)k]) { b.good[(size_t)k] = 0; if (first_refused < 0) first_refused = k; }
    else if (!(svs[(size_t)k] == views[(size_t)k].s)) { b.good[(size_t)k] = 0; if (first_unbound < 0) first_unbound = k; }
  }
  if (!any_malformed && (first_refused >= 0 || first_unbound >= 0)) {
    if (first_unbound < 0 || (first_refused >= 0 && first_refused < first_unbound)) set_error("verify_core_batch: proof %ld has y or z zero", first_refused);
    else set_error("verify_core_batch: the s of proof %ld is not s(z, y) of the circuit", first_unbound);
  }
  const bool any_bad = any_malformed || first_refused >= 0 || first_unbound >= 0;

  // 4. the digest that the randomizers bind, then the fold over the checks of the heads
  t0 = now_ms();
  uint8_t D[32];
  std::vector<uint8_t> cs_all;
  if (!cs_each) { cs_all.resize(32 * (size_t)(K * Q)); for (long k = 0; k < K; k++) memcpy(&cs_all[32 * (size_t)(k * Q)], v->cs.data(), 32 * (size_t)Q); }
  fs_core_batch_digest(v->n, Q, v->d, v->digest, v->srs_id, K, proofs, yz, cs_each ? cs_each : cs_all.data(), D);
  CircuitView cview{v->n, Q, v->cs.data(), true, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
  return fold_batch(b, seed, D, any_bad, t0, [&](long k) {
    Fr t;
    if (cs_each) cview.cs = cs_each + 32 * (size_t)(k * Q);
    proof_t(cview, views[(size_t)k], yms[(size_t)k], t);
    return core_checks<int32_t>(v->n, v->d, views[(size_t)k], yms[(size_t)k], zms[(size_t)k], t);
  }, all_accepted, each);
}

// the Fiat-Shamir form: y_k, z_k from each proof's own transcript (fs.hpp, "core proofs"), proof k's from the digest of ITS statement
void core_fs_challenges_batch(sonic_verifier* v, long K, const uint8_t* proofs, const uint8_t* cs_each, std::vector<uint8_t>& yz) {
  const long Q = v->Q;
  yz.resize(64 * (size_t)K);
  for (int64_t k = 0; k < K; k++) {
    uint8_t dk[32];
    memcpy(dk, v->digest, 32);
    // (a cs_k that is not canonical has no digest: the proof rides along under the handle's and is refused as malformed)
    if (cs_each && statement_digest(v, cs_each + 32 * (size_t)(k * Q), dk) != 0) memcpy(dk, v->digest, 32);
    fs_core_challenges_of_proof(v->n, Q, v->d, dk, v->srs_id, proofs + ProofLayout::core_proof_bytes() * (size_t)k, &yz[64 * (size_t)k]);
  }
}
int verify_core_proofs_fs_batch(sonic_verifier* v, long K, const uint8_t* proofs, const uint8_t* cs_each, const uint8_t* seed, int* all_accepted, uint8_t* each,
                                const std::vector<uint8_t>* accepted) {
  std::vector<uint8_t> yz;
  core_fs_challenges_batch(v, K, proofs, cs_each, yz);
  return verify_core_proofs_batch(v, K, proofs, yz.data(), cs_each, seed, all_accepted, each, accepted);
}

// ---- helped verification (include/sonic_hip.h, "Helped verification"): K core proofs and ONE aggregate signature over their (y_k, z_k) --------
// The aggregate vouches for s_k = s(z_k, y_k), so the verifier holds proof k's s against s_k as bytes and evaluates s(u, v) ONCE, at the
// aggregate's own point, instead of K times.  The 3K checks of the heads (core_checks) and the 3K + 1 of the signature (hsc_checks) fold
// into the same four Miller loops.  Points: proof k's five at 5k .., the aggregate's S_k, W_k, W'_k, Q_k at 5K + 4k .., then Q_v and C at
// 9K and 9K + 1 -- the proofs first, because that is where decompress_core_device leaves the points of compressed ones.  Q_v and C belong to
// no proof: their scalars are kept on the host, so that the global check (C at v against s(u, v)) and any proof's six checks can be folded
// on their own when the whole fold fails.
struct Helped {
  sonic_verifier* v;
  long K;
  std::vector<char> good;               // proof k: well-formed, y_k, z_k != 0, and its s is the aggregate's s_k
  std::vector<Fr> gv, rho_c;            // per proof: sum rho val over its six checks; the rho of its check on C (Montgomery)
  Fr g_glob, rho_glob, rho_z_glob;      // the global check: rho s(u, v), rho, rho v
  G1Affine Qv, C;
  size_t N() const { return 9 * (size_t)K + 2; }
  const Fr* scal(int which) const { return v->scalars.as<Fr>() + (size_t)which * N(); }
};

G1XYZZ span_msm(const Helped& b, int which, size_t at, long count) {
  sonic_verifier* v = b.v;
  uint8_t part[192];
  msm_blocking(v->st, v->ws, msm_plan(count), PointArray::packed(v->pts.as<G1Affine>() + at), b.scal(which) + at, count, false, nullptr, part);
  G1XYZZ s;
  memcpy(&s, part, sizeof s);
  return s;
}
// the G1 side of the fold over the six checks of each proof in [k0, k1) and, with `glob`, the global check
Sums helped_sums(const Helped& b, long k0, long k1, bool glob) {
  const long K = b.K;
  auto part = [&](int which) {
    if (k1 <= k0) return G1XYZZ::inf();
    if (k0 == 0 && k1 == K) return span_msm(b, which, 0, 9 * K);
    return g1_add(span_msm(b, which, (size_t)(5 * k0), 5 * (k1 - k0)), span_msm(b, which, (size_t)(5 * K + 4 * k0), 4 * (k1 - k0)));
  };
  Fr g = glob ? b.g_glob : Fr::zero(), rc = glob ? b.rho_glob : Fr::zero();
  for (long k = k0; k < k1; k++) if (b.good[(size_t)k]) { g = fp_add(g, b.gv[(size_t)k]); rc = fp_add(rc, b.rho_c[(size_t)k]); }
  Sums s;
  G1XYZZ A = part(0), B = g1_add(g1_mul_fr(g1_gen_host(), fp_from_mont(g)), g1_neg(part(1)));
  if (glob) { A = g1_add(A, g1_mul_fr(b.Qv, fp_from_mont(b.rho_glob))); B = g1_add(B, g1_neg(g1_mul_fr(b.Qv, fp_from_mont(b.rho_z_glob)))); }
  s.A = g1_to_affine(A); s.B = g1_to_affine(B);
  for (size_t c = 0; c < b.v->ms.size(); c++) {
    G1XYZZ F = part(2 + (int)c);
    if (b.v->ms[c] == b.v->d) F = g1_add(F, g1_mul_fr(b.C, fp_from_mont(rc)));      // every check on C has max = d
    s.C.push_back(g1_neg(g1_to_affine(F)));
  }
  return s;
}

// encodings validated into v->pts[at ..]; the buffers hold 9K + 2 points already (ensured by the caller, so that nothing moves)
void validate_span(sonic_verifier* v, const uint8_t* enc, size_t at, size_t M, uint8_t* flags_out) {
  hipStream_t st = v->st;
  HIP_OK(hipMemcpyAsync(v->raw.as<uint8_t>() + 96 * at, enc, 96 * M, hipMemcpyHostToDevice, st));
  g1_validate_enqueue(st, v->raw.as<uint8_t>() + 96 * at, v->pts.as<G1Affine>() + at, v->flags.as<uint8_t>() + at, (long)M);
  HIP_OK(hipMemcpyAsync(flags_out, v->flags.as<uint8_t>() + at, M, hipMemcpyDeviceToHost, st));
  HIP_OK(hipStreamSynchronize(st));
}
void helped_reserve(sonic_verifier* v, long K) {
  const size_t N = 9 * (size_t)K + 2;
  v->raw.ensure(96 * N); v->zraw.ensure(48 * 5 * (size_t)K); v->pts.ensure(sizeof(G1Affine) * N); v->flags.ensure(N);
}

// proofs: K x 576 bytes; yz: K x (y_k, z_k); cs_each: K x Q constants or null; aggregate: sonic_hsc_proof_size(K) bytes; accepted: null, or
// the flags of the proofs' 5K points, which decompress_core_device has validated into v->pts (helped_reserve called before it)
int verify_core_helped(sonic_verifier* v, long K, const uint8_t* proofs, const uint8_t* yz, const uint8_t* cs_each, const uint8_t* aggregate, const uint8_t* seed_in,
                       int* all_accepted, uint8_t* each, const std::vector<uint8_t>* accepted = nullptr) {
  const long Q = v->Q;
  const size_t psz = ProofLayout::core_proof_bytes();
  const AggLayout A{K};
  uint8_t seed[32];
  if (seed_in) memcpy(seed, seed_in, 32);
  else if (getrandom(seed, 32, 0) != 32) { set_error("sonic_verifier_verify_core_batch_helped: the operating system gave no random bytes for the seed"); return SONIC_ERR_INVALID_ARG; }
  if (!v->have_weights_digest) { fs_weights_digest(v->midstate, v->weights_digest); v->have_weights_digest = true; }
  double t0 = now_ms();
  auto reject_all = [&] { *all_accepted = 0; for (long k = 0; each && k < K; k++) each[k] = 0; return SONIC_OK; };

  // 1. decode: the proofs as the unhelped batch does, the aggregate into indices of the same staging buffer
  Helped b{v, K, std::vector<char>((size_t)K, 0), std::vector<Fr>((size_t)K, Fr::zero()), std::vector<Fr>((size_t)K, Fr::zero()), Fr::zero(), Fr::zero(), Fr::zero(), G1Affine::inf(), G1Affine::inf()};
  const size_t N = b.N();
  std::vector<ProofViewT<int32_t>> views((size_t)K);
  std::vector<Fr> yms((size_t)K), zms((size_t)K);
  std::vector<uint8_t> stage(96 * N, 0);
  long first_bad = -1, first_zero = -1, first_unbound = -1;
  for (long k = 0; k < K; k++) {
    int32_t idx = 0;
    uint8_t* dst = &stage[96 * (size_t)(5 * k)];
    auto take = [&](const uint8_t* enc, int32_t& o) { o = (int32_t)(5 * k) + idx++; memcpy(dst + 96 * (size_t)(o - 5 * k), enc, 96); return true; };
    b.good[(size_t)k] = parse_core_proof(proofs + psz * (size_t)k, yz + 64 * (size_t)k, yz + 64 * (size_t)k + 32, views[(size_t)k], yms[(size_t)k], zms[(size_t)k], take) ? 1 : 0;
    for (long q = 0; cs_each && q < Q && b.good[(size_t)k]; q++) { Fr c; if (!load_fr(cs_each + 32 * (size_t)(k * Q + q), c)) b.good[(size_t)k] = 0; }
    if (!b.good[(size_t)k] && first_bad < 0) first_bad = k;
  }
  HscProofViewT<int32_t> h;
  // the pairs as the aggregate's view holds them: a pair that is no pair of field elements stands as (1, 1) -- its proof is malformed, and
  // the checks of j = k are left out with it
  std::vector<uint8_t> yz_ok(yz, yz + 64 * (size_t)K);
  for (long k = 0; k < K; k++) {
    Fr t;
    if (!load_fr(yz + 64 * (size_t)k, t) || !load_fr(yz + 64 * (size_t)k + 32, t)) { memset(&yz_ok[64 * (size_t)k], 0, 64); yz_ok[64 * (size_t)k] = yz_ok[64 * (size_t)k + 32] = 1; }
  }
  long seen = 0;
  auto take_agg = [&](const uint8_t* enc, int32_t& o) {
    // parse_hsc visits S_j, W_j (j = 0 ..), then W'_j, Q_j, then Q_v, C
    const long c = seen++;
    const long at = c < 2 * K ? 4 * (c / 2) + c % 2 : (c < 4 * K ? 4 * ((c - 2 * K) / 2) + 2 + c % 2 : c);
    o = (int32_t)(5 * K + at);
    memcpy(&stage[96 * (size_t)o], enc, 96);
    return true;
  };
  bool agg_ok = parse_hsc(aggregate, K, yz_ok.data(), h, take_agg);
  host_phase("verify_core_helped:host_decode", now_ms() - t0);

  // 2. the points: the proofs' 5K (unless they came compressed and are validated already) and the aggregate's 4K + 2
  std::vector<uint8_t> flags(N, 0);
  if (accepted) { memcpy(flags.data(), accepted->data(), 5 * (size_t)K); validate_span(v, &stage[96 * 5 * (size_t)K], 5 * (size_t)K, 4 * (size_t)K + 2, &flags[5 * (size_t)K]); }
  else validate_span(v, stage.data(), 0, N, flags.data());
  for (long k = 0; k < K; k++) {
    bool ok = true;
    for (long j = 0; j < 5; j++) ok = ok && flags[(size_t)(5 * k + j)];
    if (!ok) { b.good[(size_t)k] = 0; if (first_bad < 0 || k < first_bad) first_bad = k; }
  }
  for (size_t i = 5 * (size_t)K; i < N; i++) agg_ok = agg_ok && flags[i];
  if (!agg_ok) {
    set_error("verify_core_batch_helped: the aggregate is malformed (non-canonical field element, or point off the curve or outside the order-r subgroup): every proof is rejected");
    return reject_all();
  }
  // 3. u, v are the transcript's, and not zero
  uint8_t uv[64];
  fs_aggregate_challenges(v->n, Q, v->d, v->weights_digest, v->srs_id, K, yz, aggregate, uv);
  if (memcmp(uv, aggregate + A.u(), 64) != 0 || h.u.is_zero() || h.v.is_zero()) {
    set_error("verify_core_batch_helped: the aggregate's u, v are not the ones its transcript determines for these pairs: every proof is rejected");
    return reject_all();
  }
  // 4. proof k's s is the aggregate's s_k, as bytes; y_k, z_k are invertible
  for (long k = 0; k < K; k++) {
    if (!b.good[(size_t)k]) continue;
    if (yms[(size_t)k].is_zero() || zms[(size_t)k].is_zero()) { b.good[(size_t)k] = 0; if (first_zero < 0) first_zero = k; }
    else if (memcmp(proofs + psz * (size_t)k + 544, aggregate + A.hscS() + 224 * (size_t)k + 96, 32) != 0) { b.good[(size_t)k] = 0; if (first_unbound < 0) first_unbound = k; }
  }
  if (first_bad >= 0) set_error("verify_core_batch_helped: proof %ld is malformed (non-canonical field element in the proof, its challenges or its constants, or point off the curve or "
                                "outside the order-r subgroup)", first_bad);
  else if (first_zero >= 0 && (first_unbound < 0 || first_zero < first_unbound)) set_error("verify_core_batch_helped: proof %ld has y or z zero", first_zero);
  else if (first_unbound >= 0) set_error("verify_core_batch_helped: the s of proof %ld is not the aggregate's s_k", first_unbound);
  const bool any_bad = first_bad >= 0 || first_zero >= 0 || first_unbound >= 0;
  {
    G1Affine g[2];
    HIP_OK(hipMemcpy(g, v->pts.as<G1Affine>() + 9 * (size_t)K, sizeof g, hipMemcpyDeviceToHost));
    b.Qv = g[0]; b.C = g[1];
  }
  // 5. s(u, v), once
  std::vector<Fr> svs;
  std::vector<uint8_t> sok;
  eval_s_device(v, 1, std::vector<Fr>{h.u}, std::vector<Fr>{h.v}, svs, sok);
  if (!sok[0]) { set_error("verify_core_batch_helped: the aggregate's u or v is zero: every proof is rejected"); return reject_all(); }

  // 6. the digest the randomizers bind, and the scalars of the fold: rho on W, rho z on W, rho on F by class of max
  t0 = now_ms();
  uint8_t D[32];
  std::vector<uint8_t> cs_all;
  if (!cs_each) { cs_all.resize(32 * (size_t)(K * Q)); for (long k = 0; k < K; k++) memcpy(&cs_all[32 * (size_t)(k * Q)], v->cs.data(), 32 * (size_t)Q); }
  fs_core_helped_digest(v->n, Q, v->d, v->weights_digest, v->srs_id, K, proofs, yz, cs_each ? cs_each : cs_all.data(), aggregate, D);
  const size_t nclass = v->ms.size();
  std::vector<Fr> sc((2 + nclass) * N, Fr::zero());          // Montgomery while they are summed
  std::vector<PcvCheckT<int32_t>> sig;
  hsc_checks<int32_t>(v->d, h, svs[0], sig);                   // 3K + 1, in the order the randomizers number them from 3K on
  const size_t local = 9 * (size_t)K;
  // check c of proof k (k < 0: the global check) under randomizer number `index`
  auto add = [&](long k, const PcvCheckT<int32_t>& c, int64_t index) {
    uint8_t rho[16];
    batch_randomizers(seed, D, index, 1, rho);
    Fr r = Fr::zero();
    memcpy(r.l, rho, 16);
    r = fp_to_mont(r);
    const Fr rz = fp_mul(r, c.z), rv = fp_mul(r, c.val);
    if ((size_t)c.W < local) { sc[(size_t)c.W] = fp_add(sc[(size_t)c.W], r); sc[N + (size_t)c.W] = fp_add(sc[N + (size_t)c.W], rz); }
    else { b.rho_glob = r; b.rho_z_glob = rz; }               // (W = Q_v: the global check only)
    if (k >= 0) b.gv[(size_t)k] = fp_add(b.gv[(size_t)k], rv); else b.g_glob = rv;
    if ((size_t)c.F < local) {
      size_t cls = 0;
      while (v->ms[cls] != c.maxm) cls++;
      sc[(2 + cls) * N + (size_t)c.F] = fp_add(sc[(2 + cls) * N + (size_t)c.F], r);
    } else if (k >= 0) b.rho_c[(size_t)k] = fp_add(b.rho_c[(size_t)k], r);      // (F = C; the global check's own rho on C is rho_glob)
  };
  CircuitView cview{v->n, Q, v->cs.data(), true, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
  for (long k = 0; k < K; k++) {
    if (!b.good[(size_t)k]) continue;
    Fr t;
    if (cs_each) cview.cs = cs_each + 32 * (size_t)(k * Q);
    proof_t(cview, views[(size_t)k], yms[(size_t)k], t);
    const auto head = core_checks<int32_t>(v->n, v->d, views[(size_t)k], yms[(size_t)k], zms[(size_t)k], t);
    for (long i = 0; i < 3; i++) add(k, head[(size_t)i], 3 * k + i);
    for (long i = 0; i < 3; i++) add(k, sig[(size_t)(3 * k + i)], 3 * K + 3 * k + i);
  }
  add(-1, sig[3 * (size_t)K], 6 * K);
  for (auto& x : sc) x = fp_from_mont(x);
  v->scalars.ensure(sizeof(Fr) * sc.size());
  HIP_OK(hipMemcpyAsync(v->scalars.p, sc.data(), sizeof(Fr) * sc.size(), hipMemcpyHostToDevice, v->st));
  HIP_OK(hipStreamSynchronize(v->st));
  host_phase("verify_core_helped:host_scalars", now_ms() - t0);

  // 7. the fold: every well-formed proof's six checks and the global check in one pairing product
  t0 = now_ms();
  const Sums all = helped_sums(b, 0, K, true);
  host_phase("verify_core_helped:msm", now_ms() - t0);
  t0 = now_ms();
  const bool fold_ok = fold_accepts(v, all, true);
  host_phase("verify_core_helped:host_pairing", now_ms() - t0);
  *all_accepted = (fold_ok && !any_bad) ? 1 : 0;
  if (fold_ok) { for (long k = 0; each && k < K; k++) each[k] = b.good[(size_t)k] ? 1 : 0; return SONIC_OK; }
  // it failed: the global check on its own says whether the aggregate is to blame -- then every proof is rejected -- and if it is not, each
  // well-formed proof's six checks are folded on their own, and the others' verdicts stand
  t0 = now_ms();
  if (!fold_accepts(v, helped_sums(b, 0, 0, true), true)) {
    set_error("verify_core_batch_helped: the aggregate's C does not open to s(u, v) at v: every proof is rejected");
    return reject_all();
  }
  if (!any_bad) set_error("verify_core_batch_helped: an equation of a proof or of its part of the aggregate does not hold");
  if (!each) return SONIC_OK;
  std::vector<Sums> sums((size_t)K);
  for (long k = 0; k < K; k++) { each[k] = 0; if (b.good[(size_t)k]) sums[(size_t)k] = helped_sums(b, k, k + 1, false); }
  const int nt = (int)std::min<long>(K, 16);
  auto work = [&](int w) { for (long k = w; k < K; k += nt) if (b.good[(size_t)k]) each[k] = fold_accepts(v, sums[(size_t)k], false) ? 1 : 0; };
  {
    ThreadGroup th;
    int started = 1;
    try {
      for (; started < nt; started++) th.emplace_back(work, started);
    } catch (const std::system_error&) {}
    work(0);
    for (int w = started; w < nt; w++) work(w);
    th.join();
  }
  host_phase("verify_core_helped:each", now_ms() - t0);
  return SONIC_OK;
}

// weights digest v2 of the handle's resident CSR, on the GPU (weights_digest.hip): the tree, 32 bytes back, the 76-byte hash over the root
void verifier_weights_digest_v2(sonic_verifier* v, uint8_t out[32]) {
  const uint32_t* root_d = weights_tree_enqueue(v->st, v->row_ptr.as<int32_t>(), v->col.as<int32_t>(), v->val.as<Fr>(), 3 * v->Q, v->cd.nnz, v->wdtree);
  uint32_t words[8];
  HIP_OK(hipMemcpyAsync(words, root_d, 32, hipMemcpyDeviceToHost, v->st));
  HIP_OK(hipStreamSynchronize(v->st));
  uint8_t root[32];
  wt_digest_bytes(words, root);
  fs_weights_digest_v2(v->n, v->Q, v->cd.nnz, root, out);
}

int verifier_new(const char* who, const sonic_srs_t* srs, const CircuitView& c, sonic_verifier_t** out, int digest_kind = 1) {
  if (!srs || !c.cs || !out) { set_error("%s: bad argument", who); return SONIC_ERR_INVALID_ARG; }
  *out = nullptr;
  if (digest_kind != 1 && digest_kind != 2) { set_error("%s: digest_kind = %d, must be 1 (circuit digest v1) or 2 (circuit digest v2)", who, digest_kind); return SONIC_ERR_INVALID_ARG; }
  int rc = circuit_validate(who, c);
  if (rc) return rc;
  const long n = c.n, Q = c.Q, R = 3 * Q;
  std::unique_ptr<sonic_verifier> v(new sonic_verifier());
  v->srs = srs; v->device = srs_device(srs); v->n = n; v->Q = Q; v->d = srs->d;
  for (long q = 0; q < Q; q++) { Fr k; if (!load_fr(c.cs + 32 * q, k)) { set_error("%s: cs[%ld] is not a canonical field element", who, q); return SONIC_ERR_BAD_ENCODING; } }
  v->cs.assign(c.cs, c.cs + 32 * Q);
  // the G2 elements of every fold, once: the same statuses as sonic_verify when one is at infinity or the SRS is too short
  rc = load_verifier_key(srs, v->vk);
  if (rc) return rc;
  v->ms.push_back(n);
  if (v->d != n) v->ms.push_back(v->d);
  v->hm.resize(v->ms.size());
  for (size_t i = 0; i < v->ms.size(); i++) { rc = pc_v_element(srs, v->ms[i], v->hm[i]); if (rc) return rc; }
  v->digest_kind = digest_kind;
  if (digest_kind == 1) {
    circuit_midstate(c, v->midstate);
    fs_circuit_digest_resume(v->midstate, c.cs, v->digest);
  }
  rc = sonic_fs_srs_id(srs, v->srs_id);
  if (rc) return rc;
  // the circuit as CSR, whichever form it came in (dense: the non-zero entries), values Montgomery
  std::vector<int32_t> row_ptr((size_t)R + 1, 0), col, item_row, item_begin;
  std::vector<Fr> val;
  if (c.csr) {
    const long nnz = (long)c.row_ptr[R];
    col.resize((size_t)nnz); val.resize((size_t)nnz);
    for (long r = 0; r <= R; r++) row_ptr[(size_t)r] = (int32_t)c.row_ptr[r];
    for (long k = 0; k < nnz; k++) { col[(size_t)k] = (int32_t)c.col[k]; load_fr(c.val + 32 * k, val[(size_t)k]); }
  } else {
    if (n > INT32_MAX - 1 || (double)Q * (double)n * 3 > (double)INT32_MAX) { set_error("%s: the circuit does not fit 32-bit entry indices", who); return SONIC_ERR_INVALID_ARG; }
    static const uint8_t zero[32] = {0};
    const uint8_t* mats[3] = {c.wL, c.wR, c.wO};
    for (long r = 0; r < R; r++) {
      const uint8_t* row = mats[r / Q] + 32 * ((r % Q) * n);
      for (long i = 0; i < n; i++) {
        if (memcmp(row + 32 * i, zero, 32) == 0) continue;
        Fr w;
        if (!load_fr(row + 32 * i, w)) { set_error("%s: non-canonical gate weight (row %ld, gate %ld)", who, r, i); return SONIC_ERR_BAD_ENCODING; }
        col.push_back((int32_t)i); val.push_back(w);
      }
      row_ptr[(size_t)r + 1] = (int32_t)col.size();
    }
  }
  for (long r = 0; r < R; r++)
    for (long k = row_ptr[(size_t)r]; k < row_ptr[(size_t)r + 1]; k += S_ITEM) { item_row.push_back((int32_t)r); item_begin.push_back((int32_t)k); }
  CircuitDev& cd = v->cd;
  cd.n = n; cd.Q = Q; cd.nnz = (long)col.size();
  cd.row_items = (long)item_row.size();
  cd.items = cd.row_items + (n + S_ITEM - 1) / S_ITEM;
  cd.nblk = (cd.items + S_BLOCK - 1) / S_BLOCK;
  HIP_OK(hipStreamCreateWithFlags(&v->st, hipStreamNonBlocking));
  auto up = [&](DevBuf& b, const void* src, size_t bytes) { b.alloc(bytes); if (bytes) HIP_OK(hipMemcpyAsync(b.p, src, bytes, hipMemcpyHostToDevice, v->st)); };
  try {
    up(v->row_ptr, row_ptr.data(), 4 * row_ptr.size()); up(v->col, col.data(), 4 * col.size()); up(v->val, val.data(), sizeof(Fr) * val.size());
    up(v->item_row, item_row.data(), 4 * item_row.size()); up(v->item_begin, item_begin.data(), 4 * item_begin.size());
    HIP_OK(hipStreamSynchronize(v->st));
  } catch (...) { (void)hipStreamDestroy(v->st); throw; }
  cd.row_ptr = v->row_ptr.as<int32_t>(); cd.col = v->col.as<int32_t>(); cd.val = v->val.as<Fr>();
  cd.item_row = v->item_row.as<int32_t>(); cd.item_begin = v->item_begin.as<int32_t>();
  if (digest_kind == 2) {
    // (the constants were checked above: the digest of the handle's own statement cannot fail)
    try {
      verifier_weights_digest_v2(v.get(), v->weights_digest);
    } catch (...) { (void)hipStreamDestroy(v->st); throw; }
    v->have_weights_digest = true;
    memcpy(v->wd2, v->weights_digest, 32); v->have_wd2 = true;
    fs_circuit_digest_v2(v->weights_digest, Q, c.cs, v->digest);
  }
  *out = v.release();
  return SONIC_OK;
}

// K and the size of its MSMs
int batch_size_ok(const char* who, const sonic_verifier* v, int64_t K) {
  if (K < 1 || K > MSM_TABLE_MAX_TERMS / (4 * v->Q + 7)) { set_error("%s: K = %lld outside [1, 2^26 / (4Q + 7)]", who, (long long)K); return SONIC_ERR_INVALID_ARG; }
  if ((double)K * (double)v->cd.nblk >= 2147483647.0) { set_error("%s: K = %lld times the circuit's %ld blocks exceeds one launch", who, (long long)K, v->cd.nblk); return SONIC_ERR_INVALID_ARG; }
  return SONIC_OK;
}

// the arguments of sonic_g1_subgroup_check / sonic_g2_subgroup_check; the bound is the one of the batched verifier's validation stage
int subgroup_args_ok(const char* who, const uint8_t* points, int64_t n, int method, const uint8_t* flags) {
  if (n >= 0 && n <= MSM_TABLE_MAX_TERMS && (n == 0 || (points && flags)) && (method == SONIC_SUBGROUP_DEFAULT || method == SONIC_SUBGROUP_WALK)) return SONIC_OK;
  set_error("%s: bad argument (n = %lld of at most 2^26, method = %d)", who, (long long)n, method);
  return SONIC_ERR_INVALID_ARG;
}

}  // namespace

extern "C" {

int sonic_verifier_new(const sonic_srs_t* srs, int64_t n, int64_t Q, const uint8_t* wL, const uint8_t* wR, const uint8_t* wO, const uint8_t* cs,
                       sonic_verifier_t** out) {
  API_BEGIN_ON(srs_device(srs))
  return verifier_new("sonic_verifier_new", srs, dense_view(n, Q, wL, wR, wO, cs), out);
  API_CATCH
}
int sonic_verifier_new_csr(const sonic_srs_t* srs, int64_t n, int64_t Q, const int64_t* row_ptr, const int64_t* col, const uint8_t* val, const uint8_t* cs,
                           sonic_verifier_t** out) {
  API_BEGIN_ON(srs_device(srs))
  return verifier_new("sonic_verifier_new_csr", srs, csr_view(n, Q, row_ptr, col, val, cs), out);
  API_CATCH
}
int sonic_verifier_new_digest(const sonic_srs_t* srs, int64_t n, int64_t Q, const int64_t* row_ptr, const int64_t* col, const uint8_t* val, const uint8_t* cs,
                              int digest_kind, sonic_verifier_t** out) {
  API_BEGIN_ON(srs_device(srs))
  return verifier_new(digest_kind == 1 ? "sonic_verifier_new_csr" : "sonic_verifier_new_digest", srs, csr_view(n, Q, row_ptr, col, val, cs), out, digest_kind);
  API_CATCH
}
int sonic_verifier_digest_kind(const sonic_verifier_t* v) { return v ? v->digest_kind : -1; }
int sonic_verifier_weights_digest_v2(sonic_verifier_t* v, uint8_t out[32]) {
  API_BEGIN_ON(v ? v->device : -1)
  if (!v || !out) { set_error("sonic_verifier_weights_digest_v2: bad argument"); return SONIC_ERR_INVALID_ARG; }
  std::lock_guard<std::mutex> g(v->mu);
  if (!v->have_wd2) { verifier_weights_digest_v2(v, v->wd2); v->have_wd2 = true; }
  memcpy(out, v->wd2, 32);
  API_END
}
void sonic_verifier_free(sonic_verifier_t* v) {
  if (!v) return;
  try {
    DeviceScope scope(v->device);
    (void)hipStreamSynchronize(v->st);
    (void)hipStreamDestroy(v->st);
    delete v;                            // (the device buffers go inside the scope)
  } catch (...) {}
}
int sonic_verifier_device(const sonic_verifier_t* v) { return v ? v->device : -1; }

int sonic_verifier_verify_batch(sonic_verifier_t* v, int64_t K, const uint8_t* proofs, const uint8_t* challenges, const uint8_t seed[32], int* all_accepted,
                                uint8_t* each) {
  if (!v || !proofs || !challenges || !all_accepted) { set_error("sonic_verifier_verify_batch: bad argument"); return SONIC_ERR_INVALID_ARG; }
  *all_accepted = 0;
  API_BEGIN_ON(v->device)
  int rc = batch_size_ok("sonic_verifier_verify_batch", v, K);
  if (rc) return rc;
  std::lock_guard<std::mutex> g(v->mu);
  return verify_batch_core(v, (long)K, proofs, challenges, seed, all_accepted, each);
  API_CATCH
}

int sonic_verifier_verify_fs_batch(sonic_verifier_t* v, int64_t K, const uint8_t* proofs, const uint8_t seed[32], int* all_accepted, uint8_t* each) {
  if (!v || !proofs || !all_accepted) { set_error("sonic_verifier_verify_fs_batch: bad argument"); return SONIC_ERR_INVALID_ARG; }
  *all_accepted = 0;
  API_BEGIN_ON(v->device)
  int rc = batch_size_ok("sonic_verifier_verify_fs_batch", v, K);
  if (rc) return rc;
  std::lock_guard<std::mutex> g(v->mu);
  return verify_fs_batch_core(v, (long)K, proofs, seed, all_accepted, each, nullptr);
  API_CATCH
}

// the compressed forms: decompress on the device, then the very same verifier over the rebuilt proof bytes
int sonic_verifier_verify_batch_z(sonic_verifier_t* v, int64_t K, const uint8_t* proofs_z, const uint8_t* challenges, const uint8_t seed[32], int* all_accepted,
                                  uint8_t* each) {
  if (!v || !proofs_z || !challenges || !all_accepted) { set_error("sonic_verifier_verify_batch_z: bad argument"); return SONIC_ERR_INVALID_ARG; }
  *all_accepted = 0;
  API_BEGIN_ON(v->device)
  int rc = batch_size_ok("sonic_verifier_verify_batch_z", v, K);
  if (rc) return rc;
  std::lock_guard<std::mutex> g(v->mu);
  std::vector<uint8_t> proofs, accepted;
  decompress_device(v, (long)K, proofs_z, proofs, accepted);
  return verify_batch_core(v, (long)K, proofs.data(), challenges, seed, all_accepted, each, &accepted);
  API_CATCH
}
int sonic_verifier_verify_fs_batch_z(sonic_verifier_t* v, int64_t K, const uint8_t* proofs_z, const uint8_t seed[32], int* all_accepted, uint8_t* each) {
  if (!v || !proofs_z || !all_accepted) { set_error("sonic_verifier_verify_fs_batch_z: bad argument"); return SONIC_ERR_INVALID_ARG; }
  *all_accepted = 0;
  API_BEGIN_ON(v->device)
  int rc = batch_size_ok("sonic_verifier_verify_fs_batch_z", v, K);
  if (rc) return rc;
  std::lock_guard<std::mutex> g(v->mu);
  std::vector<uint8_t> proofs, accepted;
  decompress_device(v, (long)K, proofs_z, proofs, accepted);
  return verify_fs_batch_core(v, (long)K, proofs.data(), seed, all_accepted, each, &accepted);
  API_CATCH
}

// one statement per proof: proof k against the handle's weights and cs_k (compressed: 0 = 96-byte points, 1 = 48-byte points)
int sonic_verifier_verify_batch_cs(sonic_verifier_t* v, int64_t K, const uint8_t* proofs, int compressed, const uint8_t* challenges, const uint8_t* cs,
                                   const uint8_t seed[32], int* all_accepted, uint8_t* each) {
  if (all_accepted) *all_accepted = 0;
  API_BEGIN_ON(v ? v->device : -1)                      // (first: without a device the answer is SONIC_ERR_NO_DEVICE whatever the arguments are)
  if (!v || !proofs || !challenges || !cs || !all_accepted || (compressed != 0 && compressed != 1)) { set_error("sonic_verifier_verify_batch_cs: bad argument"); return SONIC_ERR_INVALID_ARG; }
  int rc = batch_size_ok("sonic_verifier_verify_batch_cs", v, K);
  if (rc) return rc;
  std::lock_guard<std::mutex> g(v->mu);
  if (!compressed) return verify_batch_core(v, (long)K, proofs, challenges, seed, all_accepted, each, nullptr, cs);
  std::vector<uint8_t> full, accepted;
  decompress_device(v, (long)K, proofs, full, accepted);
  return verify_batch_core(v, (long)K, full.data(), challenges, seed, all_accepted, each, &accepted, cs);
  API_CATCH
}
int sonic_verifier_verify_fs_batch_cs(sonic_verifier_t* v, int64_t K, const uint8_t* proofs, int compressed, const uint8_t* cs, const uint8_t seed[32],
                                      int* all_accepted, uint8_t* each) {
  if (all_accepted) *all_accepted = 0;
  API_BEGIN_ON(v ? v->device : -1)                      // (first: without a device the answer is SONIC_ERR_NO_DEVICE whatever the arguments are)
  if (!v || !proofs || !cs || !all_accepted || (compressed != 0 && compressed != 1)) { set_error("sonic_verifier_verify_fs_batch_cs: bad argument"); return SONIC_ERR_INVALID_ARG; }
  int rc = batch_size_ok("sonic_verifier_verify_fs_batch_cs", v, K);
  if (rc) return rc;
  std::lock_guard<std::mutex> g(v->mu);
  if (!compressed) return verify_fs_batch_core(v, (long)K, proofs, seed, all_accepted, each, nullptr, cs);
  std::vector<uint8_t> full, accepted;
  decompress_device(v, (long)K, proofs, full, accepted);
  return verify_fs_batch_core(v, (long)K, full.data(), seed, all_accepted, each, &accepted, cs);
  API_CATCH
}

// K core proofs against the handle's circuit: yz = K x (y_k, z_k); cs = K x Q constants or NULL (the handle's); compressed as above
int sonic_verifier_verify_core_batch(sonic_verifier_t* v, int64_t K, const uint8_t* proofs, int compressed, const uint8_t* yz, const uint8_t* cs, const uint8_t seed[32],
                                     int* all_accepted, uint8_t* each) {
  if (all_accepted) *all_accepted = 0;
  API_BEGIN_ON(v ? v->device : -1)                      // (first: without a device the answer is SONIC_ERR_NO_DEVICE whatever the arguments are)
  if (!v || !proofs || !yz || !all_accepted || (compressed != 0 && compressed != 1)) { set_error("sonic_verifier_verify_core_batch: bad argument"); return SONIC_ERR_INVALID_ARG; }
  int rc = batch_size_ok("sonic_verifier_verify_core_batch", v, K);
  if (rc) return rc;
  std::lock_guard<std::mutex> g(v->mu);
  if (!compressed) return verify_core_proofs_batch(v, (long)K, proofs, yz, cs, seed, all_accepted, each);
  std::vector<uint8_t> full, accepted;
  decompress_core_device(v, (long)K, proofs, full, accepted);
  return verify_core_proofs_batch(v, (long)K, full.data(), yz, cs, seed, all_accepted, each, &accepted);
  API_CATCH
}
int sonic_verifier_verify_core_fs_batch(sonic_verifier_t* v, int64_t K, const uint8_t* proofs, int compressed, const uint8_t* cs, const uint8_t seed[32], int* all_accepted,
                                        uint8_t* each) {
  if (all_accepted) *all_accepted = 0;
  API_BEGIN_ON(v ? v->device : -1)
  if (!v || !proofs || !all_accepted || (compressed != 0 && compressed != 1)) { set_error("sonic_verifier_verify_core_fs_batch: bad argument"); return SONIC_ERR_INVALID_ARG; }
  int rc = batch_size_ok("sonic_verifier_verify_core_fs_batch", v, K);
  if (rc) return rc;
  std::lock_guard<std::mutex> g(v->mu);
  if (!compressed) return verify_core_proofs_fs_batch(v, (long)K, proofs, cs, seed, all_accepted, each, nullptr);
  std::vector<uint8_t> full, accepted;
  decompress_core_device(v, (long)K, proofs, full, accepted);
  return verify_core_proofs_fs_batch(v, (long)K, full.data(), cs, seed, all_accepted, each, &accepted);
  API_CATCH
}
// K core proofs and the aggregate signature over their (y_k, z_k): yz = K x (y_k, z_k), or null -- the Fiat-Shamir form, y_k, z_k from each
// proof's own transcript
static int verify_core_helped_entry(const char* who, sonic_verifier_t* v, int64_t K, const uint8_t* proofs, int compressed, const uint8_t* yz, bool fs, const uint8_t* cs,
                                    const uint8_t* aggregate, const uint8_t seed[32], int* all_accepted, uint8_t* each) {
  if (all_accepted) *all_accepted = 0;
  API_BEGIN_ON(v ? v->device : -1)                      // (first: without a device the answer is SONIC_ERR_NO_DEVICE whatever the arguments are)
  if (!v || !proofs || (!fs && !yz) || !aggregate || !all_accepted || (compressed != 0 && compressed != 1)) { set_error("%s: bad argument", who); return SONIC_ERR_INVALID_ARG; }
  int rc = batch_size_ok(who, v, K);
  if (rc) return rc;
  std::lock_guard<std::mutex> g(v->mu);
  helped_reserve(v, (long)K);
  std::vector<uint8_t> full, accepted, yzs;
  if (compressed) { decompress_core_device(v, (long)K, proofs, full, accepted); proofs = full.data(); }
  if (fs) { core_fs_challenges_batch(v, (long)K, proofs, cs, yzs); yz = yzs.data(); }
  return verify_core_helped(v, (long)K, proofs, yz, cs, aggregate, seed, all_accepted, each, compressed ? &accepted : nullptr);
  API_CATCH
}
int sonic_verifier_verify_core_batch_helped(sonic_verifier_t* v, int64_t K, const uint8_t* proofs, int compressed, const uint8_t* yz, const uint8_t* cs,
                                            const uint8_t* aggregate, const uint8_t seed[32], int* all_accepted, uint8_t* each) {
  return verify_core_helped_entry("sonic_verifier_verify_core_batch_helped", v, K, proofs, compressed, yz, false, cs, aggregate, seed, all_accepted, each);
}
int sonic_verifier_verify_core_fs_batch_helped(sonic_verifier_t* v, int64_t K, const uint8_t* proofs, int compressed, const uint8_t* cs, const uint8_t* aggregate,
                                               const uint8_t seed[32], int* all_accepted, uint8_t* each) {
  return verify_core_helped_entry("sonic_verifier_verify_core_fs_batch_helped", v, K, proofs, compressed, nullptr, true, cs, aggregate, seed, all_accepted, each);
}
// the digest of a batch of core proofs on its own (host only; fs.hpp)
int sonic_verify_core_batch_digest(int64_t n, int64_t Q, int64_t d, const uint8_t circuit_digest[32], const uint8_t srs_id[32], int64_t K, const uint8_t* proofs,
                                   const uint8_t* yz, const uint8_t* cs, uint8_t out[32]) {
  if (n < 1 || Q < 1 || d < 1 || !circuit_digest || !srs_id || K < 0 || (K > 0 && (!proofs || !yz || !cs)) || !out) { set_error("sonic_verify_core_batch_digest: bad argument"); return SONIC_ERR_INVALID_ARG; }
  fs_core_batch_digest(n, Q, d, circuit_digest, srs_id, K, proofs, yz, cs, out);
  return SONIC_OK;
}

int sonic_verifier_eval_s(sonic_verifier_t* v, int64_t K, const uint8_t* uv, uint8_t* out) {
  if (!v || !uv || !out) { set_error("sonic_verifier_eval_s: bad argument"); return SONIC_ERR_INVALID_ARG; }
  API_BEGIN_ON(v->device)
  int rc = batch_size_ok("sonic_verifier_eval_s", v, K);
  if (rc) return rc;
  std::vector<Fr> us((size_t)K), vs((size_t)K), sv;
  std::vector<uint8_t> ok;
  for (int64_t k = 0; k < K; k++)
    if (!load_fr(uv + 64 * k, us[(size_t)k]) || !load_fr(uv + 64 * k + 32, vs[(size_t)k])) { set_error("sonic_verifier_eval_s: pair %lld holds a non-canonical field element", (long long)k); return SONIC_ERR_BAD_ENCODING; }
  std::lock_guard<std::mutex> g(v->mu);
  eval_s_device(v, (long)K, us, vs, sv, ok);
  // a refused pair (u = 0 or v = 0) gets 32 bytes of 0xff -- no field element -- and the call reports the first one
  int64_t refused = -1;
  for (int64_t k = 0; k < K; k++) {
    if (!ok[(size_t)k]) { memset(out + 32 * k, 0xff, 32); if (refused < 0) refused = k; continue; }
    const Fr s = fp_from_mont(sv[(size_t)k]);
    memcpy(out + 32 * k, s.l, 32);
  }
  if (refused >= 0) { set_error("sonic_verifier_eval_s: u or v is zero in pair %lld", (long long)refused); return SONIC_ERR_INEXACT_DIVISION; }
  return SONIC_OK;
  API_CATCH
}

int sonic_g1_validate(const uint8_t* points, int64_t n, uint8_t* flags) {
  if (n < 0 || (n > 0 && (!points || !flags))) { set_error("sonic_g1_validate: bad argument"); return SONIC_ERR_INVALID_ARG; }
  if (n == 0) return SONIC_OK;
  API_BEGIN
  CallLease lease;
  hipStream_t st = lease.st();
  DevBuf raw(96 * (size_t)n), pts(sizeof(G1Affine) * (size_t)n), fl((size_t)n);
  HIP_OK(hipMemcpyAsync(raw.p, points, 96 * (size_t)n, hipMemcpyHostToDevice, st));
  g1_validate_enqueue(st, raw.as<uint8_t>(), pts.as<G1Affine>(), fl.as<uint8_t>(), (long)n);
  HIP_OK(hipMemcpyAsync(flags, fl.p, (size_t)n, hipMemcpyDeviceToHost, st));
  HIP_OK(hipStreamSynchronize(st));
  return SONIC_OK;
  API_CATCH
}

// ---- subgroup membership on its own (include/sonic_hip.h, "Subgroup membership") ----
int sonic_g1_subgroup_check(const uint8_t* points96, int64_t n, int method, uint8_t* flags) {
  if (int rc = subgroup_args_ok("sonic_g1_subgroup_check", points96, n, method, flags)) return rc;
  if (n == 0) return SONIC_OK;
  API_BEGIN
  CallLease lease;
  hipStream_t st = lease.st();
  DevBuf raw(96 * (size_t)n), fl((size_t)n);
  HIP_OK(hipMemcpyAsync(raw.p, points96, 96 * (size_t)n, hipMemcpyHostToDevice, st));
  g1_subgroup_enqueue(st, raw.as<uint8_t>(), fl.as<uint8_t>(), (long)n, method);
  HIP_OK(hipMemcpyAsync(flags, fl.p, (size_t)n, hipMemcpyDeviceToHost, st));
  HIP_OK(hipStreamSynchronize(st));
  return SONIC_OK;
  API_CATCH
}

int sonic_g2_subgroup_check(const uint8_t* points192, int64_t n, int method, uint8_t* flags) {
  if (int rc = subgroup_args_ok("sonic_g2_subgroup_check", points192, n, method, flags)) return rc;
  if (n == 0) return SONIC_OK;
  API_BEGIN
  CallLease lease;
  hipStream_t st = lease.st();
  DevBuf raw(192 * (size_t)n), fl((size_t)n);
  HIP_OK(hipMemcpyAsync(raw.p, points192, 192 * (size_t)n, hipMemcpyHostToDevice, st));
  g2_subgroup_enqueue(st, raw.as<uint8_t>(), fl.as<uint8_t>(), (long)n, method);
  HIP_OK(hipMemcpyAsync(flags, fl.p, (size_t)n, hipMemcpyDeviceToHost, st));
  HIP_OK(hipStreamSynchronize(st));
  return SONIC_OK;
  API_CATCH
}

int sonic_verify_batch_randomizers(const uint8_t seed[32], const uint8_t batch_digest[32], int64_t count, uint8_t* out) {
  if (!seed || !batch_digest || count < 0 || (count > 0 && !out)) { set_error("sonic_verify_batch_randomizers: bad argument"); return SONIC_ERR_INVALID_ARG; }
  batch_randomizers(seed, batch_digest, 0, count, out);
  return SONIC_OK;
}

}  // extern "C"
