// The G2 half of SRS.new (src/Sonic/SRS.hs:35-36,40-41):
//   basis 0: h^{x^e}       (hNegativeX[k] = e = -(k+1), hPositiveX[k] = e = k)
//   basis 1: h^{alpha x^e} (hNegativeAlphaX[k] = e = -(k+1), hPositiveAlphaX[k] = e = k)      e in [-d, d]
// The prover never reads these (the verifier reads hPositiveAlphaX[0], [1] and one h^{x^{-d+max}},
// CommitmentScheme.hs:58-68), so they are generated lazily, on the first sonic_srs_get_g2_points call: same
// scheme as the G1 side (byte table of the generator, 32 mixed additions per element, batched normalisation).
#include "internal.hpp"
#include "g2.hpp"
#include "srs_scale.hpp"
#include "compress.hpp"

namespace sonic {

__device__ __forceinline__ G2Affine g2_generator() {
  constexpr uint32_t x0[12] = G2_GEN_X0_MONT, x1[12] = G2_GEN_X1_MONT, y0[12] = G2_GEN_Y0_MONT, y1[12] = G2_GEN_Y1_MONT;
  G2Affine g;
  for (int i = 0; i < 12; i++) { g.x.c0.l[i] = x0[i]; g.x.c1.l[i] = x1[i]; g.y.c0.l[i] = y0[i]; g.y.c1.l[i] = y1[i]; }
  return g;
}

// tab[w * 256 + j] = j * 2^(8w) * H (Jacobian); one thread per w
__global__ __launch_bounds__(64, 1) void k_g2_fb_table(G2Jac* __restrict__ tab) {
  int w = blockIdx.x * blockDim.x + threadIdx.x;
  if (w >= 32) return;
  G2Affine h = g2_generator();
  G2Jac b; b.x = h.x; b.y = h.y; b.z = Fq2::one();
  for (int i = 0; i < 8 * w; i++) b = g2_dbl(b);
  const G2Affine base = g2_to_affine(b);
  G2Jac acc = G2Jac::inf();
  tab[w * 256] = acc;
  for (int j = 1; j < 256; j++) { acc = g2_add_mixed(acc, base); tab[w * 256 + j] = acc; }
}
__global__ __launch_bounds__(64, 1) void k_g2_to_affine(const G2Jac* __restrict__ in, G2Affine* __restrict__ out, long n) {
  long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) out[i] = g2_to_affine(in[i]);
}

__device__ __forceinline__ G2Jac g2_fixed_base_mul(const G2Affine* __restrict__ tab, const Fr& k_mont) {
  Fr k = fp_from_mont(k_mont);
  G2Jac acc = G2Jac::inf();
#pragma unroll 1
  for (int w = 0; w < 32; w++) {
    uint32_t b = (k.l[w >> 2] >> (8 * (w & 3))) & 0xffu;
    if (b) acc = g2_add_mixed(acc, tab[w * 256 + b]);
  }
  return acc;
}

__global__ __launch_bounds__(256, 1) void k_g2_srs_points(const G2Affine* __restrict__ tab, long e_origin, long m, Fr x, Fr xinv, Fr alpha,
                                                          G2Jac* __restrict__ out0, G2Jac* __restrict__ out1) {
  long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= m) return;
  long e = i - e_origin;
  Fr p = e >= 0 ? fp_pow_u64(x, (uint64_t)e) : fp_pow_u64(xinv, (uint64_t)(-e));
  out0[i] = g2_fixed_base_mul(tab, p);
  out1[i] = g2_fixed_base_mul(tab, fp_mul(p, alpha));
}

// Montgomery's trick in Fq2 over chunks of 64 points
__global__ __launch_bounds__(64, 1) void k_g2_batch_affine(const G2Jac* __restrict__ in, G2Affine* __restrict__ out, Fq2* __restrict__ pref, long n) {
  constexpr int CH = 64;
  long c = (long)blockIdx.x * blockDim.x + threadIdx.x;
  long lo = c * CH, hi = lo + CH;
  if (lo >= n) return;
  if (hi > n) hi = n;
  Fq2 acc = Fq2::one();
  for (long i = lo; i < hi; i++) {
    pref[i] = acc;
    G2Jac p = in[i];
    if (!p.is_inf()) acc = f2_mul(acc, p.z);
  }
  Fq2 inv = f2_inv(acc);
  for (long i = hi - 1; i >= lo; i--) {
    G2Jac p = in[i];
    if (p.is_inf()) { out[i] = G2Affine::inf(); continue; }
    Fq2 zi = f2_mul(inv, pref[i]);
    inv = f2_mul(inv, p.z);
    Fq2 zi2 = f2_sqr(zi);
    G2Affine a;
    a.x = f2_mul(p.x, zi2);
    a.y = f2_mul(p.y, f2_mul(zi2, zi));
    out[i] = a;
  }
}

__global__ void k_g2_setup_x(const Fr* in_std, Fr* out) {
  Fr x = fp_to_mont(in_std[0]), a = fp_to_mont(in_std[1]);
  out[0] = x; out[1] = fp_inv(x); out[2] = a;
}

__global__ __launch_bounds__(256) void k_g2_points_to_bytes(const G2Affine* __restrict__ in, uint8_t* __restrict__ out, long n) {
  long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  G2Affine p = in[i];
  uint32_t* w = reinterpret_cast<uint32_t*>(out + 192 * i);
  if (p.is_inf()) { for (int k = 0; k < 48; k++) w[k] = 0; return; }
  Fq a = fp_from_mont(p.x.c0), b = fp_from_mont(p.x.c1), c = fp_from_mont(p.y.c0), e = fp_from_mont(p.y.c1);
  for (int k = 0; k < 12; k++) { w[k] = a.l[k]; w[12 + k] = b.l[k]; w[24 + k] = c.l[k]; w[36 + k] = e.l[k]; }
}

// Caller-supplied G2 elements (an SRS file, sonic_srs_set_g2_points): canonical coordinates, on the twist
// y^2 = x^3 + 4(u + 1), and r P = O by the endomorphism test, g2_in_subgroup (E'(Fq2) has a large cofactor and the pairing is
// bilinear only on the order-r subgroup).  err bits as on the G1 side: 1 non-canonical, 2 off the curve, 4 outside the
// subgroup, 8 the point at infinity.
__global__ __launch_bounds__(64, 1) void k_g2_points_from_bytes(const uint8_t* __restrict__ in, G2Affine* __restrict__ out, long n, int* err) {
  long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const uint32_t* w = reinterpret_cast<const uint32_t*>(in + 192 * i);
  G2Affine p;
  for (int k = 0; k < 12; k++) { p.x.c0.l[k] = w[k]; p.x.c1.l[k] = w[12 + k]; p.y.c0.l[k] = w[24 + k]; p.y.c1.l[k] = w[36 + k]; }
  if (!fp_is_canonical(p.x.c0) || !fp_is_canonical(p.x.c1) || !fp_is_canonical(p.y.c0) || !fp_is_canonical(p.y.c1)) {
    atomicOr(err, 1); out[i] = G2Affine::inf(); return;
  }
  uint32_t nz = 0;
  for (int k = 0; k < 48; k++) nz |= w[k];
  // h^{x^e} and h^{alpha x^e} are never the identity (x, alpha != 0): a zero-filled section must not validate -- the verifier's
  // pairing with a G2 element at infinity is 1, and with all three at infinity it would accept every proof
  if (!nz) { atomicOr(err, 8); out[i] = G2Affine::inf(); return; }
  p.x.c0 = fp_to_mont(p.x.c0); p.x.c1 = fp_to_mont(p.x.c1); p.y.c0 = fp_to_mont(p.y.c0); p.y.c1 = fp_to_mont(p.y.c1);
  if (!(f2_sqr(p.y) == g2_curve_rhs(p.x))) { atomicOr(err, 2); out[i] = G2Affine::inf(); return; }
  if (!g2_in_subgroup(p)) { atomicOr(err, 4); out[i] = G2Affine::inf(); return; }
  out[i] = p;
}
void g2_points_from_bytes_enqueue(hipStream_t st, const uint8_t* d_in, G2Affine* out, long n, int* d_err) {
  if (n > 0) LAUNCH(k_g2_points_from_bytes, ceil_div(n, 64), 64, 0, st, d_in, out, n, d_err);
}
// sonic_g2_subgroup_check: the same tests with one verdict per point (0 accepted, infinity included; 1 non-canonical, 2 off the twist,
// 4 outside the subgroup) and the membership test named by METHOD: the endomorphism test every loader runs, or the definition.
template <int METHOD>
__global__ __launch_bounds__(64, 1) void k_g2_subgroup(const uint8_t* __restrict__ in, uint8_t* __restrict__ flags, long n) {
  long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const uint32_t* w = reinterpret_cast<const uint32_t*>(in + 192 * i);
  G2Affine p;
  for (int k = 0; k < 12; k++) { p.x.c0.l[k] = w[k]; p.x.c1.l[k] = w[12 + k]; p.y.c0.l[k] = w[24 + k]; p.y.c1.l[k] = w[36 + k]; }
  uint32_t nz = 0;
  for (int k = 0; k < 48; k++) nz |= w[k];
  if (!nz) { flags[i] = 0; return; }
  if (!fp_is_canonical(p.x.c0) || !fp_is_canonical(p.x.c1) || !fp_is_canonical(p.y.c0) || !fp_is_canonical(p.y.c1)) { flags[i] = 1; return; }
  p.x.c0 = fp_to_mont(p.x.c0); p.x.c1 = fp_to_mont(p.x.c1); p.y.c0 = fp_to_mont(p.y.c0); p.y.c1 = fp_to_mont(p.y.c1);
  if (!(f2_sqr(p.y) == g2_curve_rhs(p.x))) { flags[i] = 2; return; }
  flags[i] = (METHOD == SONIC_SUBGROUP_WALK ? g2_in_subgroup_walk(p) : g2_in_subgroup(p)) ? 0 : 4;
}
void g2_subgroup_enqueue(hipStream_t st, const uint8_t* d_in192, uint8_t* d_flags, long n, int method) {
  if (n <= 0) return;
  if (method == SONIC_SUBGROUP_WALK) LAUNCH(k_g2_subgroup<SONIC_SUBGROUP_WALK>, ceil_div(n, 64), 64, 0, st, d_in192, d_flags, n);
  else LAUNCH(k_g2_subgroup<SONIC_SUBGROUP_DEFAULT>, ceil_div(n, 64), 64, 0, st, d_in192, d_flags, n);
}

// fills h0 / h1 (2d+1 affine points each)
void srs_generate_g2(hipStream_t st, long d, const Fr& x_std, const Fr& alpha_std, G2Affine* h0, G2Affine* h1) {
  const long n = 2 * d + 1;
  DevBuf tabj(sizeof(G2Jac) * 8192), tab(sizeof(G2Affine) * 8192);
  LAUNCH(k_g2_fb_table, 1, 64, 0, st, tabj.as<G2Jac>());
  LAUNCH(k_g2_to_affine, ceil_div(8192, 64), 64, 0, st, (const G2Jac*)tabj.as<G2Jac>(), tab.as<G2Affine>(), 8192L);
  Fr h[2] = {x_std, alpha_std};
  DevBuf in(sizeof h), par(sizeof(Fr) * 3);
  HIP_OK(hipMemcpyAsync(in.p, h, sizeof h, hipMemcpyHostToDevice, st));
  LAUNCH(k_g2_setup_x, 1, 1, 0, st, (const Fr*)in.as<Fr>(), par.as<Fr>());
  Fr hp[3];
  HIP_OK(hipMemcpyAsync(hp, par.p, sizeof hp, hipMemcpyDeviceToHost, st));
  HIP_OK(hipStreamSynchronize(st));
  const long SLAB = 1L << 19;
  const long cap = n < SLAB ? n : SLAB;
  DevBuf x0(sizeof(G2Jac) * cap), x1(sizeof(G2Jac) * cap), pref(sizeof(Fq2) * cap);
  for (long base = 0; base < n; base += SLAB) {
    long m = n - base < SLAB ? n - base : SLAB;
    LAUNCH(k_g2_srs_points, ceil_div(m, 256), 256, 0, st, (const G2Affine*)tab.as<G2Affine>(), d - base, m, hp[0], hp[1], hp[2],
           x0.as<G2Jac>(), x1.as<G2Jac>());
    LAUNCH(k_g2_batch_affine, ceil_div(ceil_div(m, 64), 64), 64, 0, st, (const G2Jac*)x0.as<G2Jac>(), h0 + base, pref.as<Fq2>(), m);
    LAUNCH(k_g2_batch_affine, ceil_div(ceil_div(m, 64), 64), 64, 0, st, (const G2Jac*)x1.as<G2Jac>(), h1 + base, pref.as<Fq2>(), m);
  }
  HIP_OK(hipStreamSynchronize(st));
}

// ---- updatable SRS (include/sonic_hip.h, "Updatable SRS"): every G2 point times a scalar of its own -----------------------------------
// out[i] = k_i * in[i] (Jacobian, for k_g2_batch_affine or k_g2_sum), one thread per point.  rho == nullptr: slab slot i <-> exponent
// e = i - e_origin and k_i = x^e (times alpha where mul_alpha), derived in the thread as k_g2_srs_points derives it -- a contribution.
// Otherwise k_i = the low 128 bits of rho[i] -- the randomizers of the structure check -- and only 128 steps are walked.
__global__ __launch_bounds__(256, 1) void k_g2_scale_each(const G2Affine* __restrict__ in, long e_origin, long m, Fr x, Fr xinv, Fr alpha, int mul_alpha,
                                                          const Fr* __restrict__ rho, G2Jac* __restrict__ out) {
  long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= m) return;
  if (rho) { out[i] = g2_scale(in[i], rho[i], 4); return; }
  long e = i - e_origin;
  Fr p = e >= 0 ? fp_pow_u64(x, (uint64_t)e) : fp_pow_u64(xinv, (uint64_t)(-e));
  if (mul_alpha) p = fp_mul(p, alpha);
  out[i] = g2_scale(in[i], fp_from_mont(p));
}

// the sum of n Jacobian points as a block tree: every thread adds the points of its stride, the 64 threads of a block fold their sums
// in LDS (64 x 288 B), and the block's total goes to tot[blockIdx.x] for the host to add.  blockIdx.y counts independent ranges of n points,
// range_stride apart (the segment results of the windows of a G2 MSM, msm_g2.hip): range y's totals follow those of range y - 1
constexpr int G2_SUM_BLOCK = 64, G2_SUM_MAX_BLOCKS = 256;
__global__ __launch_bounds__(G2_SUM_BLOCK, 1) void k_g2_sum(const G2Jac* __restrict__ in, long n, G2Jac* __restrict__ tot, long range_stride) {
  __shared__ G2Jac sh[G2_SUM_BLOCK];
  const int t = threadIdx.x;
  in += (size_t)blockIdx.y * range_stride;
  tot += (size_t)blockIdx.y * gridDim.x;
  G2Jac acc = G2Jac::inf();
  for (long i = (long)blockIdx.x * G2_SUM_BLOCK + t; i < n; i += (long)gridDim.x * G2_SUM_BLOCK) acc = g2_add(acc, in[i]);
  sh[t] = acc;
  __syncthreads();
  for (int s = G2_SUM_BLOCK / 2; s > 0; s >>= 1) {
    if (t < s) sh[t] = g2_add(sh[t], sh[t + s]);
    __syncthreads();
  }
  if (t == 0) {
    G2Jac r = sh[0];                  // leaves the device (lazy range)
    r.x.c0 = fp_canonical(r.x.c0); r.x.c1 = fp_canonical(r.x.c1); r.y.c0 = fp_canonical(r.y.c0); r.y.c1 = fp_canonical(r.y.c1);
    r.z.c0 = fp_canonical(r.z.c0); r.z.c1 = fp_canonical(r.z.c1);
    tot[blockIdx.x] = r;
  }
}

// `ranges` sums of n Jacobian points each, range_stride apart, into tot[0 .. ranges) (canonical limbs): one launch of a block per range
// up to G2_SUM_BLOCK points, else a launch of up to G2_SUM_BLOCK blocks per range into `tmp` (ranges x G2_SUM_BLOCK points) and one over those
void g2_sum_ranges_enqueue(hipStream_t st, const G2Jac* in, long n, int ranges, long range_stride, G2Jac* tmp, G2Jac* tot) {
  const int blocks = ceil_div(n, G2_SUM_BLOCK) < G2_SUM_BLOCK ? ceil_div(n, G2_SUM_BLOCK) : G2_SUM_BLOCK;
  if (blocks <= 1) { LAUNCH(k_g2_sum, dim3(1, ranges), G2_SUM_BLOCK, 0, st, in, n, tot, range_stride); return; }
  LAUNCH(k_g2_sum, dim3(blocks, ranges), G2_SUM_BLOCK, 0, st, in, n, tmp, range_stride);
  LAUNCH(k_g2_sum, dim3(1, ranges), G2_SUM_BLOCK, 0, st, (const G2Jac*)tmp, (long)blocks, tot, (long)blocks);
}

// sum_i rho[i] * pts[i] over n points (rho: 128-bit scalars in 32-byte elements) as the 192 canonical bytes sonic_srs_get_g2_points writes;
// waits for the stream
void g2_weighted_sum(hipStream_t st, const G2Affine* pts, const Fr* d_rho, long n, uint8_t out192[192]) {
  const long SLAB = 1L << 19;
  const long cap = n < SLAB ? n : SLAB;
  const int slabs = ceil_div(n, SLAB);
  DevBuf xs(sizeof(G2Jac) * cap), tot(sizeof(G2Jac) * (size_t)G2_SUM_MAX_BLOCKS * slabs);
  std::vector<G2Jac> h;
  const Fr none = Fr::zero();
  long nt = 0;
  for (long base = 0; base < n; base += SLAB) {
    const long m = n - base < SLAB ? n - base : SLAB;
    const int blocks = ceil_div(m, G2_SUM_BLOCK) < G2_SUM_MAX_BLOCKS ? ceil_div(m, G2_SUM_BLOCK) : G2_SUM_MAX_BLOCKS;
    LAUNCH(k_g2_scale_each, ceil_div(m, 256), 256, 0, st, pts + base, 0L, m, none, none, none, 0, d_rho + base, xs.as<G2Jac>());
    LAUNCH(k_g2_sum, blocks, G2_SUM_BLOCK, 0, st, (const G2Jac*)xs.as<G2Jac>(), m, tot.as<G2Jac>() + nt, 0L);
    nt += blocks;
  }
  h.resize((size_t)nt);
  HIP_OK(hipMemcpyAsync(h.data(), tot.p, sizeof(G2Jac) * (size_t)nt, hipMemcpyDeviceToHost, st));
  HIP_OK(hipStreamSynchronize(st));
  G2Jac acc = G2Jac::inf();
  for (long k = 0; k < nt; k++) acc = g2_add(acc, h[(size_t)k]);
  uint32_t w[48];
  g2_canonical_words(g2_to_affine(acc), w);
  memcpy(out192, w, 192);
}

// o0[i] = x^e * h0[i], o1[i] = alpha x^e * h1[i] over the 2d + 1 points of each basis (x, xinv, alpha Montgomery); waits for the stream
void srs_scale_g2(hipStream_t st, long d, const G2Affine* h0, const G2Affine* h1, const Fr& x, const Fr& xinv, const Fr& alpha, G2Affine* o0, G2Affine* o1) {
  const long n = 2 * d + 1;
  const long SLAB = 1L << 19;
  const long cap = n < SLAB ? n : SLAB;
  DevBuf xs(sizeof(G2Jac) * cap), pref(sizeof(Fq2) * cap);
  for (int b = 0; b < 2; b++)
    for (long base = 0; base < n; base += SLAB) {
      const long m = n - base < SLAB ? n - base : SLAB;
      LAUNCH(k_g2_scale_each, ceil_div(m, 256), 256, 0, st, (b ? h1 : h0) + base, d - base, m, x, xinv, alpha, b, (const Fr*)nullptr, xs.as<G2Jac>());
      LAUNCH(k_g2_batch_affine, ceil_div(ceil_div(m, 64), 64), 64, 0, st, (const G2Jac*)xs.as<G2Jac>(), (b ? o1 : o0) + base, pref.as<Fq2>(), m);
    }
  HIP_OK(hipStreamSynchronize(st));
}

void g2_points_to_bytes_enqueue(hipStream_t st, const G2Affine* in, uint8_t* d_out, long n) {
  if (n > 0) LAUNCH(k_g2_points_to_bytes, ceil_div(n, 256), 256, 0, st, in, d_out, n);
}

}  // namespace sonic
