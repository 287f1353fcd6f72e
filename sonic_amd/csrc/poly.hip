// Laurent-polynomial kernels of the prover, on dense Fr coefficient arrays (Montgomery form) over
// an exponent range [lo, lo + n).  The reference works on sparse (exponent, coeff) lists
// (poly-0.4.0.0); every operation here is result-exact, zeros simply stay in the array.
//
//   scale by powers     c_e <- c_e x^e        evalY on the diagonal r(X,Y) (src/Sonic/Utils.hs:20-21
//                                              with Constraints.hs:23-31), and the first half of eval
//   prefix sums         P_j = sum_{e<=j} c_e z^e   -> f(z) = P_hi         (`eval`, CommitmentScheme.hs:43)
//   quotient            w_j = z^{-1-j} (f(z) - P_j)  (j >= 0),  -z^{-1-j} P_j  (j < 0)
//                       = (f(X) - f(z)) / (X - z)                          (`divide`, CommitmentScheme.hs:44)
//   s(X,y), s(u,Y)      evalY / evalX of sPoly (Constraints.hs:34-53, Utils.hs:17-21)
//
// Quotient identity: for e > 0, (X^e - z^e)/(X - z) = sum_{k<e} X^k z^{e-1-k}; for e < 0,
// (X^e - z^e)/(X - z) = -sum_{m=1..|e|} X^{-m} z^{e+m-1}.  Collecting the coefficient of X^j gives
// the two prefix-sum forms above, so the stand-alone openPoly (open_job) is one elementwise pass, one
// additive scan and one more elementwise pass.  The openings of a proof (open_batch_enqueue) use the
// same identity as two Horner recurrences cut into per-thread chunks -- see "Horner sweeps" below: a
// chunked Horner chain is no more sequential than a thread's p = p * step, and needs no power of z per
// coefficient.
#include "internal.hpp"
#include "poly.hpp"
#include "csr.hpp"

namespace sonic {

// Elements per thread of k_scale_powers.  A thread pays ~45 products for its starting power x^(e0 + i) and x^256 and then 2 per
// element, i.e. (45 + 2 PER) / PER products per element: 7.6 at PER = 8, 3.4 at 32.  (Until round 8 a proof's openings ran through
// these kernels too, two passes over ~38 n coefficients: at 8 they were ~5 % of a proof's instruction count.  The openings now take
// the Horner sweeps below; the stand-alone openPoly, the aggregate and the power tables of prove.hip still come here.)
#ifndef SONIC_SCALE_PER
#define SONIC_SCALE_PER 32
#endif
constexpr int SCALE_PER = SONIC_SCALE_PER;
// ... for arrays long enough to fill the chip with threads of that length.  A short array (n = 2^14: 49 K coefficients = 6 workgroups at
// 32 per thread) runs as ONE dependent chain of 45 + 2 PER products on a few waves -- 80 us per launch, twenty launches on a proof's
// critical path (profiles/r06_small_proofs.txt) -- so the elements per thread shrink until ~64 workgroups exist (never below 2).  Not more
// workgroups than that: beside another proof's bucket accumulation (streamed proofs) wave slots come free at a few hundred workgroups
// per millisecond, and a launch of 257 short workgroups took 1-2 ms to be handed all of them (profiles/r06_small_proofs.txt).
static int scale_per(long n) {
  long per = n / (256L * 64L);
  if (per > SCALE_PER) per = SCALE_PER;
  if (per < 2) per = 2;
  return (int)per;
}

// out[i] = v(i) * x^(e0 + i); v(i) depends on mode:
//   0: in[i]                     1: 1 (pure power table)
//   2: quotient numerator: j = lo_q + i >= 0 ? F - P[i] : -P[i], with F = in[nF-1] (the last prefix)
template <int MODE>
__global__ __launch_bounds__(256) void k_scale_powers(const Fr* __restrict__ in, Fr* __restrict__ out, long n, long e0,
                                                      const Fr* __restrict__ px, const Fr* __restrict__ pxinv, long lo_q, long nF, int PER) {
  // PER elements per thread, strided by the block size
  const long base = (long)blockIdx.x * (256 * PER) + threadIdx.x;
  if (base >= n) return;
  const Fr x = *px, xinv = *pxinv;
  const long e = e0 + base;
  Fr p = e >= 0 ? fp_pow_u64(x, (uint64_t)e) : fp_pow_u64(xinv, (uint64_t)(-e));
  const Fr step = fp_pow_u64(x, 256);
  Fr F;
  if (MODE == 2) F = in[nF - 1];
#pragma unroll 1
  for (int k = 0; k < PER; k++) {
    const long i = base + (long)k * 256;
    if (i >= n) break;
    Fr v;
    if (MODE == 0) v = fp_mul(in[i], p);
    else if (MODE == 1) v = p;
    else { Fr P = in[i]; v = fp_mul((lo_q + i >= 0) ? fp_sub(F, P) : fp_neg(P), p); }
    out[i] = v;
    p = fp_mul(p, step);
  }
}

void poly_scale_powers_enqueue(hipStream_t st, const Fr* in, Fr* out, long n, long e0, const Fr* d_x, const Fr* d_xinv) {
  if (n <= 0) return;
  const int per = scale_per(n);
  if (in) LAUNCH(k_scale_powers<0>, ceil_div(n, 256L * per), 256, 0, st, in, out, n, e0, d_x, d_xinv, 0L, 0L, per);
  else LAUNCH(k_scale_powers<1>, ceil_div(n, 256L * per), 256, 0, st, in, out, n, e0, d_x, d_xinv, 0L, 0L, per);
}

// q[i] (exponent lo + i, i < n - 1) from the prefix sums P (n entries, exponents lo .. lo + n - 1)
void poly_quotient_enqueue(hipStream_t st, const Fr* prefix, Fr* q, long n, long lo, const Fr* d_z, const Fr* d_zinv) {
  if (n <= 1) return;
  // z^{-1-j} = (z^-1)^{1+j}: base z^-1 (inverse base z), first exponent 1 + lo
  const int per = scale_per(n - 1);
  LAUNCH(k_scale_powers<2>, ceil_div(n - 1, 256L * per), 256, 0, st, prefix, q, n - 1, 1 + lo, d_zinv, d_z, lo, n, per);
}

// Workgroups of an elementwise launch over `items` elements (256 threads each, grid-stride loops): short arrays get at most 64 fat
// workgroups (see scale_per: a launch of many short workgroups waits for wave slots one by one beside a running accumulation); long ones
// one element per thread, as before
static unsigned elementwise_grid(long items) {
  const long full = ceil_div(items, 256L);
  return (unsigned)(items <= (1L << 19) && full > 64 ? 64 : (full > 0 ? full : 1));
}

// ---- inclusive prefix sums in Fr (tile = 1024) -----------------------------------------------
__device__ __forceinline__ Fr block_inclusive_scan_fr(Fr v, Fr* sh) {
  const int t = threadIdx.x;
  sh[t] = v;
  __syncthreads();
  for (int o = 1; o < 256; o <<= 1) {
    Fr x = t >= o ? sh[t - o] : Fr::zero();
    __syncthreads();
    sh[t] = fp_add(sh[t], x);
    __syncthreads();
  }
  Fr r = sh[t];
  __syncthreads();
  return r;
}
__global__ __launch_bounds__(256) void k_prefix_tiles(Fr* __restrict__ d, long n, Fr* __restrict__ tile_sums) {
  __shared__ Fr sh[256];
  const long base = (long)blockIdx.x * 1024 + threadIdx.x * 4;
  Fr v[4], s = Fr::zero();
  for (int k = 0; k < 4; k++) { v[k] = base + k < n ? d[base + k] : Fr::zero(); s = fp_add(s, v[k]); v[k] = s; }
  Fr incl = block_inclusive_scan_fr(s, sh);
  Fr excl = fp_sub(incl, s);
  for (int k = 0; k < 4; k++) if (base + k < n) d[base + k] = fp_add(v[k], excl);
  if (threadIdx.x == 255) tile_sums[blockIdx.x] = incl;
}
__global__ __launch_bounds__(256) void k_prefix_top(Fr* __restrict__ tile_sums, long ntiles) {
  __shared__ Fr sh[256];
  __shared__ Fr carry_sh;
  if (threadIdx.x == 0) carry_sh = Fr::zero();
  __syncthreads();
  for (long base = 0; base < ntiles; base += 256) {
    long idx = base + threadIdx.x;
    Fr v = idx < ntiles ? tile_sums[idx] : Fr::zero();
    Fr incl = block_inclusive_scan_fr(v, sh);
    Fr carry = carry_sh;
    if (idx < ntiles) tile_sums[idx] = fp_add(fp_sub(incl, v), carry);   // exclusive
    __syncthreads();
    if (threadIdx.x == 255) carry_sh = fp_add(carry, incl);
    __syncthreads();
  }
}
__global__ __launch_bounds__(256) void k_prefix_apply(Fr* __restrict__ d, long n, const Fr* __restrict__ tile_sums) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const long tile = i >> 10;
  if (tile == 0) return;
  d[i] = fp_add(d[i], tile_sums[tile]);
}
void poly_prefix_sum_enqueue(hipStream_t st, Fr* d, long n, DevBuf& tmp) {
  if (n <= 0) return;
  const long ntiles = (n + 1023) / 1024;
  tmp.ensure(sizeof(Fr) * (ntiles + 1));
  LAUNCH(k_prefix_tiles, (int)ntiles, 256, 0, st, d, n, tmp.as<Fr>());
  if (ntiles > 1) {
    LAUNCH(k_prefix_top, 1, 256, 0, st, tmp.as<Fr>(), ntiles);
    LAUNCH(k_prefix_apply, ceil_div(n, 256), 256, 0, st, d, n, (const Fr*)tmp.as<Fr>());
  }
}

// ---- Horner sweeps: several openings at once, without the power tables and without D (blockIdx.y = opening) ---------------------------
// The quotient identity above, written as recurrences over the coefficient index i (X^0 at i0 = -lo, w = the quotient):
//   below X^0, upward     w_i = z^-1 (w_{i-1} - f_i),   w_{-1} = 0          (i < i0)
//   from X^0 on, downward w_i = f_{i+1} + z w_{i+1},    w_{len-1} = 0       (i >= i0)
//   f(z) = f_{i0} + z w_{i0} - w_{i0-1}
// Each side is a sequence x_t = step(x_{t-1}, a_t), t = 0 .. M - 1 (upward: a_t = f_t; downward: a_t = f_{len-1-t}), and every step is an
// affine map of x with the same multiplier m (z^-1 or z).  A thread owns a chunk of L consecutive t.  k_sweep_chunks_b runs every chunk
// from x = 0 (L products) and scans the chunk values over the workgroup's tile: chunks compose as x -> m^L x + b, so level o of the scan
// multiplies by the one power m^(L o) (8 products a thread).  It leaves the carry into every chunk of a tile that itself starts from 0, and
// the tile's value.  k_sweep_carries_b scans the tile values the same way (multiplier m^tile), which gives the carry into every tile and,
// from the two sides' end values, f(z).  k_sweep_quotient_b repeats the recurrence from the true carry -- the chunk's carry within its tile
// plus (m^L)^t times the tile's carry, the power read from a table of 256 -- and stores w (L + 1 products).  That is 2 + 9/L products per
// coefficient and opening (plus 16 on the first wave of a workgroup for the scan's multipliers) instead of 4 + 90/PER, and the polynomial
// read twice and the quotient written once instead of seven passes.  A sequential chain of L products per thread is what k_scale_powers'
// p = p * step already is.
// A side is padded IN FRONT to whole tiles (t < 0: no coefficient; x stays 0 there under both recurrences), so that every chunk that
// carries anything is full and the last tile's inclusive value is the side's end value.
// Threads take L consecutive 32-byte coefficients, loaded four at a time: one 128-byte line per lane and group of loads.
// Openings that share their polynomial read it once each (through L2): one read feeding k recurrences would hold k x 8 registers of
// state next to the four loaded coefficients and the product's temporaries, and OPEN_BATCH_MAX = 16 of them do not fit without scratch.
struct SweepShape {
  long len, i0;        // coefficients; index of X^0
  int L;               // coefficients per thread (open_sweep_chunk)
  long M[2], nb[2], pad[2];   // per side (0: below X^0, 1: from X^0 on): elements, tiles, padding in front
};
static SweepShape sweep_shape(long lo, long len, int chunk) {
  SweepShape s;
  s.len = len; s.i0 = -lo; s.L = chunk ? chunk : open_sweep_chunk(len);
  const long tile = (long)SWEEP_BLOCK * s.L;
  s.M[0] = s.i0; s.M[1] = len - 1 - s.i0;
  for (int r = 0; r < 2; r++) { s.nb[r] = ceil_div(s.M[r], tile); s.pad[r] = s.nb[r] * tile - s.M[r]; }
  return s;
}
// OpenBatch::tiles of one opening, NB = nb[0] + nb[1] tiles (side 0's first):
//   [tile * 256 + t]          the carry into chunk t of the tile when the tile starts from 0
//   [NB * 256 + tile]         the tile's value from 0 (k_sweep_chunks_b), then the carry into the tile (k_sweep_carries_b)
//   [NB * 257 + side * 257 + t]  (m^L)^t for t < 256, and m^(256 L) at t = 256 (written only for a side of more than one tile)
template <bool UP>
__device__ __forceinline__ Fr sweep_step(const Fr& x, const Fr& a, const Fr& m) {
  return UP ? fp_mul(fp_sub(x, a), m) : fp_add(a, fp_mul(x, m));
}
// elements t0 .. t0 + L - 1 of a side from the carry x; `top` = len - 1 (downward side: a_t = f[top - t], w goes to q[top - 1 - t])
template <bool UP, bool STORE>
__device__ __forceinline__ Fr sweep_chunk(const Fr* __restrict__ f, Fr* __restrict__ q, long t0, int L, long top, Fr x, const Fr& m) {
#pragma unroll 1
  for (int g = 0; g < L; g += 4) {
    Fr a[4];
#pragma unroll
    for (int j = 0; j < 4; j++) {
      const long t = t0 + g + j;
      a[j] = (g + j < L && t >= 0) ? f[UP ? t : top - t] : Fr::zero();
    }
#pragma unroll
    for (int j = 0; j < 4; j++) {
      const long t = t0 + g + j;
      if (g + j < L && t >= 0) {
        x = sweep_step<UP>(x, a[j], m);
        if (STORE) q[UP ? t : top - 1 - t] = x;
      }
    }
  }
  return x;
}
__global__ __launch_bounds__(SWEEP_BLOCK) void k_sweep_chunks_b(const OpenBatch b, const SweepShape s) {
  __shared__ Fr sh[SWEEP_BLOCK];
  __shared__ Fr mu[9];                                   // m^(L 2^k)
  const int y = blockIdx.y, t = threadIdx.x;
  const int r = (long)blockIdx.x >= s.nb[0];
  const long tile = (long)blockIdx.x - (r ? s.nb[0] : 0), NB = s.nb[0] + s.nb[1];
  const Fr m = b.zpair[y][r ? 0 : 1];
  Fr* __restrict__ base = b.tiles[y];
  if (t < 64) {                                          // the first wave: the scan's multipliers, once per workgroup
    Fr p = fp_pow_u64(m, (uint64_t)s.L);
    for (int k = 0; k < 9; k++) {
      if (t == 0) mu[k] = p;
      if (k < 8) p = fp_mul(p, p);
    }
  }
  const long t0 = (tile * SWEEP_BLOCK + t) * s.L - s.pad[r];
  sh[t] = r == 0 ? sweep_chunk<true, false>(b.poly[y], nullptr, t0, s.L, 0, Fr::zero(), m)
                 : sweep_chunk<false, false>(b.poly[y], nullptr, t0, s.L, s.len - 1, Fr::zero(), m);
  __syncthreads();
  for (int k = 0, o = 1; o < SWEEP_BLOCK; o <<= 1, k++) {
    const Fr x = t >= o ? sh[t - o] : Fr::zero();
    __syncthreads();
    sh[t] = fp_add(sh[t], fp_mul(x, mu[k]));
    __syncthreads();
  }
  base[(long)blockIdx.x * SWEEP_BLOCK + t] = t > 0 ? sh[t - 1] : Fr::zero();
  if (t == SWEEP_BLOCK - 1) base[NB * SWEEP_BLOCK + blockIdx.x] = sh[t];
  if (tile == 0 && s.nb[r] > 1) {                        // the tile carries' power table, by the side's first workgroup
    Fr p = Fr::one();
    for (int k = 0; k < 8; k++) if ((t >> k) & 1) p = fp_mul(p, mu[k]);
    Fr* __restrict__ pw = base + NB * (SWEEP_BLOCK + 1) + r * (SWEEP_BLOCK + 1);
    pw[t] = p;
    if (t == 0) pw[SWEEP_BLOCK] = mu[8];
  }
}
// one workgroup per opening, a half of it per side: the carries into the tiles, in blocks of 256 tiles (the carry of a block enters the
// next block's first tile before the scan), the sides' end values, and f(z)
__global__ __launch_bounds__(2 * SWEEP_BLOCK) void k_sweep_carries_b(const OpenBatch b, const SweepShape s) {
  __shared__ Fr sh[2][SWEEP_BLOCK];
  __shared__ Fr fin[2];
  const int y = blockIdx.x, r = threadIdx.x / SWEEP_BLOCK, u = threadIdx.x % SWEEP_BLOCK;
  const long NB = s.nb[0] + s.nb[1], nt = s.nb[r], most = s.nb[0] > s.nb[1] ? s.nb[0] : s.nb[1];
  Fr* __restrict__ base = b.tiles[y];
  Fr* __restrict__ tt = base + NB * SWEEP_BLOCK + (r ? s.nb[0] : 0);
  Fr last = Fr::zero();
  if (most <= 1) {                                       // (a single tile starts from 0, and its value is the side's end value)
    if (nt == 1) last = tt[0];
  } else {
    const Fr muT = nt > 1 ? base[NB * (SWEEP_BLOCK + 1) + r * (SWEEP_BLOCK + 1) + SWEEP_BLOCK] : Fr::zero();
    Fr carry = Fr::zero();
    for (long bs = 0; bs < most; bs += SWEEP_BLOCK) {
      const long idx = bs + u;
      Fr v = idx < nt ? tt[idx] : Fr::zero();
      if (u == 0) v = fp_add(v, fp_mul(carry, muT));
      sh[r][u] = v;
      __syncthreads();
      Fr mu = muT;
      for (int o = 1; o < SWEEP_BLOCK; o <<= 1) {
        const Fr x = u >= o ? sh[r][u - o] : Fr::zero();
        __syncthreads();
        sh[r][u] = fp_add(sh[r][u], fp_mul(x, mu));
        __syncthreads();
        mu = fp_mul(mu, mu);
      }
      if (idx < nt) tt[idx] = u > 0 ? sh[r][u - 1] : carry;
      if (nt - 1 >= bs && nt - 1 < bs + SWEEP_BLOCK) last = sh[r][nt - 1 - bs];
      carry = sh[r][SWEEP_BLOCK - 1];
      __syncthreads();
    }
  }
  if (u == 0) fin[r] = last;
  __syncthreads();
  if (threadIdx.x == 0) *b.fz[y] = fp_sub(fp_add(b.poly[y][s.i0], fp_mul(b.zpair[y][0], fin[1])), fin[0]);
}
__global__ __launch_bounds__(SWEEP_BLOCK) void k_sweep_quotient_b(const OpenBatch b, const SweepShape s) {
  const int y = blockIdx.y, t = threadIdx.x;
  const int r = (long)blockIdx.x >= s.nb[0];
  const long tile = (long)blockIdx.x - (r ? s.nb[0] : 0), NB = s.nb[0] + s.nb[1];
  const long t0 = (tile * SWEEP_BLOCK + t) * s.L - s.pad[r];
  if (t0 + s.L <= 0) return;                             // all padding
  const Fr m = b.zpair[y][r ? 0 : 1];
  const Fr* __restrict__ base = b.tiles[y];
  Fr x = base[(long)blockIdx.x * SWEEP_BLOCK + t];
  if (tile > 0) x = fp_add(x, fp_mul(base[NB * (SWEEP_BLOCK + 1) + r * (SWEEP_BLOCK + 1) + t], base[NB * SWEEP_BLOCK + blockIdx.x]));
  if (r == 0) sweep_chunk<true, true>(b.poly[y], b.q[y], t0, s.L, 0, x, m);
  else sweep_chunk<false, true>(b.poly[y], b.q[y], t0, s.L, s.len - 1, x, m);
}
void open_batch_enqueue(hipStream_t st, const OpenBatch& b, long lo, long len, bool quotient, int chunk) {
  if (b.k <= 0 || len <= 0) return;
  const unsigned k = (unsigned)b.k;
  const SweepShape s = sweep_shape(lo, len, chunk);
  const unsigned NB = (unsigned)(s.nb[0] + s.nb[1]);     // (a polynomial of ONE coefficient has no tiles and an empty quotient: only f(z) = f_0)
  if (NB) LAUNCH(k_sweep_chunks_b, dim3(NB, k), SWEEP_BLOCK, 0, st, b, s);
  LAUNCH(k_sweep_carries_b, k, 2 * SWEEP_BLOCK, 0, st, b, s);
  if (quotient && NB) LAUNCH(k_sweep_quotient_b, dim3(NB, k), SWEEP_BLOCK, 0, st, b, s);
}

// ---- prover-specific builders ----------------------------------------------------------------
// r'(X,1) over [-2n-4, n]: aL at X^i, aR at X^-i, aO at X^{-i-n}, c_{n+i} at X^{-2n-i}
// (Constraints.hs:23-31, Protocol.hs:58-62).  Inputs Montgomery.
__global__ __launch_bounds__(256) void k_build_r1(const Fr* __restrict__ aL, const Fr* __restrict__ aR, const Fr* __restrict__ aO,
                                                  const Fr* __restrict__ cns, long n, Fr* __restrict__ r1) {
  const long len = 3 * n + 5;
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < len; i += (long)gridDim.x * 256) {   // index into [-2n-4, n]
    const long e = i - (2 * n + 4);
    Fr v = Fr::zero();
    if (e > 0) v = aL[e - 1];
    else if (e < 0 && e >= -n) v = aR[-e - 1];
    else if (e < -n && e >= -2 * n) v = aO[-e - n - 1];
    else if (e < -2 * n) v = cns[-e - 2 * n - 1];
    r1[i] = v;
  }
}
void build_r1_enqueue(hipStream_t st, const Fr* aL, const Fr* aR, const Fr* aO, const Fr* cns, long n, Fr* r1) {
  LAUNCH(k_build_r1, elementwise_grid(3 * n + 5), 256, 0, st, aL, aR, aO, cns, n, r1);
}

// s(X,y) over [-n, 2n] given ypow[e + n] = y^e for e in [-n, n + Q]:
//   X^-i: sum_q wL[q][i] y^{n+q};  X^i: sum_q wR[q][i] y^{n+q};
//   X^{i+n}: -y^i - y^-i + sum_q wO[q][i] y^{n+q}        (Constraints.hs:39-49, q = 1..Q)
__global__ __launch_bounds__(256) void k_s_of_y(const Fr* __restrict__ wL, const Fr* __restrict__ wR, const Fr* __restrict__ wO,
                                                const Fr* __restrict__ ypow, long n, long Q, Fr* __restrict__ s) {
  for (long i = (long)blockIdx.x * 256 + threadIdx.x + 1; i <= n + 1; i += (long)gridDim.x * 256) {   // 1..n
    if (i > n) { s[n] = Fr::zero(); break; }                 // X^0 slot
    Fr u = Fr::zero(), v = Fr::zero(), w = Fr::zero();
    for (long q = 0; q < Q; q++) {
      const Fr yq = ypow[2 * n + 1 + q];                     // y^{n+q+1}
      u = fp_add(u, fp_mul(wL[q * n + i - 1], yq));
      v = fp_add(v, fp_mul(wR[q * n + i - 1], yq));
      w = fp_add(w, fp_mul(wO[q * n + i - 1], yq));
    }
    w = fp_sub(fp_sub(w, ypow[n + i]), ypow[n - i]);
    s[n - i] = u;
    s[n + i] = v;
    s[2 * n + i] = w;
  }
}
void s_of_y_enqueue(hipStream_t st, const Fr* wL, const Fr* wR, const Fr* wO, const Fr* ypow, long n, long Q, Fr* s) {
  LAUNCH(k_s_of_y, elementwise_grid(n + 1), 256, 0, st, wL, wR, wO, ypow, n, Q, s);
}

// s(X,Y) = sum_q Y^{n+q} P_q(X) + sum_i (-Y^i - Y^{-i}) X^{i+n}  with  P_q(X) = sum_i wL[q][i] X^{-i} + wR[q][i] X^i + wO[q][i] X^{i+n}
// (Constraints.hs:34-53, regrouped by constraint).  P_q depends on the circuit only, so Commit(P_q) is computed once per
// prover handle and Commit(s(X,y)) = sum_q y^{n+q} Commit(P_q) + Commit(diagonal part): an n-term MSM instead of a 3n-term one.
__global__ __launch_bounds__(256) void k_weight_row_poly(const Fr* __restrict__ wL, const Fr* __restrict__ wR, const Fr* __restrict__ wO,
                                                         long n, long q, Fr* __restrict__ s) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x + 1;   // 1..n
  if (i > n) { if (i == n + 1) s[n] = Fr::zero(); return; }
  s[n - i] = wL[q * n + i - 1];
  s[n + i] = wR[q * n + i - 1];
  s[2 * n + i] = wO[q * n + i - 1];
}
void weight_row_poly_enqueue(hipStream_t st, const Fr* wL, const Fr* wR, const Fr* wO, long n, long q, Fr* s) {
  LAUNCH(k_weight_row_poly, ceil_div(n + 1, 256), 256, 0, st, wL, wR, wO, n, q, s);
}
// diag[i-1] = -(y^i + y^-i), i = 1..n (coefficients of X^{n+1..2n});  yq[q] = y^{n+1+q}
__global__ __launch_bounds__(256) void k_s_diag_part(const Fr* __restrict__ ypow, long n, long Q, Fr* __restrict__ diag, Fr* __restrict__ yq) {
  const long m = n > Q ? n : Q;
  for (long t = (long)blockIdx.x * 256 + threadIdx.x; t < m; t += (long)gridDim.x * 256) {
    if (t < n) diag[t] = fp_neg(fp_add(ypow[n + t + 1], ypow[n - t - 1]));
    if (t < Q) yq[t] = ypow[2 * n + 1 + t];
  }
}
void s_diag_part_enqueue(hipStream_t st, const Fr* ypow, long n, long Q, Fr* diag, Fr* yq) {
  LAUNCH(k_s_diag_part, elementwise_grid(n > Q ? n : Q), 256, 0, st, ypow, n, Q, diag, yq);
}

// s(u,Y) over [-n, n+Q] given upow[e + n] = u^e for e in [-n, 2n]:
//   Y^{+-i}: -u^{i+n};  Y^{n+q}: sum_i u^-i wL[q][i] + u^i wR[q][i] + u^{i+n} wO[q][i]   (Utils.hs:17-18)
__global__ __launch_bounds__(256) void k_s_of_u_diag(const Fr* __restrict__ upow, long n, Fr* __restrict__ s) {
  for (long i = (long)blockIdx.x * 256 + threadIdx.x + 1; i <= n + 1; i += (long)gridDim.x * 256) {
    if (i > n) { s[n] = Fr::zero(); break; }
    const Fr v = fp_neg(upow[2 * n + i]);
    s[n - i] = v;
    s[n + i] = v;
  }
}
// grid (blocks, Q): partial[q * nblk + blk] = sum over the block's i
__global__ __launch_bounds__(256) void k_s_of_u_rows(const Fr* __restrict__ wL, const Fr* __restrict__ wR, const Fr* __restrict__ wO,
                                                     const Fr* __restrict__ upow, long n, Fr* __restrict__ partial) {
  __shared__ Fr sh[256];
  const long q = blockIdx.y;
  Fr acc = Fr::zero();
  for (long i = (long)blockIdx.x * 256 + threadIdx.x + 1; i <= n; i += (long)gridDim.x * 256) {
    acc = fp_add(acc, fp_mul(upow[n - i], wL[q * n + i - 1]));
    acc = fp_add(acc, fp_mul(upow[n + i], wR[q * n + i - 1]));
    acc = fp_add(acc, fp_mul(upow[2 * n + i], wO[q * n + i - 1]));
  }
  sh[threadIdx.x] = acc;
  __syncthreads();
  for (int o = 128; o >= 1; o >>= 1) {
    if ((int)threadIdx.x < o) sh[threadIdx.x] = fp_add(sh[threadIdx.x], sh[threadIdx.x + o]);
    __syncthreads();
  }
  if (threadIdx.x == 0) partial[q * gridDim.x + blockIdx.x] = sh[0];
}
__global__ __launch_bounds__(64) void k_s_of_u_finish(const Fr* __restrict__ partial, int nblk, long n, long Q, Fr* __restrict__ s) {
  const long q = (long)blockIdx.x * 64 + threadIdx.x;
  if (q >= Q) return;
  Fr acc = Fr::zero();
  for (int b = 0; b < nblk; b++) acc = fp_add(acc, partial[q * nblk + b]);
  s[2 * n + 1 + q] = acc;
}
void s_of_u_enqueue(hipStream_t st, const Fr* wL, const Fr* wR, const Fr* wO, const Fr* upow, long n, long Q, Fr* s, DevBuf& tmp) {
  LAUNCH(k_s_of_u_diag, elementwise_grid(n + 1), 256, 0, st, upow, n, s);
  int nblk = ceil_div(n, 256);
  if (nblk > 256) nblk = 256;
  if (n <= (1L << 17) && nblk > 64) nblk = 64;
  tmp.ensure(sizeof(Fr) * (size_t)nblk * Q);
  LAUNCH(k_s_of_u_rows, dim3(nblk, (unsigned)Q), 256, 0, st, wL, wR, wO, upow, n, tmp.as<Fr>());
  LAUNCH(k_s_of_u_finish, ceil_div(Q, 64), 64, 0, st, (const Fr*)tmp.as<Fr>(), nblk, n, Q, s);
}

// ---- the same two polynomials from sparse gate weights (csr.hpp: ONE CSR of 3Q rows, wL / wR / wO stacked) ----------------------------
// Work proportional to n + nnz instead of Q n.  Row r is row q = r mod Q of matrix r / Q.
__device__ __forceinline__ int csr_matrix(int r, int Q) { return r >= 2 * Q ? 2 : (r >= Q ? 1 : 0); }

// s(X,y) as k_s_of_y computes it, walking column i of the column-major copy: one thread per gate i, y^{n+1+q} gathered per entry --
// from LDS when the Q powers fit (stage != 0: Q * 32 bytes of dynamic LDS), else through L2
__global__ __launch_bounds__(256) void k_s_of_y_csc(const int32_t* __restrict__ col_ptr, const int32_t* __restrict__ row, const Fr* __restrict__ val,
                                                    const Fr* __restrict__ ypow, long n, int Q, int stage, Fr* __restrict__ s) {
  extern __shared__ uint32_t yq_lds[];
  const Fr* yq = ypow + 2 * n + 1;                           // y^{n+1+q}, q = 0..Q-1
  if (stage) {
    Fr* sh = reinterpret_cast<Fr*>(yq_lds);
    for (int q = threadIdx.x; q < Q; q += 256) sh[q] = yq[q];
    __syncthreads();
    yq = sh;
  }
  for (long i = (long)blockIdx.x * 256 + threadIdx.x + 1; i <= n + 1; i += (long)gridDim.x * 256) {   // 1..n
    if (i > n) { s[n] = Fr::zero(); break; }                 // X^0 slot
    Fr u = Fr::zero(), v = Fr::zero(), w = Fr::zero();     // (three named sums, not an array indexed by the matrix: that would live in scratch)
    const int k1 = col_ptr[i];
    for (int k = col_ptr[i - 1]; k < k1; k++) {
      const int r = row[k], m = csr_matrix(r, Q);
      const Fr x = fp_mul(val[k], yq[r - m * Q]);
      if (m == 0) u = fp_add(u, x);
      else if (m == 1) v = fp_add(v, x);
      else w = fp_add(w, x);
    }
    s[n - i] = u;
    s[n + i] = v;
    s[2 * n + i] = fp_sub(fp_sub(w, ypow[n + i]), ypow[n - i]);
  }
}
void s_of_y_csc_enqueue(hipStream_t st, const int32_t* col_ptr, const int32_t* row, const Fr* val, const Fr* ypow, long n, long Q, Fr* s) {
  const int stage = Q <= 1024 ? 1 : 0;
  LAUNCH(k_s_of_y_csc, elementwise_grid(n + 1), 256, stage ? (unsigned)(sizeof(Fr) * Q) : 0u, st, col_ptr, row, val, ypow, n, (int)Q, stage, s);
}

// s(u,Y)'s coefficients of Y^{n+1+q} = sum over rows q, Q + q, 2Q + q of val * u^{-i | i | i+n}.  Rows are as skewed as circuits are
// (rndCircuit: one row of n entries per matrix, every other row empty), so they are cut into chunks of CSR_CHUNK entries
// (csr.hpp): one wave per chunk, 8 entries per lane, a shuffle reduction in Fr, one partial per chunk -- and k_s_of_u_csr_finish
// adds each q's partials in chunk order.  No atomics: the sums are exact and come out the same whatever the schedule.
__device__ __forceinline__ Fr fr_shfl_xor(const Fr& a, int mask) {
  Fr o;
#pragma unroll
  for (int k = 0; k < 8; k++) o.l[k] = (uint32_t)__shfl_xor((int)a.l[k], mask, 64);
  return o;
}
__global__ __launch_bounds__(256) void k_s_of_u_csr(const int32_t* __restrict__ row_ptr, const int32_t* __restrict__ col, const Fr* __restrict__ val,
                                                    const int32_t* __restrict__ chunk_row, const int32_t* __restrict__ chunk_begin, long nchunks,
                                                    const Fr* __restrict__ upow, long n, int Q, Fr* __restrict__ partial) {
  const long c = (long)blockIdx.x * 4 + (threadIdx.x >> 6);  // one wave per chunk
  const int lane = threadIdx.x & 63;
  if (c >= nchunks) return;                                  // (wave-uniform: no barrier below)
  const int r = chunk_row[c], m = csr_matrix(r, Q);
  const int k0 = chunk_begin[c];
  const int k1 = min(k0 + CSR_CHUNK, row_ptr[r + 1]);
  // u^-i = upow[n - i], u^i = upow[n + i], u^{i+n} = upow[2n + i], i = column + 1
  const long base = m == 0 ? n - 1 : (m == 1 ? n + 1 : 2 * n + 1);
  const long sign = m == 0 ? -1 : 1;
  Fr acc = Fr::zero();
  for (int k = k0 + lane; k < k1; k += 64) acc = fp_add(acc, fp_mul(val[k], upow[base + sign * col[k]]));
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) acc = fp_add(acc, fr_shfl_xor(acc, o));
  if (lane == 0) partial[c] = acc;
}
// grid Q: s[2n + 1 + q] = the partials of rows q, Q + q, 2Q + q
__global__ __launch_bounds__(256) void k_s_of_u_csr_finish(const int32_t* __restrict__ row_chunk, const Fr* __restrict__ partial, long n, int Q, Fr* __restrict__ s) {
  __shared__ Fr sh[256];
  const int q = blockIdx.x;
  Fr acc = Fr::zero();
  for (int m = 0; m < 3; m++) {
    const int r = m * Q + q;
    for (int c = row_chunk[r] + threadIdx.x; c < row_chunk[r + 1]; c += 256) acc = fp_add(acc, partial[c]);
  }
  sh[threadIdx.x] = acc;
  __syncthreads();
  for (int o = 128; o >= 1; o >>= 1) {
    if ((int)threadIdx.x < o) sh[threadIdx.x] = fp_add(sh[threadIdx.x], sh[threadIdx.x + o]);
    __syncthreads();
  }
  if (threadIdx.x == 0) s[2 * n + 1 + q] = sh[0];
}
void s_of_u_csr_enqueue(hipStream_t st, const int32_t* row_ptr, const int32_t* col, const Fr* val, const int32_t* chunk_row, const int32_t* chunk_begin,
                        long nchunks, const int32_t* row_chunk, const Fr* upow, long n, long Q, Fr* s, Fr* partial) {
  LAUNCH(k_s_of_u_diag, elementwise_grid(n + 1), 256, 0, st, upow, n, s);
  if (nchunks > 0) LAUNCH(k_s_of_u_csr, ceil_div(nchunks, 4L), 256, 0, st, row_ptr, col, val, chunk_row, chunk_begin, nchunks, upow, n, (int)Q, partial);
  LAUNCH(k_s_of_u_csr_finish, (unsigned)Q, 256, 0, st, row_chunk, (const Fr*)partial, n, (int)Q, s);
}

// the terms of P_q (sonic_prover_prepare on a sparse handle): rows q, Q + q, 2Q + q of the CSR at X^{-i}, X^{i}, X^{i+n}, gathered as
// (alpha-basis point, Montgomery value) pairs for a plain MSM over nnz_q terms.  A: the alpha basis positioned at exponent 0.
__global__ __launch_bounds__(256) void k_csr_row_terms(const int32_t* __restrict__ col, const Fr* __restrict__ val, int b0, int l0, int b1, int l1, int b2, int l2,
                                                       long n, PointArray A, G1Affine* __restrict__ pts, Fr* __restrict__ scal) {
  const long t = (long)blockIdx.x * 256 + threadIdx.x;
  if (t >= (long)l0 + l1 + l2) return;
  long k, e;
  if (t < l0) { k = b0 + t; e = -(long)(col[k] + 1); }
  else if (t < (long)l0 + l1) { k = b1 + (t - l0); e = col[k] + 1; }
  else { k = b2 + (t - l0 - l1); e = col[k] + 1 + n; }
  pts[t] = (A + e)[0];
  scal[t] = val[k];
}
void csr_row_terms_enqueue(hipStream_t st, const int32_t* col, const Fr* val, const int32_t seg[6], long n, PointArray A, G1Affine* pts, Fr* scal) {
  const long total = (long)seg[1] + seg[3] + seg[5];
  if (total > 0) LAUNCH(k_csr_row_terms, ceil_div(total, 256L), 256, 0, st, col, val, seg[0], seg[1], seg[2], seg[3], seg[4], seg[5], n, A, pts, scal);
}

// The two operands of t(X,y)'s product (Constraints.hs:56-65 with Y := y) in ONE launch: fa = r(X,1) and fb = r(X,y) + s(X,y), both over
// M transform points from exponent r_lo, zero beyond their coefficients.  (Two memsets of M elements, a copy, a scale-by-powers and an
// add-into before: five launches at the head of the longest dependent chain of a proof, each of which waits for wave slots when another
// proof's accumulation is running.)
__global__ __launch_bounds__(256) void k_t_operands(const Fr* __restrict__ r1, long r_len, long r_lo, const Fr* __restrict__ sy, long s_off, long s_len,
                                                    const Fr* __restrict__ ypair, Fr* __restrict__ fa, Fr* __restrict__ fb, long M, int PER) {
  const long base = (long)blockIdx.x * (256 * PER) + threadIdx.x;
  if (base >= M) return;
  Fr p = Fr::zero(), step = Fr::zero();
  if (base < r_len) {                                      // (r(X,y) = c_e y^e on the diagonal: Utils.hs:20-21)
    const Fr y = ypair[0], yinv = ypair[1];
    const long e = r_lo + base;
    p = e >= 0 ? fp_pow_u64(y, (uint64_t)e) : fp_pow_u64(yinv, (uint64_t)(-e));
    step = fp_pow_u64(y, 256);
  }
#pragma unroll 1
  for (int k = 0; k < PER; k++) {
    const long i = base + (long)k * 256;
    if (i >= M) break;
    Fr a = Fr::zero(), b = Fr::zero();
    if (i < r_len) { a = r1[i]; b = fp_mul(a, p); p = fp_mul(p, step); }
    if (i >= s_off && i < s_off + s_len) b = fp_add(b, sy[i - s_off]);
    fa[i] = a;
    fb[i] = b;
  }
}
void t_operands_enqueue(hipStream_t st, const Fr* r1, long r_len, long r_lo, const Fr* sy, long s_off, long s_len, const Fr* ypair, Fr* fa, Fr* fb, long M) {
  const int per = scale_per(M);
  LAUNCH(k_t_operands, ceil_div(M, 256L * per), 256, 0, st, r1, r_len, r_lo, sy, s_off, s_len, ypair, fa, fb, M, per);
}

// dst[off + i] += src[i]
__global__ __launch_bounds__(256) void k_add_into(Fr* __restrict__ dst, const Fr* __restrict__ src, long n) {
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long)gridDim.x * 256) dst[i] = fp_add(dst[i], src[i]);
}
void add_into_enqueue(hipStream_t st, Fr* dst, const Fr* src, long n) { if (n > 0) LAUNCH(k_add_into, elementwise_grid(n), 256, 0, st, dst, src, n); }

// *slot -= sum_q cs[q] * ypow_nq[q]   (k(y), Constraints.hs:67-68), then flags[flag_bit] if *slot != 0
__global__ __launch_bounds__(256) void k_sub_k_of_y(Fr* __restrict__ slot, const Fr* __restrict__ cs, const Fr* __restrict__ ypow_nq, long Q, int* flags, int flag_bit) {
  __shared__ Fr sh[256];
  Fr acc = Fr::zero();
  for (long q = threadIdx.x; q < Q; q += 256) acc = fp_add(acc, fp_mul(cs[q], ypow_nq[q]));
  sh[threadIdx.x] = acc;
  __syncthreads();
  for (int o = 128; o >= 1; o >>= 1) {
    if ((int)threadIdx.x < o) sh[threadIdx.x] = fp_add(sh[threadIdx.x], sh[threadIdx.x + o]);
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    Fr v = fp_sub(*slot, sh[0]);
    *slot = v;
    if (!v.is_zero()) atomicOr(flags, flag_bit);
  }
}
// The same over many blocks (k_of_y_plan.hpp), for circuits with Q of the order of n: a compiled R1CS of m = 2^18 has Q = 3 * 2^18, which is
// ~3000 dependent products per thread of the one block above, on one CU, in front of the T commitment.  Stage 1: block b sums the terms
// of its span into partial[b] (no atomics on field elements: every partial has one writer).  Stage 2: one block sums the partials --
// looping when there are more than 256 -- subtracts from the slot and raises the flag exactly as k_sub_k_of_y does.  The sums are exact
// field sums, so the slot's value does not depend on the plan.
__global__ __launch_bounds__(K_OF_Y_BLOCK) void k_k_of_y_partials(const Fr* __restrict__ cs, const Fr* __restrict__ ypow_nq, long Q, KOfYPlan plan, Fr* __restrict__ partial) {
  __shared__ Fr sh[K_OF_Y_BLOCK];
  long lo, hi;
  k_of_y_span(plan, Q, (long)blockIdx.x, &lo, &hi);
  Fr acc = Fr::zero();
  for (long q = lo + threadIdx.x; q < hi; q += K_OF_Y_BLOCK) acc = fp_add(acc, fp_mul(cs[q], ypow_nq[q]));
  sh[threadIdx.x] = acc;
  __syncthreads();
  for (int o = K_OF_Y_BLOCK / 2; o >= 1; o >>= 1) {
    if ((int)threadIdx.x < o) sh[threadIdx.x] = fp_add(sh[threadIdx.x], sh[threadIdx.x + o]);
    __syncthreads();
  }
  if (threadIdx.x == 0) partial[blockIdx.x] = sh[0];
}
__global__ __launch_bounds__(K_OF_Y_BLOCK) void k_k_of_y_finish(Fr* __restrict__ slot, const Fr* __restrict__ partial, long blocks, int* flags, int flag_bit) {
  __shared__ Fr sh[K_OF_Y_BLOCK];
  Fr acc = Fr::zero();
  for (long b = threadIdx.x; b < blocks; b += K_OF_Y_BLOCK) acc = fp_add(acc, partial[b]);
  sh[threadIdx.x] = acc;
  __syncthreads();
  for (int o = K_OF_Y_BLOCK / 2; o >= 1; o >>= 1) {
    if ((int)threadIdx.x < o) sh[threadIdx.x] = fp_add(sh[threadIdx.x], sh[threadIdx.x + o]);
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    Fr v = fp_sub(*slot, sh[0]);
    *slot = v;
    if (!v.is_zero()) atomicOr(flags, flag_bit);
  }
}
// Which form a proof over Q constraints takes: one block below the threshold (blocks = 0: small circuits launch exactly what they always
// launched), spans of K_OF_Y_SPAN_DEFAULT terms from it on.  SONIC_K_OF_Y_SPLIT=<Q> sets the threshold (0: never split),
// SONIC_K_OF_Y_SPAN=<q per block> the span: read per call like the SONIC_PROVE_* knobs, because the tests switch them inside one process.
// The default threshold is K_OF_Y_SPLIT_DEFAULT (poly.hpp, with the measurement behind it).
KOfYPlan k_of_y_choose(long Q) {
  const char* te = getenv("SONIC_K_OF_Y_SPLIT");
  const char* se = getenv("SONIC_K_OF_Y_SPAN");
  const long threshold = te ? atol(te) : K_OF_Y_SPLIT_DEFAULT;
  const long span = se && atol(se) >= 1 ? atol(se) : K_OF_Y_SPAN_DEFAULT;
  if (threshold <= 0 || Q < threshold) return KOfYPlan();
  return k_of_y_plan(Q, span);
}
void sub_k_of_y_enqueue(hipStream_t st, Fr* slot, const Fr* cs, const Fr* ypow_nq, long Q, int* flags, int flag_bit, const KOfYPlan& plan, Fr* partial) {
  if (plan.blocks <= 0) {
    LAUNCH(k_sub_k_of_y, 1, 256, 0, st, slot, cs, ypow_nq, Q, flags, flag_bit);
    return;
  }
  LAUNCH(k_k_of_y_partials, (unsigned)plan.blocks, K_OF_Y_BLOCK, 0, st, cs, ypow_nq, Q, plan, partial);
  LAUNCH(k_k_of_y_finish, 1, K_OF_Y_BLOCK, 0, st, slot, partial, plan.blocks, flags, flag_bit);
}

// flags |= bit if any of a[0..n) is non-zero
__global__ __launch_bounds__(256) void k_flag_nonzero(const Fr* __restrict__ a, long n, int* flags, int bit) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i < n && !a[i].is_zero()) atomicOr(flags, bit);
}
void flag_nonzero_enqueue(hipStream_t st, const Fr* a, long n, int* flags, int bit) {
  if (n > 0) LAUNCH(k_flag_nonzero, ceil_div(n, 256), 256, 0, st, a, n, flags, bit);
}

// ---- runs of equal coefficients (round 5) ---------------------------------------------------------------------------------------
// commitPoly of a coefficient vector that holds RUNS of one value c -- s(X, y_j) of a circuit whose weight rows repeat a value: n copies
// of two values among 3n + 1 coefficients for the reference's rndCircuit (test/Test/Reference.hs:141-155) -- needs only the two ends of a
// run: c (A[a] + ... + A[b]) = c ps[b] - c ps[a - 1] with the running sums ps of the basis (srs.hip).  Runs are found tile by tile
// (RUN_TILE consecutive coefficients all equal and non-zero); a tile's coefficients are zeroed in the copy the large MSM reads, and the
// tile contributes its closing term (+c, ps[last]) unless the next tile continues the run and its opening term (-c, ps[first - 1])
// unless the previous one does: 2 * ntiles slots, zero scalars where nothing is emitted, for one small MSM over gathered points.
__global__ __launch_bounds__(RUN_TILE) void k_run_tiles(const Fr* __restrict__ poly, long len, Fr* __restrict__ masked, Fr* __restrict__ val,
                                                       uint32_t* __restrict__ uniform, long ntiles) {
  __shared__ Fr first;
  const long t = blockIdx.x, i = t * RUN_TILE + threadIdx.x;
  const bool in = i < len;
  const Fr v = in ? poly[i] : Fr::zero();
  if (threadIdx.x == 0) first = v;
  __syncthreads();
  const Fr f = first;
  bool eq = in;
#pragma unroll
  for (int k = 0; k < 8; k++) eq = eq && v.l[k] == f.l[k];
  const bool uni = __syncthreads_and(eq ? 1 : 0) != 0 && !f.is_zero();
  if (in) masked[i] = uni ? Fr::zero() : v;
  if (threadIdx.x == 0 && t < ntiles) { uniform[t] = uni ? 1u : 0u; val[t] = f; }
}
__device__ __forceinline__ bool fr_same(const Fr& a, const Fr& b) {
  bool eq = true;
#pragma unroll
  for (int k = 0; k < 8; k++) eq = eq && a.l[k] == b.l[k];
  return eq;
}
// ps: the running sums, positioned at the point of coefficient 0; ps_first: that point's index in the table (no ps[-1] at index 0)
__global__ __launch_bounds__(256) void k_run_terms(const Fr* __restrict__ val, const uint32_t* __restrict__ uniform, long ntiles, PointArray ps,
                                                   long ps_first, Fr* __restrict__ scal, G1Affine* __restrict__ pts) {
  const long t = (long)blockIdx.x * 256 + threadIdx.x;
  if (t >= ntiles) return;
  Fr s_close = Fr::zero(), s_open = Fr::zero();
  G1Affine p_close = G1Affine::inf(), p_open = G1Affine::inf();
  if (uniform[t]) {
    const Fr v = val[t];
    const bool cont_next = t + 1 < ntiles && uniform[t + 1] && fr_same(val[t + 1], v);
    const bool cont_prev = t > 0 && uniform[t - 1] && fr_same(val[t - 1], v);
    if (!cont_next) { s_close = v; p_close = ps[(size_t)((t + 1) * RUN_TILE - 1)]; }
    if (!cont_prev && ps_first + t * RUN_TILE > 0) { s_open = fp_neg(v); p_open = (ps + (t * RUN_TILE - 1))[0]; }
  }
  scal[2 * t] = s_close; scal[2 * t + 1] = s_open;
  pts[2 * t] = p_close; pts[2 * t + 1] = p_open;
}
void run_tiles_enqueue(hipStream_t st, const Fr* poly, long len, Fr* masked, Fr* val, uint32_t* uniform) {
  if (len <= 0) return;
  LAUNCH(k_run_tiles, ceil_div(len, (long)RUN_TILE), RUN_TILE, 0, st, poly, len, masked, val, uniform, len / RUN_TILE);
}
void run_terms_enqueue(hipStream_t st, const Fr* val, const uint32_t* uniform, long ntiles, PointArray ps, long ps_first, Fr* scal, G1Affine* pts) {
  if (ntiles > 0) LAUNCH(k_run_terms, ceil_div(ntiles, 256L), 256, 0, st, val, uniform, ntiles, ps, ps_first, scal, pts);
}

// small scalar prep: out = {v, v^-1} for each of k inputs (Montgomery in, Montgomery out); 0^-1 := 0
__global__ __launch_bounds__(64) void k_fr_with_inverse(const Fr* __restrict__ in, int k, Fr* __restrict__ out) {
  int i = blockIdx.x * 64 + threadIdx.x;
  if (i >= k) return;
  Fr v = in[i];
  out[2 * i] = v;
  out[2 * i + 1] = v.is_zero() ? v : fp_inv(v);
}
void fr_with_inverse_enqueue(hipStream_t st, const Fr* in, int k, Fr* out) { LAUNCH(k_fr_with_inverse, ceil_div(k, 64), 64, 0, st, in, k, out); }

__global__ void k_fr_mul_scalar(const Fr* a, const Fr* b, Fr* out) { *out = fp_mul(*a, *b); }
void fr_mul_scalar_enqueue(hipStream_t st, const Fr* a, const Fr* b, Fr* out) { LAUNCH(k_fr_mul_scalar, 1, 1, 0, st, a, b, out); }

// sparse (sorted by exponent) -> dense: run heads sum their run
__global__ __launch_bounds__(256) void k_sparse_to_dense(const int64_t* __restrict__ exps, const Fr* __restrict__ coeffs, long nt, long lo, Fr* __restrict__ dense) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= nt) return;
  if (i > 0 && exps[i - 1] == exps[i]) return;
  Fr acc = coeffs[i];
  for (long j = i + 1; j < nt && exps[j] == exps[i]; j++) acc = fp_add(acc, coeffs[j]);
  dense[exps[i] - lo] = acc;
}
void sparse_to_dense_enqueue(hipStream_t st, const int64_t* exps, const Fr* coeffs, long nt, long lo, Fr* dense) {
  if (nt > 0) LAUNCH(k_sparse_to_dense, ceil_div(nt, 256), 256, 0, st, exps, coeffs, nt, lo, dense);
}


// out[i] = c[i] * b^{e[i]} for the terms of a sparse polynomial (e may be negative: pair = {b, b^-1}): one variable of a sparse
// bivariate Laurent polynomial substituted (evalX / evalY, Utils.hs:17-21, on poly's sparse form)
__global__ __launch_bounds__(256) void k_scale_terms(const int64_t* __restrict__ e, const Fr* __restrict__ c, long nt, const Fr* __restrict__ pair, Fr* __restrict__ out) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= nt) return;
  const int64_t ex = e[i];
  const Fr base = ex >= 0 ? pair[0] : pair[1];
  out[i] = fp_mul(c[i], fp_pow_u64(base, (uint64_t)(ex >= 0 ? ex : -ex)));
}
void scale_terms_enqueue(hipStream_t st, const int64_t* e, const Fr* c, long nt, const Fr* pair, Fr* out) {
  if (nt > 0) LAUNCH(k_scale_terms, ceil_div(nt, 256), 256, 0, st, e, c, nt, pair, out);
}

}  // namespace sonic
