// Multi-scalar multiplication on the twist: the bucket method over G2 (g2.hpp), and its entry points of the C ABI (include/sonic_hip.h,
// sonic_msm_g2*).  One chain per slab of G2_MSM_SLAB terms:
//   1. digits and sort: msm.hip's, under a no-table plan (msm_sort_enqueue) -- entries grouped by (window, bucket), off[] per bucket
//   2. k_g2_chunk_count + scan: ceil(len / G2_WALK_MAX) chunks per bucket, their running count = the first chunk of every bucket
//   3. k_g2_bucket_accum: one thread per chunk walks its entries with mixed additions, accumulator in registers
//   4. k_g2_bucket_combine: one thread per bucket adds the bucket's partial sums (one, usually)
//   5. k_g2_bucket_segments: running sums over segments of K buckets, sum_i i B_i = sum_s (s K T_s + sum_j j B_{sK+j})
//   6. k_g2_sum (srs_g2.hip) over the W ranges of segment results: the W window sums, canonical
// and the host folds the window sums by Horner (msm_g2_host.hpp) and adds the slabs.
#include <string.h>
#include <vector>
#include "srs_handle.hpp"
#include "msm_g2.hpp"
#include "compress.hpp"

namespace sonic {

// nchunk[b] for the M buckets, and a zero behind them so that the exclusive scan over M + 1 words ends in the total
__global__ __launch_bounds__(256) void k_g2_chunk_count(const uint32_t* __restrict__ off, uint32_t M, uint32_t* __restrict__ nchunk) {
  const uint32_t b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b > M) return;
  nchunk[b] = b < M ? g2_chunks(off[b + 1] - off[b]) : 0u;
}

// One thread per chunk t < chunk_off[M] (the grid is sized for the most there can be).  Its bucket is the last b with chunk_off[b] <= t:
// empty buckets repeat their successor's offset, so that b is never empty.  The accumulator stays in registers.  g2_add_mixed handles the
// accumulator or the point at infinity and P + P / P - P.  The entry and its point are loaded where they are used: carrying the next
// entry across the addition (a one-deep prefetch) made the compiler spill 52 bytes per lane, and the dependent pair of loads is a few
// per cent of an addition that runs some thousand instructions.
__global__ __launch_bounds__(64, 1) void k_g2_bucket_accum(const G2Affine* __restrict__ pts, const uint32_t* __restrict__ entries, const uint32_t* __restrict__ off,
                                                           const uint32_t* __restrict__ chunk_off, uint32_t M, G2Jac* __restrict__ partial) {
  const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= chunk_off[M]) return;
  uint32_t lo = 0, hi = M;                  // chunk_off[lo] <= t < chunk_off[hi]
  while (hi - lo > 1) {
    const uint32_t mid = lo + ((hi - lo) >> 1);
    if (chunk_off[mid] <= t) lo = mid; else hi = mid;
  }
  const uint32_t first = off[lo];
  const G2ChunkRange r = g2_chunk_range(first, off[lo + 1] - first, t - chunk_off[lo]);
  G2Jac acc = G2Jac::inf();
#pragma unroll 1
  for (uint32_t e = r.beg; e < r.end; e++) {
    const uint32_t e_cur = entries[e];
    G2Affine p = pts[e_cur & 0x7fffffffu];
    if (e_cur >> 31) p.y = f2_neg(p.y);                  // (bit 31 of an entry: the digit's sign)
    acc = g2_add_mixed(acc, p);
  }
  partial[t] = acc;
}

__global__ __launch_bounds__(64, 1) void k_g2_bucket_combine(const G2Jac* __restrict__ partial, const uint32_t* __restrict__ chunk_off, uint32_t M,
                                                             G2Jac* __restrict__ buckets) {
  const uint32_t b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= M) return;
  const uint32_t beg = chunk_off[b], end = chunk_off[b + 1];
  G2Jac acc = G2Jac::inf();
#pragma unroll 1
  for (uint32_t t = beg; t < end; t++) acc = g2_add(acc, partial[t]);          // (the first addition meets infinity and returns at once)
  buckets[b] = acc;
}

// One thread per (window, segment): over the segment's K buckets, from the top, run += B and acc += run leave run = T, the segment's
// total, and acc = sum_j j B_j (j = 1 .. K).  The segment starts s K buckets up, which adds (s K) T: a double-and-add over the c - 1 bits
// of s K < 2^(c-1).  acc waits for that multiple in segres[t], not in registers -- three live points spilled 240 bytes per lane -- and
// the compiler barrier keeps it from carrying the stored value across.
__global__ __launch_bounds__(64, 1) void k_g2_bucket_segments(const G2Jac* __restrict__ buckets, int W, int NB, int K, int nseg, int c, G2Jac* __restrict__ segres) {
  const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= (uint32_t)W * (uint32_t)nseg) return;
  const uint32_t w = t / (uint32_t)nseg, s = t % (uint32_t)nseg;
  const G2Jac* __restrict__ B = buckets + (size_t)w * NB + (size_t)s * K;
  G2Jac run = G2Jac::inf();
  {
    G2Jac acc = G2Jac::inf();
#pragma unroll 1
    for (int j = K - 1; j >= 0; j--) {
      run = g2_add(run, B[j]);
      acc = g2_add(acc, run);
    }
    segres[t] = acc;
  }
  const uint32_t m = s * (uint32_t)K;
  if (m) {
    G2Jac up = G2Jac::inf();
#pragma unroll 1
    for (int bit = c - 2; bit >= 0; bit--) {
      up = g2_dbl(up);
      if ((m >> bit) & 1u) up = g2_add(up, run);
    }
    asm volatile("" ::: "memory");
    segres[t] = g2_add(segres[t], up);
  }
}

__global__ __launch_bounds__(64, 1) void k_g2_msm_points_from_bytes(const uint8_t* __restrict__ in, G2Affine* __restrict__ out, long n, int* err) {
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
  if (!nz) { out[i] = G2Affine::inf(); return; }          // the neutral element of a sum (no point of the twist has x = y = 0)
  p.x.c0 = fp_to_mont(p.x.c0); p.x.c1 = fp_to_mont(p.x.c1); p.y.c0 = fp_to_mont(p.y.c0); p.y.c1 = fp_to_mont(p.y.c1);
  if (!(f2_sqr(p.y) == g2_curve_rhs(p.x))) { atomicOr(err, 2); out[i] = G2Affine::inf(); return; }
  out[i] = p;
}
void g2_msm_points_from_bytes_enqueue(hipStream_t st, const uint8_t* d_in, G2Affine* out, long n, int* d_err) {
  if (n > 0) LAUNCH(k_g2_msm_points_from_bytes, ceil_div(n, 64), 64, 0, st, d_in, out, n, d_err);
}

void g2_msm_blocking(hipStream_t st, MsmWorkspace& ws, const G2Affine* pts, const Fr* d_scalars, long n, int bits, bool fold, uint8_t out192[192]) {
  struct Slab { int c, W; size_t at; };
  std::vector<Slab> slabs;
  const int nslabs = ceil_div(n, G2_MSM_SLAB);
  ws.g2_wsum.ensure(sizeof(G2Jac) * (size_t)MSM_MAX_WINDOWS * nslabs);
  size_t at = 0;
  for (long base = 0; base < n; base += G2_MSM_SLAB) {
    const long m = n - base < G2_MSM_SLAB ? n - base : G2_MSM_SLAB;
    const int wo = msm_window_override();
    const int c = wo >= 4 && wo <= 16 ? wo : g2_msm_window_bits(m);
    const MsmPlan pl = msm_plan_windows(m, c, bits, fold);
    msm_sort_enqueue(st, ws, pl, d_scalars + base, m, false);
    const uint32_t M = (uint32_t)pl.W * (uint32_t)pl.NB;
    const size_t NW = (size_t)m * pl.W;
    // every non-empty bucket has at most len / G2_WALK_MAX + 1 chunks
    const size_t max_chunks = (M < NW ? M : NW) + NW / G2_WALK_MAX + 1;
    ws.g2_nchunk.ensure(4 * ((size_t)M + 1));
    ws.g2_chunk_off.ensure(4 * ((size_t)M + 1));
    ws.g2_scan_tmp.ensure(4 * ((size_t)scan_u32_tiles((size_t)M + 1) + 1));
    ws.g2_partial.ensure(sizeof(G2Jac) * max_chunks);
    ws.g2_buckets.ensure(sizeof(G2Jac) * (size_t)M);
    ws.g2_segres.ensure(sizeof(G2Jac) * (size_t)pl.W * pl.nseg);
    ws.g2_sum_tmp.ensure(sizeof(G2Jac) * (size_t)pl.W * G2_SUM_RANGE_BLOCKS);
    const uint32_t* off = ws.off.as<uint32_t>();
    const uint32_t* chunk_off = ws.g2_chunk_off.as<uint32_t>();
    LAUNCH(k_g2_chunk_count, ceil_div((long)M + 1, 256), 256, 0, st, off, M, ws.g2_nchunk.as<uint32_t>());
    scan_u32_enqueue(st, ws.g2_nchunk.as<uint32_t>(), (size_t)M + 1, ws.g2_chunk_off.as<uint32_t>(), ws.g2_scan_tmp.as<uint32_t>());
    LAUNCH(k_g2_bucket_accum, ceil_div((long)max_chunks, 64), 64, 0, st, pts + base, (const uint32_t*)ws.entries.as<uint32_t>(), off, chunk_off, M,
           ws.g2_partial.as<G2Jac>());
    LAUNCH(k_g2_bucket_combine, ceil_div((long)M, 64), 64, 0, st, (const G2Jac*)ws.g2_partial.as<G2Jac>(), chunk_off, M, ws.g2_buckets.as<G2Jac>());
    LAUNCH(k_g2_bucket_segments, ceil_div((long)pl.W * pl.nseg, 64), 64, 0, st, (const G2Jac*)ws.g2_buckets.as<G2Jac>(), pl.W, pl.NB, pl.K, pl.nseg, pl.c,
           ws.g2_segres.as<G2Jac>());
    g2_sum_ranges_enqueue(st, ws.g2_segres.as<G2Jac>(), (long)pl.nseg, pl.W, (long)pl.nseg, ws.g2_sum_tmp.as<G2Jac>(), ws.g2_wsum.as<G2Jac>() + at);
    slabs.push_back(Slab{pl.c, pl.W, at});
    at += (size_t)pl.W;
  }
  std::vector<G2Jac> h(at);
  HIP_OK(hipMemcpyAsync(h.data(), ws.g2_wsum.p, sizeof(G2Jac) * at, hipMemcpyDeviceToHost, st));
  HIP_OK(hipStreamSynchronize(st));
  G2Jac acc = G2Jac::inf();
  for (const Slab& s : slabs) acc = g2_add(acc, g2_msm_fold_windows(h.data() + s.at, s.W, s.c));
  uint32_t w[48];
  g2_canonical_words(g2_to_affine(acc), w);
  memcpy(out192, w, 192);
}

}  // namespace sonic

using namespace sonic;

// the G2 elements of exponents [e0, e0 + n) of a basis, n > 0 and the range inside [-d, d]; a view holds two elements per basis and nothing else
static const G2Affine* srs_g2_range(const char* who, const sonic_srs_t* srs, int basis, int64_t e0, int64_t n) {
  const G2Affine* h = (basis ? srs->ha : srs->h).as<G2Affine>();
  if (!srs->is_view()) return h + (e0 + srs->d);
  const SrsViewG2 q = srs_view_g2(srs->d, srs->view_n);
  if (n == 1 && e0 == q.e[basis][0]) return h;
  if (n == 1 && e0 == q.e[basis][1]) return h + 1;
  set_error("%s: exponent range [%ld, %ld] of basis %d is not held by this view of the SRS: it holds %ld and %ld", who, (long)e0, (long)(e0 + n - 1), basis,
            (long)q.e[basis][0], (long)q.e[basis][1]);
  throw HipFail{SONIC_ERR_INVALID_ARG};
}

static int msm_g2_srs_common(const sonic_srs_t* srs, int basis, int64_t e0, const void* d_scalars, const uint8_t* h_scalars, int64_t n, uint8_t* out192) {
  API_BEGIN_ON(srs_device(srs))
  if (!srs || n < 0 || !out192 || (basis != 0 && basis != 1) || (n > 0 && !d_scalars && !h_scalars)) { set_error("msm over the G2 half of an SRS: bad argument"); return SONIC_ERR_INVALID_ARG; }
  if (n == 0) { memset(out192, 0, 192); return SONIC_OK; }
  if (!srs_range_ok("msm over the G2 half of an SRS", srs, e0, n)) return SONIC_ERR_SRS_INDEX;
  {
    std::lock_guard<std::mutex> g(call_mutex());
    const int rc = srs_ensure_g2(srs, default_stream(), "msm over the G2 half of an SRS");
    if (rc) return rc;
  }
  const G2Affine* pts = srs_g2_range("msm over the G2 half of an SRS", srs, basis, e0, n);
  CallLease lease;
  hipStream_t st = lease.st();
  DevBuf sc, err(4);
  const Fr* dsc = static_cast<const Fr*>(d_scalars);
  if (h_scalars) {
    sc.alloc(32 * (size_t)n);
    HIP_OK(hipMemcpyAsync(sc.p, h_scalars, 32 * (size_t)n, hipMemcpyHostToDevice, st));
    dsc = sc.as<Fr>();
  }
  HIP_OK(hipMemsetAsync(err.p, 0, 4, st));
  fr_check_enqueue(st, dsc, n, err.as<int>());
  if (read_flags(st, err)) { set_error("msm over the G2 half of an SRS: non-canonical scalar"); return SONIC_ERR_BAD_ENCODING; }
  // SRS elements are in the order-r subgroup: the fold is valid
  g2_msm_blocking(st, lease.ws(), pts, dsc, (long)n, 255, true, out192);
  API_END
}

extern "C" {

int sonic_msm_g2(const uint8_t* points, const uint8_t* scalars, int64_t n, uint8_t out_g2[192]) {
  API_BEGIN
  if (n < 0 || !out_g2 || (n > 0 && (!points || !scalars))) { set_error("sonic_msm_g2: bad argument"); return SONIC_ERR_INVALID_ARG; }
  if (n == 0) { memset(out_g2, 0, 192); return SONIC_OK; }
  CallLease lease;
  hipStream_t st = lease.st();
  DevBuf raw(192 * (size_t)n), pts(sizeof(G2Affine) * (size_t)n), sc(32 * (size_t)n), err(4);
  HIP_OK(hipMemsetAsync(err.p, 0, 4, st));
  HIP_OK(hipMemcpyAsync(raw.p, points, 192 * (size_t)n, hipMemcpyHostToDevice, st));
  HIP_OK(hipMemcpyAsync(sc.p, scalars, 32 * (size_t)n, hipMemcpyHostToDevice, st));
  g2_msm_points_from_bytes_enqueue(st, raw.as<uint8_t>(), pts.as<G2Affine>(), (long)n, err.as<int>());
  fr_check_enqueue(st, sc.as<Fr>(), n, err.as<int>());
  if (read_flags(st, err)) { set_error("sonic_msm_g2: non-canonical input or point not on the twist"); return SONIC_ERR_BAD_ENCODING; }
  // caller-supplied points only have to be on the twist, whose group has a large cofactor: s P is the literal multiple, so no fold
  g2_msm_blocking(st, lease.ws(), pts.as<G2Affine>(), sc.as<Fr>(), (long)n, 256, false, out_g2);
  API_END
}

int sonic_msm_g2_srs(const sonic_srs_t* srs, int basis, int64_t e0, const uint8_t* scalars, int64_t n, uint8_t out_g2[192]) {
  return msm_g2_srs_common(srs, basis, e0, nullptr, scalars, n, out_g2);
}
int sonic_msm_g2_srs_dev(const sonic_srs_t* srs, int basis, int64_t e0, const void* d_scalars, int64_t n, uint8_t out_g2[192]) {
  return msm_g2_srs_common(srs, basis, e0, d_scalars, nullptr, n, out_g2);
}
int sonic_msm_g2_walk_max(void) { return G2_WALK_MAX; }

}  // extern "C"
