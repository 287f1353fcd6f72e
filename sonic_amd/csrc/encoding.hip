// Encodings at the boundary of libsonic_hip.so: canonical little-endian bytes <-> Montgomery form for G1 points and Fr elements, with the
// checks a caller's bytes get on the way in (canonical, on the curve, in the order-r subgroup), and the blocking MSM that ends in bytes.
// The kernels are private to this file: the SRS and MSM entry points launch them through the *_enqueue functions (internal.hpp).
#include <string.h>
#include "internal.hpp"

namespace sonic {

// inf_ok: index at which the point at infinity is accepted (-1: everywhere, as for the operands of sonic_msm_g1; -2: nowhere; an SRS has
// exactly one such slot, the omitted g^alpha); elsewhere infinity sets err bit 8 -- g^{x^e} and g^{alpha x^e} are never the
// identity for x, alpha != 0, and a zero-filled SRS must not pass for a valid one
__global__ __launch_bounds__(256) void k_points_from_bytes(const uint8_t* __restrict__ in, PointArrayMut out, long n, int* err, long inf_ok) {
  long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const uint32_t* w = reinterpret_cast<const uint32_t*>(in + 96 * i);
  G1Affine p;
  for (int k = 0; k < 12; k++) { p.x.l[k] = w[k]; p.y.l[k] = w[12 + k]; }
  if (!fp_is_canonical(p.x) || !fp_is_canonical(p.y)) { atomicOr(err, 1); out[i] = G1Affine::inf(); return; }   // before is_inf: (q, q) is not O
  if (p.is_inf()) { if (inf_ok != -1 && i != inf_ok) atomicOr(err, 8); out[i] = p; return; }
  p.x = fp_to_mont(p.x); p.y = fp_to_mont(p.y);
  Fq four = fp_dbl(fp_dbl(Fq::one()));
  if (fp_sqr(p.y) != fp_add(fp_mul(fp_sqr(p.x), p.x), four)) { atomicOr(err, 2); out[i] = G1Affine::inf(); return; }
  out[i] = p;
}
// r P == O for every point, by the endomorphism test (g1_in_subgroup, g1.hpp): SRS elements must lie in the order-r subgroup because
// MSMs over an SRS fold scalars with r P = O (msm.hpp).  Sets err bit 4 otherwise.
__global__ __launch_bounds__(256) void k_points_subgroup_check(PointArray in, long n, int* err) {
  long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const G1Affine p = in[i];
  if (p.is_inf()) return;
  if (!g1_in_subgroup(p)) atomicOr(err, 4);
}
__global__ __launch_bounds__(256) void k_points_to_bytes(PointArray in, uint8_t* __restrict__ out, long n) {
  long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  G1Affine p = in[i];
  uint32_t* w = reinterpret_cast<uint32_t*>(out + 96 * i);
  if (p.is_inf()) { for (int k = 0; k < 24; k++) w[k] = 0; return; }
  Fq x = fp_from_mont(p.x), y = fp_from_mont(p.y);
  for (int k = 0; k < 12; k++) { w[k] = x.l[k]; w[12 + k] = y.l[k]; }
}
__global__ __launch_bounds__(256) void k_fr_check(const Fr* __restrict__ in, long n, int* err) {
  long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  Fr a = in[i];
  if (!fp_is_canonical(a)) atomicOr(err, 1);
}
__global__ __launch_bounds__(256) void k_fr_to_mont(Fr* __restrict__ a, long n, int* err) {
  long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  Fr v = a[i];
  if (!fp_is_canonical(v)) { atomicOr(err, 1); return; }
  a[i] = fp_to_mont(v);
}
__global__ __launch_bounds__(256) void k_fr_from_mont(Fr* __restrict__ a, long n) {
  long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  a[i] = fp_from_mont(a[i]);
}

void fr_to_mont_enqueue(hipStream_t st, Fr* d, long n, int* d_err) { if (n > 0) LAUNCH(k_fr_to_mont, ceil_div(n, 256), 256, 0, st, d, n, d_err); }
void fr_from_mont_enqueue(hipStream_t st, Fr* d, long n) { if (n > 0) LAUNCH(k_fr_from_mont, ceil_div(n, 256), 256, 0, st, d, n); }
void fr_check_enqueue(hipStream_t st, const Fr* d, long n, int* d_err) { if (n > 0) LAUNCH(k_fr_check, ceil_div(n, 256), 256, 0, st, d, n, d_err); }
void points_from_bytes_enqueue(hipStream_t st, const uint8_t* d_in96, PointArrayMut out, long n, int* d_err, long inf_ok) {
  if (n > 0) LAUNCH(k_points_from_bytes, ceil_div(n, 256), 256, 0, st, d_in96, out, n, d_err, inf_ok);
}
void points_subgroup_check_enqueue(hipStream_t st, PointArray in, long n, int* d_err) { if (n > 0) LAUNCH(k_points_subgroup_check, ceil_div(n, 256), 256, 0, st, in, n, d_err); }
void points_to_bytes_enqueue(hipStream_t st, PointArray in, uint8_t* d_out96, long n) { if (n > 0) LAUNCH(k_points_to_bytes, ceil_div(n, 256), 256, 0, st, in, d_out96, n); }
int read_flags(hipStream_t st, DevBuf& flags) {
  int h = 0;
  HIP_OK(hipMemcpyAsync(&h, flags.p, 4, hipMemcpyDeviceToHost, st));
  HIP_OK(hipStreamSynchronize(st));
  return h;
}

// one MSM, finished and normalised, result on the host
void msm_blocking(hipStream_t st, MsmWorkspace& ws, const MsmPlan& pl, PointArray d_pts, const Fr* d_sc, long n, bool mont,
                  uint8_t* out96, uint8_t* out_partial192) {
  DevBuf slot(sizeof(MsmSlot));
  msm_enqueue(st, ws, pl, d_pts, d_sc, n, mont, slot.as<MsmSlot>());
  MsmSlot h;
  HIP_OK(hipMemcpyAsync(&h, slot.p, sizeof(MsmSlot), hipMemcpyDeviceToHost, st));
  HIP_OK(hipStreamSynchronize(st));
  G1XYZZ sum = msm_finish_host(h);
  if (out96) g1_canonical_bytes_host(sum, out96);
  if (out_partial192) memcpy(out_partial192, &sum, sizeof sum);
}

}  // namespace sonic
