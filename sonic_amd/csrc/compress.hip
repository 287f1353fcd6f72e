// Compressed point encodings (include/sonic_hip.h, "Compressed encodings"; point-level code: compress.hpp): the four bulk kernels, one
// thread per point, their C entry points, and one proof's re-encoding on the host.  The batched verifier (verify_batch.hip) and the
// compressed SRS container (srs_api.hip) run the same kernels through the *_enqueue functions.
#include <string.h>
#include "verify_host.hpp"
#include "compress.hpp"
#include "proof_layout.hpp"

namespace sonic {
namespace {

// 48 bytes -> the affine point for an MSM or a basis array, its canonical 96 bytes and a verdict (compress.hpp); a refused point is
// written as infinity, as k_g1_validate does.  The subgroup test is the shared one (g1_in_subgroup: the endomorphism test).
__global__ __launch_bounds__(256) void k_g1_decompress(const uint8_t* __restrict__ in, PointArrayMut out, uint8_t* __restrict__ bytes96, uint8_t* __restrict__ flags,
                                                       long n, int check_subgroup) {
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  G1Affine p;
  uint8_t v = g1_decompress_point(in + 48 * i, p);
  if (!v && check_subgroup && !p.is_inf() && !g1_in_subgroup(p)) { v = Z_OUTSIDE_SUBGROUP; p = G1Affine::inf(); }
  if (out.p) out[i] = p;
  if (bytes96) g1_canonical_words(p, reinterpret_cast<uint32_t*>(bytes96 + 96 * i));
  flags[i] = v;
}
__global__ __launch_bounds__(256) void k_g1_compress(PointArray in, uint8_t* __restrict__ out48, long n) {
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  g1_compress_point(in[i], out48 + 48 * i);
}
// the same over the twist; block size and bounds of the other G2 kernels (srs_g2.hip)
__global__ __launch_bounds__(64, 1) void k_g2_decompress(const uint8_t* __restrict__ in, G2Affine* __restrict__ out, uint8_t* __restrict__ bytes192,
                                                         uint8_t* __restrict__ flags, long n, int check_subgroup) {
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  G2Affine p;
  uint8_t v = g2_decompress_point(in + 96 * i, p);
  if (!v && check_subgroup && !p.is_inf() && !g2_in_subgroup(p)) { v = Z_OUTSIDE_SUBGROUP; p = G2Affine::inf(); }
  if (out) out[i] = p;
  if (bytes192) g2_canonical_words(p, reinterpret_cast<uint32_t*>(bytes192 + 192 * i));
  flags[i] = v;
}
__global__ __launch_bounds__(64, 1) void k_g2_compress(const G2Affine* __restrict__ in, uint8_t* __restrict__ out96, long n) {
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  g2_compress_point(in[i], out96 + 96 * i);
}

}  // namespace

void g1_decompress_enqueue(hipStream_t st, const uint8_t* d_in48, PointArrayMut out, uint8_t* d_bytes96, uint8_t* d_flags, long n, bool check_subgroup) {
  if (n > 0) LAUNCH(k_g1_decompress, ceil_div(n, 256), 256, 0, st, d_in48, out, d_bytes96, d_flags, n, check_subgroup ? 1 : 0);
}
void g2_decompress_enqueue(hipStream_t st, const uint8_t* d_in96, G2Affine* out, uint8_t* d_bytes192, uint8_t* d_flags, long n, bool check_subgroup) {
  if (n > 0) LAUNCH(k_g2_decompress, ceil_div(n, 64), 64, 0, st, d_in96, out, d_bytes192, d_flags, n, check_subgroup ? 1 : 0);
}
void g1_compress_enqueue(hipStream_t st, PointArray in, uint8_t* d_out48, long n) {
  if (n > 0) LAUNCH(k_g1_compress, ceil_div(n, 256), 256, 0, st, in, d_out48, n);
}
void g2_compress_enqueue(hipStream_t st, const G2Affine* in, uint8_t* d_out96, long n) {
  if (n > 0) LAUNCH(k_g2_compress, ceil_div(n, 64), 64, 0, st, in, d_out96, n);
}

}  // namespace sonic

using namespace sonic;

namespace {

// the verdicts of a bulk decompression: into the caller's array, or (flags == NULL) the first refused point fails the call
int report_flags(const char* who, const std::vector<uint8_t>& fl, uint8_t* flags) {
  if (flags) { memcpy(flags, fl.data(), fl.size()); return SONIC_OK; }
  for (size_t i = 0; i < fl.size(); i++)
    if (fl[i]) {
      set_error("%s: point %zu is %s", who, i, (fl[i] & Z_MALFORMED) ? "malformed" : (fl[i] & Z_OFF_CURVE) ? "not on the curve" : "outside the order-r subgroup");
      return SONIC_ERR_BAD_ENCODING;
    }
  return SONIC_OK;
}

}  // namespace

extern "C" {

int sonic_g1_decompress(const uint8_t* in48, int64_t n, int check_subgroup, uint8_t* out96, uint8_t* flags) {
  if (n < 0 || (n > 0 && (!in48 || !out96))) { set_error("sonic_g1_decompress: bad argument"); return SONIC_ERR_INVALID_ARG; }
  if (n == 0) return SONIC_OK;
  API_BEGIN
  CallLease lease;
  hipStream_t st = lease.st();
  DevBuf raw(48 * (size_t)n), bytes(96 * (size_t)n), fl((size_t)n);
  std::vector<uint8_t> hfl((size_t)n);
  HIP_OK(hipMemcpyAsync(raw.p, in48, 48 * (size_t)n, hipMemcpyHostToDevice, st));
  g1_decompress_enqueue(st, raw.as<uint8_t>(), PointArrayMut{nullptr, 0}, bytes.as<uint8_t>(), fl.as<uint8_t>(), (long)n, check_subgroup != 0);
  HIP_OK(hipMemcpyAsync(out96, bytes.p, 96 * (size_t)n, hipMemcpyDeviceToHost, st));
  HIP_OK(hipMemcpyAsync(hfl.data(), fl.p, (size_t)n, hipMemcpyDeviceToHost, st));
  HIP_OK(hipStreamSynchronize(st));
  return report_flags("sonic_g1_decompress", hfl, flags);
  API_CATCH
}

int sonic_g2_decompress(const uint8_t* in96, int64_t n, int check_subgroup, uint8_t* out192, uint8_t* flags) {
  if (n < 0 || (n > 0 && (!in96 || !out192))) { set_error("sonic_g2_decompress: bad argument"); return SONIC_ERR_INVALID_ARG; }
  if (n == 0) return SONIC_OK;
  API_BEGIN
  CallLease lease;
  hipStream_t st = lease.st();
  DevBuf raw(96 * (size_t)n), bytes(192 * (size_t)n), fl((size_t)n);
  std::vector<uint8_t> hfl((size_t)n);
  HIP_OK(hipMemcpyAsync(raw.p, in96, 96 * (size_t)n, hipMemcpyHostToDevice, st));
  g2_decompress_enqueue(st, raw.as<uint8_t>(), nullptr, bytes.as<uint8_t>(), fl.as<uint8_t>(), (long)n, check_subgroup != 0);
  HIP_OK(hipMemcpyAsync(out192, bytes.p, 192 * (size_t)n, hipMemcpyDeviceToHost, st));
  HIP_OK(hipMemcpyAsync(hfl.data(), fl.p, (size_t)n, hipMemcpyDeviceToHost, st));
  HIP_OK(hipStreamSynchronize(st));
  return report_flags("sonic_g2_decompress", hfl, flags);
  API_CATCH
}

int sonic_g1_compress(const uint8_t* points96, int64_t n, uint8_t* out48) {
  if (n < 0 || (n > 0 && (!points96 || !out48))) { set_error("sonic_g1_compress: bad argument"); return SONIC_ERR_INVALID_ARG; }
  if (n == 0) return SONIC_OK;
  API_BEGIN
  CallLease lease;
  hipStream_t st = lease.st();
  DevBuf raw(96 * (size_t)n), pts(sizeof(G1Affine) * (size_t)n), fl((size_t)n), z(48 * (size_t)n);
  std::vector<uint8_t> hfl((size_t)n);
  HIP_OK(hipMemcpyAsync(raw.p, points96, 96 * (size_t)n, hipMemcpyHostToDevice, st));
  g1_validate_enqueue(st, raw.as<uint8_t>(), pts.as<G1Affine>(), fl.as<uint8_t>(), (long)n);
  g1_compress_enqueue(st, PointArray::packed(pts.as<G1Affine>()), z.as<uint8_t>(), (long)n);
  HIP_OK(hipMemcpyAsync(hfl.data(), fl.p, (size_t)n, hipMemcpyDeviceToHost, st));
  HIP_OK(hipMemcpyAsync(out48, z.p, 48 * (size_t)n, hipMemcpyDeviceToHost, st));
  HIP_OK(hipStreamSynchronize(st));
  for (int64_t i = 0; i < n; i++)
    if (!hfl[(size_t)i]) { set_error("sonic_g1_compress: point %lld is non-canonical, off the curve or outside the order-r subgroup", (long long)i); return SONIC_ERR_BAD_ENCODING; }
  return SONIC_OK;
  API_CATCH
}

int sonic_g2_compress(const uint8_t* points192, int64_t n, uint8_t* out96) {
  if (n < 0 || (n > 0 && (!points192 || !out96))) { set_error("sonic_g2_compress: bad argument"); return SONIC_ERR_INVALID_ARG; }
  if (n == 0) return SONIC_OK;
  API_BEGIN
  CallLease lease;
  hipStream_t st = lease.st();
  DevBuf raw(192 * (size_t)n), pts(sizeof(G2Affine) * (size_t)n), err(4), z(96 * (size_t)n);
  HIP_OK(hipMemsetAsync(err.p, 0, 4, st));
  HIP_OK(hipMemcpyAsync(raw.p, points192, 192 * (size_t)n, hipMemcpyHostToDevice, st));
  g2_points_from_bytes_enqueue(st, raw.as<uint8_t>(), pts.as<G2Affine>(), (long)n, err.as<int>());      // the validation of sonic_srs_set_g2_points
  g2_compress_enqueue(st, pts.as<G2Affine>(), z.as<uint8_t>(), (long)n);
  int herr = 0;
  HIP_OK(hipMemcpyAsync(&herr, err.p, 4, hipMemcpyDeviceToHost, st));
  HIP_OK(hipMemcpyAsync(out96, z.p, 96 * (size_t)n, hipMemcpyDeviceToHost, st));
  HIP_OK(hipStreamSynchronize(st));
  // (bit 8, the point at infinity, is an SRS rule: here infinity has an encoding like every other point)
  if (herr & 7) { set_error("sonic_g2_compress: %s", (herr & 1) ? "non-canonical coordinate" : (herr & 2) ? "point not on the twist" : "point outside the order-r subgroup"); return SONIC_ERR_BAD_ENCODING; }
  return SONIC_OK;
  API_CATCH
}

// ---- one proof, on the host ----
size_t sonic_proof_size_compressed(int64_t Q) { return Q < 0 ? 0 : ProofLayout{(long)Q}.proof_bytes_compressed(); }

int sonic_proof_compress(int64_t Q, const uint8_t* proof, uint8_t* out) {
  if (Q < 1 || !proof || !out) { set_error("sonic_proof_compress: bad argument"); return SONIC_ERR_INVALID_ARG; }
  const bool ok = proof_repack((long)Q, proof, 96, out, 48, [](const uint8_t* in, uint8_t* o) {
    G1Affine p;
    const bool k = load_g1(in, p);
    g1_compress_point(k ? p : G1Affine::inf(), o);
    return k;
  });
  if (!ok) { set_error("sonic_proof_compress: the proof holds a point that is non-canonical, off the curve or outside the order-r subgroup"); return SONIC_ERR_BAD_ENCODING; }
  return SONIC_OK;
}

int sonic_proof_decompress(int64_t Q, const uint8_t* proof_z, uint8_t* out_proof) {
  if (Q < 1 || !proof_z || !out_proof) { set_error("sonic_proof_decompress: bad argument"); return SONIC_ERR_INVALID_ARG; }
  bool ok = proof_repack((long)Q, proof_z, 48, out_proof, 96, [](const uint8_t* in, uint8_t* o) {
    G1Affine p;
    bool k = g1_decompress_point(in, p) == 0;
    if (k && !p.is_inf() && !g1_in_subgroup(p)) { k = false; p = G1Affine::inf(); }
    uint32_t w[24];
    g1_canonical_words(p, w);
    memcpy(o, w, 96);
    return k;
  });
  // the field elements travel as they are; a non-canonical one is refused here as the verifiers refuse it
  const uint8_t* p = out_proof;
  proof_record_order((long)Q, [&](long) { p += 96; }, [&](long) { Fr f; ok = load_fr(p, f) && ok; p += 32; });
  if (!ok) { set_error("sonic_proof_decompress: malformed point, point off the curve or outside the order-r subgroup, or non-canonical field element"); return SONIC_ERR_BAD_ENCODING; }
  return SONIC_OK;
}

// a core proof's 576 <-> 336 bytes: the same point encodings over the head's five points (proof_layout.hpp, core_proof_repack)
int sonic_core_proof_compress(const uint8_t* proof, uint8_t* out) {
  if (!proof || !out) { set_error("sonic_core_proof_compress: bad argument"); return SONIC_ERR_INVALID_ARG; }
  const bool ok = core_proof_repack(proof, 96, out, 48, [](const uint8_t* in, uint8_t* o) {
    G1Affine p;
    const bool k = load_g1(in, p);
    g1_compress_point(k ? p : G1Affine::inf(), o);
    return k;
  });
  if (!ok) { set_error("sonic_core_proof_compress: the proof holds a point that is non-canonical, off the curve or outside the order-r subgroup"); return SONIC_ERR_BAD_ENCODING; }
  return SONIC_OK;
}

int sonic_core_proof_decompress(const uint8_t* proof_z, uint8_t* out_proof) {
  if (!proof_z || !out_proof) { set_error("sonic_core_proof_decompress: bad argument"); return SONIC_ERR_INVALID_ARG; }
  bool ok = core_proof_repack(proof_z, 48, out_proof, 96, [](const uint8_t* in, uint8_t* o) {
    G1Affine p;
    bool k = g1_decompress_point(in, p) == 0;
    if (k && !p.is_inf() && !g1_in_subgroup(p)) { k = false; p = G1Affine::inf(); }
    uint32_t w[24];
    g1_canonical_words(p, w);
    memcpy(o, w, 96);
    return k;
  });
  const uint8_t* p = out_proof;
  core_proof_record_order([&](long) { p += 96; }, [&](long) { Fr f; ok = load_fr(p, f) && ok; p += 32; });
  if (!ok) { set_error("sonic_core_proof_decompress: malformed point, point off the curve or outside the order-r subgroup, or non-canonical field element"); return SONIC_ERR_BAD_ENCODING; }
  return SONIC_OK;
}

}  // extern "C"
