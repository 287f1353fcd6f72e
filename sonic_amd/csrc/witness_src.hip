// Witness sources (include/sonic_hip.h, "Witness sources"; the description and the int64 conversion: witness_src.hpp): how an assignment
// reaches a prover handle from wherever it lies.  One kernel, one launch:
//   k_witness_ingest<kind, aO given>   grid (blocks of 256 gates, assignments): a thread loads gate i of assignment b from aL, aR and, when
//                given, aO; checks canonical form (32-byte elements) as k_fr_to_mont does; converts to Montgomery form; forms aO = aL aR
//                when aO is absent; writes the three planes the prover reads -- the handle's aL, aR, aO, or the staged planes of
//                sonic_prover_eval_constraints_src.
// Adjacent lanes read adjacent elements: a 32-byte element as two 16-byte loads (the pointers are 32-byte aligned: the rule of the header),
// an integer as one 8-byte load; the planes are written with 16-byte stores.  No LDS.  The kernel is bound by memory and by its launch:
// 96 bytes in (24 for integers with aO derived) and 96 out per gate, against three Montgomery products.
// A device source is read where it lies.  A host source is copied as it is into the handle's wit_raw first and read by the same kernel.
#include "prover.hpp"

namespace sonic {
namespace {

constexpr int WI_BLOCK = 256;

// element i of a vector in standard form; false: not canonical
template <int KIND>
__device__ __forceinline__ bool wit_load(const uint8_t* __restrict__ v, long i, Fr& out) {
  if constexpr (KIND == SONIC_WIT_I64) {
    out = wit_i64_to_fr(*reinterpret_cast<const int64_t*>(v + 8 * i));
    return true;
  } else {
    const uint4* q = reinterpret_cast<const uint4*>(v + 32 * i);
    const uint4 lo = q[0], hi = q[1];
    out.l[0] = lo.x; out.l[1] = lo.y; out.l[2] = lo.z; out.l[3] = lo.w;
    out.l[4] = hi.x; out.l[5] = hi.y; out.l[6] = hi.z; out.l[7] = hi.w;
    return fp_is_canonical(out);
  }
}
__device__ __forceinline__ void wit_store(Fr* __restrict__ plane, long at, const Fr& v) {
  uint4* o = reinterpret_cast<uint4*>(plane + at);
  o[0] = make_uint4(v.l[0], v.l[1], v.l[2], v.l[3]);
  o[1] = make_uint4(v.l[4], v.l[5], v.l[6], v.l[7]);
}

// stride: bytes between the assignments of the source; out_stride: elements between those of the planes
template <int KIND, bool HAS_AO>
__global__ __launch_bounds__(WI_BLOCK) void k_witness_ingest(const uint8_t* __restrict__ aL, const uint8_t* __restrict__ aR, const uint8_t* __restrict__ aO, long stride, long n,
                                                             Fr* __restrict__ oL, Fr* __restrict__ oR, Fr* __restrict__ oO, long out_stride, int* __restrict__ err) {
  const long i = (long)blockIdx.x * WI_BLOCK + threadIdx.x, b = blockIdx.y;
  if (i >= n) return;
  Fr l, r, o = Fr::zero();
  bool ok = wit_load<KIND>(aL + b * stride, i, l);
  ok = wit_load<KIND>(aR + b * stride, i, r) && ok;
  if constexpr (HAS_AO) ok = wit_load<KIND>(aO + b * stride, i, o) && ok;
  if (ok) {
    l = fp_to_mont(l);
    r = fp_to_mont(r);
    if constexpr (HAS_AO) o = fp_to_mont(o);
    else o = fp_mul(l, r);
  } else {
    // (a refused gate is written as zeros: nothing downstream reads a value that is not below r)
    atomicOr(err, FLAG_BAD_ENCODING);
    l = r = o = Fr::zero();
  }
  const long at = b * out_stride + i;
  wit_store(oL, at, l);
  wit_store(oR, at, r);
  wit_store(oO, at, o);
}

// v: device pointers
void witness_ingest_enqueue(hipStream_t st, const WitnessView& v, long nb, long n, Fr* oL, Fr* oR, Fr* oO, long out_stride, int* d_err) {
  const dim3 grid((unsigned)ceil_div(n, WI_BLOCK), (unsigned)nb);
  const bool i64 = v.kind == SONIC_WIT_I64;
  if (i64 && v.aO) LAUNCH((k_witness_ingest<SONIC_WIT_I64, true>), grid, WI_BLOCK, 0, st, v.aL, v.aR, v.aO, (long)v.stride, n, oL, oR, oO, out_stride, d_err);
  else if (i64) LAUNCH((k_witness_ingest<SONIC_WIT_I64, false>), grid, WI_BLOCK, 0, st, v.aL, v.aR, v.aO, (long)v.stride, n, oL, oR, oO, out_stride, d_err);
  else if (v.aO) LAUNCH((k_witness_ingest<SONIC_WIT_FR32, true>), grid, WI_BLOCK, 0, st, v.aL, v.aR, v.aO, (long)v.stride, n, oL, oR, oO, out_stride, d_err);
  else LAUNCH((k_witness_ingest<SONIC_WIT_FR32, false>), grid, WI_BLOCK, 0, st, v.aL, v.aR, v.aO, (long)v.stride, n, oL, oR, oO, out_stride, d_err);
}

}  // namespace

int witness_view_of(const char* who, const sonic_witness_src_t* src, long n, long B, WitnessView* out) {
  char msg[256];
  const int rc = wit_view_checked(src, n, B, out, msg, sizeof msg);
  if (rc) set_error("%s: %s", who, msg);
  return rc;
}

// the device's half of the checks: every vector of a device source is device memory of `device`, and the allocation it lies in holds all
// B blocks (where the runtime tells the allocation's range)
int witness_on_device_of(const char* who, const WitnessView& v, long n, long B, int device) {
  if (!v.on_device) return SONIC_OK;
  const uint8_t* ptr[3] = {v.aL, v.aR, v.aO};
  const char* name[3] = {"aL", "aR", "aO"};
  const size_t need = (size_t)(B - 1) * (size_t)v.stride + (size_t)n * (size_t)v.elem();
  for (int k = 0; k < 3; k++) {
    if (!ptr[k]) continue;
    hipPointerAttribute_t at;
    const hipError_t e = hipPointerGetAttributes(&at, ptr[k]);
    if (e != hipSuccess || at.type == hipMemoryTypeUnregistered || at.type == hipMemoryTypeHost) {
      if (e != hipSuccess) (void)hipGetLastError();      // (an address the runtime does not know: not a failure of the device)
      set_error("%s: on_device = 1, but %s is a host pointer, not memory of device %d (the handle's GPU)", who, name[k], device);
      return SONIC_ERR_INVALID_ARG;
    }
    if (at.type != hipMemoryTypeDevice) { set_error("%s: %s is neither host nor plain device memory (memory type %d); the handle lives on device %d", who, name[k], (int)at.type, device); return SONIC_ERR_INVALID_ARG; }
    if (at.device != device) {
      set_error("%s: %s lies on device %d, the handle on device %d (a device source must lie on the GPU of every handle that reads it; no peer copy is made)", who, name[k], at.device, device);
      return SONIC_ERR_INVALID_ARG;
    }
    hipDeviceptr_t base = nullptr;
    size_t size = 0;
    if (hipMemGetAddressRange(&base, &size, (hipDeviceptr_t)ptr[k]) != hipSuccess) { (void)hipGetLastError(); continue; }
    const size_t off = (size_t)(ptr[k] - static_cast<const uint8_t*>(base));
    if (off > size || need > size - off) {
      set_error("%s: %s needs %zu bytes (%ld assignments of %ld elements), its allocation has %zu from there", who, name[k], need, B, n, size - (off > size ? size : off));
      return SONIC_ERR_INVALID_ARG;
    }
  }
  return SONIC_OK;
}

void WitnessReady::record(const WitnessView& v) {
  if (!v.on_device || !v.hip_stream) return;
  if (!ev) HIP_OK(hipEventCreateWithFlags(&ev, hipEventDisableTiming));
  HIP_OK(hipEventRecord(ev, static_cast<hipStream_t>(v.hip_stream)));
}

void witness_load_enqueue(sonic_prover* p, hipStream_t st, const WitnessView& v, long nb, Fr* oL, Fr* oR, Fr* oO, long out_stride, int* d_err) {
  const long n = p->n;
  WitnessView d = v;
  if (!v.on_device) {
    const size_t row = (size_t)n * (size_t)v.elem(), plane = (size_t)nb * row;
    const uint8_t* src[3] = {v.aL, v.aR, v.aO};
    p->wit_raw.ensure((v.aO ? 3 : 2) * plane);
    uint8_t* raw = p->wit_raw.as<uint8_t>();
    for (int k = 0; k < 3; k++) {
      if (!src[k]) continue;
      if ((size_t)v.stride == row) HIP_OK(hipMemcpyAsync(raw + k * plane, src[k], plane, hipMemcpyHostToDevice, st));
      else for (long b = 0; b < nb; b++) HIP_OK(hipMemcpyAsync(raw + k * plane + (size_t)b * row, src[k] + (size_t)b * (size_t)v.stride, row, hipMemcpyHostToDevice, st));
    }
    d.aL = raw; d.aR = raw + plane; d.aO = v.aO ? raw + 2 * plane : nullptr;
    d.stride = (int64_t)row; d.on_device = true;
  }
  witness_ingest_enqueue(st, d, nb, n, oL, oR, oO, out_stride, d_err);
}

}  // namespace sonic

extern "C" {

int sonic_prover_set_witness(sonic_prover_t* p, const sonic_witness_src_t* src) {
  API_BEGIN_ON(p ? p->device : -1)
  const char* who = "sonic_prover_set_witness";
  if (!p) { set_error("%s: bad argument", who); return SONIC_ERR_INVALID_ARG; }
  WitnessView v;
  int rc = witness_view_of(who, src, p->n, 1, &v);
  if (rc) return rc;
  std::lock_guard<std::mutex> g(p->mu);
  if (p->in_flight) { set_error("%s: a submitted proof is still reading the current assignment (collect it first)", who); return SONIC_ERR_INVALID_ARG; }
  rc = witness_on_device_of(who, v, p->n, 1, p->device);
  if (rc) return rc;
  WitnessReady ready;
  ready.record(v);
  hipStream_t st = p->st;
  for (DevBuf* b : {&p->aL, &p->aR, &p->aO}) b->ensure(sizeof(Fr) * (size_t)p->n);
  EnqueueLock enq(p);
  if (ready.ev) HIP_OK(hipStreamWaitEvent(st, ready.ev, 0));
  HIP_OK(hipMemsetAsync(p->flags.p, 0, 4, st));
  p->have_assignment = false;      // (until the source is known to be good)
  p->assignment_changed();
  witness_load_enqueue(p, st, v, 1, p->aL.as<Fr>(), p->aR.as<Fr>(), p->aO.as<Fr>(), p->n, p->flags.as<int>());
  const int f = read_flags(st, p->flags);
  if (f) return flags_to_status(f, who);
  p->have_assignment = true;
  API_END
}

}  // extern "C"
