// R1CS front end, device half (include/sonic_hip.h, "R1CS front end"; the mapping and the host layout: r1cs.hpp).  A handle holds A, B, C
// of one rank-1 constraint system in HBM -- stacked as 3m rows, 32-bit indices, Montgomery values -- and turns K witness vectors z into K
// Sonic assignments and their constants.  Fr sums are exact, so nothing depends on the order of summation; there are no atomics on field
// elements and no tolerance anywhere.
//
// Kernels, per chunk of witnesses (grid.y = the witnesses of the chunk):
//   k_r1cs_ingest<kind>   a thread per element of z: loads it (witness_src.hpp's int64 conversion, or 32 bytes as two 16-byte loads), checks
//                 canonical form, flags z[0] != 1 with an integer atomic min over the witness index, keeps the canonical public inputs
//                 z[1..n_pub] for the constants, writes z in Montgomery form
//   k_r1cs_short  a thread per row of at most R1CS_ROW_CHUNK entries: real systems are mostly rows of 1-5 entries, and a wave per row would
//                 idle 59 lanes of 64 on them
//   k_r1cs_long   a block of 256 per longer row (a sum over all variables is common): lanes stride over the row, shuffle reduction per
//                 wave, LDS sum of the four waves
//   k_r1cs_fill   a thread per gate: constraint gates from the sums, variable gates from z, aO of a variable gate as the product, all
//                 three planes written in canonical form; per witness the count and smallest index of constraint gates with aL aR != aO,
//                 reduced as k_gates of statement.hip reduces them (a copy: that file is left as it is)
// One thread carries one witness: the simplest form.  Carrying two or four would reuse each val load at 8 VGPRs per accumulator; that
// variant has not been measured (README, "R1CS front end").
#include "prover.hpp"
#include "r1cs.hpp"

struct sonic_r1cs {
  int device = -1;
  R1csShape shape{};
  // the caller's matrices, kept for sonic_r1cs_circuit (host only)
  std::vector<int64_t> h_row_ptr[3], h_col[3];
  std::vector<uint8_t> h_val[3];
  R1csView view{};
  std::vector<uint8_t> cs_fixed;
  // device layout (r1cs.hpp, R1csDeviceLayout)
  DevBuf row_ptr, col, val, short_rows, long_rows;
  long n_short = 0, n_long = 0;
  hipStream_t st = nullptr;
  std::mutex mu;
  // staging of one chunk of witnesses: the raw copy of a host z, z in Montgomery form, the 3m sums, the public inputs, status words
  DevBuf raw, zm, sums, pub, status, bad;
  ~sonic_r1cs() { if (st) (void)hipStreamDestroy(st); }
};

namespace sonic {
namespace {

constexpr int R1_BLOCK = 256;                 // four wave64
constexpr long R1_STAGE_ELEMS = 1L << 20;     // field elements of z (and of the sums) per chunk: 32 MB each at most, one witness when it is larger

// status words: [0] the FLAG_* bits, [1] the smallest witness index with z[0] != 1 (~0: none)
template <int KIND>
__global__ __launch_bounds__(R1_BLOCK) void k_r1cs_ingest(const uint8_t* __restrict__ z, long stride, long N, long n_pub, long k0, Fr* __restrict__ zm,
                                                          Fr* __restrict__ pub, unsigned long long* __restrict__ status) {
  const long j = (long)blockIdx.x * R1_BLOCK + threadIdx.x, b = blockIdx.y;
  if (j >= N) return;
  const uint8_t* src = z + b * stride;
  Fr v;
  bool ok = true;
  if constexpr (KIND == SONIC_WIT_I64) {
    v = wit_i64_to_fr(*reinterpret_cast<const int64_t*>(src + 8 * j));
  } else {
    const uint4* q = reinterpret_cast<const uint4*>(src + 32 * j);
    const uint4 lo = q[0], hi = q[1];
    v.l[0] = lo.x; v.l[1] = lo.y; v.l[2] = lo.z; v.l[3] = lo.w;
    v.l[4] = hi.x; v.l[5] = hi.y; v.l[6] = hi.z; v.l[7] = hi.w;
    ok = fp_is_canonical(v);
  }
  if (!ok) {
    atomicOr(reinterpret_cast<unsigned int*>(status), (unsigned int)FLAG_BAD_ENCODING);
    v = Fr::zero();
  } else if (j == 0) {
    uint32_t rest = v.l[0] ^ 1u;
#pragma unroll
    for (int i = 1; i < FR_LIMBS; i++) rest |= v.l[i];
    if (rest) atomicMin(&status[1], (unsigned long long)(k0 + b));
  }
  if (j >= 1 && j <= n_pub) pub[b * n_pub + (j - 1)] = v;
  zm[b * N + j] = fp_to_mont(v);
}

// sums[b][r] = sum over row r of val * z_b[col]
__global__ __launch_bounds__(R1_BLOCK) void k_r1cs_short(const int32_t* __restrict__ row_ptr, const int32_t* __restrict__ col, const Fr* __restrict__ val,
                                                         const int32_t* __restrict__ rows, long nrows, long rows_all, const Fr* __restrict__ zm, long N,
                                                         Fr* __restrict__ sums) {
  const long t = (long)blockIdx.x * R1_BLOCK + threadIdx.x, b = blockIdx.y;
  if (t >= nrows) return;
  const int r = rows[t];
  const Fr* z = zm + b * N;
  Fr acc = Fr::zero();
  for (int e = row_ptr[r]; e < row_ptr[r + 1]; e++) acc = fp_add(acc, fp_mul(val[e], z[col[e]]));
  sums[b * rows_all + r] = acc;
}

__device__ __forceinline__ Fr r1_shfl_xor(const Fr& a, int mask) {
  Fr o;
#pragma unroll
  for (int k = 0; k < 8; k++) o.l[k] = (uint32_t)__shfl_xor((int)a.l[k], mask, 64);
  return o;
}

__global__ __launch_bounds__(R1_BLOCK) void k_r1cs_long(const int32_t* __restrict__ row_ptr, const int32_t* __restrict__ col, const Fr* __restrict__ val,
                                                        const int32_t* __restrict__ rows, long rows_all, const Fr* __restrict__ zm, long N, Fr* __restrict__ sums) {
  __shared__ Fr sh[R1_BLOCK / 64];
  const long b = blockIdx.y;
  const int r = rows[blockIdx.x];
  const Fr* z = zm + b * N;
  Fr acc = Fr::zero();
  for (int e = row_ptr[r] + (int)threadIdx.x; e < row_ptr[r + 1]; e += R1_BLOCK) acc = fp_add(acc, fp_mul(val[e], z[col[e]]));
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) acc = fp_add(acc, r1_shfl_xor(acc, o));
  if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = acc;
  __syncthreads();
  if (threadIdx.x == 0) sums[b * rows_all + r] = fp_add(fp_add(sh[0], sh[1]), fp_add(sh[2], sh[3]));
}

__device__ __forceinline__ void r1_store(uint8_t* __restrict__ plane, long byte_at, const Fr& v) {
  uint4* o = reinterpret_cast<uint4*>(plane + byte_at);
  o[0] = make_uint4(v.l[0], v.l[1], v.l[2], v.l[3]);
  o[1] = make_uint4(v.l[4], v.l[5], v.l[6], v.l[7]);
}

// bad[2 b] += the broken constraint gates of the block, bad[2 b + 1] = min with the smallest broken index (the host sets it to ~0 first)
__global__ __launch_bounds__(R1_BLOCK) void k_r1cs_fill(const Fr* __restrict__ sums, const Fr* __restrict__ zm, long m, long N, long n, uint8_t* __restrict__ oL,
                                                        uint8_t* __restrict__ oR, uint8_t* __restrict__ oO, long out_stride, unsigned long long* __restrict__ bad) {
  __shared__ unsigned long long first[R1_BLOCK];
  __shared__ unsigned int count[R1_BLOCK];
  const long b = blockIdx.y, i = (long)blockIdx.x * R1_BLOCK + threadIdx.x;
  bool broken = false;
  if (i < n) {
    Fr l, r, o;
    if (i < m) {
      const Fr* s = sums + b * 3 * m;
      l = s[i]; r = s[m + i]; o = s[2 * m + i];
      broken = !(fp_mul(l, r) == o);
    } else {
      const long j = 2 * (i - m) + 1;
      const Fr* z = zm + b * N;
      l = z[j];
      r = j + 1 < N ? z[j + 1] : Fr::zero();
      o = fp_mul(l, r);
    }
    const long at = b * out_stride + 32 * i;
    r1_store(oL, at, fp_from_mont(l));
    r1_store(oR, at, fp_from_mont(r));
    r1_store(oO, at, fp_from_mont(o));
  }
  first[threadIdx.x] = broken ? (unsigned long long)i : ~0ull;
  count[threadIdx.x] = broken ? 1u : 0u;
  __syncthreads();
  for (int s = R1_BLOCK / 2; s >= 1; s >>= 1) {
    if ((int)threadIdx.x < s) {
      count[threadIdx.x] += count[threadIdx.x + s];
      if (first[threadIdx.x + s] < first[threadIdx.x]) first[threadIdx.x] = first[threadIdx.x + s];
    }
    __syncthreads();
  }
  if (threadIdx.x == 0 && count[0]) {
    atomicAdd(&bad[2 * b], (unsigned long long)count[0]);
    atomicMin(&bad[2 * b + 1], first[0]);
  }
}

// `ptr` is plain device memory of `device`, and the allocation it lies in holds `need` bytes from there (where the runtime tells the range):
// the checks of witness_on_device_of (witness_src.hip), for one pointer
int r1cs_on_device(const char* who, const char* name, const void* ptr, size_t need, int device) {
  hipPointerAttribute_t at;
  const hipError_t e = hipPointerGetAttributes(&at, ptr);
  if (e != hipSuccess || at.type == hipMemoryTypeUnregistered || at.type == hipMemoryTypeHost) {
    if (e != hipSuccess) (void)hipGetLastError();      // (an address the runtime does not know: not a failure of the device)
    set_error("%s: %s is a host pointer, not memory of device %d (the handle's GPU)", who, name, device);
    return SONIC_ERR_INVALID_ARG;
  }
  if (at.type != hipMemoryTypeDevice) { set_error("%s: %s is neither host nor plain device memory (memory type %d); the handle lives on device %d", who, name, (int)at.type, device); return SONIC_ERR_INVALID_ARG; }
  if (at.device != device) { set_error("%s: %s lies on device %d, the handle on device %d (no peer copy is made)", who, name, at.device, device); return SONIC_ERR_INVALID_ARG; }
  hipDeviceptr_t base = nullptr;
  size_t size = 0;
  if (hipMemGetAddressRange(&base, &size, (hipDeviceptr_t)ptr) != hipSuccess) { (void)hipGetLastError(); return SONIC_OK; }
  const size_t off = (size_t)(static_cast<const uint8_t*>(ptr) - static_cast<const uint8_t*>(base));
  if (off > size || need > size - off) { set_error("%s: %s needs %zu bytes, its allocation has %zu from there", who, name, need, size - (off > size ? size : off)); return SONIC_ERR_INVALID_ARG; }
  return SONIC_OK;
}

void upload_i32(hipStream_t st, DevBuf& dst, const std::vector<int32_t>& v) {
  dst.ensure(4 * std::max<size_t>(1, v.size()));
  if (!v.empty()) HIP_OK(hipMemcpyAsync(dst.p, v.data(), 4 * v.size(), hipMemcpyHostToDevice, st));
}

int r1cs_new_impl(const char* who, int64_t m, int64_t N, int64_t n_pub, const sonic_r1cs_matrix_t* A, const sonic_r1cs_matrix_t* B, const sonic_r1cs_matrix_t* C,
                  sonic_r1cs_t** out) {
  if (!A || !B || !C || !out) { set_error("%s: bad argument", who); return SONIC_ERR_INVALID_ARG; }
  R1csView v{m, N, n_pub, {*A, *B, *C}};
  char msg[256] = "";
  const int rc = r1cs_validate(v, msg, sizeof msg);
  if (rc) { set_error("%s: %s", who, msg); return rc; }
  std::unique_ptr<sonic_r1cs> r(new sonic_r1cs);
  r->device = current_ctx().dev;
  for (int k = 0; k < 3; k++) {
    const int64_t nnz = v.M[k].row_ptr[m];
    r->h_row_ptr[k].assign(v.M[k].row_ptr, v.M[k].row_ptr + m + 1);
    if (nnz) { r->h_col[k].assign(v.M[k].col, v.M[k].col + nnz); r->h_val[k].assign(v.M[k].val, v.M[k].val + 32 * nnz); }
    r->view.M[k] = sonic_r1cs_matrix_t{r->h_row_ptr[k].data(), r->h_col[k].data(), r->h_val[k].data()};
  }
  r->view.m = m; r->view.N = N; r->view.n_pub = n_pub;
  r->shape = r1cs_shape(r->view);
  R1csDeviceLayout L;
  r1cs_device_layout(r->view, L);
  r->n_short = (long)L.short_rows.size();
  r->n_long = (long)L.long_rows.size();
  HIP_OK(hipStreamCreateWithFlags(&r->st, hipStreamNonBlocking));
  r->status.alloc(16);
  HIP_OK(hipMemsetAsync(r->status.p, 0, 16, r->st));
  upload_i32(r->st, r->row_ptr, L.row_ptr);
  upload_i32(r->st, r->col, L.col);
  upload_i32(r->st, r->short_rows, L.short_rows);
  upload_i32(r->st, r->long_rows, L.long_rows);
  upload_fr_mont(r->st, r->val, L.val.data(), (long)L.col.size(), r->status.as<int>());
  HIP_OK(hipStreamSynchronize(r->st));      // (L goes out of scope; the values were validated above, so the flag stays clear)
  *out = r.release();
  return SONIC_OK;
}

}  // namespace
}  // namespace sonic

extern "C" {

int sonic_r1cs_new_on(int device, int64_t m, int64_t N, int64_t n_pub, const sonic_r1cs_matrix_t* A, const sonic_r1cs_matrix_t* B, const sonic_r1cs_matrix_t* C,
                      sonic_r1cs_t** out) {
  API_BEGIN_ON(device)
  return r1cs_new_impl("sonic_r1cs_new", m, N, n_pub, A, B, C, out);
  API_CATCH
}
int sonic_r1cs_new(int64_t m, int64_t N, int64_t n_pub, const sonic_r1cs_matrix_t* A, const sonic_r1cs_matrix_t* B, const sonic_r1cs_matrix_t* C, sonic_r1cs_t** out) {
  return sonic_r1cs_new_on(-1, m, N, n_pub, A, B, C, out);
}

void sonic_r1cs_free(sonic_r1cs_t* r) {
  if (!r) return;
  try { DeviceScope scope(r->device); delete r; } catch (const HipFail&) { delete r; }
}

int sonic_r1cs_device(const sonic_r1cs_t* r) { return r ? r->device : -1; }

int sonic_r1cs_shape(const sonic_r1cs_t* r, int64_t out[4]) {
  if (!r || !out) { set_error("sonic_r1cs_shape: bad argument"); return SONIC_ERR_INVALID_ARG; }
  out[0] = r->shape.n; out[1] = r->shape.Q; out[2] = r->shape.nnz; out[3] = r->shape.g;
  return SONIC_OK;
}

int sonic_r1cs_circuit(const sonic_r1cs_t* r, int64_t* row_ptr, int64_t* col, uint8_t* val, uint8_t* cs_fixed) {
  API_HOST_BEGIN
  if (!r || !row_ptr || !col || !val || !cs_fixed) { set_error("sonic_r1cs_circuit: bad argument"); return SONIC_ERR_INVALID_ARG; }
  r1cs_compile(r->view, row_ptr, col, val, cs_fixed);
  API_END
}

int sonic_r1cs_row_chunk(void) { return R1CS_ROW_CHUNK; }

int sonic_r1cs_assign(sonic_r1cs_t* r, int64_t K, const void* z, int kind, int on_device, int64_t z_stride, void* hip_stream, void* d_aL, void* d_aR, void* d_aO,
                      int64_t out_stride, uint8_t* out_cs, int64_t* out_bad) {
  API_BEGIN_ON(r ? r->device : -1)
  const char* who = "sonic_r1cs_assign";
  if (!r || !z || !d_aL || !d_aR || !d_aO) { set_error("%s: bad argument", who); return SONIC_ERR_INVALID_ARG; }
  const long m = r->view.m, N = r->view.N, n_pub = r->view.n_pub, n = r->shape.n, Q = r->shape.Q;
  if (K < 1 || K > MSM_TABLE_MAX_TERMS / std::max(n, N)) { set_error("%s: K = %lld outside [1, 2^26 / max(n, N)]", who, (long long)K); return SONIC_ERR_INVALID_ARG; }
  if (kind != SONIC_WIT_FR32 && kind != SONIC_WIT_I64) { set_error("%s: unknown kind %d (SONIC_WIT_FR32 = 0, SONIC_WIT_I64 = 1)", who, kind); return SONIC_ERR_INVALID_ARG; }
  if (on_device != 0 && on_device != 1) { set_error("%s: on_device = %d is neither 0 (host) nor 1 (device)", who, on_device); return SONIC_ERR_INVALID_ARG; }
  const long elem = wit_elem_bytes(kind), packed = N * elem;
  if (z_stride != 0 && z_stride < packed) { set_error("%s: z_stride %lld is below N * element size = %ld (0 = packed)", who, (long long)z_stride, packed); return SONIC_ERR_INVALID_ARG; }
  const long zs = z_stride ? (long)z_stride : packed;
  if (on_device) {
    if ((uintptr_t)z % (uintptr_t)elem) { set_error("%s: device pointer z is not %ld-byte aligned", who, elem); return SONIC_ERR_INVALID_ARG; }
    if (zs % elem) { set_error("%s: z_stride %ld of a device source is not a multiple of %ld", who, zs, elem); return SONIC_ERR_INVALID_ARG; }
  } else if (hip_stream) { set_error("%s: hip_stream is for device sources (a host source is complete when the call is made)", who); return SONIC_ERR_INVALID_ARG; }
  if (out_stride != 0 && (out_stride < 32 * n || out_stride % 32)) { set_error("%s: out_stride %lld must be a multiple of 32 and at least 32 n = %ld (0 = packed)", who, (long long)out_stride, 32 * n); return SONIC_ERR_INVALID_ARG; }
  const long os = out_stride ? (long)out_stride : 32 * n;
  void* outs[3] = {d_aL, d_aR, d_aO};
  const char* names[3] = {"d_aL", "d_aR", "d_aO"};
  for (int k = 0; k < 3; k++)
    if ((uintptr_t)outs[k] % 32) { set_error("%s: device pointer %s is not 32-byte aligned", who, names[k]); return SONIC_ERR_INVALID_ARG; }
  std::lock_guard<std::mutex> g(r->mu);
  for (int k = 0; k < 3; k++) {
    const int rc = r1cs_on_device(who, names[k], outs[k], (size_t)(K - 1) * (size_t)os + 32 * (size_t)n, r->device);
    if (rc) return rc;
  }
  if (on_device) {
    const int rc = r1cs_on_device(who, "z", z, (size_t)(K - 1) * (size_t)zs + (size_t)packed, r->device);
    if (rc) return rc;
  }
  hipStream_t st = r->st;
  WitnessReady ready;
  if (on_device && hip_stream) {
    WitnessView wv;
    wv.on_device = true; wv.hip_stream = hip_stream;
    ready.record(wv);
    HIP_OK(hipStreamWaitEvent(st, ready.ev, 0));
  }
  // witnesses per chunk
  long Kc = std::min<long>(K, std::max<long>(1, R1_STAGE_ELEMS / std::max(N, 3 * m)));
  Kc = std::min<long>(Kc, 65535);                              // grid.y
  if (const char* cap = getenv("SONIC_R1CS_STAGE")) { const long c = atol(cap); if (c >= 1) Kc = std::min(Kc, c); }
  const long nchunks = (K + Kc - 1) / Kc;
  if (!on_device) r->raw.ensure((size_t)Kc * (size_t)packed);
  r->zm.ensure(sizeof(Fr) * (size_t)Kc * (size_t)N);
  r->sums.ensure(sizeof(Fr) * (size_t)Kc * 3 * (size_t)m);
  r->pub.ensure(sizeof(Fr) * (size_t)Kc * (size_t)std::max<long>(1, n_pub));
  r->bad.ensure(16 * (size_t)Kc);
  const unsigned long long status_init[2] = {0, ~0ull};
  HIP_OK(hipMemcpyAsync(r->status.p, status_init, 16, hipMemcpyHostToDevice, st));
  const uint8_t* zb = static_cast<const uint8_t*>(z);
  auto ingest = [&](long k0, long nb) {
    const uint8_t* src = zb + (size_t)k0 * (size_t)zs;
    long stride = zs;
    if (!on_device) {
      uint8_t* raw = r->raw.as<uint8_t>();
      if (zs == packed) HIP_OK(hipMemcpyAsync(raw, src, (size_t)nb * (size_t)packed, hipMemcpyHostToDevice, st));
      else for (long b = 0; b < nb; b++) HIP_OK(hipMemcpyAsync(raw + (size_t)b * (size_t)packed, src + (size_t)b * (size_t)zs, (size_t)packed, hipMemcpyHostToDevice, st));
      src = raw; stride = packed;
    }
    const dim3 grid((unsigned)ceil_div(N, R1_BLOCK), (unsigned)nb);
    if (kind == SONIC_WIT_I64) LAUNCH((k_r1cs_ingest<SONIC_WIT_I64>), grid, R1_BLOCK, 0, st, src, stride, N, n_pub, k0, r->zm.as<Fr>(), r->pub.as<Fr>(), r->status.as<unsigned long long>());
    else LAUNCH((k_r1cs_ingest<SONIC_WIT_FR32>), grid, R1_BLOCK, 0, st, src, stride, N, n_pub, k0, r->zm.as<Fr>(), r->pub.as<Fr>(), r->status.as<unsigned long long>());
  };      // (the raw plane is reused by the next chunk: the stream runs copy and kernel in order)
  // every witness is checked before anything is written: a refusal leaves the outputs untouched.  One chunk: ingested once.
  for (long k0 = 0; k0 < K; k0 += Kc) ingest(k0, std::min<long>(Kc, K - k0));
  unsigned long long status[2];
  HIP_OK(hipMemcpyAsync(status, r->status.p, 16, hipMemcpyDeviceToHost, st));
  HIP_OK(hipStreamSynchronize(st));
  if ((int)status[0]) return flags_to_status((int)status[0], who);
  if (status[1] != ~0ull) { set_error("%s: witness %llu has z[0] != 1 (column 0 is the constant one)", who, status[1]); return SONIC_ERR_INVALID_ARG; }
  std::vector<unsigned long long> bad_init(2 * (size_t)Kc), bad_host(2 * (size_t)Kc);
  for (long b = 0; b < Kc; b++) { bad_init[2 * (size_t)b] = 0; bad_init[2 * (size_t)b + 1] = ~0ull; }
  std::vector<uint8_t> pub_host(32 * (size_t)Kc * (size_t)std::max<long>(1, n_pub));
  if (out_cs && r->cs_fixed.empty()) {
    std::vector<int64_t> rp(3 * (size_t)Q + 1), cl((size_t)r->shape.nnz);
    std::vector<uint8_t> vl(32 * (size_t)r->shape.nnz);
    r->cs_fixed.resize(32 * (size_t)Q);
    r1cs_compile(r->view, rp.data(), cl.data(), vl.data(), r->cs_fixed.data());
  }
  for (long k0 = 0; k0 < K; k0 += Kc) {
    const long nb = std::min<long>(Kc, K - k0);
    if (nchunks > 1) ingest(k0, nb);
    const int32_t *rp = r->row_ptr.as<int32_t>(), *cl = r->col.as<int32_t>();
    const Fr* vl = r->val.as<Fr>();
    if (r->n_short) LAUNCH(k_r1cs_short, dim3((unsigned)ceil_div(r->n_short, R1_BLOCK), (unsigned)nb), R1_BLOCK, 0, st, rp, cl, vl, (const int32_t*)r->short_rows.as<int32_t>(), r->n_short, 3 * m, (const Fr*)r->zm.as<Fr>(), N, r->sums.as<Fr>());
    if (r->n_long) LAUNCH(k_r1cs_long, dim3((unsigned)r->n_long, (unsigned)nb), R1_BLOCK, 0, st, rp, cl, vl, (const int32_t*)r->long_rows.as<int32_t>(), 3 * m, (const Fr*)r->zm.as<Fr>(), N, r->sums.as<Fr>());
    HIP_OK(hipMemcpyAsync(r->bad.p, bad_init.data(), 16 * (size_t)nb, hipMemcpyHostToDevice, st));
    const size_t off = (size_t)k0 * (size_t)os;
    LAUNCH(k_r1cs_fill, dim3((unsigned)ceil_div(n, R1_BLOCK), (unsigned)nb), R1_BLOCK, 0, st, (const Fr*)r->sums.as<Fr>(), (const Fr*)r->zm.as<Fr>(), m, N, n, static_cast<uint8_t*>(d_aL) + off,
           static_cast<uint8_t*>(d_aR) + off, static_cast<uint8_t*>(d_aO) + off, os, r->bad.as<unsigned long long>());
    if (out_bad) HIP_OK(hipMemcpyAsync(bad_host.data(), r->bad.p, 16 * (size_t)nb, hipMemcpyDeviceToHost, st));
    if (out_cs && n_pub) HIP_OK(hipMemcpyAsync(pub_host.data(), r->pub.p, 32 * (size_t)nb * (size_t)n_pub, hipMemcpyDeviceToHost, st));
    HIP_OK(hipStreamSynchronize(st));       // the staging buffers and the host copies are reused by the next chunk
    for (long b = 0; out_bad && b < nb; b++) {
      out_bad[2 * (k0 + b)] = (int64_t)bad_host[2 * (size_t)b];
      out_bad[2 * (k0 + b) + 1] = bad_host[2 * (size_t)b] ? (int64_t)bad_host[2 * (size_t)b + 1] : -1;
    }
    for (long b = 0; out_cs && b < nb; b++) {
      uint8_t* dst = out_cs + 32 * (size_t)(k0 + b) * (size_t)Q;
      memcpy(dst, r->cs_fixed.data(), 32 * (size_t)Q);
      if (n_pub) memcpy(dst + 32 * (size_t)(3 * m), pub_host.data() + 32 * (size_t)b * (size_t)n_pub, 32 * (size_t)n_pub);
    }
  }
  API_END
}

}  // extern "C"
