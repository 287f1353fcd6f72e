// One resident circuit, many statements (include/sonic_hip.h, "One circuit, many statements").  In the reference a statement is
// (ArithCircuit, Assignment) with cs = wL.aL + wR.aR + wO.aO (test/Test/Reference.hs:138): the gate weights are the program, the constants
// are the public inputs and change with every proof.  This file holds what a prover handle needs for that:
//   sonic_prover_eval_constraints   cs of B assignments under the handle's resident weights, and the multiplication gates they break -- the
//                                   hot path: a sparse (CSR handle) or dense matrix-vector product over Fr, on the device
//   sonic_prover_set_constants      the handle's cs overwritten in place
// and the host-only halves of the circuit digest (fs.hpp: midstate + resume).  sonic_prove_batch_statements is beside sonic_prove_batch in
// prove_multi.hip, the verifier's side in verify_batch.hip.
//
// Kernels.  Fr sums are exact, so the result does not depend on the order of summation and there are no atomics in them:
//   k_cs_csr     grid (chunks / 4, b): one wave per chunk of at most CSR_CHUNK entries of one stacked row (the handle's chunk_row /
//                chunk_begin, the cut k_s_of_u_csr uses: a row of n entries is n / 512 waves, an empty row none), 8 products per lane, a
//                shuffle reduction, one partial per (b, chunk)
//   k_cs_dense   grid (blocks of 256 gates, b): a thread holds its gate's aL, aR, aO and walks the Q rows; per row a shuffle reduction per
//                wave and an LDS sum of the block's four waves, one partial per (b, q, block)
//   k_cs_finish  grid (Q, b): adds the partials of rows q, Q + q, 2Q + q (sparse) or of row q's blocks (dense) in LDS, writes canonical bytes
//   k_gates      grid (blocks of 256 gates, b): aL[i] aR[i] != aO[i]; a block reduction of the count and of the smallest index, then one
//                atomic add and one atomic min per block on the assignment's pair
// Assignments pass through a staging buffer of STAGE_ELEMS field elements per vector in chunks of whole assignments, so B is bounded by the
// host's memory, not the device's.
#include "prover.hpp"

namespace sonic {
namespace {

constexpr int CS_BLOCK = 256;                 // four wave64
constexpr long STAGE_ELEMS = 1L << 20;        // per vector: 3 x 32 MB of staging at most (one assignment when n is larger)
constexpr long PARTIAL_ELEMS = 1L << 20;      // partial sums per chunk of assignments: 32 MB at most (one assignment's when it needs more)

__device__ __forceinline__ Fr cs_shfl_xor(const Fr& a, int mask) {
  Fr o;
#pragma unroll
  for (int k = 0; k < 8; k++) o.l[k] = (uint32_t)__shfl_xor((int)a.l[k], mask, 64);
  return o;
}
__device__ __forceinline__ Fr cs_wave_sum(Fr acc) {
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) acc = fp_add(acc, cs_shfl_xor(acc, o));
  return acc;
}

// a: the three vectors of assignment b at aL + b * stride, aR + ..., aO + ... (Montgomery)
__global__ __launch_bounds__(CS_BLOCK) void k_cs_csr(const int32_t* __restrict__ row_ptr, const int32_t* __restrict__ col, const Fr* __restrict__ val,
                                                     const int32_t* __restrict__ chunk_row, const int32_t* __restrict__ chunk_begin, long nchunks, int Q,
                                                     const Fr* __restrict__ aL, const Fr* __restrict__ aR, const Fr* __restrict__ aO, long stride,
                                                     Fr* __restrict__ partial) {
  const long c = (long)blockIdx.x * 4 + (threadIdx.x >> 6);      // one wave per chunk
  const int lane = threadIdx.x & 63;
  if (c >= nchunks) return;                                      // (wave-uniform: no barrier below)
  const long b = blockIdx.y;
  const int r = chunk_row[c], m = r / Q;
  const int k0 = chunk_begin[c];
  const int k1 = min(k0 + CSR_CHUNK, row_ptr[r + 1]);
  const Fr* a = (m == 0 ? aL : m == 1 ? aR : aO) + b * stride;
  Fr acc = Fr::zero();
  for (int k = k0 + lane; k < k1; k += 64) acc = fp_add(acc, fp_mul(val[k], a[col[k]]));
  acc = cs_wave_sum(acc);
  if (lane == 0) partial[b * nchunks + c] = acc;
}

__global__ __launch_bounds__(CS_BLOCK) void k_cs_dense(const Fr* __restrict__ wL, const Fr* __restrict__ wR, const Fr* __restrict__ wO, long n, int Q,
                                                       const Fr* __restrict__ aL, const Fr* __restrict__ aR, const Fr* __restrict__ aO, long stride,
                                                       long nblk, Fr* __restrict__ partial) {
  __shared__ Fr sh[CS_BLOCK / 64];
  const long b = blockIdx.y, i = (long)blockIdx.x * CS_BLOCK + threadIdx.x;
  const bool in = i < n;
  Fr l = Fr::zero(), r = Fr::zero(), o = Fr::zero();
  if (in) { l = aL[b * stride + i]; r = aR[b * stride + i]; o = aO[b * stride + i]; }
  for (int q = 0; q < Q; q++) {
    Fr acc = Fr::zero();
    if (in) {
      const long at = (long)q * n + i;
      acc = fp_add(fp_add(fp_mul(wL[at], l), fp_mul(wR[at], r)), fp_mul(wO[at], o));
    }
    acc = cs_wave_sum(acc);
    if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = acc;
    __syncthreads();
    if (threadIdx.x == 0) partial[(b * Q + q) * nblk + blockIdx.x] = fp_add(fp_add(sh[0], sh[1]), fp_add(sh[2], sh[3]));
    __syncthreads();
  }
}

// row_chunk != null: the partials of (b, chunk), rows q, Q + q, 2Q + q; null: those of (b, q, block), `per` blocks each
__global__ __launch_bounds__(CS_BLOCK) void k_cs_finish(const int32_t* __restrict__ row_chunk, long per, int Q, const Fr* __restrict__ partial, Fr* __restrict__ out) {
  __shared__ Fr sh[CS_BLOCK];
  const int q = blockIdx.x;
  const long b = blockIdx.y;
  Fr acc = Fr::zero();
  if (row_chunk) {
    const Fr* p = partial + b * per;
    for (int m = 0; m < 3; m++) {
      const int r = m * Q + q;
      for (int c = row_chunk[r] + (int)threadIdx.x; c < row_chunk[r + 1]; c += CS_BLOCK) acc = fp_add(acc, p[c]);
    }
  } else {
    const Fr* p = partial + (b * Q + q) * per;
    for (long c = threadIdx.x; c < per; c += CS_BLOCK) acc = fp_add(acc, p[c]);
  }
  sh[threadIdx.x] = acc;
  __syncthreads();
  for (int s = CS_BLOCK / 2; s >= 1; s >>= 1) {
    if ((int)threadIdx.x < s) sh[threadIdx.x] = fp_add(sh[threadIdx.x], sh[threadIdx.x + s]);
    __syncthreads();
  }
  if (threadIdx.x == 0) out[b * Q + q] = fp_from_mont(sh[0]);
}

// gates[2 b] += the broken gates of the block, gates[2 b + 1] = min with the smallest broken index (the host sets it to ~0 first)
__global__ __launch_bounds__(CS_BLOCK) void k_gates(const Fr* __restrict__ aL, const Fr* __restrict__ aR, const Fr* __restrict__ aO, long stride, long n,
                                                    unsigned long long* __restrict__ gates) {
  __shared__ unsigned long long first[CS_BLOCK];
  __shared__ unsigned int count[CS_BLOCK];
  const long b = blockIdx.y, i = (long)blockIdx.x * CS_BLOCK + threadIdx.x;
  bool bad = false;
  if (i < n) bad = !(fp_mul(aL[b * stride + i], aR[b * stride + i]) == aO[b * stride + i]);
  first[threadIdx.x] = bad ? (unsigned long long)i : ~0ull;
  count[threadIdx.x] = bad ? 1u : 0u;
  __syncthreads();
  for (int s = CS_BLOCK / 2; s >= 1; s >>= 1) {
    if ((int)threadIdx.x < s) {
      count[threadIdx.x] += count[threadIdx.x + s];
      if (first[threadIdx.x + s] < first[threadIdx.x]) first[threadIdx.x] = first[threadIdx.x + s];
    }
    __syncthreads();
  }
  if (threadIdx.x == 0 && count[0]) {
    atomicAdd(&gates[2 * b], (unsigned long long)count[0]);
    atomicMin(&gates[2 * b + 1], first[0]);
  }
}

}  // namespace
}  // namespace sonic

// What sonic_prover_eval_constraints and sonic_prover_eval_constraints_src share, under p->mu and inside the caller's device scope: B
// assignments in chunks through the staging planes -- three host buffers of canonical bytes (copied, then converted in place), or a
// witness source `w` (witness_src.hpp: read by the one launch of k_witness_ingest; a device source where it lies) -- or, with neither, the
// handle's resident assignment.
static int eval_constraints_run(const char* who, sonic_prover_t* p, int64_t B, const uint8_t* aL, const uint8_t* aR, const uint8_t* aO, const WitnessView* w,
                                uint8_t* out_cs, int64_t* out_gates) {
  const bool resident = !aL && !w;
  const long n = p->n, Q = p->Q;
  hipStream_t st = p->st;
  sonic_prover::CsrBufs& sp = p->sp;
  sonic_prover::StatementBufs& sb = p->stm;
  const long nblk = (n + CS_BLOCK - 1) / CS_BLOCK;
  const long per_b = p->csr ? sp.nchunks : Q * nblk;            // partial sums per assignment
  long Bc = std::min<long>(B, std::max<long>(1, STAGE_ELEMS / n));
  Bc = std::min<long>(Bc, std::max<long>(1, PARTIAL_ELEMS / std::max<long>(1, per_b)));
  Bc = std::min<long>(Bc, 65535);                              // grid.y
  if (!resident) sb.stage.ensure(sizeof(Fr) * 3 * (size_t)Bc * (size_t)n);
  sb.partial.ensure(sizeof(Fr) * (size_t)Bc * (size_t)std::max<long>(1, per_b));
  sb.out.ensure(sizeof(Fr) * (size_t)Bc * (size_t)Q);
  sb.gates.ensure(16 * (size_t)Bc);
  std::vector<unsigned long long> gates_init(2 * (size_t)Bc), gates_host(2 * (size_t)Bc);
  for (long b = 0; b < Bc; b++) { gates_init[2 * (size_t)b] = 0; gates_init[2 * (size_t)b + 1] = ~0ull; }
  HIP_OK(hipMemsetAsync(p->flags.p, 0, 4, st));
  for (long b0 = 0; b0 < B; b0 += Bc) {
    const long nb = std::min<long>(Bc, B - b0);
    const Fr *dL = p->aL.as<Fr>(), *dR = p->aR.as<Fr>(), *dO = p->aO.as<Fr>();
    if (w) {
      Fr* s = sb.stage.as<Fr>();
      witness_load_enqueue(p, st, w->block(b0), nb, s, s + nb * n, s + 2 * nb * n, n, p->flags.as<int>());
      dL = s; dR = s + nb * n; dO = s + 2 * nb * n;
    } else if (!resident) {
      Fr* s = sb.stage.as<Fr>();
      const size_t bytes = 32 * (size_t)nb * (size_t)n, off = 32 * (size_t)b0 * (size_t)n;
      HIP_OK(hipMemcpyAsync(s, aL + off, bytes, hipMemcpyHostToDevice, st));
      HIP_OK(hipMemcpyAsync(s + nb * n, aR + off, bytes, hipMemcpyHostToDevice, st));
      HIP_OK(hipMemcpyAsync(s + 2 * nb * n, aO + off, bytes, hipMemcpyHostToDevice, st));
      fr_to_mont_enqueue(st, s, 3 * nb * n, p->flags.as<int>());
      dL = s; dR = s + nb * n; dO = s + 2 * nb * n;
    }
    Fr* partial = sb.partial.as<Fr>();
    if (p->csr) {
      if (sp.nchunks > 0)
        LAUNCH(k_cs_csr, dim3((unsigned)ceil_div(sp.nchunks, 4L), (unsigned)nb), CS_BLOCK, 0, st, (const int32_t*)sp.row_ptr.as<int32_t>(), (const int32_t*)sp.col.as<int32_t>(),
               (const Fr*)sp.val.as<Fr>(), (const int32_t*)sp.chunk_row.as<int32_t>(), (const int32_t*)sp.chunk_begin.as<int32_t>(), sp.nchunks, (int)Q, dL, dR, dO, n, partial);
      LAUNCH(k_cs_finish, dim3((unsigned)Q, (unsigned)nb), CS_BLOCK, 0, st, (const int32_t*)sp.row_chunk.as<int32_t>(), sp.nchunks, (int)Q, (const Fr*)partial, sb.out.as<Fr>());
    } else {
      LAUNCH(k_cs_dense, dim3((unsigned)nblk, (unsigned)nb), CS_BLOCK, 0, st, (const Fr*)p->wL.as<Fr>(), (const Fr*)p->wR.as<Fr>(), (const Fr*)p->wO.as<Fr>(), n, (int)Q, dL, dR, dO, n,
             nblk, partial);
      LAUNCH(k_cs_finish, dim3((unsigned)Q, (unsigned)nb), CS_BLOCK, 0, st, (const int32_t*)nullptr, nblk, (int)Q, (const Fr*)partial, sb.out.as<Fr>());
    }
    HIP_OK(hipMemcpyAsync(out_cs + 32 * (size_t)b0 * (size_t)Q, sb.out.p, 32 * (size_t)nb * (size_t)Q, hipMemcpyDeviceToHost, st));
    const bool gates_derived = w && !w->aO;      // aO = aL aR by construction: no gate can break, and none is looked at
    if (out_gates && !gates_derived) {
      HIP_OK(hipMemcpyAsync(sb.gates.p, gates_init.data(), 16 * (size_t)nb, hipMemcpyHostToDevice, st));
      LAUNCH(k_gates, dim3((unsigned)nblk, (unsigned)nb), CS_BLOCK, 0, st, dL, dR, dO, n, n, sb.gates.as<unsigned long long>());
      HIP_OK(hipMemcpyAsync(gates_host.data(), sb.gates.p, 16 * (size_t)nb, hipMemcpyDeviceToHost, st));
    }
    HIP_OK(hipStreamSynchronize(st));       // the staging buffer and gates_host are reused by the next chunk
    for (long b = 0; out_gates && gates_derived && b < nb; b++) { out_gates[2 * (b0 + b)] = 0; out_gates[2 * (b0 + b) + 1] = -1; }
    for (long b = 0; out_gates && !gates_derived && b < nb; b++) {
      out_gates[2 * (b0 + b)] = (int64_t)gates_host[2 * (size_t)b];
      out_gates[2 * (b0 + b) + 1] = gates_host[2 * (size_t)b] ? (int64_t)gates_host[2 * (size_t)b + 1] : -1;
    }
  }
  const int f = read_flags(st, p->flags);
  if (f) return flags_to_status(f, who);
  return SONIC_OK;
}

extern "C" {

int sonic_prover_eval_constraints(sonic_prover_t* p, int64_t B, const uint8_t* aL, const uint8_t* aR, const uint8_t* aO, uint8_t* out_cs, int64_t* out_gates) {
  API_BEGIN_ON(p ? p->device : -1)
  const char* who = "sonic_prover_eval_constraints";
  if (!p || !out_cs) { set_error("%s: bad argument", who); return SONIC_ERR_INVALID_ARG; }
  const bool resident = !aL && !aR && !aO;
  if (!resident && !(aL && aR && aO)) { set_error("%s: aL, aR, aO must be given together (or all NULL: the handle's resident assignment)", who); return SONIC_ERR_INVALID_ARG; }
  const long n = p->n;
  if (B < 1 || B > MSM_TABLE_MAX_TERMS / n) { set_error("%s: B = %lld outside [1, 2^26 / n]", who, (long long)B); return SONIC_ERR_INVALID_ARG; }
  if (resident && B != 1) { set_error("%s: the resident assignment is one assignment (B = 1)", who); return SONIC_ERR_INVALID_ARG; }
  std::lock_guard<std::mutex> g(p->mu);
  if (resident && !p->have_assignment) { set_error("%s: no assignment set", who); return SONIC_ERR_INVALID_ARG; }
  if (p->in_flight) { set_error("%s: a submitted proof is still reading the handle's buffers (collect it first)", who); return SONIC_ERR_INVALID_ARG; }
  EnqueueLock enq(p);
  return eval_constraints_run(who, p, B, aL, aR, aO, nullptr, out_cs, out_gates);
  API_CATCH
}

// the same over a witness source (include/sonic_hip.h, "Witness sources"): assignment b is block b of each vector
int sonic_prover_eval_constraints_src(sonic_prover_t* p, int64_t B, const sonic_witness_src_t* src, uint8_t* out_cs, int64_t* out_gates) {
  API_BEGIN_ON(p ? p->device : -1)
  const char* who = "sonic_prover_eval_constraints_src";
  if (!p || !out_cs) { set_error("%s: bad argument", who); return SONIC_ERR_INVALID_ARG; }
  const long n = p->n;
  if (B < 1 || B > MSM_TABLE_MAX_TERMS / n) { set_error("%s: B = %lld outside [1, 2^26 / n]", who, (long long)B); return SONIC_ERR_INVALID_ARG; }
  WitnessView v;
  int rc = witness_view_of(who, src, n, B, &v);
  if (rc) return rc;
  std::lock_guard<std::mutex> g(p->mu);
  if (p->in_flight) { set_error("%s: a submitted proof is still reading the handle's buffers (collect it first)", who); return SONIC_ERR_INVALID_ARG; }
  rc = witness_on_device_of(who, v, n, B, p->device);
  if (rc) return rc;
  WitnessReady ready;
  ready.record(v);
  EnqueueLock enq(p);
  if (ready.ev) HIP_OK(hipStreamWaitEvent(p->st, ready.ev, 0));
  return eval_constraints_run(who, p, B, nullptr, nullptr, nullptr, &v, out_cs, out_gates);
  API_CATCH
}

int sonic_prover_set_constants(sonic_prover_t* p, const uint8_t* cs) {
  API_BEGIN_ON(p ? p->device : -1)
  if (!p || !cs) { set_error("sonic_prover_set_constants: bad argument"); return SONIC_ERR_INVALID_ARG; }
  std::lock_guard<std::mutex> g(p->mu);
  if (p->in_flight) { set_error("sonic_prover_set_constants: a submitted proof is still reading the current constants (collect it first)"); return SONIC_ERR_INVALID_ARG; }
  // checked on the host, before anything is written: a refused cs leaves the old constants
  for (long q = 0; q < p->Q; q++) {
    Fr k;
    memcpy(k.l, cs + 32 * q, 32);
    if (!fp_is_canonical(k)) { set_error("sonic_prover_set_constants: cs[%ld] is not a canonical field element", q); return SONIC_ERR_BAD_ENCODING; }
  }
  // in place: p->cs keeps its address (DevBuf::ensure of the size it has), so a captured proof graph stays valid and is kept
  EnqueueLock enq(p);
  HIP_OK(hipMemsetAsync(p->flags.p, 0, 4, p->st));
  upload_fr_mont(p->st, p->cs, cs, p->Q, p->flags.as<int>());
  HIP_OK(hipStreamSynchronize(p->st));
  API_END
}

// ---- the circuit digest in two halves (fs.hpp); host only, no device ----
int sonic_fs_circuit_midstate(int64_t n, int64_t Q, const uint8_t* wL, const uint8_t* wR, const uint8_t* wO, uint8_t out[SONIC_FS_MIDSTATE_SIZE]) {
  return circuit_midstate_checked("sonic_fs_circuit_midstate", dense_view(n, Q, wL, wR, wO, nullptr), out);
}
int sonic_fs_circuit_midstate_csr(int64_t n, int64_t Q, const int64_t* row_ptr, const int64_t* col, const uint8_t* val, uint8_t out[SONIC_FS_MIDSTATE_SIZE]) {
  return circuit_midstate_checked("sonic_fs_circuit_midstate_csr", csr_view(n, Q, row_ptr, col, val, nullptr), out);
}
int sonic_fs_circuit_digest_resume(const uint8_t midstate[SONIC_FS_MIDSTATE_SIZE], const uint8_t* cs, uint8_t out[32]) {
  if (!midstate || !cs || !out) { set_error("sonic_fs_circuit_digest_resume: bad argument"); return SONIC_ERR_INVALID_ARG; }
  int64_t bad = -1;
  const int rc = fs_circuit_digest_resume(midstate, cs, out, &bad);
  if (rc == 1) { set_error("sonic_fs_circuit_digest_resume: the midstate's length field is not 36 + 96 Q n for its Q (or bytes follow the pending ones)"); return SONIC_ERR_INVALID_ARG; }
  if (rc == 2) { set_error("sonic_fs_circuit_digest_resume: cs[%lld] is not a canonical field element", (long long)bad); return SONIC_ERR_BAD_ENCODING; }
  return SONIC_OK;
}
int sonic_verify_batch_digest_v2(int64_t n, int64_t Q, int64_t d, const uint8_t circuit_digest[32], const uint8_t srs_id[32], int64_t K, const uint8_t* proofs,
                                 const uint8_t* challenges, const uint8_t* cs, uint8_t out[32]) {
  if (n < 1 || Q < 1 || d < 1 || K < 0 || !circuit_digest || !srs_id || !out || (K > 0 && (!proofs || !challenges || !cs))) { set_error("sonic_verify_batch_digest_v2: bad argument"); return SONIC_ERR_INVALID_ARG; }
  fs_batch_digest_v2(n, Q, d, circuit_digest, srs_id, K, proofs, sonic_proof_size(Q), challenges, cs, out);
  return SONIC_OK;
}

}  // extern "C"
