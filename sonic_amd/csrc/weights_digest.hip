// Weights digest v2 and circuit digest v2 (the definition: fs.hpp; the hash itself: weights_tree.hpp, shared with the host): a SHA-256 tree
// over the entries of a handle's resident CSR -- int32 indices, Montgomery values, where the prover handle (CsrBufs) and the verifier handle
// keep them.  One thread per digest; a leaf's thread finds the row of its first entry by binary search in row_ptr, walks row_ptr beside its
// 16 entries and converts each value in registers.  One launch per level; the root stays in `tree`, 32 bytes come back.  Nothing dense is
// ever formed: the cost is O(nnz), where circuit digest v1 hashes 96 Q n bytes.
//
// As in witness.hip a block is ONE wave: a thread runs 1 + 16 SHA blocks in a row, so the leaves spread over as many CUs as there are waves.
#include "prover.hpp"
#include "weights_tree.hpp"

namespace sonic {

constexpr int WD_BLOCK = 64;

__global__ __launch_bounds__(WD_BLOCK) void k_weights_leaves(const int32_t* __restrict__ row_ptr, const int32_t* __restrict__ col, const Fr* __restrict__ val, long R,
                                                             long nnz, long leaves, uint32_t* __restrict__ out) {
  const long i = (long)blockIdx.x * WD_BLOCK + threadIdx.x;
  if (i >= leaves) return;
  uint32_t d[8];
  wd_leaf<int32_t, true>(row_ptr, col, val, R, nnz, i, d);
  uint4* o = reinterpret_cast<uint4*>(out + 8 * i);
  o[0] = make_uint4(d[0], d[1], d[2], d[3]);
  o[1] = make_uint4(d[4], d[5], d[6], d[7]);
}

__global__ __launch_bounds__(WD_BLOCK) void k_weights_nodes(const uint32_t* __restrict__ below, long c, int level, long nodes, uint32_t* __restrict__ out) {
  const long j = (long)blockIdx.x * WD_BLOCK + threadIdx.x;
  if (j >= nodes) return;
  uint32_t d[8];
  wd_node(below, c, level, j, d);
  for (int k = 0; k < 8; k++) out[8 * j + k] = d[k];
}

// queues the whole tree over a resident CSR of R = 3Q rows and nnz entries (row_ptr: R + 1) into `tree` (wd_tree_digests(nnz) x 8 words,
// grown to fit) and returns where the root's eight state words will be
const uint32_t* weights_tree_enqueue(hipStream_t st, const int32_t* row_ptr, const int32_t* col, const Fr* val, long R, long nnz, DevBuf& tree) {
  tree.ensure(32 * (size_t)wd_tree_digests(nnz));
  long c = wd_leaf_count(nnz);
  uint32_t* below = tree.as<uint32_t>();
  LAUNCH(k_weights_leaves, ceil_div(c, WD_BLOCK), WD_BLOCK, 0, st, row_ptr, col, val, R, nnz, c, below);
  for (int level = 1; c > 1; level++) {
    uint32_t* here = below + 8 * c;
    const long m = wt_node_count(c);
    LAUNCH(k_weights_nodes, ceil_div(m, WD_BLOCK), WD_BLOCK, 0, st, (const uint32_t*)below, c, level, m, here);
    below = here; c = m;
  }
  return below;
}

}  // namespace sonic

extern "C" {

// ---- host only, no device: the ABI's CSR (int64 indices, canonical values) through the same functions --------------------------------
int sonic_fs_weights_digest_v2_csr(int64_t n, int64_t Q, const int64_t* row_ptr, const int64_t* col, const uint8_t* val, uint8_t out[32]) {
  API_HOST_BEGIN
  const char* who = "sonic_fs_weights_digest_v2_csr";
  if (!out) { set_error("%s: bad argument", who); return SONIC_ERR_INVALID_ARG; }
  const int rc = circuit_validate(who, csr_view(n, Q, row_ptr, col, val, nullptr));
  if (rc) return rc;
  const long R = 3 * Q, nnz = (long)row_ptr[R];
  std::vector<uint32_t> tree(8 * (size_t)wd_tree_digests(nnz));
  uint8_t root[32];
  wd_tree_host<int64_t, false>(row_ptr, col, val, R, tree.data(), root);
  fs_weights_digest_v2(n, Q, nnz, root, out);
  API_END
}

int sonic_fs_circuit_digest_v2(const uint8_t weights_digest[32], int64_t Q, const uint8_t* cs, uint8_t out[32]) {
  if (!weights_digest || Q < 1 || !cs || !out) { set_error("sonic_fs_circuit_digest_v2: bad argument (need Q >= 1)"); return SONIC_ERR_INVALID_ARG; }
  int64_t bad = -1;
  if (fs_circuit_digest_v2(weights_digest, Q, cs, out, &bad) != 0) {
    set_error("sonic_fs_circuit_digest_v2: cs[%lld] is not a canonical field element", (long long)bad);
    return SONIC_ERR_BAD_ENCODING;
  }
  return SONIC_OK;
}

// ---- on the GPU, from the handle's resident CSR -------------------------------------------------------------------------------------
int sonic_prover_weights_digest_v2(sonic_prover_t* p, uint8_t out[32]) {
  API_BEGIN_ON(p ? p->device : -1)
  if (!p || !out) { set_error("sonic_prover_weights_digest_v2: bad argument"); return SONIC_ERR_INVALID_ARG; }
  std::lock_guard<std::mutex> g(p->mu);
  if (p->in_flight) { set_error("sonic_prover_weights_digest_v2: a submitted proof has not been collected yet"); return SONIC_ERR_INVALID_ARG; }
  if (!p->csr) {
    set_error("sonic_prover_weights_digest_v2: the handle holds dense weights; weights digest v2 is defined over CSR entries: make the handle from CSR (sonic_prover_new_csr)");
    return SONIC_ERR_INVALID_ARG;
  }
  if (!p->have_weights_digest_v2) {
    EnqueueLock enq(p);
    const sonic_prover::CsrBufs& b = p->sp;
    const uint32_t* root_d = weights_tree_enqueue(p->st, b.row_ptr.as<int32_t>(), b.col.as<int32_t>(), b.val.as<Fr>(), 3 * p->Q, b.nnz, p->wdtree);
    HIP_OK(hipMemcpyAsync(p->h_root, root_d, 32, hipMemcpyDeviceToHost, p->st));
    HIP_OK(hipStreamSynchronize(p->st));
    uint8_t root[32];
    wt_digest_bytes(p->h_root, root);
    fs_weights_digest_v2(p->n, p->Q, b.nnz, root, p->weights_digest_v2);
    p->have_weights_digest_v2 = true;
  }
  memcpy(out, p->weights_digest_v2, 32);
  API_END
}

}  // extern "C"
