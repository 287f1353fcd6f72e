// Witness digest v2 on the GPU (the definition: fs.hpp; the hash itself: witness_tree.hpp, shared with the host): a SHA-256 tree over the
// handle's resident assignment.  One thread per digest.  The leaves read aL, aR, aO where they lie, in Montgomery form, convert each
// element in registers and hash it: the assignment is neither copied nor downloaded.  One launch per level; the root stays in `tree`.
//
// At n = 2^18 there are 24 576 leaves of 18 blocks each -- 384 waves for 1024 SIMDs -- so the kernel is bound by the latency of one
// thread's 18 x 64 rounds, not by throughput: a block is ONE wave, so that the leaves spread over as many CUs as there are waves.
#include "internal.hpp"
#include "witness_tree.hpp"

namespace sonic {

constexpr int WT_BLOCK = 64;

__global__ __launch_bounds__(WT_BLOCK) void k_witness_leaves(const Fr* __restrict__ aL, const Fr* __restrict__ aR, const Fr* __restrict__ aO, long n, long leaves,
                                                             uint32_t* __restrict__ out) {
  const long i = (long)blockIdx.x * WT_BLOCK + threadIdx.x;
  if (i >= leaves) return;
  uint32_t d[8];
  wt_leaf(aL, aR, aO, n, i, d);
  uint4* o = reinterpret_cast<uint4*>(out + 8 * i);
  o[0] = make_uint4(d[0], d[1], d[2], d[3]);
  o[1] = make_uint4(d[4], d[5], d[6], d[7]);
}

__global__ __launch_bounds__(WT_BLOCK) void k_witness_nodes(const uint32_t* __restrict__ below, long c, int level, long nodes, uint32_t* __restrict__ out) {
  const long j = (long)blockIdx.x * WT_BLOCK + threadIdx.x;
  if (j >= nodes) return;
  uint32_t d[8];
  wt_node(below, c, level, j, d);
  for (int k = 0; k < 8; k++) out[8 * j + k] = d[k];
}

// queues the whole tree over the Montgomery arrays aL, aR, aO (n each) into `tree` (wt_tree_digests(n) x 8 words, grown to fit) and
// returns where the root's eight state words will be
const uint32_t* witness_tree_enqueue(hipStream_t st, const Fr* aL, const Fr* aR, const Fr* aO, long n, DevBuf& tree) {
  tree.ensure(32 * (size_t)wt_tree_digests(n));
  long c = wt_leaf_count(n);
  uint32_t* below = tree.as<uint32_t>();
  LAUNCH(k_witness_leaves, ceil_div(c, WT_BLOCK), WT_BLOCK, 0, st, aL, aR, aO, n, c, below);
  for (int level = 1; c > 1; level++) {
    uint32_t* here = below + 8 * c;
    const long m = wt_node_count(c);
    LAUNCH(k_witness_nodes, ceil_div(m, WT_BLOCK), WT_BLOCK, 0, st, (const uint32_t*)below, c, level, m, here);
    below = here; c = m;
  }
  return below;
}

}  // namespace sonic
