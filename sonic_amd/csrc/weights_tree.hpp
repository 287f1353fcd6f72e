// Weights digest v2 (the definition: fs.hpp): a SHA-256 tree over the ENTRIES of the stacked CSR of 3Q rows, written once for the host and
// the device on top of witness_tree.hpp -- the same compression function, the same 64-byte headers (under labels of its own), the same
// messages of 1 .. 32 items of 32 bytes and the same node levels.  The kernels of weights_digest.hip, the host calls
// (sonic_fs_weights_digest_v2_csr) and the host test program (tests/host/weights_digest_host.cpp) compile the functions below.
//
// Entry k (CSR order) is two items: le64 r || le64 c || 16 zero bytes (r the stacked row, c the column) and the 32 canonical bytes of its
// value; a leaf holds WD_LEAF_ENTRIES = 16 entries.  An explicit zero is an entry like any other.
#pragma once
#include "witness_tree.hpp"

namespace sonic {

constexpr int WD_LEAF_ENTRIES = WT_LEAF_ITEMS / 2;

HD long wd_leaf_count(long nnz) { return nnz <= 0 ? 1 : (nnz + WD_LEAF_ENTRIES - 1) / WD_LEAF_ENTRIES; }
// digests of all levels, the leaves included (8 words each)
inline long wd_tree_digests(long nnz) {
  long c = wd_leaf_count(nnz), total = c;
  while (c > 1) { c = wt_node_count(c); total += c; }
  return total;
}

// the row of entry e < nnz = row_ptr[R]: the r with row_ptr[r] <= e < row_ptr[r + 1] (empty rows are never it)
template <class Idx>
HD long wd_row_of(const Idx* row_ptr, long R, long e) {
  long lo = 0, hi = R - 1;                               // the first r with row_ptr[r + 1] > e; r = R - 1 has it, as e < row_ptr[R]
  while (lo < hi) {
    const long mid = (lo + hi) >> 1;
    if ((long)row_ptr[mid + 1] > e) hi = mid; else lo = mid + 1;
  }
  return lo;
}

// The items of a leaf.  wt_hash_items asks for them in order, each once, so the row is found once (wd_row_of, the leaf's first entry)
// and then advanced through row_ptr: past the rows that end at or before the entry, the empty ones among them.  e < row_ptr[R] bounds
// the walk: r + 1 never passes R.  MONT: the values are Montgomery Fr (a handle's resident CSR, int32 indices), converted in registers;
// else 32 canonical bytes each (the ABI's CSR, int64 indices).
template <class Idx, bool MONT>
struct WdEntries {
  const Idx *row_ptr, *col;
  const void* val;
  long first;                                            // the leaf's first entry, 16 i
  mutable long r;                                        // the row of the entry the walk is at
  HD void operator()(int k, uint32_t* w) const {
    const long e = first + (k >> 1);
    if (!(k & 1)) {
      while ((long)row_ptr[r + 1] <= e) r++;
      const uint64_t c = (uint64_t)col[e];
      w[0] = wt_bswap((uint32_t)r); w[1] = wt_bswap((uint32_t)((uint64_t)r >> 32));
      w[2] = wt_bswap((uint32_t)c); w[3] = wt_bswap((uint32_t)(c >> 32));
      w[4] = w[5] = w[6] = w[7] = 0;
    } else if (MONT) {
      const Fr v = fp_from_mont(static_cast<const Fr*>(val)[e]);
      for (int j = 0; j < 8; j++) w[j] = wt_bswap(v.l[j]);
    } else {
      const uint8_t* b = static_cast<const uint8_t*>(val) + 32 * e;
      for (int j = 0; j < 8; j++) w[j] = (uint32_t)b[4 * j] << 24 | (uint32_t)b[4 * j + 1] << 16 | (uint32_t)b[4 * j + 2] << 8 | b[4 * j + 3];
    }
  }
};

// leaf i of a validated CSR of R = 3Q rows and nnz = row_ptr[R] entries (nnz = 0: the one leaf over zero items)
template <class Idx, bool MONT>
HD void wd_leaf(const Idx* row_ptr, const Idx* col, const void* val, long R, long nnz, long i, uint32_t out[8]) {
  uint32_t h[16];
  wt_header_of("sonic-hip/weights-leaf/v2", 0, (uint64_t)i, h);
  const long first = WD_LEAF_ENTRIES * i, left = nnz - first;
  const int entries = (int)(left < WD_LEAF_ENTRIES ? (left > 0 ? left : 0) : WD_LEAF_ENTRIES);
  const long r0 = entries > 0 ? wd_row_of(row_ptr, R, first) : 0;
  wt_hash_items(h, 2 * entries, WdEntries<Idx, MONT>{row_ptr, col, val, first, r0}, out);
}
// node j of `level` (1: the first level of nodes) over the c digests of the level below
HD void wd_node(const uint32_t* below, long c, int level, long j, uint32_t out[8]) {
  uint32_t h[16];
  wt_header_of("sonic-hip/weights-node/v2", (uint64_t)level, (uint64_t)j, h);
  const long left = c - WT_FANOUT * j;
  wt_hash_items(h, (int)(left < WT_FANOUT ? left : WT_FANOUT), WtDigests{below + 8 * WT_FANOUT * j}, out);
}

// The whole tree on the host, one digest after the other: what the kernels compute with one thread per digest.  `tree` holds
// wd_tree_digests(nnz) x 8 words; the root is its last digest.
template <class Idx, bool MONT>
inline void wd_tree_host(const Idx* row_ptr, const Idx* col, const void* val, long R, uint32_t* tree, uint8_t root[32]) {
  const long nnz = (long)row_ptr[R];
  long c = wd_leaf_count(nnz);
  for (long i = 0; i < c; i++) wd_leaf<Idx, MONT>(row_ptr, col, val, R, nnz, i, tree + 8 * i);
  uint32_t* below = tree;
  for (int level = 1; c > 1; level++) {
    uint32_t* here = below + 8 * c;
    const long m = wt_node_count(c);
    for (long j = 0; j < m; j++) wd_node(below, c, level, j, here + 8 * j);
    below = here; c = m;
  }
  wt_digest_bytes(below, root);
}

}  // namespace sonic
