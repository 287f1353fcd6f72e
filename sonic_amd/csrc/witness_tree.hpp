// Witness digest v2 (the definition: fs.hpp): a SHA-256 tree over the canonical bytes of aL || aR || aO, written once for the host and the
// device.  The compression function, the 64-byte headers and the assembly of a leaf's or a node's message are the text below; the
// kernels of witness.hip and the host walk at the end of this file (tests/host/fs_stream_host.cpp) compile the same functions.
//
// Every message is a 64-byte header followed by `count` items of 32 bytes, 1 <= count <= 32: a leaf's items are field elements (eight
// 32-bit limbs, little-endian bytes: one message word is one limb byte-swapped), a node's items are the digests below it (eight state
// words, big-endian bytes: a message word is a state word as it is).  So a block is the header or two items, and the padding either
// fills the second half of the last block (count odd) or is a block of its own (count even).
#pragma once
#include <stdint.h>
#include "field.hpp"

namespace sonic {

constexpr int WT_LEAF_ITEMS = 32;      // field elements per leaf: 1024 bytes
constexpr int WT_FANOUT = 32;          // digests per node

static HD constexpr uint32_t wt_k(int i) {
  constexpr uint32_t K[64] = {
      0x428a2f98u, 0x71374491u, 0xb5c0fbcfu, 0xe9b5dba5u, 0x3956c25bu, 0x59f111f1u, 0x923f82a4u, 0xab1c5ed5u, 0xd807aa98u, 0x12835b01u, 0x243185beu,
      0x550c7dc3u, 0x72be5d74u, 0x80deb1feu, 0x9bdc06a7u, 0xc19bf174u, 0xe49b69c1u, 0xefbe4786u, 0x0fc19dc6u, 0x240ca1ccu, 0x2de92c6fu, 0x4a7484aau,
      0x5cb0a9dcu, 0x76f988dau, 0x983e5152u, 0xa831c66du, 0xb00327c8u, 0xbf597fc7u, 0xc6e00bf3u, 0xd5a79147u, 0x06ca6351u, 0x14292967u, 0x27b70a85u,
      0x2e1b2138u, 0x4d2c6dfcu, 0x53380d13u, 0x650a7354u, 0x766a0abbu, 0x81c2c92eu, 0x92722c85u, 0xa2bfe8a1u, 0xa81a664bu, 0xc24b8b70u, 0xc76c51a3u,
      0xd192e819u, 0xd6990624u, 0xf40e3585u, 0x106aa070u, 0x19a4c116u, 0x1e376c08u, 0x2748774cu, 0x34b0bcb5u, 0x391c0cb3u, 0x4ed8aa4au, 0x5b9cca4fu,
      0x682e6ff3u, 0x748f82eeu, 0x78a5636fu, 0x84c87814u, 0x8cc70208u, 0x90befffau, 0xa4506cebu, 0xbef9a3f7u, 0xc67178f2u};
  return K[i];
}
HD uint32_t wt_rotr(uint32_t x, int k) { return (x >> k) | (x << (32 - k)); }
HD uint32_t wt_bswap(uint32_t x) { return (x >> 24) | ((x >> 8) & 0xff00u) | ((x << 8) & 0xff0000u) | (x << 24); }

HD void wt_iv(uint32_t s[8]) {
  s[0] = 0x6a09e667u; s[1] = 0xbb67ae85u; s[2] = 0x3c6ef372u; s[3] = 0xa54ff53au; s[4] = 0x510e527fu; s[5] = 0x9b05688cu; s[6] = 0x1f83d9abu; s[7] = 0x5be0cd19u;
}

// one block (FIPS 180-4, 6.2.2): w = its sixteen big-endian words, overwritten by the rolling message schedule.  Fully unrolled, so
// that w stays in registers and the round constants are immediates.
HD void wt_compress(uint32_t s[8], uint32_t w[16]) {
  uint32_t a = s[0], b = s[1], c = s[2], d = s[3], e = s[4], f = s[5], g = s[6], h = s[7];
#pragma unroll
  for (int i = 0; i < 64; i++) {
    if (i >= 16) {
      const uint32_t x = w[(i + 1) & 15], y = w[(i + 14) & 15];
      w[i & 15] += (wt_rotr(x, 7) ^ wt_rotr(x, 18) ^ (x >> 3)) + w[(i + 9) & 15] + (wt_rotr(y, 17) ^ wt_rotr(y, 19) ^ (y >> 10));
    }
    const uint32_t t1 = h + (wt_rotr(e, 6) ^ wt_rotr(e, 11) ^ wt_rotr(e, 25)) + ((e & f) ^ (~e & g)) + wt_k(i) + w[i & 15];
    const uint32_t t2 = (wt_rotr(a, 2) ^ wt_rotr(a, 13) ^ wt_rotr(a, 22)) + ((a & b) ^ (a & c) ^ (b & c));
    h = g; g = f; f = e; e = d + t1; d = c; c = b; b = a; a = t1 + t2;
  }
  s[0] += a; s[1] += b; s[2] += c; s[3] += d; s[4] += e; s[5] += f; s[6] += g; s[7] += h;
}

// H_leaf(i) (node = false: the label zero-padded to 56 bytes, then le64 i) and H_node(level, j) (the label zero-padded to 48 bytes, then
// le64 level, le64 j), as message words.  Both labels are 25 bytes, and a leaf's bytes 48 .. 55 are padding: level = 0.
// (wt_header_of: the same header under another 25-byte label -- the tree of weights digest v2, weights_tree.hpp)
HD void wt_header_of(const char* label, uint64_t level, uint64_t index, uint32_t h[16]) {
  for (int k = 0; k < 12; k++) h[k] = 0;
  for (int b = 0; b < 25; b++) h[b >> 2] |= (uint32_t)(uint8_t)label[b] << (24 - 8 * (b & 3));
  h[12] = wt_bswap((uint32_t)level); h[13] = wt_bswap((uint32_t)(level >> 32));
  h[14] = wt_bswap((uint32_t)index); h[15] = wt_bswap((uint32_t)(index >> 32));
}
HD void wt_header(bool node, uint64_t level, uint64_t index, uint32_t h[16]) {
  wt_header_of(node ? "sonic-hip/witness-node/v2" : "sonic-hip/witness-leaf/v2", level, index, h);
}

// SHA-256(header || item 0 .. item count-1) as eight state words; item(k, w) writes item k as eight message words
template <class Item>
HD void wt_hash_items(const uint32_t header[16], int count, const Item& item, uint32_t out[8]) {
  uint32_t w[16];
  wt_iv(out);
  const int nblocks = 2 + count / 2;                    // the header, ceil(count / 2) blocks of items, and the padding where it needs its own
  for (int blk = 0; blk < nblocks; blk++) {
    if (blk == 0) {
      for (int k = 0; k < 16; k++) w[k] = header[k];
    } else {
#pragma unroll
      for (int half = 0; half < 2; half++) {
        const int k = 2 * (blk - 1) + half;
        if (k < count) item(k, w + 8 * half);
        else {
          for (int j = 0; j < 8; j++) w[8 * half + j] = 0;
          if (k == count) w[8 * half] = 0x80000000u;
        }
      }
      if (blk == nblocks - 1) w[15] = (uint32_t)(64 + 32 * count) * 8;      // the length in bits (at most 8704: the high word stays 0)
    }
    wt_compress(out, w);
  }
}

// the items of a leaf: element e of aL || aR || aO lives in array e / n at e % n; Montgomery form in memory, canonical in the message
struct WtElements {
  const Fr *aL, *aR, *aO;
  long n, first;                                         // the leaf's first element, 32 i
  HD void operator()(int k, uint32_t* w) const {
    const long e = first + k;
    const Fr* src = e >= 2 * n ? aO + (e - 2 * n) : e >= n ? aR + (e - n) : aL + e;
    const Fr v = fp_from_mont(*src);
    for (int j = 0; j < 8; j++) w[j] = wt_bswap(v.l[j]);
  }
};
// the items of a node: the digests of the level below, as the state words the kernels keep them in
struct WtDigests {
  const uint32_t* below;                                 // the node's first child, 8 words each
  HD void operator()(int k, uint32_t* w) const { for (int j = 0; j < 8; j++) w[j] = below[8 * k + j]; }
};

HD long wt_leaf_count(long n) { return (3 * n + WT_LEAF_ITEMS - 1) / WT_LEAF_ITEMS; }
HD long wt_node_count(long below) { return (below + WT_FANOUT - 1) / WT_FANOUT; }
// digests of all levels, the leaves included: what a buffer that holds the whole tree needs (8 words each)
inline long wt_tree_digests(long n) {
  long c = wt_leaf_count(n), total = c;
  while (c > 1) { c = wt_node_count(c); total += c; }
  return total;
}

HD void wt_leaf(const Fr* aL, const Fr* aR, const Fr* aO, long n, long i, uint32_t out[8]) {
  uint32_t h[16];
  wt_header(false, 0, (uint64_t)i, h);
  const long left = 3 * n - WT_LEAF_ITEMS * i;
  wt_hash_items(h, (int)(left < WT_LEAF_ITEMS ? left : WT_LEAF_ITEMS), WtElements{aL, aR, aO, n, WT_LEAF_ITEMS * i}, out);
}
// node j of `level` (1: the first level of nodes) over the c digests of the level below
HD void wt_node(const uint32_t* below, long c, int level, long j, uint32_t out[8]) {
  uint32_t h[16];
  wt_header(true, (uint64_t)level, (uint64_t)j, h);
  const long left = c - WT_FANOUT * j;
  wt_hash_items(h, (int)(left < WT_FANOUT ? left : WT_FANOUT), WtDigests{below + 8 * WT_FANOUT * j}, out);
}

// the root's bytes from its state words
inline void wt_digest_bytes(const uint32_t s[8], uint8_t out[32]) {
  for (int i = 0; i < 8; i++) { out[4 * i] = (uint8_t)(s[i] >> 24); out[4 * i + 1] = (uint8_t)(s[i] >> 16); out[4 * i + 2] = (uint8_t)(s[i] >> 8); out[4 * i + 3] = (uint8_t)s[i]; }
}

// The whole tree on the host, one digest after the other: what the kernels compute with one thread per digest.  `tree` holds
// wt_tree_digests(n) x 8 words; the root is its last digest.  (Montgomery inputs, as the handle keeps them.)
inline void wt_tree_host(const Fr* aL, const Fr* aR, const Fr* aO, long n, uint32_t* tree, uint8_t root[32]) {
  long c = wt_leaf_count(n);
  for (long i = 0; i < c; i++) wt_leaf(aL, aR, aO, n, i, tree + 8 * i);
  uint32_t* below = tree;
  for (int level = 1; c > 1; level++) {
    uint32_t* here = below + 8 * c;
    const long m = wt_node_count(c);
    for (long j = 0; j < m; j++) wt_node(below, c, level, j, here + 8 * j);
    below = here; c = m;
  }
  wt_digest_bytes(below, root);
}

}  // namespace sonic
