// k * P for a point of its own and a scalar of its own, in G1 and G2, and the randomizers of the SRS structure check: the arithmetic of
// the updatable SRS (include/sonic_hip.h, "Updatable SRS"), written once for the host and the device.  k_g1_scale_each (srs.hip) and
// k_g2_scale_each (srs_g2.hip) run these with one thread per point; tests/host/srs_update_host.cpp compiles the same text with g++.
#pragma once
#include "g2.hpp"
#include "witness_tree.hpp"

namespace sonic {

// limb j of a scalar.  The limbs live in registers, and a register array indexed by a run-time value goes to scratch: the limb is
// picked by eight constant-index selects instead (as g1_in_subgroup_walk reads r), once per 32 bits.
HD uint32_t fr_limb(const Fr& k, int j) {
  uint32_t wd = 0;
#pragma unroll
  for (int i = 0; i < FR_LIMBS; i++) if (i == j) wd = k.l[i];
  return wd;
}

// k * P by left-to-right double-and-add over the low 32 * limbs bits of k (standard form, k < r), XYZZ accumulator.  The leading zero
// bits double infinity, which g1_dbl returns at once.  P must be in the order-r subgroup or infinity; the formulas handle every
// exceptional position themselves.
HD G1XYZZ g1_scale(const G1Affine& p, const Fr& k_std, int limbs = FR_LIMBS) {
  G1XYZZ acc = G1XYZZ::inf();
  if (p.is_inf()) return acc;
#pragma unroll 1
  for (int j = limbs - 1; j >= 0; j--) {
    const uint32_t wd = fr_limb(k_std, j);
#pragma unroll 1
    for (int b = 31; b >= 0; b--) {
      acc = g1_dbl(acc);
      if ((wd >> b) & 1u) acc = g1_add_mixed(acc, p);
    }
  }
  return acc;
}

// the same on the twist, Jacobian accumulator
HD G2Jac g2_scale(const G2Affine& p, const Fr& k_std, int limbs = FR_LIMBS) {
  G2Jac acc = G2Jac::inf();
  if (p.is_inf()) return acc;
#pragma unroll 1
  for (int j = limbs - 1; j >= 0; j--) {
    const uint32_t wd = fr_limb(k_std, j);
#pragma unroll 1
    for (int b = 31; b >= 0; b--) {
      acc = g2_dbl(acc);
      if ((wd >> b) & 1u) acc = g2_add_mixed(acc, p);
    }
  }
  return acc;
}

// Randomizer `index` (= e + d) of sonic_srs_check under a 32-byte seed, given as eight big-endian words:
//   rho = the first 16 bytes of SHA-256("sonic-hip/srs-check/v1" || seed || le64 index), read as a little-endian integer, 0 -> 1
// The message is 62 bytes: two blocks, the second holding nothing but the length.  out: four limbs, least significant first.
constexpr int SRS_CHECK_LABEL_LEN = 22;
HD void srs_check_rho(const uint32_t seed_be[8], uint64_t index, uint32_t out[4]) {
  const char* label = "sonic-hip/srs-check/v1";
  uint32_t w[16], s[8];
  for (int k = 0; k < 16; k++) w[k] = 0;
  for (int b = 0; b < SRS_CHECK_LABEL_LEN; b++) w[b >> 2] |= (uint32_t)(uint8_t)label[b] << (24 - 8 * (b & 3));
  // bytes 22 .. 53: the seed, two bytes off the word grid
#pragma unroll
  for (int k = 0; k < 8; k++) { w[5 + k] |= seed_be[k] >> 16; w[6 + k] |= seed_be[k] << 16; }
  // bytes 54 .. 61: le64 index; byte 62: 0x80
  const uint32_t lo = (uint32_t)index, hi = (uint32_t)(index >> 32);
  w[13] |= (lo & 0xffu) << 8 | ((lo >> 8) & 0xffu);
  w[14] = ((lo >> 16) & 0xffu) << 24 | (lo >> 24) << 16 | (hi & 0xffu) << 8 | ((hi >> 8) & 0xffu);
  w[15] = ((hi >> 16) & 0xffu) << 24 | (hi >> 24) << 16 | 0x8000u;
  wt_iv(s);
  wt_compress(s, w);
  for (int k = 0; k < 15; k++) w[k] = 0;
  w[15] = 62 * 8;
  wt_compress(s, w);
  for (int k = 0; k < 4; k++) out[k] = wt_bswap(s[k]);         // digest bytes 4k .. 4k+3, little-endian
  if ((out[0] | out[1] | out[2] | out[3]) == 0) out[0] = 1;
}

}  // namespace sonic
