// The compressed BLS12-381 point encodings (the Zcash / IETF pairing-friendly-curves serialization; normative text in
// include/sonic_hip.h), point by point, host and device: compress.hip's kernels run these one thread per point, the host runs them for
// one proof (sonic_proof_compress / sonic_proof_decompress) and in the CPU unit tests (tests/host/compress_host.cpp).
//
//   G1, 48 bytes: x big-endian; byte 0 carries 0x80 (compressed, always), 0x40 (infinity: exactly c0 00 .. 00), 0x20 (y > (q-1)/2).
//   G2, 96 bytes: x.c1 (with the flags) then x.c0; sign: y.c1 > (q-1)/2 when y.c1 != 0, else y.c0 > (q-1)/2.
//
// Neither curve has a point with y = 0 (both group orders are odd), so the sign bit of a finite point is never ambiguous.
// Verdicts: 0 accepted, Z_MALFORMED, Z_OFF_CURVE, Z_OUTSIDE_SUBGROUP -- the error bits of the SRS loaders.
#pragma once
#include "g2.hpp"

namespace sonic {

constexpr uint8_t Z_MALFORMED = 1, Z_OFF_CURVE = 2, Z_OUTSIDE_SUBGROUP = 4;
constexpr uint8_t Z_COMPRESSED = 0x80, Z_INFINITY = 0x40, Z_SIGN = 0x20;

// 48 big-endian bytes -> the integer below 2^381 (standard form, not yet compared with q); returns the three flag bits.  On the device the
// encodings sit in buffers of the library's own at multiples of 48 bytes, so they are read and written as aligned 32-bit words.
HD uint8_t fq_from_be48(const uint8_t* b, Fq& x) {
#pragma unroll
  for (int k = 0; k < 12; k++) {
#if defined(__HIP_DEVICE_COMPILE__)
    x.l[k] = __builtin_bswap32(reinterpret_cast<const uint32_t*>(b)[11 - k]);
#else
    const uint8_t* s = b + 4 * (11 - k);
    x.l[k] = ((uint32_t)s[0] << 24) | ((uint32_t)s[1] << 16) | ((uint32_t)s[2] << 8) | (uint32_t)s[3];
#endif
  }
  const uint8_t fl = (uint8_t)(x.l[11] >> 24) & 0xe0;
  x.l[11] &= 0x1fffffffu;
  return fl;
}
HD void fq_to_be48(const Fq& x_std, uint8_t flags, uint8_t* b) {
#pragma unroll
  for (int k = 0; k < 12; k++) {
    const uint32_t w = x_std.l[k] | (k == 11 ? (uint32_t)flags << 24 : 0u);
#if defined(__HIP_DEVICE_COMPILE__)
    reinterpret_cast<uint32_t*>(b)[11 - k] = __builtin_bswap32(w);
#else
    uint8_t* s = b + 4 * (11 - k);
    s[0] = (uint8_t)(w >> 24); s[1] = (uint8_t)(w >> 16); s[2] = (uint8_t)(w >> 8); s[3] = (uint8_t)w;
#endif
  }
}

// ---- G1 ----
// 48 bytes -> the Montgomery affine point (infinity when refused).  Not the subgroup test.
HD uint8_t g1_decompress_point(const uint8_t* z, G1Affine& p) {
  p = G1Affine::inf();
  Fq x_std;
  const uint8_t fl = fq_from_be48(z, x_std);
  if (!(fl & Z_COMPRESSED)) return Z_MALFORMED;
  if (fl & Z_INFINITY) return ((fl & Z_SIGN) || !x_std.is_zero_strict()) ? Z_MALFORMED : 0;
  if (!fp_is_canonical(x_std)) return Z_MALFORMED;
  const Fq x = fp_to_mont(x_std);
  bool ok;
  const Fq y = fq_sqrt(fp_add(fp_mul(fp_sqr(x), x), fp_dbl(fp_dbl(Fq::one()))), &ok);
  if (!ok) return Z_OFF_CURVE;
  p.x = x;
  p.y = fq_is_high(fp_from_mont(y)) != ((fl & Z_SIGN) != 0) ? fp_neg(y) : y;
  return 0;
}
// the canonical 96 bytes of a Montgomery affine point, as 24 little-endian words (zeros for infinity)
HD void g1_canonical_words(const G1Affine& p, uint32_t* w) {
  if (p.is_inf()) { for (int k = 0; k < 24; k++) w[k] = 0; return; }
  const Fq x = fp_from_mont(p.x), y = fp_from_mont(p.y);
  for (int k = 0; k < 12; k++) { w[k] = x.l[k]; w[12 + k] = y.l[k]; }
}
// Montgomery affine point -> 48 bytes
HD void g1_compress_point(const G1Affine& p, uint8_t* z) {
  if (p.is_inf()) { fq_to_be48(Fq::zero(), Z_COMPRESSED | Z_INFINITY, z); return; }
  fq_to_be48(fp_from_mont(p.x), Z_COMPRESSED | (fq_is_high(fp_from_mont(p.y)) ? Z_SIGN : 0), z);
}

// ---- G2 ----
HD uint8_t g2_decompress_point(const uint8_t* z, G2Affine& p) {
  p = G2Affine::inf();
  Fq2 x_std;
  const uint8_t fl = fq_from_be48(z, x_std.c1);
  const uint8_t fl0 = fq_from_be48(z + 48, x_std.c0);
  if (!(fl & Z_COMPRESSED) || fl0) return Z_MALFORMED;                 // the second half carries no flags
  if (fl & Z_INFINITY) return ((fl & Z_SIGN) || !x_std.c0.is_zero_strict() || !x_std.c1.is_zero_strict()) ? Z_MALFORMED : 0;
  if (!fp_is_canonical(x_std.c0) || !fp_is_canonical(x_std.c1)) return Z_MALFORMED;
  Fq2 x; x.c0 = fp_to_mont(x_std.c0); x.c1 = fp_to_mont(x_std.c1);
  bool ok;
  const Fq2 y = fq2_sqrt(g2_curve_rhs(x), &ok);
  if (!ok) return Z_OFF_CURVE;
  p.x = x;
  p.y = fq2_is_high(fp_from_mont(y.c0), fp_from_mont(y.c1)) != ((fl & Z_SIGN) != 0) ? f2_neg(y) : y;
  return 0;
}
// the 192 bytes of the header's G2 layout, as 48 little-endian words (zeros for infinity)
HD void g2_canonical_words(const G2Affine& p, uint32_t* w) {
  if (p.is_inf()) { for (int k = 0; k < 48; k++) w[k] = 0; return; }
  const Fq a = fp_from_mont(p.x.c0), b = fp_from_mont(p.x.c1), c = fp_from_mont(p.y.c0), e = fp_from_mont(p.y.c1);
  for (int k = 0; k < 12; k++) { w[k] = a.l[k]; w[12 + k] = b.l[k]; w[24 + k] = c.l[k]; w[36 + k] = e.l[k]; }
}
HD void g2_compress_point(const G2Affine& p, uint8_t* z) {
  if (p.is_inf()) { fq_to_be48(Fq::zero(), Z_COMPRESSED | Z_INFINITY, z); fq_to_be48(Fq::zero(), 0, z + 48); return; }
  const bool high = fq2_is_high(fp_from_mont(p.y.c0), fp_from_mont(p.y.c1));
  fq_to_be48(fp_from_mont(p.x.c1), Z_COMPRESSED | (high ? Z_SIGN : 0), z);
  fq_to_be48(fp_from_mont(p.x.c0), 0, z + 48);
}

}  // namespace sonic
