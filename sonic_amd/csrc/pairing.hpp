// The pairing of the verifier (host and device, one copy of the formulas): pcV's equation eA <> eB == eC (src/Sonic/CommitmentScheme.hs:58-68) as a product of
// three Miller loops and one final exponentiation.
//
// The reference takes `pairing` from pairing-1.0.0; only equalities of pairing products are ever tested, so any bilinear,
// non-degenerate map on (G1, G2) accepts exactly the same proofs.  Used here: the ate loop over |x| = 0xd201000000010000 with the
// running point kept on the twist E': y^2 = x^3 + 4(1 + u) in Jacobian coordinates, lines evaluated at the G1 point as sparse
// elements of Fq12 = Fq2[w]/(w^6 - xi), xi = 1 + u (the untwisting map is (x, y) -> (x / w^2, y / w^3)), and the exponent
// 3 (q^12 - 1) / r = (q^6 - 1)(q^2 + 1) * [ (x - 1)^2 (x + q)(x^2 + q^2 - 1) + 3 ]   (identity checked in tests/test_pairing_host.py).
// Lines are scaled by elements of Fq2 and by w^3 (in Fq4): both die in the factor q^4 - 1 of the exponent.
//
// tests/pairing_selftest.cpp compiles this header with g++ and checks it against the plain polynomial-basis pairing the verifier
// used before (tests/pairing_plain.hpp: affine arithmetic in Fq12, exponent (q^12 - 1)/r bit by bit): value == plain^3.
#pragma once
#include "g2.hpp"
#include "constants.hpp"

// PHD: host and device, inlined on the device as everything else in the limb headers is; a plain `inline` for a host compiler, which
// decides for itself (forcing the whole tower into one function makes the sanitizer builds of the host tests take many minutes)
#if defined(__HIPCC__)
#define PHD HD
#else
#define PHD inline
#endif

namespace sonic {
namespace pairing {

PHD Fq2 f2_conj(const Fq2& a) { Fq2 r; r.c0 = a.c0; r.c1 = fp_neg(a.c1); return r; }
PHD Fq2 f2_mul_xi(const Fq2& a) { Fq2 r; r.c0 = fp_sub(a.c0, a.c1); r.c1 = fp_add(a.c0, a.c1); return r; }   // (a0 + a1 u)(1 + u)
PHD Fq2 f2_mul_fq(const Fq2& a, const Fq& s) { Fq2 r; r.c0 = fp_mul(a.c0, s); r.c1 = fp_mul(a.c1, s); return r; }

// Fq6 = Fq2[v] / (v^3 - xi)
struct F6 {
  Fq2 a0, a1, a2;
  static HD F6 zero() { F6 r; r.a0 = r.a1 = r.a2 = Fq2::zero(); return r; }
  static HD F6 one() { F6 r = zero(); r.a0 = Fq2::one(); return r; }
  HD bool is_zero() const { return a0.is_zero() && a1.is_zero() && a2.is_zero(); }
  HD bool operator==(const F6& o) const { return a0 == o.a0 && a1 == o.a1 && a2 == o.a2; }
};
PHD F6 f6_add(const F6& a, const F6& b) { F6 r; r.a0 = f2_add(a.a0, b.a0); r.a1 = f2_add(a.a1, b.a1); r.a2 = f2_add(a.a2, b.a2); return r; }
PHD F6 f6_sub(const F6& a, const F6& b) { F6 r; r.a0 = f2_sub(a.a0, b.a0); r.a1 = f2_sub(a.a1, b.a1); r.a2 = f2_sub(a.a2, b.a2); return r; }
PHD F6 f6_neg(const F6& a) { F6 r; r.a0 = f2_neg(a.a0); r.a1 = f2_neg(a.a1); r.a2 = f2_neg(a.a2); return r; }
PHD F6 f6_mul_v(const F6& a) { F6 r; r.a0 = f2_mul_xi(a.a2); r.a1 = a.a0; r.a2 = a.a1; return r; }
PHD F6 f6_mul(const F6& a, const F6& b) {
  const Fq2 t0 = f2_mul(a.a0, b.a0), t1 = f2_mul(a.a1, b.a1), t2 = f2_mul(a.a2, b.a2);
  F6 r;
  r.a0 = f2_add(t0, f2_mul_xi(f2_sub(f2_sub(f2_mul(f2_add(a.a1, a.a2), f2_add(b.a1, b.a2)), t1), t2)));
  r.a1 = f2_add(f2_sub(f2_sub(f2_mul(f2_add(a.a0, a.a1), f2_add(b.a0, b.a1)), t0), t1), f2_mul_xi(t2));
  r.a2 = f2_add(f2_sub(f2_sub(f2_mul(f2_add(a.a0, a.a2), f2_add(b.a0, b.a2)), t0), t2), t1);
  return r;
}
PHD F6 f6_inv(const F6& a) {
  const Fq2 c0 = f2_sub(f2_sqr(a.a0), f2_mul_xi(f2_mul(a.a1, a.a2)));
  const Fq2 c1 = f2_sub(f2_mul_xi(f2_sqr(a.a2)), f2_mul(a.a0, a.a1));
  const Fq2 c2 = f2_sub(f2_sqr(a.a1), f2_mul(a.a0, a.a2));
  const Fq2 t = f2_inv(f2_add(f2_mul(a.a0, c0), f2_mul_xi(f2_add(f2_mul(a.a2, c1), f2_mul(a.a1, c2)))));
  F6 r;
  r.a0 = f2_mul(c0, t); r.a1 = f2_mul(c1, t); r.a2 = f2_mul(c2, t);
  return r;
}

// Fq12 = Fq6[w] / (w^2 - v): c0 + c1 w; as a polynomial in w over Fq2 the coefficient of w^i is (c0.a0, c1.a0, c0.a1, c1.a1, c0.a2, c1.a2)[i]
struct F12 {
  F6 c0, c1;
  static HD F12 one() { F12 r; r.c0 = F6::one(); r.c1 = F6::zero(); return r; }
  HD bool operator==(const F12& o) const { return c0 == o.c0 && c1 == o.c1; }
  HD bool is_one() const { return *this == one(); }
};
PHD F12 f12_mul(const F12& a, const F12& b) {
  const F6 t0 = f6_mul(a.c0, b.c0), t1 = f6_mul(a.c1, b.c1);
  F12 r;
  r.c1 = f6_sub(f6_sub(f6_mul(f6_add(a.c0, a.c1), f6_add(b.c0, b.c1)), t0), t1);
  r.c0 = f6_add(t0, f6_mul_v(t1));
  return r;
}
PHD F12 f12_sqr(const F12& a) {
  const F6 ab = f6_mul(a.c0, a.c1);
  F12 r;
  r.c0 = f6_sub(f6_sub(f6_mul(f6_add(a.c0, a.c1), f6_add(a.c0, f6_mul_v(a.c1))), ab), f6_mul_v(ab));
  r.c1 = f6_add(ab, ab);
  return r;
}
PHD F12 f12_conj(const F12& a) { F12 r; r.c0 = a.c0; r.c1 = f6_neg(a.c1); return r; }       // a^(q^6)
PHD F12 f12_inv(const F12& a) {
  const F6 t = f6_inv(f6_sub(f6_mul(a.c0, a.c0), f6_mul_v(f6_mul(a.c1, a.c1))));
  F12 r;
  r.c0 = f6_mul(a.c0, t);
  r.c1 = f6_neg(f6_mul(a.c1, t));
  return r;
}

// a * (l0 + l2 w^2 + l3 w^3): the shape of every line below.  With L0 = (l0, l2, 0) and L1 = (0, l3, 0) in Fq6 the three Fq6
// products of the Karatsuba step have one or two zero coefficients: 13 instead of 18 Fq2 products.
PHD F6 f6_mul_01(const F6& a, const Fq2& b0, const Fq2& b1) {       // a * (b0 + b1 v)
  const Fq2 t0 = f2_mul(a.a0, b0), t1 = f2_mul(a.a1, b1);
  F6 r;
  r.a0 = f2_add(t0, f2_mul_xi(f2_mul(a.a2, b1)));
  r.a1 = f2_sub(f2_sub(f2_mul(f2_add(a.a0, a.a1), f2_add(b0, b1)), t0), t1);
  r.a2 = f2_add(f2_mul(a.a2, b0), t1);
  return r;
}
PHD F6 f6_mul_1(const F6& a, const Fq2& b1) {                       // a * (b1 v)
  F6 r;
  r.a0 = f2_mul_xi(f2_mul(a.a2, b1));
  r.a1 = f2_mul(a.a0, b1);
  r.a2 = f2_mul(a.a1, b1);
  return r;
}
PHD F12 f12_mul_line(const F12& a, const Fq2& l0, const Fq2& l2, const Fq2& l3) {
  const F6 t0 = f6_mul_01(a.c0, l0, l2), t1 = f6_mul_1(a.c1, l3);
  F12 r;
  r.c1 = f6_sub(f6_sub(f6_mul_01(f6_add(a.c0, a.c1), l0, f2_add(l2, l3)), t0), t1);
  r.c0 = f6_add(t0, f6_mul_v(t1));
  return r;
}

// (alpha w^i)^q = conj(alpha) gamma_i w^i with gamma_i = xi^(i (q - 1) / 6): constants.hpp, derived by tools/gen_constants.py (the host test
// program tests/host/pairing_host.cpp recomputes them by a run-time exponentiation and compares)
template <int I>
PHD Fq2 frobenius_gamma() {
  static_assert(I >= 1 && I <= 5, "gamma_0 = 1 has no table");
  constexpr uint32_t c0[5][12] = {FROB_GAMMA1_C0_MONT, FROB_GAMMA2_C0_MONT, FROB_GAMMA3_C0_MONT, FROB_GAMMA4_C0_MONT, FROB_GAMMA5_C0_MONT};
  constexpr uint32_t c1[5][12] = {FROB_GAMMA1_C1_MONT, FROB_GAMMA2_C1_MONT, FROB_GAMMA3_C1_MONT, FROB_GAMMA4_C1_MONT, FROB_GAMMA5_C1_MONT};
  Fq2 g;
  for (int k = 0; k < 12; k++) { g.c0.l[k] = c0[I - 1][k]; g.c1.l[k] = c1[I - 1][k]; }
  return g;
}
PHD F12 f12_frobenius(const F12& a) {
  F12 r;
  r.c0.a0 = f2_conj(a.c0.a0);
  r.c1.a0 = f2_mul(f2_conj(a.c1.a0), frobenius_gamma<1>());
  r.c0.a1 = f2_mul(f2_conj(a.c0.a1), frobenius_gamma<2>());
  r.c1.a1 = f2_mul(f2_conj(a.c1.a1), frobenius_gamma<3>());
  r.c0.a2 = f2_mul(f2_conj(a.c0.a2), frobenius_gamma<4>());
  r.c1.a2 = f2_mul(f2_conj(a.c1.a2), frobenius_gamma<5>());
  return r;
}

constexpr uint64_t ATE_LOOP = BLS_Z_ABS;        // |x| = 0xd201000000010000; the curve parameter x is negative

// The walks below take the 63 bits under the top bit of |x| as runs: the doublings up to and including the next set bit, then one
// addition (five runs), then the doublings that are left -- as g2_in_subgroup walks |z|.  The run lengths come from a 64-bit word that is
// the same in every lane; nothing is indexed at run time.

// f_{|x|, Q}(P) up to factors in proper subfields; P in G1, Q on the twist (both affine, neither checked here)
PHD F12 miller_loop(const G1Affine& p, const G2Affine& q) {
  if (p.is_inf() || q.is_inf()) return F12::one();
  G2Jac R; R.x = q.x; R.y = q.y; R.z = Fq2::one();
  F12 f = F12::one();
  uint64_t w = ATE_LOOP << 1;                                       // the bits still to walk, left-aligned
  int left = 63;
#pragma unroll 1
  while (left > 0) {
    const int run = w ? __builtin_clzll(w) + 1 : left;
#pragma unroll 1
    for (int i = 0; i < run; i++) {
      // tangent at R = (X, Y, Z): (2 Y^2 - 3 X^3) + 3 X^2 Z^2 xP w^2 - 2 Y Z^3 yP w^3
      const Fq2 X2 = f2_sqr(R.x), Z2 = f2_sqr(R.z), Y2 = f2_sqr(R.y);
      const Fq2 X2_3 = f2_add(f2_dbl(X2), X2);
      const Fq2 l0 = f2_sub(f2_dbl(Y2), f2_mul(X2_3, R.x));
      const Fq2 l2 = f2_mul_fq(f2_mul(X2_3, Z2), p.x);
      const Fq2 l3 = f2_neg(f2_mul_fq(f2_dbl(f2_mul(f2_mul(R.y, R.z), Z2)), p.y));
      f = f12_mul_line(f12_sqr(f), l0, l2, l3);
      R = g2_dbl(R);
    }
    if (w) {
      // chord through R = (X, Y, Z) and Q = (x2, y2): H = x2 Z^2 - X, N = y2 Z^3 - Y:
      //   (y2 Z H - N x2) + N xP w^2 - Z H yP w^3
      const Fq2 Z2 = f2_sqr(R.z);
      const Fq2 H = f2_sub(f2_mul(q.x, Z2), R.x);
      const Fq2 N = f2_sub(f2_mul(q.y, f2_mul(Z2, R.z)), R.y);
      if (H.is_zero()) {
        // R = +-Q: cannot happen for a point of order r inside the loop; a caller that hands over anything else gets the
        // degenerate value 1 (an equation between such values proves nothing, and none is accepted: points are subgroup-checked)
        return F12::one();
      }
      const Fq2 ZH = f2_mul(R.z, H);
      const Fq2 l0 = f2_sub(f2_mul(q.y, ZH), f2_mul(N, q.x));
      const Fq2 l2 = f2_mul_fq(N, p.x);
      const Fq2 l3 = f2_neg(f2_mul_fq(ZH, p.y));
      f = f12_mul_line(f, l0, l2, l3);
      R = g2_add_mixed(R, q);
    }
    w = run < 64 ? w << run : 0;
    left -= run;
  }
  return f;
}

// g^|x| for g in the cyclotomic subgroup (plain squarings: the verifier does ~320 of them per check).  Out of line on the device: the
// final exponentiation calls it five times, and five inlined copies of a squaring and a product are more code than the instruction cache holds.
static HD_NOINLINE F12 f12_pow_absx(const F12& g) {
  F12 acc = g;
  uint64_t w = ATE_LOOP << 1;
  int left = 63;
#pragma unroll 1
  while (left > 0) {
    const int run = w ? __builtin_clzll(w) + 1 : left;
#pragma unroll 1
    for (int i = 0; i < run; i++) acc = f12_sqr(acc);
    if (w) acc = f12_mul(acc, g);
    w = run < 64 ? w << run : 0;
    left -= run;
  }
  return acc;
}
PHD F12 f12_pow_x(const F12& h) { return f12_conj(f12_pow_absx(h)); }                       // h^x, x = -|x|
PHD F12 f12_pow_xm1(const F12& h) { return f12_conj(f12_mul(f12_pow_absx(h), h)); }         // h^(x-1) = 1 / h^(|x|+1)

// f^(3 (q^12 - 1) / r)
PHD F12 final_exponentiation(const F12& f) {
  // easy part: (q^6 - 1)(q^2 + 1); afterwards the inverse is the conjugate
  F12 g = f12_mul(f12_conj(f), f12_inv(f));
  g = f12_mul(f12_frobenius(f12_frobenius(g)), g);
  // hard part: (x - 1)^2 (x + q)(x^2 + q^2 - 1) + 3 with x = -|x|
  const F12 a = f12_pow_xm1(f12_pow_xm1(g));
  const F12 b = f12_mul(f12_pow_x(a), f12_frobenius(a));
  const F12 c = f12_mul(f12_mul(f12_pow_x(f12_pow_x(b)), f12_frobenius(f12_frobenius(b))), f12_conj(b));
  return f12_mul(c, f12_mul(f12_sqr(g), g));
}

// ---- the value at the boundary: 576 bytes, the layout of sonic_srs_pairing -- c0.a0, c0.a1, c0.a2, c1.a0, c1.a1, c1.a2, each Fq2 as
// c0 then c1, each Fq as 48 little-endian bytes of the canonical standard form ----
PHD void f12_to_words(const F12& v, uint32_t* out144) {
  const Fq2* cs[6] = {&v.c0.a0, &v.c0.a1, &v.c0.a2, &v.c1.a0, &v.c1.a1, &v.c1.a2};
  for (int j = 0; j < 6; j++) {
    const Fq c0 = fp_from_mont(cs[j]->c0), c1 = fp_from_mont(cs[j]->c1);
    for (int k = 0; k < 12; k++) { out144[24 * j + k] = c0.l[k]; out144[24 * j + 12 + k] = c1.l[k]; }
  }
}
// the inverse; false (and nothing written) for a coordinate that is not below q
PHD bool f12_from_words(const uint32_t* in144, F12& v) {
  Fq2* cs[6] = {&v.c0.a0, &v.c0.a1, &v.c0.a2, &v.c1.a0, &v.c1.a1, &v.c1.a2};
  for (int j = 0; j < 6; j++) {
    Fq c0, c1;
    for (int k = 0; k < 12; k++) { c0.l[k] = in144[24 * j + k]; c1.l[k] = in144[24 * j + 12 + k]; }
    if (!fp_is_canonical(c0) || !fp_is_canonical(c1)) return false;
    cs[j]->c0 = fp_to_mont(c0); cs[j]->c1 = fp_to_mont(c1);
  }
  return true;
}

}  // namespace pairing
}  // namespace sonic
