// G2 of BLS12-381: the twist y^2 = x^3 + 4(u + 1) over Fq2 = Fq[u]/(u^2 + 1).
// Only SRS.new touches G2 (src/Sonic/SRS.hs:35-36,40-41: hNegativeX, hPositiveX, h*AlphaX); the prover never
// reads these vectors, the verifier reads three elements.  Jacobian accumulators (3 x Fq2) keep the register
// footprint below the XYZZ form's.
#pragma once
#include "g1.hpp"

namespace sonic {

struct Fq2 {
  Fq c0, c1;
  static HD Fq2 zero() { Fq2 r; r.c0 = Fq::zero(); r.c1 = Fq::zero(); return r; }
  static HD Fq2 one() { Fq2 r; r.c0 = Fq::one(); r.c1 = Fq::zero(); return r; }
  HD bool is_zero() const { return c0.is_zero() && c1.is_zero(); }
  HD bool operator==(const Fq2& o) const { return c0 == o.c0 && c1 == o.c1; }
};
HD Fq2 f2_add(const Fq2& a, const Fq2& b) { Fq2 r; r.c0 = fp_add(a.c0, b.c0); r.c1 = fp_add(a.c1, b.c1); return r; }
HD Fq2 f2_sub(const Fq2& a, const Fq2& b) { Fq2 r; r.c0 = fp_sub(a.c0, b.c0); r.c1 = fp_sub(a.c1, b.c1); return r; }
HD Fq2 f2_dbl(const Fq2& a) { return f2_add(a, a); }
HD Fq2 f2_neg(const Fq2& a) { Fq2 r; r.c0 = fp_neg(a.c0); r.c1 = fp_neg(a.c1); return r; }
// (a0 + a1 u)(b0 + b1 u) = (a0 b0 - a1 b1) + ((a0 + a1)(b0 + b1) - a0 b0 - a1 b1) u
HD Fq2 f2_mul(const Fq2& a, const Fq2& b) {
  Fq t0 = fp_mul(a.c0, b.c0), t1 = fp_mul(a.c1, b.c1);
  Fq t2 = fp_mul(fp_add(a.c0, a.c1), fp_add(b.c0, b.c1));
  Fq2 r;
  r.c0 = fp_sub(t0, t1);
  r.c1 = fp_sub(fp_sub(t2, t0), t1);
  return r;
}
// (a0 + a1 u)^2 = (a0 + a1)(a0 - a1) + 2 a0 a1 u
HD Fq2 f2_sqr(const Fq2& a) {
  Fq2 r;
  r.c0 = fp_mul(fp_add(a.c0, a.c1), fp_sub(a.c0, a.c1));
  r.c1 = fp_dbl(fp_mul(a.c0, a.c1));
  return r;
}
HD Fq2 f2_inv(const Fq2& a) {
  Fq d = fp_inv(fp_add(fp_sqr(a.c0), fp_sqr(a.c1)));
  Fq2 r;
  r.c0 = fp_mul(a.c0, d);
  r.c1 = fp_neg(fp_mul(a.c1, d));
  return r;
}

// A square root in Fq2 = Fq[u]/(u^2 + 1) from square roots in Fq (fq_sqrt), *ok = whether a is a square.  a1 = 0: sqrt(a0) when a0 is a
// square, else sqrt(-a0) u (-1 is a non-residue).  Otherwise with s = sqrt(a0^2 + a1^2) (the norm of a square is a square) and
// t = (a0 + s)/2 -- or (a0 - s)/2 when that is no square -- x0 = sqrt(t), x1 = a1 / (2 x0): x0^2 - x1^2 = a0 and 2 x0 x1 = a1.  The result
// is checked by squaring it.  Which of the two roots comes back is decided by the caller (fq2_is_high).
HD Fq2 fq2_sqrt(const Fq2& a, bool* ok) {
  Fq2 r = Fq2::zero();
  bool k;
  if (a.c1.is_zero()) {
    r.c0 = fq_sqrt(a.c0, &k);
    if (!k) { r.c1 = fq_sqrt(fp_neg(a.c0), &k); r.c0 = Fq::zero(); }
  } else {
    const Fq s = fq_sqrt(fp_add(fp_sqr(a.c0), fp_sqr(a.c1)), &k);
    if (!k) { *ok = false; return Fq2::zero(); }
    constexpr uint32_t h[FQ_LIMBS] = FQ_INV2_MONT;
    Fq half;
    for (int i = 0; i < FQ_LIMBS; i++) half.l[i] = h[i];
    r.c0 = fq_sqrt(fp_mul(fp_add(a.c0, s), half), &k);
    if (!k) r.c0 = fq_sqrt(fp_mul(fp_sub(a.c0, s), half), &k);
    r.c1 = fp_mul(fp_mul(a.c1, half), fp_inv(r.c0));
  }
  *ok = f2_sqr(r) == a;
  return r;
}
// the sign of a compressed G2 encoding: y.c1 > (q-1)/2 when y.c1 != 0, else y.c0 > (q-1)/2 (standard form, below q)
HD bool fq2_is_high(const Fq& c0_std, const Fq& c1_std) { return c1_std.is_zero_strict() ? fq_is_high(c0_std) : fq_is_high(c1_std); }

struct G2Affine {
  Fq2 x, y;
  HD bool is_inf() const { return x.is_zero() && y.is_zero(); }
  static HD G2Affine inf() { G2Affine p; p.x = Fq2::zero(); p.y = Fq2::zero(); return p; }
};
struct G2Jac {
  Fq2 x, y, z;
  HD bool is_inf() const { return z.is_zero(); }
  static HD G2Jac inf() { G2Jac p; p.x = Fq2::one(); p.y = Fq2::one(); p.z = Fq2::zero(); return p; }
};

HD G2Jac g2_dbl(const G2Jac& p) {           // dbl-2009-l, a = 0
  if (p.is_inf() || p.y.is_zero()) return G2Jac::inf();
  Fq2 A = f2_sqr(p.x), B = f2_sqr(p.y), C = f2_sqr(B);
  Fq2 t = f2_sub(f2_sub(f2_sqr(f2_add(p.x, B)), A), C);
  Fq2 D = f2_dbl(t);
  Fq2 E = f2_add(f2_dbl(A), A), F = f2_sqr(E);
  G2Jac r;
  r.x = f2_sub(F, f2_dbl(D));
  Fq2 C8 = f2_dbl(f2_dbl(f2_dbl(C)));
  r.y = f2_sub(f2_mul(E, f2_sub(D, r.x)), C8);
  r.z = f2_dbl(f2_mul(p.y, p.z));
  return r;
}
HD G2Jac g2_add_mixed(const G2Jac& p, const G2Affine& q) {   // madd-2007-bl
  if (q.is_inf()) return p;
  if (p.is_inf()) { G2Jac r; r.x = q.x; r.y = q.y; r.z = Fq2::one(); return r; }
  Fq2 Z1Z1 = f2_sqr(p.z), U2 = f2_mul(q.x, Z1Z1), S2 = f2_mul(f2_mul(q.y, p.z), Z1Z1);
  if (U2 == p.x) {
    if (S2 == p.y) return g2_dbl(p);
    return G2Jac::inf();
  }
  Fq2 H = f2_sub(U2, p.x), HH = f2_sqr(H), I = f2_dbl(f2_dbl(HH)), J = f2_mul(H, I);
  Fq2 rr = f2_dbl(f2_sub(S2, p.y)), V = f2_mul(p.x, I);
  G2Jac r;
  r.x = f2_sub(f2_sub(f2_sqr(rr), J), f2_dbl(V));
  r.y = f2_sub(f2_mul(rr, f2_sub(V, r.x)), f2_dbl(f2_mul(p.y, J)));
  r.z = f2_sub(f2_sub(f2_sqr(f2_add(p.z, H)), Z1Z1), HH);
  return r;
}
// p + q, both Jacobian (add-2007-bl): the tree of the G2 sums (srs_g2.hip, k_g2_sum) and the host's additions of block totals
HD G2Jac g2_add(const G2Jac& p, const G2Jac& q) {
  if (q.is_inf()) return p;
  if (p.is_inf()) return q;
  Fq2 Z1Z1 = f2_sqr(p.z), Z2Z2 = f2_sqr(q.z);
  Fq2 U1 = f2_mul(p.x, Z2Z2), U2 = f2_mul(q.x, Z1Z1);
  Fq2 S1 = f2_mul(f2_mul(p.y, q.z), Z2Z2), S2 = f2_mul(f2_mul(q.y, p.z), Z1Z1);
  if (U1 == U2) {
    if (S1 == S2) return g2_dbl(p);
    return G2Jac::inf();
  }
  Fq2 H = f2_sub(U2, U1), I = f2_sqr(f2_dbl(H)), J = f2_mul(H, I);
  Fq2 rr = f2_dbl(f2_sub(S2, S1)), V = f2_mul(U1, I);
  G2Jac r;
  r.x = f2_sub(f2_sub(f2_sqr(rr), J), f2_dbl(V));
  r.y = f2_sub(f2_mul(rr, f2_sub(V, r.x)), f2_dbl(f2_mul(S1, J)));
  r.z = f2_mul(f2_sub(f2_sub(f2_sqr(f2_add(p.z, q.z)), Z1Z1), Z2Z2), H);
  return r;
}
// r P == O for a finite point of the twist (E'(Fq2) has a large cofactor and the pairing is bilinear only on the order-r subgroup): the
// literal double-and-add over the bits of r, the DEFINITION of membership and the differential reference of the test below
// (sonic_g2_subgroup_check with SONIC_SUBGROUP_WALK); no loader runs it.
HD bool g2_in_subgroup_walk(const G2Affine& p) {
  constexpr uint32_t rl[8] = FR_P;
  G2Jac acc; acc.x = p.x; acc.y = p.y; acc.z = Fq2::one();       // top bit (254) of r
#pragma unroll 1
  for (int bit = 253; bit >= 0; bit--) {
    acc = g2_dbl(acc);
    uint32_t word = 0;
#pragma unroll
    for (int k = 0; k < 8; k++) if (k == (bit >> 5)) word = rl[k];
    if ((word >> (bit & 31)) & 1u) acc = g2_add_mixed(acc, p);
  }
  return acc.is_inf();
}
// psi = twist . Frobenius . untwist on E'(Fq2): psi(x, y) = (conj(x) c_x, conj(y) c_y), c_x = (1 + u)^(-(q-1)/3), c_y = (1 + u)^(-(q-1)/2)
HD G2Affine g2_psi(const G2Affine& p) {
  constexpr uint32_t x0[12] = G2_PSI_CX_C0_MONT, x1[12] = G2_PSI_CX_C1_MONT, y0[12] = G2_PSI_CY_C0_MONT, y1[12] = G2_PSI_CY_C1_MONT;
  Fq2 cx, cy;
  for (int i = 0; i < 12; i++) { cx.c0.l[i] = x0[i]; cx.c1.l[i] = x1[i]; cy.c0.l[i] = y0[i]; cy.c1.l[i] = y1[i]; }
  Fq2 xb = p.x, yb = p.y;
  xb.c1 = fp_neg(xb.c1); yb.c1 = fp_neg(yb.c1);
  G2Affine r;
  r.x = f2_mul(xb, cx);
  r.y = f2_mul(yb, cy);
  return r;
}
// The membership test of every G2 input: a finite point P of the twist is in the order-r subgroup iff psi(P) = z P.  psi^2 - t psi + q = 0
// on E'(Fq2) with t = z + 1, so psi(P) = z P gives (z^2 - (z + 1) z + q) P = (q - z) P = O; q - z = h1 r, and the order of P divides
// #E'(Fq2) = h2 r with gcd(h1, h2) = 1, so it divides r.  z is negative: the comparison is against -(|z| P), in the
// accumulator's Jacobian coordinates (x = X / Z^2, y = Y / Z^3), without an inversion.  |z| has 64 bits of which 6 are set: 63 doublings
// and 5 additions, walked as g1_in_subgroup walks z^2, with the general addition.  Shared by k_g2_points_from_bytes, k_g2_decompress and
// k_g2_subgroup.
HD bool g2_in_subgroup(const G2Affine& p) {
  G2Jac acc; acc.x = p.x; acc.y = p.y; acc.z = Fq2::one();       // top bit (63) of |z|
  uint64_t w = BLS_Z_ABS << 1;                                    // the bits still to walk, left-aligned
  int left = 63;
#pragma unroll 1
  while (left > 0) {
    const int run = w ? __builtin_clzll(w) + 1 : left;            // up to and including the next set bit, or to the end
#pragma unroll 1
    for (int i = 0; i < run; i++) acc = g2_dbl(acc);
    if (w) acc = g2_add_mixed(acc, p);
    w = run < 64 ? w << run : 0;
    left -= run;
  }
  if (acc.is_inf()) return false;                                 // psi(P) is finite
  const G2Affine s = g2_psi(p);
  const Fq2 z2 = f2_sqr(acc.z);
  return f2_mul(s.x, z2) == acc.x && f2_mul(f2_neg(s.y), f2_mul(z2, acc.z)) == acc.y;
}
// on the twist y^2 = x^3 + 4 (u + 1): the right-hand side for an x (Montgomery)
HD Fq2 g2_curve_rhs(const Fq2& x) {
  Fq2 b; b.c0 = fp_dbl(fp_dbl(Fq::one())); b.c1 = b.c0;
  return f2_add(f2_mul(f2_sqr(x), x), b);
}

HD G2Affine g2_to_affine(const G2Jac& p) {
  if (p.is_inf()) return G2Affine::inf();
  Fq2 zi = f2_inv(p.z), zi2 = f2_sqr(zi);
  G2Affine r;
  r.x = f2_mul(p.x, zi2);
  r.y = f2_mul(p.y, f2_mul(zi2, zi));
  return r;
}

}  // namespace sonic
