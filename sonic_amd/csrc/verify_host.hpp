// Host side of the verifiers, shared by verify.hip (sonic_verify*, one proof, every pcV equation on its own) and verify_batch.hip (the
// batched verifier, K proofs folded into one pairing product): decoding, the verifier's G2 elements, the pcV equation, s(u, v) on the host,
// and -- the point of this header -- ONE function that lists the pcV checks of a proof (proof_checks), so that the two verifiers cannot
// drift apart in what they check.
//
// The lists are templates over the point type P: sonic_verify* parse points into G1Affine (load_g1: canonical, on the curve, in the order-r
// subgroup, all on the host); the batched verifier parses them into indices of a staging buffer that the device validates (k_g1_validate).
#pragma once
#include <string.h>
#include <vector>
#include "internal.hpp"
#include "g2.hpp"
#include "pairing.hpp"
#include "fs.hpp"
#include "csr.hpp"

namespace sonic {

// ---- host-side group / field helpers -------------------------------------------------------------------
inline G1XYZZ g1_mul_fr(const G1Affine& p, const Fr& k_std) {
  G1XYZZ acc = G1XYZZ::inf();
  const G1XYZZ base = G1XYZZ::from_affine(p);
  bool started = false;
  for (int i = 255; i >= 0; i--) {
    if (started) acc = g1_dbl(acc);
    if ((k_std.l[i >> 5] >> (i & 31)) & 1) { acc = g1_add(acc, base); started = true; }
  }
  return acc;
}
inline G1Affine g1_gen_host() {
  constexpr uint32_t gx[12] = G1_GEN_X_MONT, gy[12] = G1_GEN_Y_MONT;
  G1Affine g;
  for (int i = 0; i < 12; i++) { g.x.l[i] = gx[i]; g.y.l[i] = gy[i]; }
  return g;
}
inline bool load_fr(const uint8_t* b, Fr& mont) { Fr s; memcpy(s.l, b, 32); if (!fp_is_canonical(s)) return false; mont = fp_to_mont(s); return true; }
inline bool load_g1(const uint8_t* b, G1Affine& p) {
  memcpy(p.x.l, b, 48); memcpy(p.y.l, b + 48, 48);
  if (p.is_inf()) return true;
  if (!fp_is_canonical(p.x) || !fp_is_canonical(p.y)) return false;
  p.x = fp_to_mont(p.x); p.y = fp_to_mont(p.y);
  Fq four = fp_dbl(fp_dbl(Fq::one()));
  if (!(fp_sqr(p.y) == fp_add(fp_mul(fp_sqr(p.x), p.x), four))) return false;
  // E(Fq) has cofactor points (e.g. (0, 2), order 3) and the pairing is bilinear only on the order-r subgroup: points that
  // come from a prover must satisfy r P = O before they reach the Miller loop
  constexpr uint32_t rl[8] = FR_P;
  Fr r_std; for (int i = 0; i < 8; i++) r_std.l[i] = rl[i];
  return g1_mul_fr(p, r_std).is_inf();
}
inline bool load_g2(const uint8_t* b, G2Affine& p) {
  memcpy(p.x.c0.l, b, 48); memcpy(p.x.c1.l, b + 48, 48); memcpy(p.y.c0.l, b + 96, 48); memcpy(p.y.c1.l, b + 144, 48);
  if (p.is_inf()) return true;
  p.x.c0 = fp_to_mont(p.x.c0); p.x.c1 = fp_to_mont(p.x.c1); p.y.c0 = fp_to_mont(p.y.c0); p.y.c1 = fp_to_mont(p.y.c1);
  return true;
}
inline Fr fr_pow(const Fr& a, uint64_t e) { return fp_pow_u64(a, e); }

struct VerifierKey { G2Affine h_alpha, h_alpha_x; };   // hPositiveAlphaX[0], [1]

inline int fetch_g2(const sonic_srs* srs, int basis, int64_t e, G2Affine& out) {
  uint8_t b[192];
  int rc = sonic_srs_get_g2_points(srs, basis, e, 1, b);
  if (rc) return rc;
  load_g2(b, out);
  // fail closed: the Miller loop of a G2 element at infinity is 1, so a verifier key at infinity would accept anything.  No valid
  // SRS (x, alpha != 0) holds one; sonic_srs_set_g2_points / sonic_srs_load refuse them, this is the second line of defence.
  if (out.is_inf()) { set_error("verifier: the SRS holds the point at infinity as G2 element (basis %d, exponent %ld)", basis, (long)e); return SONIC_ERR_BAD_ENCODING; }
  return SONIC_OK;
}

inline int load_verifier_key(const sonic_srs* srs, VerifierKey& vk) {
  int rc = fetch_g2(srs, 1, 0, vk.h_alpha);
  if (!rc) rc = fetch_g2(srs, 1, 1, vk.h_alpha_x);
  return rc;
}

// pcV srs max F z (v, W)  (CommitmentScheme.hs:51-68), in two steps: the G2 element h^{x^{-d+max}} comes from the SRS handle
// (device memory, the library's call mutex), the pairing equation itself is pure host arithmetic -- so a verifier's checks
// fetch their elements first and then run side by side on host threads (a proof with Q constraints has 4 + 3Q of them at
// ~6-9 ms each: three Miller loops, one final exponentiation, two scalar multiples in G1).
inline int pc_v_element(const sonic_srs* srs, int64_t maxm, G2Affine& hxi) {
  const int64_t d = srs_d(srs);
  const int64_t difference = -d + maxm;                              // h^{x^{-d+max}}: hPositiveX / hNegativeX
  if (difference > d || difference < -d) { set_error("pcV: hPositiveX / hNegativeX is not long enough: %ld", (long)difference); return SONIC_ERR_SRS_INDEX; }
  return fetch_g2(srs, 0, difference, hxi);
}
inline bool pc_v_equation(const VerifierKey& vk, const G2Affine& hxi, const G1Affine& F, const Fr& z_m, const Fr& v_m, const G1Affine& W) {
  const Fr v = fp_from_mont(v_m), negz = fp_from_mont(fp_neg(z_m));
  G1Affine left = g1_to_affine(g1_add(g1_mul_fr(g1_gen_host(), v), g1_mul_fr(W, negz)));   // g^v W^{-z}
  G1Affine negF = g1_neg(F);
  using namespace pairing;
  const F12 f = f12_mul(f12_mul(miller_loop(W, vk.h_alpha_x), miller_loop(left, vk.h_alpha)), miller_loop(negF, hxi));
  return final_exponentiation(f).is_one();                           // eA <> eB == eC
}

// ---- a proof and the list of its checks, over a point type P --------------------------------------------
// one pcV check: e(W, h^{alpha x}) e(g^val W^{-z}, h^alpha) = e(F, h^{x^{maxm - d}})
template <class P> struct PcvCheckT { int64_t maxm; P F; Fr z, val; P W; };
using PcvCheck = PcvCheckT<G1Affine>;

// an HscProof (Signature.hs:22-29) with the (y_j, z_j) it is checked at, parsed
template <class P> struct HscProofViewT { std::vector<P> Sj, Wj, Wpj, Qj; std::vector<Fr> sj, spj, ys, zs; P Qv, C; Fr u, v; };
using HscProofView = HscProofViewT<G1Affine>;
// a Proof (Protocol.hs:28-38): R, T, a, Wa, b, Wb, Wt, s, then its HscProof
template <class P> struct ProofViewT { P R, T, Wa, Wb, Wt; Fr a, b, s; HscProofViewT<P> h; };

// [S_j, s_j, W_j]_j, [s'_j, W'_j, Q_j]_j, Q_v, C, u, v (m entries per list: sonic_hsc_proof_size(m) bytes) and the m pairs of yzs;
// false: a non-canonical field element, or a point that load_point refuses (load_g1: off the curve or outside the order-r subgroup)
template <class P, class LoadPoint>
bool parse_hsc(const uint8_t* p, int64_t m, const uint8_t* yzs, HscProofViewT<P>& h, LoadPoint&& load_point) {
  auto G = [&](P& o) { bool k = load_point(p, o); p += 96; return k; };
  auto F = [&](Fr& o) { bool k = load_fr(p, o); p += 32; return k; };
  for (auto* g : {&h.Sj, &h.Wj, &h.Wpj, &h.Qj}) g->resize((size_t)m);
  for (auto* f : {&h.sj, &h.spj, &h.ys, &h.zs}) f->resize((size_t)m);
  bool enc = true;
  for (int64_t j = 0; j < m; j++) enc = enc && G(h.Sj[j]) && F(h.sj[j]) && G(h.Wj[j]);
  for (int64_t j = 0; j < m; j++) enc = enc && F(h.spj[j]) && G(h.Wpj[j]) && G(h.Qj[j]);
  enc = enc && G(h.Qv) && G(h.C) && F(h.u) && F(h.v);
  for (int64_t j = 0; j < m; j++) enc = enc && load_fr(yzs + 64 * j, h.ys[j]) && load_fr(yzs + 64 * j + 32, h.zs[j]);
  return enc;
}
inline bool parse_hsc(const uint8_t* p, int64_t m, const uint8_t* yzs, HscProofView& h) { return parse_hsc(p, m, yzs, h, load_g1); }

// sonic_proof_size(Q) bytes of proof and the challenges y, z, (y_j, z_j)_j it is checked at
template <class P, class LoadPoint>
bool parse_proof(const uint8_t* proof, int64_t Q, const uint8_t y[32], const uint8_t z[32], const uint8_t* yzs, ProofViewT<P>& v, Fr& ym, Fr& zm,
                 LoadPoint&& load_point) {
  const uint8_t* p = proof;
  auto G = [&](P& o) { bool k = load_point(p, o); p += 96; return k; };
  auto F = [&](Fr& o) { bool k = load_fr(p, o); p += 32; return k; };
  return G(v.R) && G(v.T) && F(v.a) && G(v.Wa) && F(v.b) && G(v.Wb) && G(v.Wt) && F(v.s) && parse_hsc(p, Q, yzs, v.h, load_point) && load_fr(y, ym) &&
         load_fr(z, zm);
}

// t = a (b + s) - k(y), k(y) = sum_q cs[q] y^{n+q} (Protocol.hs:120; Constraints.hs:67-68); false: a non-canonical cs[q]
template <class P>
bool proof_t(const CircuitView& c, const ProofViewT<P>& v, const Fr& ym, Fr& t) {
  Fr ky = Fr::zero(), pw = fr_pow(ym, (uint64_t)c.n);
  for (int64_t q = 0; q < c.Q; q++) { Fr k; if (!load_fr(c.cs + 32 * q, k)) return false; pw = fp_mul(pw, ym); ky = fp_add(ky, fp_mul(k, pw)); }
  t = fp_sub(fp_mul(v.a, fp_add(v.b, v.s)), ky);
  return true;
}

// the end of hscVerify once s(u,v) is known: its 3m + 1 pcV checks (Signature.hs:82-89), appended to those the caller brings
template <class P>
void hsc_checks(int64_t d, const HscProofViewT<P>& h, const Fr& sv, std::vector<PcvCheckT<P>>& checks) {
  for (size_t j = 0; j < h.Sj.size(); j++) {                       // Signature.hs:82-88
    checks.push_back(PcvCheckT<P>{d, h.Sj[j], h.zs[j], h.sj[j], h.Wj[j]});
    checks.push_back(PcvCheckT<P>{d, h.Sj[j], h.u, h.spj[j], h.Wpj[j]});
    checks.push_back(PcvCheckT<P>{d, h.C, h.ys[j], h.spj[j], h.Qj[j]});
  }
  checks.push_back(PcvCheckT<P>{d, h.C, h.v, sv, h.Qv});           // Signature.hs:89
}

// the three checks of the head (Protocol.hs:123-125): ALL the pcV checks of a core proof, whose fourth condition -- the proof's s is
// s(z, y) -- the verifier establishes itself (s_of_uv at u = z, v = y); of a full proof the first three
template <class P>
std::vector<PcvCheckT<P>> core_checks(int64_t n, int64_t d, const ProofViewT<P>& v, const Fr& ym, const Fr& zm, const Fr& t) {
  return std::vector<PcvCheckT<P>>{PcvCheckT<P>{n, v.R, zm, v.a, v.Wa},                       // Protocol.hs:123
                                   PcvCheckT<P>{n, v.R, fp_mul(ym, zm), v.b, v.Wb},           // :124
                                   PcvCheckT<P>{d, v.T, zm, t, v.Wt}};                        // :125
}

// THE list of a proof's 4 + 3Q checks (Protocol.hs:123-125, then hscVerify's), in the order both verifiers number them
template <class P>
std::vector<PcvCheckT<P>> proof_checks(int64_t n, int64_t d, const ProofViewT<P>& v, const Fr& ym, const Fr& zm, const Fr& t, const Fr& sv) {
  std::vector<PcvCheckT<P>> checks = core_checks(n, d, v, ym, zm, t);
  hsc_checks(d, v.h, sv, checks);
  return checks;
}

// 576 bytes of core proof (R, T, a, Wa, b, Wb, Wt, s) and the challenges y, z it is checked at; the signature part of the view stays empty
template <class P, class LoadPoint>
bool parse_core_proof(const uint8_t* proof, const uint8_t y[32], const uint8_t z[32], ProofViewT<P>& v, Fr& ym, Fr& zm, LoadPoint&& load_point) {
  const uint8_t* p = proof;
  auto G = [&](P& o) { bool k = load_point(p, o); p += 96; return k; };
  auto F = [&](Fr& o) { bool k = load_fr(p, o); p += 32; return k; };
  return G(v.R) && G(v.T) && F(v.a) && G(v.Wa) && F(v.b) && G(v.Wb) && G(v.Wt) && F(v.s) && load_fr(y, ym) && load_fr(z, zm);
}

// s(u, v) for the s(X,Y) of a circuit (Signature.hs:81; Constraints.hs:34-53): sum_i u^-i U_i(v) + u^i V_i(v) + u^{i+n} W_i(v).  Dense
// weights: O(Q n), gate by gate.  Sparse ones (validated by the caller): O(nnz + n) -- per row q of each matrix the entries sum
// val * u^{-i | i | i+n}, scaled by v^{n+q}; the diagonal terms u^{i+n} (-v^i - v^-i) are summed on their own.
inline int s_of_uv(const CircuitView& c, const Fr& u, const Fr& v, Fr& sv) {
  const int64_t n = c.n, Q = c.Q;
  if (u.is_zero() || v.is_zero()) { set_error("hscVerify: u or v is zero"); return SONIC_ERR_INEXACT_DIVISION; }
  const Fr uinv = fp_inv(u), vinv = fp_inv(v);
  sv = Fr::zero();
  if (!c.csr) {
    std::vector<Fr> vq(Q);
    { Fr x = fr_pow(v, (uint64_t)n); for (int64_t q = 0; q < Q; q++) { x = fp_mul(x, v); vq[q] = x; } }
    const Fr un = fr_pow(u, (uint64_t)n);
    Fr up = Fr::one(), um = Fr::one(), vp = Fr::one(), vm = Fr::one();
    for (int64_t i = 1; i <= n; i++) {
      up = fp_mul(up, u); um = fp_mul(um, uinv); vp = fp_mul(vp, v); vm = fp_mul(vm, vinv);
      Fr Ui = Fr::zero(), Vi = Fr::zero(), Wi = Fr::zero(), w;
      for (int64_t q = 0; q < Q; q++) {
        if (!load_fr(c.wL + 32 * (q * n + i - 1), w)) return SONIC_ERR_BAD_ENCODING; Ui = fp_add(Ui, fp_mul(w, vq[q]));
        if (!load_fr(c.wR + 32 * (q * n + i - 1), w)) return SONIC_ERR_BAD_ENCODING; Vi = fp_add(Vi, fp_mul(w, vq[q]));
        if (!load_fr(c.wO + 32 * (q * n + i - 1), w)) return SONIC_ERR_BAD_ENCODING; Wi = fp_add(Wi, fp_mul(w, vq[q]));
      }
      Wi = fp_sub(fp_sub(Wi, vp), vm);
      sv = fp_add(sv, fp_add(fp_add(fp_mul(um, Ui), fp_mul(up, Vi)), fp_mul(fp_mul(up, un), Wi)));
    }
    return SONIC_OK;
  }
  // upos[e] = u^e (e in [0, 2n]), uneg[i] = u^-i (i in [0, n])
  std::vector<Fr> upos((size_t)(2 * n + 1)), uneg((size_t)(n + 1));
  upos[0] = uneg[0] = Fr::one();
  for (int64_t e = 1; e <= 2 * n; e++) upos[(size_t)e] = fp_mul(upos[(size_t)e - 1], u);
  for (int64_t i = 1; i <= n; i++) uneg[(size_t)i] = fp_mul(uneg[(size_t)i - 1], uinv);
  Fr vq = fr_pow(v, (uint64_t)n);
  for (int64_t q = 0; q < Q; q++) {
    vq = fp_mul(vq, v);                                              // v^{n+q+1}
    Fr rowsum = Fr::zero(), w;
    for (int mat = 0; mat < 3; mat++) {
      const int64_t r = mat * Q + q;
      for (int64_t k = c.row_ptr[r]; k < c.row_ptr[r + 1]; k++) {
        if (!load_fr(c.val + 32 * k, w)) return SONIC_ERR_BAD_ENCODING;
        const int64_t i = c.col[k] + 1;
        const Fr& up = mat == 0 ? uneg[(size_t)i] : upos[(size_t)(mat == 1 ? i : i + n)];
        rowsum = fp_add(rowsum, fp_mul(w, up));
      }
    }
    sv = fp_add(sv, fp_mul(rowsum, vq));
  }
  Fr vp = Fr::one(), vm = Fr::one();
  for (int64_t i = 1; i <= n; i++) {
    vp = fp_mul(vp, v); vm = fp_mul(vm, vinv);
    sv = fp_sub(sv, fp_mul(upos[(size_t)(i + n)], fp_add(vp, vm)));
  }
  return SONIC_OK;
}

}  // namespace sonic
