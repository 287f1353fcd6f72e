// The proof that goes with a contribution to an updatable SRS (include/sonic_hip.h, "Updatable SRS"): its layout, its challenge, its
// nonces, its maker and the part of its verifier that needs no reference string.  Host only, no HIP in here:
// tests/host/srs_update_host.cpp compiles it with g++, and tests/srs_update_ref.py restates it with hashlib and Python integers.
//
// A contributor holds shares x1, alpha1 (non-zero, below r) and turns a string with trapdoor (x, alpha) into the one with (x x1, alpha alpha1):
//   G0'[e] = x1^e G0[e],  G1'[e] = alpha1 x1^e G1[e],  H0'[e] = x1^e H0[e],  H1'[e] = alpha1 x1^e H1[e]        e in [-d, d]
// (G0 = g^{x^e}, G1 = g^{alpha x^e}, H0, H1 the same over h).  The proof is two Schnorr proofs of knowledge under one challenge:
//
//   proof (448 bytes) = X = x1 g (96) || A = alpha1 g (96) || Rx = kx g (96) || Ra = ka g (96) || sx (32) || sa (32)
//   points as canonical affine x || y, little-endian; scalars canonical, little-endian
//
//   st0 = SHA256("sonic-hip/srs-update/v1" || le64 d || srs id of the OLD string)          (srs id: fs.hpp)
//   st1 = SHA256(st0 || "points" || X || A || Rx || Ra)                                    (absorb, fs.hpp)
//   c   = challenge("c", 0) of st1: 512 bits reduced mod r, 1 in place of 0                (challenge, fs.hpp)
//   sx  = kx + c x1,   sa = ka + c alpha1                                                  (mod r)
//
// The nonces kx, ka come from the operating system.  For reproducible tests a caller may pass a 32-byte seed instead:
//   k_i = wide-reduce(SHA256(L || 0x00) || SHA256(L || 0x01)),  L = "sonic-hip/srs-update-nonce/v1" || seed || x1 || alpha1 || old id || le32 i
//   kx = k_0, ka = k_1, 1 in place of 0.  The shares are inside the hash (as the witness is inside the prover's blinders, fs.hpp): one
//   seed used for two contributions does not give them one nonce.
//
// A verifier with both strings accepts iff
//   - both strings have the same d;
//   - X, A, Rx, Ra are canonical, on the curve, in the order-r subgroup and not infinity; sx, sa are canonical;
//   - sx g = Rx + c X  and  sa g = Ra + c A;                                              (schnorr_ok, below)
//   - e(G0'[1], h) = e(X, H0[1])  and  e(g, H1'[0]) = e(A, H1[0]);                        (pairs_equal, below; the caller fetches the points)
//   - the new string passes sonic_srs_check (where the caller asks for it).
// The check says the new string is well-formed for SOME (x*, alpha*); the two pairing equations say x* = x x1 and alpha* = alpha alpha1
// for the discrete logs x1, alpha1 of X and A; the Schnorr proofs say the contributor knew them; the old id inside c keeps a proof
// from being replayed on another string.
#pragma once
#include <errno.h>
#include <string.h>
#include <sys/random.h>
#include "fs.hpp"
#include "g1_host.hpp"
#include "pairing.hpp"
#include "srs_scale.hpp"

namespace sonic {
namespace srs_update {

constexpr size_t PROOF_BYTES = 448;
constexpr size_t OFF_X = 0, OFF_A = 96, OFF_RX = 192, OFF_RA = 288, OFF_SX = 384, OFF_SA = 416;

inline G1Affine g1_gen() {
  constexpr uint32_t gx[12] = G1_GEN_X_MONT, gy[12] = G1_GEN_Y_MONT;
  G1Affine g;
  for (int i = 0; i < 12; i++) { g.x.l[i] = gx[i]; g.y.l[i] = gy[i]; }
  return g;
}
inline G2Affine g2_gen() {
  constexpr uint32_t x0[12] = G2_GEN_X0_MONT, x1[12] = G2_GEN_X1_MONT, y0[12] = G2_GEN_Y0_MONT, y1[12] = G2_GEN_Y1_MONT;
  G2Affine g;
  for (int i = 0; i < 12; i++) { g.x.c0.l[i] = x0[i]; g.x.c1.l[i] = x1[i]; g.y.c0.l[i] = y0[i]; g.y.c1.l[i] = y1[i]; }
  return g;
}

// n bytes from the operating system: interrupted and short reads are continued; false when it gives none
inline bool os_random(void* out, size_t n) {
  uint8_t* p = static_cast<uint8_t*>(out);
  while (n > 0) {
    const ssize_t got = getrandom(p, n, 0);
    if (got < 0) { if (errno == EINTR) continue; return false; }
    p += got; n -= (size_t)got;
  }
  return true;
}

// zeroes memory that held a share, its inverse or a nonce, in a way the compiler may not drop
inline void wipe(void* p, size_t n) {
  volatile uint8_t* b = static_cast<volatile uint8_t*>(p);
  for (size_t i = 0; i < n; i++) b[i] = 0;
}

// 96 canonical bytes -> a point a proof may hold: canonical coordinates, on the curve, r P = O, not infinity
inline bool load_point(const uint8_t* b, G1Affine& p) {
  memcpy(p.x.l, b, 48); memcpy(p.y.l, b + 48, 48);
  if (p.is_inf() || !fp_is_canonical(p.x) || !fp_is_canonical(p.y)) return false;
  p.x = fp_to_mont(p.x); p.y = fp_to_mont(p.y);
  const Fq four = fp_dbl(fp_dbl(Fq::one()));
  if (!(fp_sqr(p.y) == fp_add(fp_mul(fp_sqr(p.x), p.x), four))) return false;
  return g1_in_subgroup(p);
}
inline bool load_scalar(const uint8_t* b, Fr& std_form) { memcpy(std_form.l, b, 32); return fp_is_canonical(std_form); }

// c (32 canonical bytes) from d, the old string's id and the four points of a proof (its first 384 bytes)
inline void challenge(int64_t d, const uint8_t old_id[32], const uint8_t* points384, uint8_t out32[32]) {
  FsTranscript t;
  Sha256 h;
  h.update("sonic-hip/srs-update/v1", 23);
  FsTranscript::le64(h, d);
  h.update(old_id, 32);
  h.finish(t.st);
  t.absorb("points", points384, 384);
  t.challenge("c", 0, out32);
}

// nonce i (0: kx, 1: ka) of a seeded contribution, 32 canonical bytes
inline void seeded_nonce(const uint8_t seed[32], const uint8_t x1[32], const uint8_t alpha1[32], const uint8_t old_id[32], uint32_t i, uint8_t out32[32]) {
  uint8_t w[64];
  for (uint8_t half = 0; half < 2; half++) {
    Sha256 h;
    h.update("sonic-hip/srs-update-nonce/v1", 29); h.update(seed, 32); h.update(x1, 32); h.update(alpha1, 32); h.update(old_id, 32);
    const uint8_t idx[5] = {(uint8_t)i, (uint8_t)(i >> 8), (uint8_t)(i >> 16), (uint8_t)(i >> 24), half};
    h.update(idx, 5);
    h.finish(w + 32 * half);
  }
  Fr k = fs_wide_reduce(w);
  if (k.is_zero()) k.l[0] = 1;
  memcpy(out32, k.l, 32);
  wipe(w, sizeof w); wipe(k.l, 32);
}

// the proof of a contribution with shares x1, alpha1 and nonces kx, ka (all 32 canonical bytes, non-zero).  The caller wipes its inputs.
inline void make_proof(int64_t d, const uint8_t old_id[32], const uint8_t x1[32], const uint8_t alpha1[32], const uint8_t kx[32], const uint8_t ka[32],
                       uint8_t proof[PROOF_BYTES]) {
  Fr s[4];
  memcpy(s[0].l, x1, 32); memcpy(s[1].l, alpha1, 32); memcpy(s[2].l, kx, 32); memcpy(s[3].l, ka, 32);
  G1XYZZ pts[4];
  const G1Affine g = g1_gen();
  for (int i = 0; i < 4; i++) pts[i] = g1_scale(g, s[i]);
  g1_canonical_bytes_host_batch(pts, 4, proof);
  uint8_t cb[32];
  challenge(d, old_id, proof, cb);
  Fr c;
  memcpy(c.l, cb, 32);
  c = fp_to_mont(c);
  for (int i = 0; i < 2; i++) {
    Fr r = fp_from_mont(fp_add(fp_to_mont(s[2 + i]), fp_mul(c, fp_to_mont(s[i]))));
    memcpy(proof + OFF_SX + 32 * i, r.l, 32);
    wipe(r.l, 32);
  }
  wipe(s, sizeof s); wipe(pts, sizeof pts);
}

// the string-independent half of the verifier: the encodings and the two Schnorr equations; X and A come back for the pairing equations
inline bool schnorr_ok(int64_t d, const uint8_t old_id[32], const uint8_t proof[PROOF_BYTES], G1Affine& X, G1Affine& A) {
  G1Affine Rx, Ra;
  Fr sx, sa;
  if (!load_point(proof + OFF_X, X) || !load_point(proof + OFF_A, A) || !load_point(proof + OFF_RX, Rx) || !load_point(proof + OFF_RA, Ra)) return false;
  if (!load_scalar(proof + OFF_SX, sx) || !load_scalar(proof + OFF_SA, sa)) return false;
  uint8_t cb[32];
  challenge(d, old_id, proof, cb);
  Fr c;
  memcpy(c.l, cb, 32);
  const G1Affine g = g1_gen();
  const G1XYZZ both[4] = {g1_scale(g, sx), g1_add_mixed(g1_scale(X, c), Rx), g1_scale(g, sa), g1_add_mixed(g1_scale(A, c), Ra)};
  uint8_t b[4 * 96];
  g1_canonical_bytes_host_batch(both, 4, b);
  return memcmp(b, b + 96, 96) == 0 && memcmp(b + 192, b + 288, 96) == 0;
}

// e(P1, Q1) == e(P2, Q2): two Miller loops and one final exponentiation.  Points are validated by the caller.
inline bool pairs_equal(const G1Affine& P1, const G2Affine& Q1, const G1Affine& P2, const G2Affine& Q2) {
  using namespace pairing;
  const G1Affine n2 = P2.is_inf() ? P2 : g1_neg(P2);
  return final_exponentiation(f12_mul(miller_loop(P1, Q1), miller_loop(n2, Q2))).is_one();
}

}  // namespace srs_update
}  // namespace sonic
