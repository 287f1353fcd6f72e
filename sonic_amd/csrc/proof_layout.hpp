// The numbering of a proof, in ONE place (host only, no HIP; also compiled by tests/host): the MSM slots of its 7 + 4Q commitments and
// openings, the side slots whose sums the host adds to S_j and C, the 3 + 2Q evaluations, the 8 + 2Q transcript elements with their
// {v, v^-1} pairs, and the canonical bytes.  prove.hip and share_plan.hpp use these names only; tests/test_proof_layout_host.py holds
// them against the Python restatements (sonic_amd/protocol.py, tests/test_share_cpu.py).
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <string.h>

namespace sonic {

struct ProofLayout {
  long Q;
  // counts
  constexpr long K() const { return 7 + 4 * Q; }                    // commitments and openings = main MSM slots
  constexpr long F() const { return 3 + 2 * Q; }                    // evaluations
  constexpr long slots_total() const { return 7 + 5 * Q + 1; }      // K results, Q second halves of the S_j, 1 second half of C
  constexpr long transcript_len() const { return 8 + 2 * Q; }
  constexpr long n_pairs() const { return 5 + 2 * Q; }
  constexpr size_t proof_bytes() const { return (size_t)(K() * 96 + (F() + 2) * 32); }
  constexpr size_t proof_bytes_compressed() const { return (size_t)(K() * 48 + (F() + 2) * 32); }      // every point as its 48 bytes
  // MSM slots, the order of a share's pieces: R, T, W_a, W_b, W_t, [S_j, W_j]_j, [W'_j, Q_j]_j, Q_v, C
  static constexpr long R = 0, T = 1, Wa = 2, Wb = 3, Wt = 4;
  constexpr long S(long j) const { return 5 + 2 * j; }
  constexpr long W(long j) const { return 6 + 2 * j; }
  constexpr long Wp(long j) const { return 5 + 2 * Q + 2 * j; }
  constexpr long Qj(long j) const { return 6 + 2 * Q + 2 * j; }
  constexpr long Qv() const { return 5 + 4 * Q; }
  constexpr long C() const { return 6 + 4 * Q; }
  // side slots: S_j's second half (sum_q y_j^{n+q} C_q of a prepared handle, or the runs of equal coefficients) and C's Q-term half
  constexpr long S_extra(long j) const { return K() + j; }
  constexpr long C_extra() const { return K() + Q; }
  // evaluations, and the slot whose first piece reports each: a <- W_a, b <- W_b, s <- W_t, s_j <- W_j, s'_j <- Q_j
  static constexpr long a = 0, b = 1, s = 2;
  constexpr long s_j(long j) const { return 3 + j; }
  constexpr long sp_j(long j) const { return 3 + Q + j; }
  constexpr long eval_owner_slot(long i) const { return i == a ? Wa : i == b ? Wb : i == s ? Wt : i < sp_j(0) ? W(i - s_j(0)) : Qj(i - sp_j(0)); }
  // transcript: the blinders 0..3, then the challenges in draw order
  static constexpr long n_blinders = 4, y = 4, z = 5;
  constexpr long y_j(long j) const { return 6 + j; }
  constexpr long z_j(long j) const { return 6 + Q + j; }
  constexpr long u() const { return 6 + 2 * Q; }
  constexpr long v() const { return 7 + 2 * Q; }
  // {v, v^-1} pairs of the evaluation points (PAIRS: two field elements each)
  static constexpr long pY = 0, pZ = 1, pYZ = 2, pU = 3, pV = 4;
  constexpr long pYj(long j) const { return 5 + j; }
  constexpr long pZj(long j) const { return 5 + Q + j; }
  // exponent ranges of a proof's dense polynomials over n multiplication gates: r(X, 1) with its four blinders, s(X, y_j), t(X, y) and
  // s(u, Y) with its Q constraint terms; R is committed with max = n, the others with max = d (prove.hip; srs_view.hpp sizes a view by them)
  static constexpr long r_lo(long n) { return -2 * n - 4; }
  static constexpr long r_len(long n) { return 3 * n + 5; }
  static constexpr long s_lo(long n) { return -n; }
  static constexpr long s_len(long n) { return 3 * n + 1; }
  static constexpr long t_lo(long n) { return -4 * n - 8; }
  static constexpr long t_len(long n) { return 7 * n + 9; }
  static constexpr long u_lo(long n) { return -n; }
  constexpr long u_len(long n) const { return 2 * n + Q + 1; }
  // a CORE proof (include/sonic_hip.h, "Core proofs"): the head of the record -- R, T, a, W_a, b, W_b, W_t, s -- and nothing of the
  // signature, whatever Q is: the slots 0 .. 4, the evaluations 0 .. 2, the transcript elements 0 .. 5 (4 blinders, y, z)
  static constexpr long core_K = 5, core_F = 3, core_transcript_len = 6;
  // the pairs a core proof reads are pY, pZ, pYZ; it uploads the five-pair prefix (pU, pV as {1, 1}: never drawn, never read).  These
  // prefixes are what ProofLayout{0} counts, and what a prover handle holds until its first proof with a signature (prover.hpp)
  static constexpr long core_n_pairs = 5;
  static constexpr size_t core_proof_bytes() { return (size_t)(core_K * 96 + core_F * 32); }                  // 576
  static constexpr size_t core_proof_bytes_compressed() { return (size_t)(core_K * 48 + core_F * 32); }       // 336
};

// canonical proof bytes from the 7 + 4Q points (slot order) and the 3 + 2Q evaluations: record order of `Proof` (Protocol.hs:28-38)
// then `HscProof` (Signature.hs:22-29)
// the record order itself: onG(slot) for a point, onF(i) for evaluation i, then onF(-1), onF(-2) for u and v
// (a core proof's record order: the head of a proof's, which proof_record_order opens with)
template <class OnG, class OnF>
inline void core_proof_record_order(OnG&& onG, OnF&& onF) {
  using L = ProofLayout;
  onG(L::R); onG(L::T); onF(L::a); onG(L::Wa); onF(L::b); onG(L::Wb); onG(L::Wt); onF(L::s);
}
template <class OnG, class OnF>
inline void proof_record_order(long Q, OnG&& onG, OnF&& onF) {
  const ProofLayout L{Q};
  core_proof_record_order(onG, onF);
  for (long j = 0; j < Q; j++) { onG(L.S(j)); onF(L.s_j(j)); onG(L.W(j)); }             // hscS
  for (long j = 0; j < Q; j++) { onF(L.sp_j(j)); onG(L.Wp(j)); onG(L.Qj(j)); }          // hscW
  onG(L.Qv()); onG(L.C());
  onF(-1); onF(-2);
}
inline void proof_layout(long Q, const uint8_t* pts, const uint8_t* frs, const uint8_t* transcript, uint8_t* out_proof) {
  const ProofLayout L{Q};
  uint8_t* o = out_proof;
  proof_record_order(Q, [&](long slot) { memcpy(o, pts + 96 * (size_t)slot, 96); o += 96; },
                     [&](long i) { memcpy(o, i >= 0 ? frs + 32 * (size_t)i : transcript + 32 * (size_t)(i == -1 ? L.u() : L.v()), 32); o += 32; });
}
// The same proof with every point in another encoding -- 96 <-> 48 bytes (compress.hpp): `in` is walked in record order with points of
// in_pt bytes, `out` gets points of out_pt bytes made by point(in, out) (false: refused, the walk goes on and the result is false) and
// the field elements as they are.
template <class Point>
inline bool proof_repack(long Q, const uint8_t* in, size_t in_pt, uint8_t* out, size_t out_pt, Point&& point) {
  bool ok = true;
  proof_record_order(Q, [&](long) { ok = point(in, out) && ok; in += in_pt; out += out_pt; }, [&](long) { memcpy(out, in, 32); in += 32; out += 32; });
  return ok;
}

// the two for a core proof: 576 bytes from the points of the slots 0 .. 4 and the evaluations a, b, s; and its 96 <-> 48 byte repack
inline void core_proof_layout(const uint8_t* pts, const uint8_t* frs, uint8_t* out_proof) {
  uint8_t* o = out_proof;
  core_proof_record_order([&](long slot) { memcpy(o, pts + 96 * (size_t)slot, 96); o += 96; }, [&](long i) { memcpy(o, frs + 32 * (size_t)i, 32); o += 32; });
}
template <class Point>
inline bool core_proof_repack(const uint8_t* in, size_t in_pt, uint8_t* out, size_t out_pt, Point&& point) {
  bool ok = true;
  core_proof_record_order([&](long) { ok = point(in, out) && ok; in += in_pt; out += out_pt; }, [&](long) { memcpy(out, in, 32); in += 32; out += 32; });
  return ok;
}

// S_j's point is its slot's sum plus its side slot's, C's likewise: `side` holds the sums of the side slots K .. K + Q (the empty sum
// where none ran), s_extra / c_extra say which of the two rules the proof runs with (prepared or runs; symmetric sums)
template <class Point, class Add>
inline void fold_side_slots(const ProofLayout& L, bool s_extra, bool c_extra, Point* sums, const Point* side, Add add) {
  for (long j = 0; s_extra && j < L.Q; j++) sums[L.S(j)] = add(sums[L.S(j)], side[L.S_extra(j) - L.K()]);
  if (c_extra) sums[L.C()] = add(sums[L.C()], side[L.C_extra() - L.K()]);
}

}  // namespace sonic
