// Opt-in Fiat-Shamir transcript for prove / verify.  The reference's prover DRAWS its challenges (`rnd`, MonadRandom) --
// y after R (src/Sonic/Protocol.hs:66), z after T (:76), y_j / z_j after the openings (:84-85), u after the S_j
// (src/Sonic/Signature.hs:48), v after C and the W'_j / Q_j (:60) -- and hands them to the verifier in RndOracle.  Here each draw
// can instead be a hash of everything that precedes it, in that same order, so that a proof carries its own challenges:
//
//   st_0 = SHA256("sonic-hip/fs/v2" || le64 n || le64 Q || le64 d || circuit digest || srs id)
//   srs id = SHA256("sonic-hip/srs/v1" || le64 d || g^x || g^{alpha x} || g^{1/x} || g^{alpha/x})   (gPositiveX[1], gPositiveAlphaX[0],
//            gNegativeX[0], gNegativeAlphaX[0] of SRS.hs:33-39, 96 canonical bytes each: they determine x and alpha, so a proof is
//            tied to ONE reference string and not to every string of the same d)
//   absorb(label, data):  st <- SHA256(st || label || data)
//   challenge(label, i):  wide = SHA256(st || label || le32 i || 0x00) || SHA256(st || label || le32 i || 0x01)   (64 bytes, little-endian integer)
//                         c = wide mod r, and 1 in place of 0 (evaluation points must be invertible)
//   circuit digest = SHA256("sonic-hip/circuit/v1" || le64 n || le64 Q || wL || wR || wO || cs)    (canonical bytes, row-major)
//
//   absorb("R", R)                                      -> y   = challenge("y", 0)
//   absorb("T", T)                                      -> z   = challenge("z", 0)
//   absorb("open", a || Wa || b || Wb || Wt || s)       -> y_j = challenge("yj", j), z_j = challenge("zj", j)
//   absorb("hscS", [S_j || s_j || W_j]_j)               -> u   = challenge("u", 0)
//   absorb("hscW", C || [s'_j || W'_j || Q_j]_j)        -> v   = challenge("v", 0)
//
// The four blinders c_{n+1..n+4} (Protocol.hs:58) are the prover's secret randomness, not challenges: blinder i =
// wide-reduce(SHA256("sonic-hip/blinder/v2" || seed || circuit digest || srs id || witness digest || le32 i || 0/1)) for a caller-supplied
// 32-byte seed, witness digest = SHA256("sonic-hip/witness/v1" || aL || aR || aO) (canonical bytes).  Statement and witness are mixed in
// the manner of RFC 6979: with the seed alone, two proofs of different assignments under one seed would share their blinders and
// R_1 - R_2 would be an unblinded commitment to the difference of the witnesses.  (v1, round 3, had neither this nor the srs id.)
// The parity tests compare against an independent restatement of this definition with python's hashlib (test infrastructure).
//
// Witness digest v2 (sonic_prover_submit_fs / collect_fs, sonic_prove_batch_fs, sonic_prover_witness_digest_v2): the same blinder
// formula over a digest that the GPU computes from the resident assignment, a SHA-256 tree (witness_tree.hpp, witness.hip).  The blocking
// sonic_prover_prove_fs keeps v1.  Blinders are the prover's private randomness: no verifier sees which digest went into them.
//   B      = the canonical little-endian bytes of aL || aR || aO: 96 n bytes, 3n elements of 32 bytes
//   leaves   L = ceil(96 n / 1024);  leaf_i = SHA256(H_leaf(i) || B[1024 i : min(1024 (i+1), 96 n)])
//            H_leaf(i) = 64 bytes: "sonic-hip/witness-leaf/v2" zero-padded to 56 bytes, then le64 i
//   nodes    level 0 is the leaves; while a level has c > 1 digests the next one has ceil(c / 32) nodes,
//            node_j = SHA256(H_node(level, j) || the digests 32 j .. min(32 (j+1), c) - 1 of the level below)
//            H_node(level, j) = 64 bytes: "sonic-hip/witness-node/v2" zero-padded to 48 bytes, then le64 level (1 for the first level of
//            nodes), then le64 j
//   root   = the single digest left (leaf_0 when L = 1)
//   witness digest v2 = SHA256("sonic-hip/witness/v2" || le64 n || root)
// The 64-byte headers keep every message block aligned to whole field elements: one block is two elements, sixteen 32-bit limbs
// byte-swapped.
//
// Weights digest v2 and circuit digest v2 (sonic_fs_weights_digest_v2_csr, sonic_fs_circuit_digest_v2, sonic_prover_weights_digest_v2,
// sonic_verifier_weights_digest_v2, a verifier handle of digest kind 2): circuit digest v1 hashes the 96 Q n dense bytes the weights stand
// for, which at Q ~ n (a compiled R1CS) is seconds of hashing; v2 hashes the ENTRIES, O(nnz), as a tree the GPU computes from the resident
// CSR (weights_tree.hpp, weights_digest.hip).  The framing is exactly that of witness digest v2: a 64-byte header, then 1 .. 32 items of
// 32 bytes, fan-out 32.
//   input    the validated stacked CSR of 3Q rows (csr.hpp: wL rows 0 .. Q-1, wR rows Q .. 2Q-1, wO rows 2Q .. 3Q-1), AS GIVEN: an explicit
//            zero value is an entry.  Two CSRs of the same matrix that differ in explicit zeros therefore have DIFFERENT digests (v1 does
//            not tell them apart): prover and verifier must hold the same CSR, not merely the same matrix.
//   items    entry k (0 <= k < nnz, CSR order) is two items: item 2k = le64 r || le64 c || 16 zero bytes, r in [0, 3Q) the stacked row,
//            c in [0, n) the column; item 2k + 1 = the 32 canonical little-endian bytes of val[k]
//   leaves   L = max(1, ceil(nnz / 16));  leaf_i = SHA256(H_leaf(i) || items 32 i .. min(32 (i+1), 2 nnz) - 1); nnz = 0: one leaf over
//            zero items
//   nodes    as in witness digest v2: while a level has c > 1 digests the next one has ceil(c / 32) nodes,
//            node_j = SHA256(H_node(level, j) || the digests 32 j .. min(32 (j+1), c) - 1 of the level below)
//   headers  H_leaf and H_node are the witness headers under the labels "sonic-hip/weights-leaf/v2" and "sonic-hip/weights-node/v2"
//            (25 bytes each, like the witness labels)
//   root   = the single digest left (leaf_0 when L = 1)
//   weights digest v2 = SHA256("sonic-hip/weights/v2" || le64 n || le64 Q || le64 nnz || root)
//   circuit digest v2 = SHA256("sonic-hip/circuit/v2" || weights digest v2 || le64 Q || cs),   cs = Q x 32 canonical bytes
// so a statement's digest costs 32 Q bytes of hashing from the weights digest: the split that midstate / resume gives v1.  Every
// transcript, batch digest and aggregate takes the 32 bytes of a circuit or weights digest as they are, so v2 bytes go wherever v1 bytes
// went; a proof made under one kind is a rejected proof under the other.
#pragma once
#include <string>
#include "field.hpp"
#include "sha256.hpp"

namespace sonic {

// a - r on the plain 256-bit integers (a >= r)
inline Fr fs_minus_r(const Fr& a) {
  const Fr m = Fr::modulus();
  Fr o;
  uint64_t br = 0;
  for (int i = 0; i < 8; i++) { const uint64_t t = (uint64_t)a.l[i] - m.l[i] - br; o.l[i] = (uint32_t)t; br = (t >> 32) & 1; }
  return o;
}
// 64 little-endian bytes mod r -> canonical (standard-form) Fr
inline Fr fs_wide_reduce(const uint8_t w[64]) {
  Fr lo, hi;
  memcpy(lo.l, w, 32); memcpy(hi.l, w + 32, 32);
  // 2^256 < 3 r: at most two subtractions bring a 256-bit value below r
  for (int k = 0; k < 2; k++) { if (!fp_is_canonical(lo)) lo = fs_minus_r(lo); if (!fp_is_canonical(hi)) hi = fs_minus_r(hi); }
  // hi * 2^256 mod r is exactly the Montgomery encoding of hi
  return fp_add(lo, fp_to_mont(hi));
}

struct FsTranscript {
  uint8_t st[32];
  void init(int64_t n, int64_t Q, int64_t d, const uint8_t digest[32], const uint8_t srs_id[32], const char* label = "sonic-hip/fs/v2") {
    Sha256 h;
    h.update(label, strlen(label));
    le64(h, n); le64(h, Q); le64(h, d);
    h.update(digest, 32);
    h.update(srs_id, 32);
    h.finish(st);
  }
  void absorb(const char* label, const uint8_t* data, size_t len) {
    Sha256 h;
    h.update(st, 32); h.update(label, strlen(label)); h.update(data, len);
    h.finish(st);
  }
  void challenge(const char* label, uint32_t i, uint8_t out32[32]) const {
    uint8_t w[64];
    for (uint8_t half = 0; half < 2; half++) {
      Sha256 h;
      h.update(st, 32); h.update(label, strlen(label));
      const uint8_t idx[5] = {(uint8_t)i, (uint8_t)(i >> 8), (uint8_t)(i >> 16), (uint8_t)(i >> 24), half};
      h.update(idx, 5);
      h.finish(w + 32 * half);
    }
    Fr c = fs_wide_reduce(w);
    if (c.is_zero()) c.l[0] = 1;
    memcpy(out32, c.l, 32);
  }
  static void le64(Sha256& h, int64_t v) { uint8_t b[8]; for (int i = 0; i < 8; i++) b[i] = (uint8_t)((uint64_t)v >> (8 * i)); h.update(b, 8); }
};

// pts: g^x, g^{alpha x}, g^{1/x}, g^{alpha/x} as 4 x 96 canonical bytes
inline void fs_srs_id_of_points(int64_t d, const uint8_t pts[4 * 96], uint8_t out32[32]) {
  Sha256 h;
  h.update("sonic-hip/srs/v1", 16);
  FsTranscript::le64(h, d);
  h.update(pts, 4 * 96);
  h.finish(out32);
}

inline void fs_blinder(const uint8_t seed[32], const uint8_t digest[32], const uint8_t srs_id[32], const uint8_t witness_digest[32], uint32_t i,
                       uint8_t out32[32]) {
  uint8_t w[64];
  for (uint8_t half = 0; half < 2; half++) {
    Sha256 h;
    h.update("sonic-hip/blinder/v2", 20); h.update(seed, 32); h.update(digest, 32); h.update(srs_id, 32); h.update(witness_digest, 32);
    const uint8_t idx[5] = {(uint8_t)i, (uint8_t)(i >> 8), (uint8_t)(i >> 16), (uint8_t)(i >> 24), half};
    h.update(idx, 5);
    h.finish(w + 32 * half);
  }
  Fr c = fs_wide_reduce(w);
  memcpy(out32, c.l, 32);
}

// witness digest v2 from the root of the tree (above)
inline void fs_witness_digest_v2(int64_t n, const uint8_t root[32], uint8_t out32[32]) {
  Sha256 h;
  h.update("sonic-hip/witness/v2", 20);
  FsTranscript::le64(h, n);
  h.update(root, 32);
  h.finish(out32);
}

// weights digest v2 from the root of the tree over the CSR entries, and circuit digest v2 from it (above)
inline void fs_weights_digest_v2(int64_t n, int64_t Q, int64_t nnz, const uint8_t root[32], uint8_t out32[32]) {
  Sha256 h;
  h.update("sonic-hip/weights/v2", 20);
  FsTranscript::le64(h, n); FsTranscript::le64(h, Q); FsTranscript::le64(h, nnz);
  h.update(root, 32);
  h.finish(out32);
}
// 0 = done; 2 = cs[q] is not canonical (*bad_q = q): the codes of fs_circuit_digest_resume
inline int fs_circuit_digest_v2(const uint8_t weights_digest[32], int64_t Q, const uint8_t* cs, uint8_t out32[32], int64_t* bad_q = nullptr) {
  for (int64_t q = 0; q < Q; q++) {
    Fr k;
    memcpy(k.l, cs + 32 * q, 32);
    if (!fp_is_canonical(k)) { if (bad_q) *bad_q = q; return 2; }
  }
  Sha256 h;
  h.update("sonic-hip/circuit/v2", 20);
  h.update(weights_digest, 32);
  FsTranscript::le64(h, Q);
  h.update(cs, (size_t)(32 * Q));
  h.finish(out32);
  return 0;
}

// The challenges a proof determines, in transcript order y, z, y_1..y_Q, z_1..z_Q, u, v (each 32 bytes), from the canonical proof
// bytes (include/sonic_hip.h): what the verifier recomputes.
inline void fs_challenges_of_proof(int64_t n, int64_t Q, int64_t d, const uint8_t digest[32], const uint8_t srs_id[32], const uint8_t* proof,
                                   uint8_t* out) {
  FsTranscript t;
  t.init(n, Q, d, digest, srs_id);
  const uint8_t* R = proof, * T = proof + 96, * open = proof + 192;       // a Wa b Wb Wt s = 32 + 96 + 32 + 96 + 96 + 32 = 384 bytes
  const uint8_t* hscS = proof + 576, * hscW = hscS + Q * 224, * Qv = hscW + Q * 224, * Cc = Qv + 96;
  t.absorb("R", R, 96);
  t.challenge("y", 0, out);
  t.absorb("T", T, 96);
  t.challenge("z", 0, out + 32);
  t.absorb("open", open, 384);
  for (int64_t j = 0; j < Q; j++) { t.challenge("yj", (uint32_t)j, out + 32 * (2 + j)); t.challenge("zj", (uint32_t)j, out + 32 * (2 + Q + j)); }
  t.absorb("hscS", hscS, (size_t)Q * 224);
  t.challenge("u", 0, out + 32 * (2 + 2 * Q));
  std::string w(reinterpret_cast<const char*>(Cc), 96);
  w.append(reinterpret_cast<const char*>(hscW), (size_t)Q * 224);
  t.absorb("hscW", reinterpret_cast<const uint8_t*>(w.data()), w.size());
  t.challenge("v", 0, out + 32 * (3 + 2 * Q));
}

// ---- core proofs (include/sonic_hip.h, "Core proofs"): R, T, a, W_a, b, W_b, W_t, s and no signature -----------------------------------
// The transcript of a core proof, under a label of its own so that a core proof can never be replayed as the head of a full one (nor
// the head of a full one pass for a core proof): the same state machine,
//   st_0 = SHA256("sonic-hip/fs-core/v1" || le64 n || le64 Q || le64 d || circuit digest || srs id)
//   absorb("R", R) -> y = challenge("y", 0);   absorb("T", T) -> z = challenge("z", 0)
// and the same blinders (above, over witness digest v2).  The openings are not absorbed: nothing is drawn after them.
constexpr const char* FS_CORE_LABEL = "sonic-hip/fs-core/v1";
// y, z (64 bytes) from the 576 canonical bytes of a core proof: what the verifier recomputes
inline void fs_core_challenges_of_proof(int64_t n, int64_t Q, int64_t d, const uint8_t digest[32], const uint8_t srs_id[32], const uint8_t* proof, uint8_t* out_yz) {
  FsTranscript t;
  t.init(n, Q, d, digest, srs_id, FS_CORE_LABEL);
  t.absorb("R", proof, 96);
  t.challenge("y", 0, out_yz);
  t.absorb("T", proof + 96, 96);
  t.challenge("z", 0, out_yz + 32);
}
// The digest of a batch of core proofs (sonic_verifier_verify_core_batch), from which the randomizers are derived as for the other batches
// (check index 3k + i):
//   D = SHA-256("sonic-hip/batch-digest/core/v1" || le64 n || le64 Q || le64 d || circuit digest || srs id || le64 K ||
//               K x (576 proof bytes || y_k || z_k || cs_k))
inline void fs_core_batch_digest(int64_t n, int64_t Q, int64_t d, const uint8_t digest[32], const uint8_t srs_id[32], int64_t K, const uint8_t* proofs,
                                 const uint8_t* yz, const uint8_t* cs, uint8_t out[32]) {
  const size_t ksz = 32 * (size_t)Q;
  Sha256 h;
  h.update("sonic-hip/batch-digest/core/v1", 30);
  FsTranscript::le64(h, n); FsTranscript::le64(h, Q); FsTranscript::le64(h, d);
  h.update(digest, 32); h.update(srs_id, 32);
  FsTranscript::le64(h, K);
  for (int64_t k = 0; k < K; k++) { h.update(proofs + 576 * (size_t)k, 576); h.update(yz + 64 * (size_t)k, 64); h.update(cs + ksz * (size_t)k, ksz); }
  h.finish(out);
}

// ---- the circuit digest in two halves: one circuit, many statements ----------------------------------------------------------------
// The constants cs are the LAST bytes of the circuit digest, and they are what changes from statement to statement (the reference's
// cs = wL.aL + wR.aR + wO.aO, test/Test/Reference.hs:138); the weights are the program.  The midstate is the SHA-256 state after
// "sonic-hip/circuit/v1" || le64 n || le64 Q || wL || wR || wO, from which every statement's digest costs Q x 32 more bytes of hashing.
// Layout, FS_MIDSTATE_SIZE = 112 bytes, every integer little-endian, the same on every host:
//     0 ..  31   the chaining value: eight 32-bit words h0 .. h7
//    32 ..  95   the bytes of the block that is not full yet: (length mod 64) of them, then zeros
//    96 .. 103   length: the number of bytes hashed so far, 64 bits; = 36 + 96 Q n
//   104 .. 111   Q, 64 bits
// resume refuses a midstate whose fields disagree: Q < 1, a length that is not 36 + 96 Q n for an integer n >= 1, a non-zero byte behind
// the pending ones.  There is ONE code path: the whole digest (csr.hpp, circuit_digest) is midstate + resume.
constexpr size_t FS_MIDSTATE_SIZE = 112;
constexpr uint64_t FS_CIRCUIT_HEAD = 36;      // the label and the two le64

inline void fs_circuit_begin(Sha256& h, int64_t n, int64_t Q) {
  h.update("sonic-hip/circuit/v1", 20);
  FsTranscript::le64(h, n); FsTranscript::le64(h, Q);
}
inline void fs_circuit_absorb_dense(Sha256& h, int64_t n, int64_t Q, const uint8_t* wL, const uint8_t* wR, const uint8_t* wO) {
  h.update(wL, (size_t)(32 * Q * n)); h.update(wR, (size_t)(32 * Q * n)); h.update(wO, (size_t)(32 * Q * n));
}
// sparse rows are streamed in order as the dense bytes they stand for (32 zero bytes per absent entry); of a validated CSR (csr.hpp)
inline void fs_circuit_absorb_csr(Sha256& h, int64_t n, int64_t Q, const int64_t* row_ptr, const int64_t* col, const uint8_t* val) {
  static const uint8_t zeros[32 * 1024] = {0};
  auto gap = [&](int64_t cnt) {
    for (; cnt > 0; cnt -= 1024) h.update(zeros, 32 * (size_t)(cnt < 1024 ? cnt : 1024));
  };
  for (int64_t r = 0; r < 3 * Q; r++) {
    int64_t at = 0;
    for (int64_t k = row_ptr[r]; k < row_ptr[r + 1]; k++) {
      gap(col[k] - at);
      h.update(val + 32 * k, 32);
      at = col[k] + 1;
    }
    gap(n - at);
  }
}
inline void fs_midstate_save(const Sha256& h, int64_t Q, uint8_t out[FS_MIDSTATE_SIZE]) {
  uint32_t chain[8];
  uint64_t len;
  h.get_state(chain, out + 32, &len);
  for (int i = 0; i < 8; i++) for (int b = 0; b < 4; b++) out[4 * i + b] = (uint8_t)(chain[i] >> (8 * b));
  for (int b = 0; b < 8; b++) { out[96 + b] = (uint8_t)(len >> (8 * b)); out[104 + b] = (uint8_t)((uint64_t)Q >> (8 * b)); }
}
// the Q a midstate holds (0 when its fields disagree)
inline int64_t fs_midstate_Q(const uint8_t mid[FS_MIDSTATE_SIZE]) {
  uint64_t len = 0, Q = 0;
  for (int b = 0; b < 8; b++) { len |= (uint64_t)mid[96 + b] << (8 * b); Q |= (uint64_t)mid[104 + b] << (8 * b); }
  if (Q < 1 || Q > (uint64_t)1 << 40 || len < FS_CIRCUIT_HEAD + 96 * Q || (len - FS_CIRCUIT_HEAD) % (96 * Q) != 0) return 0;
  for (size_t i = (size_t)(len % 64); i < 64; i++) if (mid[32 + i]) return 0;
  return (int64_t)Q;
}
// 0 = done; 1 = the midstate's fields disagree; 2 = cs[q] is not canonical (*bad_q = q)
inline int fs_circuit_digest_resume(const uint8_t mid[FS_MIDSTATE_SIZE], const uint8_t* cs, uint8_t out[32], int64_t* bad_q = nullptr, bool check_cs = true) {
  const int64_t Q = fs_midstate_Q(mid);
  if (Q < 1) return 1;
  for (int64_t q = 0; check_cs && q < Q; q++) {
    Fr k;
    memcpy(k.l, cs + 32 * q, 32);
    if (!fp_is_canonical(k)) { if (bad_q) *bad_q = q; return 2; }
  }
  uint32_t chain[8];
  uint64_t len = 0;
  for (int i = 0; i < 8; i++) chain[i] = (uint32_t)mid[4 * i] | (uint32_t)mid[4 * i + 1] << 8 | (uint32_t)mid[4 * i + 2] << 16 | (uint32_t)mid[4 * i + 3] << 24;
  for (int b = 0; b < 8; b++) len |= (uint64_t)mid[96 + b] << (8 * b);
  Sha256 h;
  h.put_state(chain, mid + 32, len);
  h.update(cs, (size_t)(32 * Q));
  h.finish(out);
  return 0;
}

// The digest of a batch whose proofs carry their OWN constants (sonic_verifier_verify_batch_cs; verify_batch.hip): v1 with cs_k behind
// proof k's challenges, under a label of its own, so that the randomizers bind the constants each proof is checked against.
//   D = SHA-256("sonic-hip/batch-digest/v2" || le64 n || le64 Q || le64 d || the handle's circuit digest || srs id || le64 K ||
//               K x (proof bytes || its 2 + 2Q challenges || cs_k))
inline void fs_batch_digest_v2(int64_t n, int64_t Q, int64_t d, const uint8_t digest[32], const uint8_t srs_id[32], int64_t K, const uint8_t* proofs,
                               size_t proof_bytes, const uint8_t* challenges, const uint8_t* cs, uint8_t out[32]) {
  const size_t csz = 32 * (size_t)(2 + 2 * Q), ksz = 32 * (size_t)Q;
  Sha256 h;
  h.update("sonic-hip/batch-digest/v2", 25);
  FsTranscript::le64(h, n); FsTranscript::le64(h, Q); FsTranscript::le64(h, d);
  h.update(digest, 32); h.update(srs_id, 32);
  FsTranscript::le64(h, K);
  for (int64_t k = 0; k < K; k++) { h.update(proofs + proof_bytes * (size_t)k, proof_bytes); h.update(challenges + csz * (size_t)k, csz); h.update(cs + ksz * (size_t)k, ksz); }
  h.finish(out);
}

// ---- helped verification (include/sonic_hip.h, "Helped verification"): one aggregate signature over the (y_k, z_k) of K core proofs ----
// s(X, Y) depends on the gate weights only, and one circuit serves many statements with their own cs_k, so the aggregate's transcript
// binds a digest of the weights, not the circuit digest (which ends in cs):
//   weights digest = SHA256("sonic-hip/weights/v1" || the FS_MIDSTATE_SIZE bytes of the circuit's midstate, above)
// An aggregate is an HscProof with m = K in the layout every HscProof has ([S_j, s_j, W_j]_j, [s'_j, W'_j, Q_j]_j, Q_v, C, u, v), whose
// u and v are NOT the helper's to choose:
//   st_0 = SHA256("sonic-hip/fs-agg/v1" || le64 n || le64 Q || le64 d || weights digest || srs id)
//   absorb("pairs", le64 K || K x (y_k || z_k))
//   absorb("hscS", [S_j || s_j || W_j]_j)          -> u = challenge("u", 0)
//   absorb("hscW", C || [s'_j || W'_j || Q_j]_j)   -> v = challenge("v", 0)
// u follows every S_j, s_j, W_j: S_j is checked against C at the point u, so a helper that knew u before it committed S_j could commit
// to a polynomial that agrees with s(X, y_j) at u only.  v follows C and every s'_j, W'_j, Q_j for the same reason one variable on:
// C is checked against s(u, v), which the verifier evaluates itself, at the point v.
constexpr const char* FS_AGG_LABEL = "sonic-hip/fs-agg/v1";
inline void fs_weights_digest(const uint8_t mid[FS_MIDSTATE_SIZE], uint8_t out[32]) {
  Sha256 h;
  h.update("sonic-hip/weights/v1", 20);
  h.update(mid, FS_MIDSTATE_SIZE);
  h.finish(out);
}
// where the parts of an aggregate for K pairs lie
struct AggLayout {
  int64_t K;
  size_t hscS() const { return 0; }
  size_t hscW() const { return 224 * (size_t)K; }
  size_t Qv() const { return 448 * (size_t)K; }
  size_t C() const { return Qv() + 96; }
  size_t u() const { return Qv() + 192; }
  size_t v() const { return Qv() + 224; }
  size_t bytes() const { return Qv() + 256; }
};
// the transcript in the three steps the helper walks it in (aggregate.hip); fs_aggregate_challenges is the three in a row
inline void fs_agg_begin(FsTranscript& t, int64_t n, int64_t Q, int64_t d, const uint8_t weights_digest[32], const uint8_t srs_id[32], int64_t K, const uint8_t* yz) {
  t.init(n, Q, d, weights_digest, srs_id, FS_AGG_LABEL);
  std::string w(8, '\0');
  for (int i = 0; i < 8; i++) w[(size_t)i] = (char)(uint8_t)((uint64_t)K >> (8 * i));
  w.append(reinterpret_cast<const char*>(yz), 64 * (size_t)K);
  t.absorb("pairs", reinterpret_cast<const uint8_t*>(w.data()), w.size());
}
inline void fs_agg_u(FsTranscript& t, int64_t K, const uint8_t* hscS, uint8_t out_u[32]) {
  t.absorb("hscS", hscS, 224 * (size_t)K);
  t.challenge("u", 0, out_u);
}
inline void fs_agg_v(FsTranscript& t, int64_t K, const uint8_t* Cc, const uint8_t* hscW, uint8_t out_v[32]) {
  std::string w(reinterpret_cast<const char*>(Cc), 96);
  w.append(reinterpret_cast<const char*>(hscW), 224 * (size_t)K);
  t.absorb("hscW", reinterpret_cast<const uint8_t*>(w.data()), w.size());
  t.challenge("v", 0, out_v);
}
// u || v (64 bytes) that the bytes of an aggregate determine: what the verifier recomputes and compares with the aggregate's own
inline void fs_aggregate_challenges(int64_t n, int64_t Q, int64_t d, const uint8_t weights_digest[32], const uint8_t srs_id[32], int64_t K, const uint8_t* yz,
                                    const uint8_t* aggregate, uint8_t out_uv[64]) {
  const AggLayout A{K};
  FsTranscript t;
  fs_agg_begin(t, n, Q, d, weights_digest, srs_id, K, yz);
  fs_agg_u(t, K, aggregate + A.hscS(), out_uv);
  fs_agg_v(t, K, aggregate + A.C(), aggregate + A.hscW(), out_uv + 32);
}
// The digest of a helped batch, from which its randomizers are derived as for the other batches (check index 3k + i for the heads,
// 3K + the position in hsc_checks' order for the signature):
//   D = SHA-256("sonic-hip/batch-digest/helped/v1" || le64 n || le64 Q || le64 d || weights digest || srs id || le64 K ||
//               K x (576 proof bytes || y_k || z_k || cs_k) || aggregate bytes)
inline void fs_core_helped_digest(int64_t n, int64_t Q, int64_t d, const uint8_t weights_digest[32], const uint8_t srs_id[32], int64_t K, const uint8_t* proofs,
                                  const uint8_t* yz, const uint8_t* cs, const uint8_t* aggregate, uint8_t out[32]) {
  const size_t ksz = 32 * (size_t)Q;
  Sha256 h;
  h.update("sonic-hip/batch-digest/helped/v1", 32);
  FsTranscript::le64(h, n); FsTranscript::le64(h, Q); FsTranscript::le64(h, d);
  h.update(weights_digest, 32); h.update(srs_id, 32);
  FsTranscript::le64(h, K);
  for (int64_t k = 0; k < K; k++) { h.update(proofs + 576 * (size_t)k, 576); h.update(yz + 64 * (size_t)k, 64); h.update(cs + ksz * (size_t)k, ksz); }
  h.update(aggregate, AggLayout{K}.bytes());
  h.finish(out);
}

}  // namespace sonic
