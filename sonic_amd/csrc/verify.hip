// The verifier side of the reference's API, on the host CPU: pcV (src/Sonic/CommitmentScheme.hs:51-68),
// hscVerify (src/Sonic/Signature.hs:74-90) and verify (src/Sonic/Protocol.hs:111-130).
//
// This is outside the accelerated hot path: (4+3Q) x 3 pairings and O(nQ) field work per
// proof, independent of the MSM sizes, so it runs on the host with the same limb headers the kernels use.
// The three G2 elements it needs come from the GPU-generated SRS (sonic_srs_get_g2_points).
//
// Pairing: only equalities of pairing products are tested (eA <> eB == eC), so any bilinear non-degenerate
// pairing on (G1, G2) accepts exactly the same proofs as pairing-1.0.0's.  Used here (pairing.hpp): the ate Miller loop over
// |x| = 0xd201000000010000 with the running point on the twist and sparse lines in Fq12 = Fq2[w]/(w^6 - (1+u)) as a
// 2-3-2 tower, one shared final exponentiation 3 (q^12 - 1)/r per check: ~6 ms per pcV on one host core (the plain
// polynomial-basis pairing of rounds 1-2, now tests/pairing_plain.hpp, took 170 ms).
#include <string.h>
#include <algorithm>
#include <system_error>
#include <thread>
#include <vector>
#include "verify_host.hpp"

namespace sonic {
namespace {

// (decoding, the G2 elements, the pcV equation, the list of a proof's checks and s(u, v): verify_host.hpp, shared with the batched verifier)
int pc_v(const sonic_srs* srs, const VerifierKey& vk, int64_t maxm, const G1Affine& F, const Fr& z_m, const Fr& v_m, const G1Affine& W, bool& ok) {
  G2Affine hxi;
  int rc = pc_v_element(srs, maxm, hxi);
  if (rc) return rc;
  ok = pc_v_equation(vk, hxi, F, z_m, v_m, W);
  return SONIC_OK;
}

// all checks of a verifier: elements first (one per distinct max), equations on up to 16 host threads
int run_checks(const sonic_srs* srs, const VerifierKey& vk, const std::vector<PcvCheck>& checks, bool& all) {
  std::vector<int64_t> maxs;
  std::vector<G2Affine> elems;
  std::vector<int> which(checks.size());
  for (size_t i = 0; i < checks.size(); i++) {
    size_t k = 0;
    while (k < maxs.size() && maxs[k] != checks[i].maxm) k++;
    if (k == maxs.size()) {
      G2Affine h;
      int rc = pc_v_element(srs, checks[i].maxm, h);
      if (rc) return rc;
      maxs.push_back(checks[i].maxm); elems.push_back(h);
    }
    which[i] = (int)k;
  }
  std::vector<char> ok(checks.size(), 0);
  const int nt = (int)std::min<size_t>(checks.size(), 16);
  auto work = [&](int w, int stride) {
    for (size_t i = w; i < checks.size(); i += stride)
      ok[i] = pc_v_equation(vk, elems[which[i]], checks[i].F, checks[i].z, checks[i].val, checks[i].W) ? 1 : 0;
  };
  ThreadGroup th;
  int started = 0;
  try {
    for (; started < nt; started++) th.emplace_back(work, started, nt);
  } catch (const std::system_error&) {}        // thread limit of the host process: the calling thread takes the rest
  for (int w = started; w < nt; w++) work(w, nt);
  for (auto& t : th) t.join();
  for (char c : ok) all = all && c;
  return SONIC_OK;
}

// a list of checks (verify_host.hpp: proof_checks, hsc_checks), run
int checks_accept(const sonic_srs* srs, const VerifierKey& vk, const std::vector<PcvCheck>& checks, int* accepted) {
  bool all = true;
  int rc = run_checks(srs, vk, checks, all);
  if (rc) return rc;
  *accepted = all ? 1 : 0;
  return SONIC_OK;
}
// the end of hscVerify once s(u,v) is known: its 3m + 1 pcV checks (Signature.hs:82-89)
int hsc_accepts(const sonic_srs* srs, const VerifierKey& vk, const HscProofView& h, const Fr& sv, int* accepted) {
  std::vector<PcvCheck> checks;
  hsc_checks(srs_d(srs), h, sv, checks);
  return checks_accept(srs, vk, checks, accepted);
}

// verify srs circuit proof y z yzs  (Protocol.hs:111-130) for a validated circuit in either form; yzs = Q pairs (y_j, z_j), 64 bytes each
int verify_circuit(const sonic_srs* srs, const CircuitView& c, const uint8_t* proof, const uint8_t y[32], const uint8_t z[32], const uint8_t* yzs, int* accepted) {
  ProofViewT<G1Affine> pv;
  Fr ym, zm, t, sv;
  if (!parse_proof(proof, c.Q, y, z, yzs, pv, ym, zm, load_g1)) { set_error("verify: non-canonical field element, or point off the curve or outside the order-r subgroup"); return SONIC_ERR_BAD_ENCODING; }
  if (!proof_t(c, pv, ym, t)) return SONIC_ERR_BAD_ENCODING;         // k(y), Protocol.hs:120
  VerifierKey vk;
  int rc = load_verifier_key(srs, vk);
  if (!rc) rc = s_of_uv(c, pv.h.u, pv.h.v, sv);                      // hscVerify, Signature.hs:74-90
  if (rc) return rc;
  return checks_accept(srs, vk, proof_checks(c.n, srs_d(srs), pv, ym, zm, t, sv), accepted);
}

}  // namespace
}  // namespace sonic

using namespace sonic;

extern "C" {

int sonic_pc_v(const sonic_srs_t* srs, int64_t max, const uint8_t commitment[96], const uint8_t z[32], const uint8_t v[32],
               const uint8_t w[96], int* accepted) {
  API_HOST_BEGIN
    if (!srs || !commitment || !z || !v || !w || !accepted) return SONIC_ERR_INVALID_ARG;
    G1Affine F, W; Fr zm, vm;
    if (!load_g1(commitment, F) || !load_g1(w, W) || !load_fr(z, zm) || !load_fr(v, vm)) { set_error("pcV: bad encoding"); return SONIC_ERR_BAD_ENCODING; }
    VerifierKey vk;
    int rc = load_verifier_key(srs, vk);
    if (rc) return rc;
    bool ok = false;
    rc = pc_v(srs, vk, max, F, zm, vm, W, ok);
    *accepted = ok ? 1 : 0;
    return rc;
  API_CATCH
}

}  // extern "C"

// the entry points that take a circuit, in either form: an argument check, a view, one implementation
static int verify_entry(const char* who, const sonic_srs_t* srs, const CircuitView& c, const uint8_t* proof, const uint8_t y[32], const uint8_t z[32],
                        const uint8_t* yzs, int* accepted) {
  API_HOST_BEGIN
    if (!srs || !c.cs || !proof || !y || !z || !yzs || !accepted) { set_error("%s: bad argument", who); return SONIC_ERR_INVALID_ARG; }
    *accepted = 0;
    int rc = circuit_validate(who, c);
    if (rc) return rc;
    return verify_circuit(srs, c, proof, y, z, yzs, accepted);
  API_CATCH
}

extern "C" {

// verify srs circuit proof y z yzs  (Protocol.hs:111-130); yzs = Q pairs (y_j, z_j), 64 bytes each
int sonic_verify(const sonic_srs_t* srs, int64_t n, int64_t Q, const uint8_t* wL, const uint8_t* wR, const uint8_t* wO,
                 const uint8_t* cs, const uint8_t* proof, const uint8_t y[32], const uint8_t z[32], const uint8_t* yzs, int* accepted) {
  return verify_entry("sonic_verify", srs, dense_view(n, Q, wL, wR, wO, cs), proof, y, z, yzs, accepted);
}

// the same with sparse gate weights (csr.hpp): s(u, v) in O(nnz + n) instead of O(Q n)
int sonic_verify_csr(const sonic_srs_t* srs, int64_t n, int64_t Q, const int64_t* row_ptr, const int64_t* col, const uint8_t* val,
                     const uint8_t* cs, const uint8_t* proof, const uint8_t y[32], const uint8_t z[32], const uint8_t* yzs, int* accepted) {
  return verify_entry("sonic_verify_csr", srs, csr_view(n, Q, row_ptr, col, val, cs), proof, y, z, yzs, accepted);
}

// what ties a Fiat-Shamir transcript to ONE reference string (fs.hpp): four G1 elements that determine x and alpha
// (constant for a handle: computed on first use -- four point fetches from the device -- and cached in the handle, srs_cached_id)
static int make_srs_id(const sonic_srs* srs, uint8_t out[32]) {
  API_HOST_BEGIN
    uint8_t pts[4 * 96];
    int rc = sonic_srs_get_points(srs, 0, 1, 1, pts);                 // g^x            gPositiveX[1]
    if (!rc) rc = sonic_srs_get_points(srs, 1, 1, 1, pts + 96);       // g^{alpha x}    gPositiveAlphaX[0]
    if (!rc) rc = sonic_srs_get_points(srs, 0, -1, 1, pts + 192);     // g^{1/x}        gNegativeX[0]
    if (!rc) rc = sonic_srs_get_points(srs, 1, -1, 1, pts + 288);     // g^{alpha/x}    gNegativeAlphaX[0]
    if (rc) return rc;
    fs_srs_id_of_points(srs_d(srs), pts, out);
    return SONIC_OK;
  API_CATCH
}
int sonic_fs_srs_id(const sonic_srs_t* srs, uint8_t out[32]) {
  if (!srs || !out) return SONIC_ERR_INVALID_ARG;
  return srs_cached_id(srs, &make_srs_id, out);
}

// srsPairing = pairing gen (hPositiveAlphaX !! 0) = e(g, h^alpha) (SRS.hs:21,42): the reduced ate pairing
// f_{x, Q}(P)^((q^12 - 1)/r) with the (negative) curve parameter x.  The verifier's own pairing (pairing.hpp) computes
// v = f_{|x|, Q}(P)^(3 (q^12 - 1)/r) -- any non-degenerate bilinear map serves its equality tests -- so the record field is derived
// from it exactly: v lies in the order-r subgroup, v^(1/3 mod r) = f_{|x|,Q}(P)^((q^12-1)/r), and the sign of x turns that into its
// inverse, which in the cyclotomic subgroup is the conjugate.  (Which representative pairing-1.0.0 itself returns is [dep, unverified]:
// the package is not in the reference tree; this is the textbook definition.)
int sonic_srs_pairing(const sonic_srs_t* srs, uint8_t out[576]) {
  API_HOST_BEGIN
    if (!srs || !out) return SONIC_ERR_INVALID_ARG;
    G2Affine ha;
    int rc = fetch_g2(srs, 1, 0, ha);                                  // hPositiveAlphaX[0] = h^alpha
    if (rc) return rc;
    using namespace pairing;
    const F12 v = final_exponentiation(miller_loop(g1_gen_host(), ha));
    // 1/3 mod r as an integer: Fr arithmetic of the limb headers
    Fr three = fp_add(fp_add(Fr::one(), Fr::one()), Fr::one());
    const Fr e = fp_from_mont(fp_inv(three));
    F12 acc = F12::one();
    for (int i = 255; i >= 0; i--) {
      acc = f12_sqr(acc);
      if ((e.l[i >> 5] >> (i & 31)) & 1) acc = f12_mul(acc, v);
    }
    const F12 res = f12_conj(acc);
    const F6* halves[2] = {&res.c0, &res.c1};
    uint8_t* o = out;
    for (int i = 0; i < 2; i++) {
      const Fq2* cs[3] = {&halves[i]->a0, &halves[i]->a1, &halves[i]->a2};
      for (int j = 0; j < 3; j++) {
        const Fq c0 = fp_from_mont(cs[j]->c0), c1 = fp_from_mont(cs[j]->c1);
        memcpy(o, c0.l, 48); memcpy(o + 48, c1.l, 48); o += 96;
      }
    }
    return SONIC_OK;
  API_CATCH
}

}  // extern "C"

// verify for a proof made by sonic_prover_prove_fs: the challenges y, z, (y_j, z_j) are not handed over (RndOracle) but recomputed from
// the statement and the proof (fs.hpp), and the proof's u, v must be the ones its own transcript yields
static int verify_fs_entry(const char* who, const sonic_srs_t* srs, const CircuitView& c, const uint8_t* proof, int* accepted) {
  API_HOST_BEGIN
    if (!srs || !c.cs || !proof || !accepted) { set_error("%s: bad argument", who); return SONIC_ERR_INVALID_ARG; }
    *accepted = 0;
    int rc = circuit_validate(who, c);
    if (rc) return rc;
    const int64_t n = c.n, Q = c.Q;
    uint8_t digest[32], srs_id[32];
    circuit_digest(c, digest);
    rc = sonic_fs_srs_id(srs, srs_id);
    if (rc) return rc;
    std::vector<uint8_t> ch(32 * (size_t)(4 + 2 * Q));
    fs_challenges_of_proof(n, Q, srs_d(srs), digest, srs_id, proof, ch.data());
    const uint8_t* uv = proof + sonic_proof_size(Q) - 64;
    if (memcmp(uv, &ch[32 * (2 + 2 * Q)], 64) != 0) return SONIC_OK;          // u, v are not this transcript's: rejected
    std::vector<uint8_t> yzs(64 * (size_t)Q);
    for (int64_t j = 0; j < Q; j++) { memcpy(&yzs[64 * j], &ch[32 * (2 + j)], 32); memcpy(&yzs[64 * j + 32], &ch[32 * (2 + Q + j)], 32); }
    return verify_circuit(srs, c, proof, &ch[0], &ch[32], yzs.data(), accepted);
  API_CATCH
}

extern "C" {

int sonic_verify_fs(const sonic_srs_t* srs, int64_t n, int64_t Q, const uint8_t* wL, const uint8_t* wR, const uint8_t* wO,
                    const uint8_t* cs, const uint8_t* proof, int* accepted) {
  return verify_fs_entry("sonic_verify_fs", srs, dense_view(n, Q, wL, wR, wO, cs), proof, accepted);
}
int sonic_verify_fs_csr(const sonic_srs_t* srs, int64_t n, int64_t Q, const int64_t* row_ptr, const int64_t* col, const uint8_t* val,
                        const uint8_t* cs, const uint8_t* proof, int* accepted) {
  return verify_fs_entry("sonic_verify_fs_csr", srs, csr_view(n, Q, row_ptr, col, val, cs), proof, accepted);
}

// sonic_fs_circuit_digest (prove.hip) from the sparse rows: the same 32 bytes (circuit_digest, csr.hpp)
int sonic_fs_circuit_digest_csr(int64_t n, int64_t Q, const int64_t* row_ptr, const int64_t* col, const uint8_t* val, const uint8_t* cs, uint8_t out[32]) {
  return circuit_digest_checked("sonic_fs_circuit_digest_csr", csr_view(n, Q, row_ptr, col, val, cs), out);
}

// hscVerify :: SRS -> BiVLaurent Fr -> [(Fr, Fr)] -> HscProof -> Bool (Signature.hs:74-90) for the s(X,Y) of a circuit;
// hsc = the bytes sonic_prover_hsc_prove wrote (m pairs)
int sonic_hsc_verify(const sonic_srs_t* srs, int64_t n, int64_t Q, const uint8_t* wL, const uint8_t* wR, const uint8_t* wO,
                     int64_t m, const uint8_t* yzs, const uint8_t* hsc, int* accepted) {
  API_HOST_BEGIN
    if (!srs || n < 1 || Q < 1 || !wL || !wR || !wO || m < 0 || (m > 0 && !yzs) || !hsc || !accepted) return SONIC_ERR_INVALID_ARG;
    *accepted = 0;
    HscProofView h;
    Fr sv;
    if (!parse_hsc(hsc, m, yzs, h)) { set_error("hscVerify: non-canonical field element, or point off the curve or outside the order-r subgroup"); return SONIC_ERR_BAD_ENCODING; }
    VerifierKey vk;
    int rc = load_verifier_key(srs, vk);
    if (!rc) rc = s_of_uv(dense_view(n, Q, wL, wR, wO, nullptr), h.u, h.v, sv);
    if (rc) return rc;
    return hsc_accepts(srs, vk, h, sv, accepted);
  API_CATCH
}


// hscVerify :: SRS -> BiVLaurent Fr -> [(Fr, Fr)] -> HscProof -> Bool (Signature.hs:74-90) for any sparse bivariate Laurent polynomial
// (the counterpart of sonic_hsc_prove_poly): s(u,v) = eval (evalY v sXY) u on the host, then the 3m + 1 pcV checks
int sonic_hsc_verify_poly(const sonic_srs_t* srs, int64_t n_terms, const int64_t* x_exps, const int64_t* y_exps, const uint8_t* coeffs,
                          int64_t m, const uint8_t* yzs, const uint8_t* hsc, int* accepted) {
  API_HOST_BEGIN
    if (!srs || n_terms < 0 || (n_terms > 0 && (!x_exps || !y_exps || !coeffs)) || m < 0 || (m > 0 && !yzs) || !hsc || !accepted) return SONIC_ERR_INVALID_ARG;
    *accepted = 0;
    HscProofView h;
    if (!parse_hsc(hsc, m, yzs, h)) { set_error("hscVerify: non-canonical field element, or point off the curve or outside the order-r subgroup"); return SONIC_ERR_BAD_ENCODING; }
    const Fr &u = h.u, &v = h.v;
    Fr sv = Fr::zero();
    const Fr uinv = u.is_zero() ? u : fp_inv(u), vinv = v.is_zero() ? v : fp_inv(v);
    for (int64_t i = 0; i < n_terms; i++) {
      Fr c;
      if (!load_fr(coeffs + 32 * i, c)) { set_error("hscVerify: non-canonical coefficient"); return SONIC_ERR_BAD_ENCODING; }
      const int64_t ex = x_exps[i], ey = y_exps[i];
      if ((ex < 0 && u.is_zero()) || (ey < 0 && v.is_zero())) { set_error("hscVerify: u or v is zero and s(X,Y) has negative powers"); return SONIC_ERR_INEXACT_DIVISION; }
      const Fr px = fr_pow(ex >= 0 ? u : uinv, (uint64_t)(ex >= 0 ? ex : -ex)), py = fr_pow(ey >= 0 ? v : vinv, (uint64_t)(ey >= 0 ? ey : -ey));
      sv = fp_add(sv, fp_mul(c, fp_mul(px, py)));
    }
    VerifierKey vk;
    int rc = load_verifier_key(srs, vk);
    if (rc) return rc;
    return hsc_accepts(srs, vk, h, sv, accepted);
  API_CATCH
}

}  // extern "C"

// ---- core proofs (include/sonic_hip.h, "Core proofs") ------------------------------------------------------------------------------
// The unhelped verifier: no signature vouches for the proof's s, so the verifier evaluates s(z, y) itself -- O(nnz + n) field work
// (s_of_uv) -- and a proof whose s differs is rejected before any pairing; then the three pcV equations of the head (core_checks).
static int verify_core_circuit(const sonic_srs* srs, const CircuitView& c, const uint8_t* proof, const uint8_t y[32], const uint8_t z[32], int* accepted) {
  ProofViewT<G1Affine> pv;
  Fr ym, zm, t, sv;
  if (!parse_core_proof(proof, y, z, pv, ym, zm, load_g1)) { set_error("verify_core: non-canonical field element, or point off the curve or outside the order-r subgroup"); return SONIC_ERR_BAD_ENCODING; }
  if (ym.is_zero() || zm.is_zero()) { set_error("verify_core: y or z is zero"); return SONIC_ERR_INEXACT_DIVISION; }
  if (!proof_t(c, pv, ym, t)) return SONIC_ERR_BAD_ENCODING;         // k(y), Protocol.hs:120
  VerifierKey vk;
  int rc = load_verifier_key(srs, vk);
  if (!rc) rc = s_of_uv(c, zm, ym, sv);                              // s(X, Y) at X = z, Y = y
  if (rc) return rc;
  if (!(sv == pv.s)) return SONIC_OK;                                // the proof's s is not s(z, y): rejected
  return checks_accept(srs, vk, core_checks(c.n, srs_d(srs), pv, ym, zm, t), accepted);
}

static int verify_core_entry(const char* who, const sonic_srs_t* srs, const CircuitView& c, const uint8_t* proof, const uint8_t* y, const uint8_t* z, bool fs, int* accepted) {
  API_HOST_BEGIN
    if (!srs || !c.cs || !proof || (!fs && (!y || !z)) || !accepted) { set_error("%s: bad argument", who); return SONIC_ERR_INVALID_ARG; }
    *accepted = 0;
    int rc = circuit_validate(who, c);
    if (rc) return rc;
    uint8_t yz[64];
    if (fs) {      // y, z are the ones the proof's own transcript yields (fs.hpp, "core proofs")
      uint8_t digest[32], srs_id[32];
      circuit_digest(c, digest);
      rc = sonic_fs_srs_id(srs, srs_id);
      if (rc) return rc;
      fs_core_challenges_of_proof(c.n, c.Q, srs_d(srs), digest, srs_id, proof, yz);
      y = yz; z = yz + 32;
    }
    return verify_core_circuit(srs, c, proof, y, z, accepted);
  API_CATCH
}

extern "C" {

int sonic_verify_core(const sonic_srs_t* srs, int64_t n, int64_t Q, const uint8_t* wL, const uint8_t* wR, const uint8_t* wO, const uint8_t* cs,
                      const uint8_t* proof, const uint8_t y[32], const uint8_t z[32], int* accepted) {
  return verify_core_entry("sonic_verify_core", srs, dense_view(n, Q, wL, wR, wO, cs), proof, y, z, false, accepted);
}
int sonic_verify_core_csr(const sonic_srs_t* srs, int64_t n, int64_t Q, const int64_t* row_ptr, const int64_t* col, const uint8_t* val, const uint8_t* cs,
                          const uint8_t* proof, const uint8_t y[32], const uint8_t z[32], int* accepted) {
  return verify_core_entry("sonic_verify_core_csr", srs, csr_view(n, Q, row_ptr, col, val, cs), proof, y, z, false, accepted);
}
int sonic_verify_core_fs(const sonic_srs_t* srs, int64_t n, int64_t Q, const uint8_t* wL, const uint8_t* wR, const uint8_t* wO, const uint8_t* cs,
                         const uint8_t* proof, int* accepted) {
  return verify_core_entry("sonic_verify_core_fs", srs, dense_view(n, Q, wL, wR, wO, cs), proof, nullptr, nullptr, true, accepted);
}
int sonic_verify_core_fs_csr(const sonic_srs_t* srs, int64_t n, int64_t Q, const int64_t* row_ptr, const int64_t* col, const uint8_t* val, const uint8_t* cs,
                             const uint8_t* proof, int* accepted) {
  return verify_core_entry("sonic_verify_core_fs_csr", srs, csr_view(n, Q, row_ptr, col, val, cs), proof, nullptr, nullptr, true, accepted);
}

}  // extern "C"
