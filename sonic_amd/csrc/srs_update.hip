// The updatable half of the SRS behind the C ABI (include/sonic_hip.h, "Updatable SRS"): the structure check of a whole string, a
// contribution that re-randomises it into a new handle, and the verifier of a contribution.  The kernels: k_g1_scale_each and
// k_srs_check_rho (srs.hip), k_g2_scale_each and k_g2_sum (srs_g2.hip); the proof of a contribution: srs_update.hpp.  The G1 sums of the
// check are the library's MSMs over the handle; the pairings stay on the host.
#include <string.h>
#include <memory>
#include <stdlib.h>
#include "srs_handle.hpp"
#include "g2.hpp"
#include "msm_g2.hpp"
#include "srs_update.hpp"

using namespace sonic;

namespace {

// what a contribution keeps on the host while it runs: the shares, the inverse, the nonces.  Wiped when the call leaves, whichever way.
struct Secrets {
  uint8_t x1[32], a1[32], kx[32], ka[32];
  Fr x, xinv, alpha;          // Montgomery
  ~Secrets() { srs_update::wipe(this, sizeof *this); }
};

void load_g1_mont(const uint8_t* b, G1Affine& p) {          // points the library itself wrote: canonical bytes, zeros for infinity
  memcpy(p.x.l, b, 48); memcpy(p.y.l, b + 48, 48);
  if (!p.is_inf()) { p.x = fp_to_mont(p.x); p.y = fp_to_mont(p.y); }
}
void load_g2_mont(const uint8_t* b, G2Affine& p) {
  memcpy(p.x.c0.l, b, 48); memcpy(p.x.c1.l, b + 48, 48); memcpy(p.y.c0.l, b + 96, 48); memcpy(p.y.c1.l, b + 144, 48);
  if (!p.is_inf()) { p.x.c0 = fp_to_mont(p.x.c0); p.x.c1 = fp_to_mont(p.x.c1); p.y.c0 = fp_to_mont(p.y.c0); p.y.c1 = fp_to_mont(p.y.c1); }
}
int fetch_g1(const sonic_srs_t* s, int basis, int64_t e, G1Affine& p) {
  uint8_t b[96];
  const int rc = sonic_srs_get_points(s, basis, e, 1, b);
  if (!rc) load_g1_mont(b, p);
  return rc;
}
int fetch_g2(const sonic_srs_t* s, int basis, int64_t e, G2Affine& p) {
  uint8_t b[192];
  const int rc = sonic_srs_get_g2_points(s, basis, e, 1, b);
  if (!rc) load_g2_mont(b, p);
  return rc;
}

// sum_{i < n} rho[i0 + i] * basis[e0 + i]: one MSM over the handle with its scalars resident (nothing to do for n = 0)
int msm_part(const sonic_srs_t* s, int basis, int64_t e0, const Fr* d_rho, int64_t i0, int64_t n, G1XYZZ& out) {
  out = G1XYZZ::inf();
  if (n <= 0) return SONIC_OK;
  uint8_t part[192];
  const int rc = sonic_msm_g1_srs_partial_dev(s, basis, e0, d_rho + i0, n, part);
  if (!rc) memcpy(&out, part, sizeof out);
  return rc;
}

}  // namespace

extern "C" {

int sonic_srs_check(const sonic_srs_t* srs, const uint8_t seed[32], int* failed) {
  API_BEGIN_ON(srs_device(srs))
  if (!srs || !failed) { set_error("sonic_srs_check: bad argument"); return SONIC_ERR_INVALID_ARG; }
  *failed = 0;
  if (srs->is_view()) { set_error("sonic_srs_check: a circuit-sized view is not a reference string (check the string it was made from)"); return SONIC_ERR_INVALID_ARG; }
  const int64_t d = srs->d, n = 2 * d + 1;
  uint8_t sd[32];
  DevBuf rho;
  uint8_t Bb[192], Cb[192];
  {
    std::lock_guard<std::mutex> g(call_mutex());
    hipStream_t st = default_stream();
    const int rc = srs_ensure_g2(srs, st, "sonic_srs_check");
    if (rc) return rc;
    // the string is fixed by now: the seed is drawn after it and need not bind it
    if (seed) memcpy(sd, seed, 32);
    else if (!srs_update::os_random(sd, 32)) { set_error("sonic_srs_check: the operating system gave no random bytes for the seed"); return SONIC_ERR_HIP; }
    rho.alloc(sizeof(Fr) * (size_t)n);
    srs_check_rho_enqueue(st, sd, (long)n, rho.as<Fr>());
    // B = sum_e rho_e H0[e], C = sum_e rho_e H1[e]: the G2 MSM over 129 bits (128-bit randomizers and the recoding's carry), or with
    // SONIC_G2_MSM=0, read per call, the walk over all 128 bits of every randomizer (for comparing the two in one process)
    const char* knob = getenv("SONIC_G2_MSM");
    if (knob && atoi(knob) == 0) {
      g2_weighted_sum(st, srs->h.as<G2Affine>(), rho.as<Fr>(), (long)n, Bb);
      g2_weighted_sum(st, srs->ha.as<G2Affine>(), rho.as<Fr>(), (long)n, Cb);
    } else {
      CallLease lease;          // (for its workspace: the chains run on the stream the randomizers were queued on)
      g2_msm_blocking(st, lease.ws(), srs->h.as<G2Affine>(), rho.as<Fr>(), (long)n, 129, true, Bb);
      g2_msm_blocking(st, lease.ws(), srs->ha.as<G2Affine>(), rho.as<Fr>(), (long)n, 129, true, Cb);
    }
  }
  // R0: the string stands over the fixed generators
  uint8_t b0[96], gb[96], h0[192], hb[192];
  int rc = sonic_srs_get_points(srs, 0, 0, 1, b0);
  if (!rc) rc = sonic_srs_get_g2_points(srs, 0, 0, 1, h0);
  if (rc) return rc;
  uint32_t w[48];
  const G1Affine g = srs_update::g1_gen();
  const G2Affine h = srs_update::g2_gen();
  g1_canonical_bytes_host(G1XYZZ::from_affine(g), gb);
  { const Fq a = fp_from_mont(h.x.c0), b = fp_from_mont(h.x.c1), c = fp_from_mont(h.y.c0), e = fp_from_mont(h.y.c1);
    for (int k = 0; k < 12; k++) { w[k] = a.l[k]; w[12 + k] = b.l[k]; w[24 + k] = c.l[k]; w[36 + k] = e.l[k]; } }
  memcpy(hb, w, 192);
  if (memcmp(b0, gb, 96) != 0 || memcmp(h0, hb, 192) != 0) *failed |= SONIC_SRS_CHECK_R0;
  // the G1 sums: exponents [-d, -1], 0, [1, d-1], d of basis 0 under their own randomizers; [-d+1, d] under those of [-d, d-1]; the two
  // halves of basis 1 around its empty slot, which no MSM touches
  const Fr* r = rho.as<Fr>();
  G1XYZZ lo, mid, hi, top, shifted, alo, ahi;
  if ((rc = msm_part(srs, 0, -d, r, 0, d, lo)) || (rc = msm_part(srs, 0, 0, r, d, 1, mid)) || (rc = msm_part(srs, 0, 1, r, d + 1, d - 1, hi)) ||
      (rc = msm_part(srs, 0, d, r, 2 * d, 1, top)) || (rc = msm_part(srs, 0, -d + 1, r, 0, 2 * d, shifted)) || (rc = msm_part(srs, 1, -d, r, 0, d, alo)) ||
      (rc = msm_part(srs, 1, 1, r, d + 1, d, ahi)))
    return rc;
  const G1XYZZ side = g1_add(lo, hi);
  const G1XYZZ sums[5] = {g1_add(side, mid), shifted, g1_add(alo, ahi), g1_add(side, top), g1_add(g1_add(side, mid), top)};
  G1Affine a[5];          // P, P+, A, A0, the sum over all of basis 0
  g1_batch_affine_host(sums, 5, a);
  G2Affine hx, halpha, B, Cc;
  if ((rc = fetch_g2(srs, 0, 1, hx)) || (rc = fetch_g2(srs, 1, 0, halpha))) return rc;
  load_g2_mont(Bb, B); load_g2_mont(Cb, Cc);
  using srs_update::pairs_equal;
  if (!pairs_equal(a[0], hx, a[1], h)) *failed |= SONIC_SRS_CHECK_R1;              // e(P, H0[1]) = e(P+, h)
  if (!pairs_equal(a[2], h, a[3], halpha)) *failed |= SONIC_SRS_CHECK_R2;          // e(A, h) = e(A0, H1[0])
  if (!pairs_equal(g, B, a[4], h)) *failed |= SONIC_SRS_CHECK_R3;                  // e(g, B) = e(sum, h)
  if (!pairs_equal(g, Cc, a[4], halpha)) *failed |= SONIC_SRS_CHECK_R4;            // e(g, C) = e(sum, H1[0])
  API_END
}

int sonic_srs_update(const sonic_srs_t* srs, const uint8_t x1[32], const uint8_t alpha1[32], const uint8_t seed[32], sonic_srs_t** out, uint8_t proof[448]) {
  API_BEGIN_ON(srs_device(srs))
  if (!srs || !x1 || !alpha1 || !out || !proof) { set_error("sonic_srs_update: bad argument"); return SONIC_ERR_INVALID_ARG; }
  if (srs->is_view()) { set_error("sonic_srs_update: a circuit-sized view is not a reference string (update the string and make the view from the result)"); return SONIC_ERR_INVALID_ARG; }
  if (!sonic_srs_has_g2(srs)) { set_error("sonic_srs_update: this SRS has no G2 half (built from G1 points only): a contribution updates both halves"); return SONIC_ERR_INVALID_ARG; }
  Secrets k;
  memcpy(k.x1, x1, 32); memcpy(k.a1, alpha1, 32);
  Fr xs, as;
  memcpy(xs.l, x1, 32); memcpy(as.l, alpha1, 32);
  struct WipeFr { Fr &a, &b; ~WipeFr() { srs_update::wipe(a.l, 32); srs_update::wipe(b.l, 32); } } wipe_std{xs, as};
  if (!fp_is_canonical(xs) || !fp_is_canonical(as)) { set_error("sonic_srs_update: a share is not < r"); return SONIC_ERR_BAD_ENCODING; }
  if (xs.is_zero() || as.is_zero()) { set_error("sonic_srs_update: a share is zero (the string it would give has no trapdoor to hide)"); return SONIC_ERR_INVALID_ARG; }
  k.x = fp_to_mont(xs); k.xinv = fp_inv(k.x); k.alpha = fp_to_mont(as);
  uint8_t old_id[32];
  int rc = sonic_fs_srs_id(srs, old_id);
  if (rc) return rc;
  if (seed) { srs_update::seeded_nonce(seed, k.x1, k.a1, old_id, 0, k.kx); srs_update::seeded_nonce(seed, k.x1, k.a1, old_id, 1, k.ka); }
  else {
    uint8_t w[128];
    if (!srs_update::os_random(w, 128)) { set_error("sonic_srs_update: the operating system gave no random bytes for the nonces"); return SONIC_ERR_HIP; }
    for (int i = 0; i < 2; i++) {
      Fr v = fs_wide_reduce(w + 64 * i);
      if (v.is_zero()) v.l[0] = 1;
      memcpy(i ? k.ka : k.kx, v.l, 32);
      srs_update::wipe(v.l, 32);
    }
    srs_update::wipe(w, sizeof w);
  }
  std::lock_guard<std::mutex> g(call_mutex());
  hipStream_t st = default_stream();
  if ((rc = srs_ensure_g2(srs, st, "sonic_srs_update"))) return rc;
  const int64_t d = srs->d, n = 2 * d + 1;
  std::unique_ptr<sonic_srs> s(srs_alloc(d));
  srs_scale_g1_enqueue(st, srs, s.get(), k.x, k.xinv, k.alpha);
  srs_build_tables(st, s.get());
  DevBuf h0(sizeof(G2Affine) * (size_t)n), h1(sizeof(G2Affine) * (size_t)n);
  srs_scale_g2(st, (long)d, srs->h.as<G2Affine>(), srs->ha.as<G2Affine>(), k.x, k.xinv, k.alpha, h0.as<G2Affine>(), h1.as<G2Affine>());
  s->h = std::move(h0); s->ha = std::move(h1);
  s->have_trapdoor = false;
  srs_update::make_proof(d, old_id, k.x1, k.a1, k.kx, k.ka, proof);
  *out = s.release();
  API_END
}

int sonic_srs_verify_update(const sonic_srs_t* old_srs, const sonic_srs_t* new_srs, const uint8_t proof[448], int check_new, int* ok) {
  API_BEGIN_ON(srs_device(new_srs))
  if (!old_srs || !new_srs || !proof || !ok) { set_error("sonic_srs_verify_update: bad argument"); return SONIC_ERR_INVALID_ARG; }
  *ok = 0;
  if (old_srs->is_view() || new_srs->is_view()) { set_error("sonic_srs_verify_update: a circuit-sized view is not a reference string"); return SONIC_ERR_INVALID_ARG; }
  if (old_srs->d != new_srs->d) return SONIC_OK;
  uint8_t old_id[32];
  int rc = sonic_fs_srs_id(old_srs, old_id);
  if (rc) return rc;
  G1Affine X, A, g0x;
  if (!srs_update::schnorr_ok(old_srs->d, old_id, proof, X, A)) return SONIC_OK;
  G2Affine hx_old, ha_old, ha_new;
  if ((rc = fetch_g1(new_srs, 0, 1, g0x)) || (rc = fetch_g2(old_srs, 0, 1, hx_old)) || (rc = fetch_g2(old_srs, 1, 0, ha_old)) || (rc = fetch_g2(new_srs, 1, 0, ha_new))) return rc;
  if (!srs_update::pairs_equal(g0x, srs_update::g2_gen(), X, hx_old)) return SONIC_OK;            // e(G0'[1], h) = e(X, H0[1])
  if (!srs_update::pairs_equal(srs_update::g1_gen(), ha_new, A, ha_old)) return SONIC_OK;         // e(g, H1'[0]) = e(A, H1[0])
  if (check_new) {
    int failed = 0;
    if ((rc = sonic_srs_check(new_srs, nullptr, &failed))) return rc;
    if (failed) return SONIC_OK;
  }
  *ok = 1;
  API_END
}

}  // extern "C"
