// The SRS handle (sonic_srs_t of include/sonic_hip.h) as a type, for the translation units that work on its device side: construction and
// the C entry points (srs_api.hip), generation and the table builders (srs.hip), the MSM entry points (msm_api.hip), the prover and the
// batched verifier.  NOT for verify.hip, verify_host.hpp or internal.hpp: the verifier's host path is also built as plain C++ with a
// stand-in handle (tests/host/san_verify.cpp) and sees the handle only through srs_d and srs_cached_id (internal.hpp).
#pragma once
#include "internal.hpp"
#include "srs_view.hpp"

struct sonic_srs {
  int64_t d;
  // which exponents the handle holds and where (srs_view.hpp): the one window [-d, d] of a whole string, slot(e) = e + d, or the windows
  // of a circuit-sized view.  Every address into g, ga, ps is basis + geo.slot(e), every table stride geo.npts(), gs's geo.sym_n().
  sonic::SrsGeometry geo;
  int64_t view_n = 0;         // a view: the n it was made for (its G2 half holds h^{x^{n-d}}); 0: a whole string
  bool is_view() const { return view_n > 0; }
  int device = 0;             // the GPU that holds the handle's memory: every call that takes the handle runs there (DeviceScope)
  // Fiat-Shamir id of the reference string (fs.hpp): constant for an SRS, made on first use (four point fetches) and cached
  mutable std::mutex id_mu;
  mutable bool have_id = false;
  mutable uint8_t id[32] = {0};
  // basis b, window table w, exponent e  ->  tab[b][w * geo.npts() + geo.slot(e)] (a whole string: w * (2d+1) + e + d) = 2^(msm_even_shift(tab_W, w)) * g^{(alpha^b) x^e}
  // (w = 0 is the basis itself; tab_W = 1 when the window tables are switched off)
  int tab_c = 0, tab_W = 1;
  // endomorphism tables (endo.hpp): tab_W windows over 130 bits instead of 255 -- 7 tables instead of 13 at c = 19 / 20 -- for SRS
  // sizes whose full tables do not fit; every MSM then runs as two half-scalar MSMs (msm_enqueue_batch)
  bool tab_endo = false;
  sonic::DevBuf g, ga;
  sonic::DevBuf ps;          // running sums of the alpha basis (srs.hip, srs_build_prefix); empty when memory was short
  sonic::DevBuf gs;          // symmetric sums A[e] + A[-e] of the alpha basis with their window tables (srs_build_sym); empty when memory was short
  // verifier half: generated on first use from the trapdoor SRS.new was given -- which is wiped as soon as that has
  // happened -- or attached by sonic_srs_set_g2_points / read from a version-2 file
  mutable bool have_trapdoor = false;
  mutable sonic::Fr x_std, alpha_std;
  mutable std::mutex g2_mu;
  mutable sonic::DevBuf h, ha;        // G2Affine[2d+1] each; a view: G2Affine[2] each, the exponents of srs_view_g2(d, view_n)
  ~sonic_srs() { wipe_trapdoor(); }
  void wipe_trapdoor() const {
    volatile uint32_t* a = x_std.l; volatile uint32_t* b = alpha_std.l;
    for (int i = 0; i < 8; i++) { a[i] = 0; b[i] = 0; }
    have_trapdoor = false;
  }
  // table 0 of a basis, exponent e at slot geo.slot(e); window table w follows at + w geo.npts()
  sonic::PointArray basis(int b) const { return sonic::PointArray{(b ? ga : g).as<char>(), SONIC_SRS_POINT_BYTES}; }
  sonic::PointArrayMut basis_mut(int b) { return sonic::PointArrayMut{(b ? ga : g).as<char>(), SONIC_SRS_POINT_BYTES}; }
  // running sums of the alpha basis (p == nullptr: not held)
  sonic::PointArray prefix() const { return sonic::PointArray{ps.as<char>(), SONIC_SRS_POINT_BYTES}; }
  sonic::PointArrayMut prefix_mut() { return sonic::PointArrayMut{ps.as<char>(), SONIC_SRS_POINT_BYTES}; }
  // symmetric sums of the alpha basis: geo.sym_n() slots per window table, slot e for exponent e (p == nullptr: not held)
  sonic::PointArray sym() const { return sonic::PointArray{gs.as<char>(), SONIC_SRS_POINT_BYTES}; }
  sonic::PointArrayMut sym_mut() { return sonic::PointArrayMut{gs.as<char>(), SONIC_SRS_POINT_BYTES}; }
};

namespace sonic {

// what API_BEGIN_ON takes for an entry point over a handle: -1 for a null handle (= the default device: the null check then reports the argument)
inline int srs_device(const sonic_srs* s) { return s ? s->device : -1; }
// exponents [e0, e0 + n) must lie inside the handle's [-d, d]; `who` opens the message
inline bool srs_range_ok(const char* who, const sonic_srs* s, int64_t e0, int64_t n) {
  if (e0 >= -s->d && e0 + n - 1 <= s->d) return true;
  set_error("%s: exponent range [%ld, %ld] outside [-%ld, %ld]", who, (long)e0, (long)(e0 + n - 1), (long)s->d, (long)s->d);
  return false;
}

// exponents [e0, e0 + n) -- already inside [-d, d] -- must lie inside one window of the handle: always true of a whole string; a view
// says which range it was asked for and which windows it holds (the caller returns SONIC_ERR_INVALID_ARG)
inline bool srs_held_ok(const char* who, const sonic_srs* s, int64_t e0, int64_t n) {
  if (s->geo.contains(e0, n)) return true;
  const SrsGeometry& g = s->geo;
  if (g.two()) set_error("%s: exponent range [%ld, %ld] is not held by this view of the SRS: its windows are [%ld, %ld] and [%ld, %ld] of [-%ld, %ld]", who,
                         (long)e0, (long)(e0 + n - 1), (long)g.lo0, (long)g.hi0, (long)g.lo1, (long)g.hi1, (long)s->d, (long)s->d);
  else set_error("%s: exponent range [%ld, %ld] is not held by this view of the SRS: its window is [%ld, %ld] of [-%ld, %ld]", who,
                 (long)e0, (long)(e0 + n - 1), (long)g.lo0, (long)g.hi0, (long)s->d, (long)s->d);
  return false;
}
// the points of an MSM job over exponents [e0, e0 + n) of basis b; a range the handle does not hold ends the call with
// SONIC_ERR_INVALID_ARG before anything of the job is launched (never a wrong point)
inline PointArray srs_job_points(const char* who, const sonic_srs* s, int b, int64_t e0, int64_t n) {
  if (n <= 0) return s->basis(b);
  if (!srs_held_ok(who, s, e0, n)) throw HipFail{SONIC_ERR_INVALID_ARG};
  return s->basis(b) + s->geo.slot(e0);
}

// a prover or verifier of (n, Q) over a view: the view's windows must contain the circuit's own (a smaller circuit than the view's passes)
inline bool srs_view_admits(const char* who, const sonic_srs* s, int64_t n, int64_t Q) {
  if (srs_view_d_needed(s->d, n)) return true;          // (the callers' own d rule answers)
  const SrsGeometry need = srs_view_geometry(s->d, n, Q);
  return srs_held_ok(who, s, need.lo0, need.len0()) && srs_held_ok(who, s, need.lo1, need.len1());
}

// an empty handle on the current device, sized by srs_policy.hpp (srs_api.hip): a whole string, or a view with the geometry of (n, Q)
sonic_srs* srs_alloc(int64_t d);
sonic_srs* srs_alloc_view(int64_t d, int64_t n, int64_t Q);
// plan for an MSM over n consecutive points of the handle (srs_api.hip)
MsmPlan srs_msm_plan(const sonic_srs* s, long n);
// SRS generation (srs.hip): fills both bases of `s` from x, alpha (standard-form Fr on the host), then its tables
void srs_generate(hipStream_t st, sonic_srs* s, const Fr& x_std, const Fr& alpha_std);
// fills window tables 1 .. W-1 of both bases from table 0, the running sums and the symmetric sums (srs.hip)
void srs_build_tables(hipStream_t st, sonic_srs* s);
// updatable SRS (srs.hip): dst's two bases = src's with every point scaled, basis 0 by x^e, basis 1 by alpha x^e (Montgomery scalars; both
// handles whole strings of one d; waits for the stream; the caller builds dst's tables), and the randomizers of the structure check:
// rho[i] for i = e + d in [0, n), standard form, upper four limbs zero (srs_scale.hpp)
void srs_scale_g1_enqueue(hipStream_t st, const sonic_srs* src, sonic_srs* dst, const Fr& x, const Fr& xinv, const Fr& alpha);
void srs_check_rho_enqueue(hipStream_t st, const uint8_t seed[32], long n, Fr* d_rho);
// makes sure the G2 half is resident, generating it where the handle still can (srs_api.hip); the caller holds call_mutex
int srs_ensure_g2(const sonic_srs* srs, hipStream_t st, const char* who);

}  // namespace sonic
