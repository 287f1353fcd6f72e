// The SRS handle behind the C ABI (include/sonic_hip.h): sizing and allocation (the rule itself: srs_policy.hpp), the plan of an MSM over a
// handle, SRS.new, construction from points, the lazy G2 half, point read-back, both on-disk containers and the device-to-device replica.  The
// handle as a type: srs_handle.hpp; generation in srs.hip and srs_g2.hip.
#include <string.h>
#include <functional>
#include <memory>
#include <string>
#include <vector>
#include "srs_handle.hpp"
#include "srs_policy.hpp"
#include "g2.hpp"
#include "srs_file.hpp"

namespace sonic {

int64_t srs_d(const sonic_srs* s) { return s->d; }
int srs_cached_id(const sonic_srs* s, int (*make)(const sonic_srs*, uint8_t*), uint8_t out[32]) {
  // only a success is kept (a transient failure of the first attempt -- no memory for the leased context, a busy device --
  // used to be remembered with its status, and sonic_prover_prove_fs / sonic_verify_fs failed on that handle from then on although its
  // points were fine): a failed attempt is simply made again by the next call
  std::lock_guard<std::mutex> g(s->id_mu);
  if (!s->have_id) {
    uint8_t tmp[32];
    const int rc = make(s, tmp);
    if (rc) return rc;
    memcpy(s->id, tmp, 32);
    s->have_id = true;
  }
  memcpy(out, s->id, 32);
  return SONIC_OK;
}

// read the knobs, then ask, allocate, ask, allocate, ask, allocate: the free memory is read again before every question (srs_policy.hpp)
// (a whole string: view_n = 0, the width by d; a view: the width by its n, srs_view_window_policy; the memory questions by the point
// counts of the geometry either way)
static sonic_srs* srs_alloc_geo(const SrsGeometry& geo, int64_t view_n) {
  std::unique_ptr<sonic_srs> s(new sonic_srs());
  s->d = geo.d; s->geo = geo; s->view_n = view_n;
  s->device = current_ctx().dev;
  const SrsKnobs knobs = srs_knobs_from_env();
  const size_t n = (size_t)geo.npts(), sym_n = (size_t)geo.sym_n();
  size_t free_b = 0, total_b = 0;
  (void)hipMemGetInfo(&free_b, &total_b);
  const SrsWindows win = view_n ? srs_view_window_policy(view_n, geo.npts(), free_b, knobs) : srs_window_policy(geo.d, n, free_b, knobs);
  s->tab_c = win.c; s->tab_W = win.W; s->tab_endo = win.endo;
  s->g.alloc((size_t)SONIC_SRS_POINT_BYTES * n * win.W);
  s->ga.alloc((size_t)SONIC_SRS_POINT_BYTES * n * win.W);
  (void)hipMemGetInfo(&free_b, &total_b);
  if (srs_holds_prefix_of(n, free_b, knobs)) s->ps.alloc(srs_prefix_bytes_of(n));
  (void)hipMemGetInfo(&free_b, &total_b);
  if (srs_holds_sym_of(sym_n, win.W, win.endo, free_b, knobs)) s->gs.alloc(srs_sym_bytes_of(sym_n, win.W));
  return s.release();
}
sonic_srs* srs_alloc(int64_t d) { return srs_alloc_geo(srs_full_geometry(d), 0); }
sonic_srs* srs_alloc_view(int64_t d, int64_t n, int64_t Q) { return srs_alloc_geo(srs_view_geometry(d, n, Q), n); }

// plan for an MSM over n consecutive SRS points: shared-bucket plan over the window tables unless the MSM is
// tiny compared with the bucket set, the tables are off, or a test forces a window size
// Entry encoding limits (msm.hip, k_part_scatter / entry_point): over window tables an entry packs the term index into 26 bits and
// the window into 5, without tables the index has 31 bits.  MSMs of 2^26 terms and more therefore run over per-window buckets
// even when the SRS has tables, and 2^31 terms are refused (msm_enqueue_batch, sonic_msm_plan).
MsmPlan srs_msm_plan(const sonic_srs* s, long n) {
  // (up to round 5 an MSM of fewer than 1/16 of the bucket count fell back to per-window buckets without the tables: 64 four-bit windows,
  // 64 bucket sets, a chain that cannot be batched and 255 doublings of host tail per MSM -- 0.9 ms each, which is what the reference's
  // own criterion shape, n = 1 / d = 25, paid fifteen times per proof: profiles/r05_criterion_shape.txt.  Over the tables the same MSM
  // is a batchable job whose cost is the butterfly over the shared bucket set: 0.12 ms at 2^16 buckets, 0.55 ms at 2^19.)
  if (s->tab_W > 1 && s->tab_W <= MSM_TABLE_MAX_WINDOWS && n < MSM_TABLE_MAX_TERMS && msm_window_override() == 0)
    return msm_plan_tables(n > 0 ? n : 1, s->tab_c, s->tab_W, s->geo.npts(), s->tab_endo);
  return msm_plan(n > 0 ? n : 1);
}
}  // namespace sonic

using namespace sonic;

extern "C" {

int sonic_srs_new(int64_t d, const uint8_t x[32], const uint8_t alpha[32], sonic_srs_t** out) { return sonic_srs_new_on(-1, d, x, alpha, out); }
int sonic_srs_new_on(int device, int64_t d, const uint8_t x[32], const uint8_t alpha[32], sonic_srs_t** out) {
  API_BEGIN_ON(device)
  if (d < 1 || !x || !alpha || !out) { set_error("sonic_srs_new: bad argument"); return SONIC_ERR_INVALID_ARG; }
  Fr xs, as;
  memcpy(xs.l, x, 32); memcpy(as.l, alpha, 32);
  if (!fp_is_canonical(xs) || !fp_is_canonical(as)) { set_error("sonic_srs_new: x or alpha not < r"); return SONIC_ERR_BAD_ENCODING; }
  if (xs.is_zero()) { set_error("sonic_srs_new: x = 0 has no inverse (recip x, SRS.hs:29)"); return SONIC_ERR_INEXACT_DIVISION; }
  std::lock_guard<std::mutex> g(call_mutex());
  sonic_srs* s = srs_alloc(d);
  try { srs_generate(default_stream(), s, xs, as); } catch (...) { sonic_srs_free(s); throw; }
  s->have_trapdoor = true; s->x_std = xs; s->alpha_std = as;
  *out = s;
  API_END
}

int sonic_srs_from_points(int64_t d, const uint8_t* basis0, const uint8_t* basis1, sonic_srs_t** out) {
  return sonic_srs_from_points_on(-1, d, basis0, basis1, out);
}
// The tail every way of filling a handle's G1 bases shares (caller-supplied points, either file container): r P = O for every point of
// both bases, the error bits the head and the walk have collected in `err` (1 non-canonical or malformed, 2 off the curve, 4 outside the
// subgroup, 8 infinity where none may be), then the window tables.  Takes the handle: it is deleted when the points are refused.
static int srs_finish_g1(const char* who, hipStream_t st, sonic_srs* s, DevBuf& err, sonic_srs_t** out) {
  const long n = s->geo.npts();
  for (int b = 0; b < 2; b++) points_subgroup_check_enqueue(st, s->basis(b), n, err.as<int>());
  const int herr = read_flags(st, err);
  if (herr) {
    delete s;
    set_error("%s: %s", who, (herr & 1) ? "non-canonical coordinate" : (herr & 2) ? "point not on curve" : (herr & 4) ? "point outside the order-r subgroup" : "point at infinity (only the omitted g^alpha, basis 1 slot e = 0, may be empty)");
    return SONIC_ERR_BAD_ENCODING;
  }
  srs_build_tables(st, s);
  *out = s;
  return SONIC_OK;
}
int sonic_srs_from_points_on(int device, int64_t d, const uint8_t* basis0, const uint8_t* basis1, sonic_srs_t** out) {
  API_BEGIN_ON(device)
  if (d < 1 || !basis0 || !basis1 || !out) { set_error("sonic_srs_from_points: bad argument"); return SONIC_ERR_INVALID_ARG; }
  std::lock_guard<std::mutex> g(call_mutex());
  hipStream_t st = default_stream();
  const long n = 2 * d + 1;
  sonic_srs* s = srs_alloc(d);
  DevBuf raw(96 * n), err(4);
  HIP_OK(hipMemsetAsync(err.p, 0, 4, st));
  for (int b = 0; b < 2; b++) {
    HIP_OK(hipMemcpyAsync(raw.p, b ? basis1 : basis0, 96 * n, hipMemcpyHostToDevice, st));
    points_from_bytes_enqueue(st, raw.as<uint8_t>(), s->basis_mut(b), n, err.as<int>(), b ? (long)d : -2L);        // basis 1 has the empty slot e = 0 (SRS.hs:38); basis 0 has none
  }
  return srs_finish_g1("sonic_srs_from_points", st, s, err, out);
  API_END
}

void sonic_srs_free(sonic_srs_t* srs) {
  if (!srs) return;
  // (when the handle's device cannot be made current the parked one-shot shells over this SRS must still be unlinked -- a later
  // SRS allocated at the same address would otherwise match a shell whose tables are gone)
  try { DeviceScope scope(srs->device); drop_one_shot_of(srs); delete srs; } catch (const HipFail&) { unlink_one_shot_of(srs); delete srs; }
}
int64_t sonic_srs_d(const sonic_srs_t* srs) { return srs ? srs->d : -1; }
int sonic_srs_device(const sonic_srs_t* srs) { return srs ? srs->device : -1; }

int sonic_srs_get_points(const sonic_srs_t* srs, int basis, int64_t e0, int64_t n, uint8_t* out) {
  API_BEGIN_ON(srs_device(srs))
  if (!srs || !out || n < 0) return SONIC_ERR_INVALID_ARG;
  if (!srs_range_ok("sonic_srs_get_points", srs, e0, n)) return SONIC_ERR_SRS_INDEX;
  if (n == 0) return SONIC_OK;
  const bool sym_read = basis == SONIC_BASIS_ALPHA_SYM;            // (reads exponents max(e0, 0) .. of its own table)
  if (!sym_read && !srs_held_ok("sonic_srs_get_points", srs, e0, n)) return SONIC_ERR_INVALID_ARG;
  if (sym_read && e0 + n > srs->geo.sym_n()) {
    set_error("sonic_srs_get_points: this view of the SRS holds the symmetric sums of exponents 0 .. %ld, asked for [%ld, %ld]", (long)srs->geo.sym_n() - 1, (long)e0, (long)(e0 + n - 1));
    return SONIC_ERR_INVALID_ARG;
  }
  CallLease lease;
  hipStream_t st = lease.st();
  DevBuf raw(96 * n);
  PointArray src;                   // the slot of exponent `lo`: exponents [lo, e0 + n) are read, what lies below them stays as `raw` was filled
  int64_t lo = e0;
  if (basis == SONIC_BASIS_ALPHA_SYM) {        // diagnostic: the symmetric sums of the alpha basis (srs_build_sym; entries e <= 0 are empty)
    if (!srs->gs.p) { set_error("sonic_srs_get_points: this SRS holds no symmetric sums"); return SONIC_ERR_INVALID_ARG; }
    // (the table holds exponents 0 .. d: slot 0 and everything below it read as the empty sum)
    HIP_OK(hipMemsetAsync(raw.p, 0, 96 * n, st));
    if (lo < 0) lo = 0;
    src = srs->sym() + lo;
  } else if (basis == SONIC_BASIS_ALPHA_PREFIX) {     // diagnostic: the running sums of the alpha basis (srs_build_prefix)
    if (!srs->ps.p) { set_error("sonic_srs_get_points: this SRS holds no running sums"); return SONIC_ERR_INVALID_ARG; }
    src = srs->prefix() + srs->geo.slot(e0);
  } else {                                     // diagnostic: basis = b + 2 w reads window table w (2^(c w) multiples) of basis b
    const int w = basis >> 1;
    if (w >= srs->tab_W) { set_error("sonic_srs_get_points: no window table %d", w); return SONIC_ERR_INVALID_ARG; }
    src = srs->basis(basis & 1) + (size_t)w * srs->geo.npts() + srs->geo.slot(e0);
  }
  points_to_bytes_enqueue(st, src, raw.as<uint8_t>() + 96 * (lo - e0), (long)(e0 + n - lo));
  HIP_OK(hipMemcpyAsync(out, raw.p, 96 * n, hipMemcpyDeviceToHost, st));
  HIP_OK(hipStreamSynchronize(st));
  API_END
}

}  // extern "C"
// makes sure the G2 half is resident; caller holds call_mutex
int sonic::srs_ensure_g2(const sonic_srs* srs, hipStream_t st, const char* who) {
  std::lock_guard<std::mutex> g2(srs->g2_mu);
  if (srs->h.p) return SONIC_OK;
  if (srs->is_view()) { set_error("%s: this view of the SRS has no G2 half (the string it was made from could not supply one)", who); return SONIC_ERR_INVALID_ARG; }
  if (!srs->have_trapdoor) { set_error("%s: this SRS has no G2 half (built from G1 points only)", who); return SONIC_ERR_INVALID_ARG; }
  const size_t cnt = (size_t)(2 * srs->d + 1);
  // generated into local buffers and attached only when the generation has finished: a failure half way (e.g. no memory for
  // its Jacobian scratch at large d) must leave the handle without a G2 half and with its trapdoor, not with uninitialised
  // memory that a later call would serve -- all-zero bytes decode as the point at infinity, and a verifier whose three G2
  // elements are at infinity accepts every proof
  DevBuf h0(sizeof(G2Affine) * cnt), h1(sizeof(G2Affine) * cnt);
  srs_generate_g2(st, srs->d, srs->x_std, srs->alpha_std, h0.as<G2Affine>(), h1.as<G2Affine>());
  srs->h = std::move(h0);
  srs->ha = std::move(h1);
  srs->wipe_trapdoor();          // x and alpha have served their last purpose
  return SONIC_OK;
}
extern "C" {

int sonic_srs_get_g2_points(const sonic_srs_t* srs, int basis, int64_t e0, int64_t n, uint8_t* out) {
  API_BEGIN_ON(srs_device(srs))
  if (!srs || !out || n < 0 || (basis != 0 && basis != 1)) return SONIC_ERR_INVALID_ARG;
  if (!srs_range_ok("sonic_srs_get_g2_points", srs, e0, n)) return SONIC_ERR_SRS_INDEX;
  std::lock_guard<std::mutex> g(call_mutex());
  hipStream_t st = default_stream();
  int rc = srs_ensure_g2(srs, st, "sonic_srs_get_g2_points");
  if (rc) return rc;
  if (n == 0) return SONIC_OK;
  DevBuf raw(192 * n);
  int64_t at = e0 + srs->d;
  if (srs->is_view()) {                 // two elements per basis, and nothing else
    const SrsViewG2 q = srs_view_g2(srs->d, srs->view_n);
    at = n == 1 && e0 == q.e[basis][0] ? 0 : n == 1 && e0 == q.e[basis][1] ? 1 : -1;
    if (at < 0) {
      set_error("sonic_srs_get_g2_points: exponent range [%ld, %ld] of basis %d is not held by this view of the SRS: it holds %ld and %ld", (long)e0,
                (long)(e0 + n - 1), basis, (long)q.e[basis][0], (long)q.e[basis][1]);
      return SONIC_ERR_INVALID_ARG;
    }
  }
  g2_points_to_bytes_enqueue(st, (basis ? srs->ha : srs->h).as<G2Affine>() + at, raw.as<uint8_t>(), n);
  HIP_OK(hipMemcpyAsync(out, raw.p, 192 * n, hipMemcpyDeviceToHost, st));
  HIP_OK(hipStreamSynchronize(st));
  API_END
}

// the tail of both ways of attaching a G2 half (192-byte points, the compressed container): the error bits its validation has collected
// in `err`, then the two vectors go to the handle and the trapdoor goes away
static int srs_attach_g2(const char* who, hipStream_t st, sonic_srs_t* srs, DevBuf& err, DevBuf& h0, DevBuf& h1) {
  const int herr = read_flags(st, err);
  if (herr) {
    set_error("%s: %s", who, (herr & 1) ? "non-canonical coordinate" : (herr & 2) ? "point not on the twist" : (herr & 4) ? "point outside the order-r subgroup" : "point at infinity (h^{x^e}, h^{alpha x^e} are never the identity)");
    return SONIC_ERR_BAD_ENCODING;
  }
  std::lock_guard<std::mutex> g2(srs->g2_mu);
  srs->h = std::move(h0);
  srs->ha = std::move(h1);
  srs->wipe_trapdoor();
  return SONIC_OK;
}

int sonic_srs_set_g2_points(sonic_srs_t* srs, const uint8_t* basis0, const uint8_t* basis1) {
  API_BEGIN_ON(srs_device(srs))
  if (!srs || !basis0 || !basis1) return SONIC_ERR_INVALID_ARG;
  if (srs->is_view()) { set_error("sonic_srs_set_g2_points: a circuit-sized view is not a reference string (attach the G2 half to the string and make the view from it)"); return SONIC_ERR_INVALID_ARG; }
  std::lock_guard<std::mutex> g(call_mutex());
  hipStream_t st = default_stream();
  const long n = 2 * srs->d + 1;
  DevBuf raw(192 * n), err(4), h0(sizeof(G2Affine) * n), h1(sizeof(G2Affine) * n);
  HIP_OK(hipMemsetAsync(err.p, 0, 4, st));
  for (int b = 0; b < 2; b++) {
    HIP_OK(hipMemcpyAsync(raw.p, b ? basis1 : basis0, 192 * n, hipMemcpyHostToDevice, st));
    g2_points_from_bytes_enqueue(st, raw.as<uint8_t>(), (b ? h1 : h0).as<G2Affine>(), n, err.as<int>());
  }
  return srs_attach_g2("sonic_srs_set_g2_points", st, srs, err, h0, h1);
  API_END
}

int sonic_srs_has_g2(const sonic_srs_t* srs) {
  if (!srs) return 0;
  std::lock_guard<std::mutex> g2(srs->g2_mu);
  return (srs->h.p != nullptr || srs->have_trapdoor) ? 1 : 0;
}

// ---- on-disk SRS: "SONICSRS" | u32 version = 2 | u32 flags (bit 0: G2 half follows) | i64 d | basis0, basis1: (2d+1) x 96 B |
// [h basis0, h basis1: (2d+1) x 192 B], canonical affine encodings.  The reference has no persistence at all; this
// amortises SRS.new across runs, and with the G2 half a loaded SRS verifies as well as proves -- without the trapdoor.
int sonic_srs_save(const sonic_srs_t* srs, const char* path, int with_g2) {
  API_BEGIN_ON(srs_device(srs))
  if (!srs || !path || with_g2 < 0 || with_g2 > 2) return SONIC_ERR_INVALID_ARG;
  if (srs->is_view()) { set_error("sonic_srs_save: a circuit-sized view is not a reference string and has no container"); return SONIC_ERR_INVALID_ARG; }
  if (with_g2 == 2) with_g2 = sonic_srs_has_g2(srs) ? 1 : 0;          // "if the handle has (or can generate) it"
  if (with_g2) {
    std::lock_guard<std::mutex> g(call_mutex());
    int rc = srs_ensure_g2(srs, default_stream(), "sonic_srs_save");
    if (rc) return rc;
  }
  FILE* f = fopen(path, "wb");
  if (!f) { set_error("sonic_srs_save: cannot open %s", path); return SONIC_ERR_INVALID_ARG; }
  int64_t d = srs->d;
  bool ok = srs_file_write_header(f, d, with_g2 != 0);
  const int64_t n = 2 * d + 1, CH = 1 << 16;
  std::vector<uint8_t> buf(192 * (size_t)CH);
  for (int b = 0; b < (with_g2 ? 4 : 2) && ok; b++)
    for (int64_t i = 0; i < n && ok; i += CH) {
      int64_t m = n - i < CH ? n - i : CH;
      const size_t sz = b < 2 ? 96 : 192;
      int rc = b < 2 ? sonic_srs_get_points(srs, b, -d + i, m, buf.data()) : sonic_srs_get_g2_points(srs, b - 2, -d + i, m, buf.data());
      if (rc) { fclose(f); return rc; }
      ok = fwrite(buf.data(), sz, (size_t)m, f) == (size_t)m;
    }
  ok = (fclose(f) == 0) && ok;
  if (!ok) { set_error("sonic_srs_save: write to %s failed", path); return SONIC_ERR_INVALID_ARG; }
  API_END
}

// ---- the compressed container (srs_file.hpp): "SONICSRZ" | u32 version = 1 | u32 flags | i64 d | the G1 bases as (2d+1) x 48 B | [the G2
// bases as (2d+1) x 96 B].  Half the bytes; the half that is gone is recomputed on the device when the file is loaded.
int sonic_srs_save_compressed(const sonic_srs_t* srs, const char* path, int with_g2) {
  API_BEGIN_ON(srs_device(srs))
  if (!srs || !path || with_g2 < 0 || with_g2 > 2) return SONIC_ERR_INVALID_ARG;
  if (srs->is_view()) { set_error("sonic_srs_save_compressed: a circuit-sized view is not a reference string and has no container"); return SONIC_ERR_INVALID_ARG; }
  if (with_g2 == 2) with_g2 = sonic_srs_has_g2(srs) ? 1 : 0;
  std::lock_guard<std::mutex> g(call_mutex());
  hipStream_t st = default_stream();
  if (with_g2) {
    int rc = srs_ensure_g2(srs, st, "sonic_srs_save_compressed");
    if (rc) return rc;
  }
  FILE* f = fopen(path, "wb");
  if (!f) { set_error("sonic_srs_save_compressed: cannot open %s", path); return SONIC_ERR_INVALID_ARG; }
  struct Closer { FILE* f; ~Closer() { if (f) fclose(f); } } closer{f};
  const int64_t d = srs->d, n = 2 * d + 1, CH = 1 << 16;
  bool ok = srs_zfile_write_header(f, d, with_g2 != 0);
  std::vector<uint8_t> buf(96 * (size_t)CH);
  DevBuf z(96 * (size_t)CH);
  for (int b = 0; b < (with_g2 ? 4 : 2) && ok; b++)
    for (int64_t i = 0; i < n && ok; i += CH) {
      const int64_t m = n - i < CH ? n - i : CH;
      const size_t sz = b < 2 ? 48 : 96;
      if (b < 2) g1_compress_enqueue(st, srs->basis(b) + i, z.as<uint8_t>(), m);
      else g2_compress_enqueue(st, (b == 3 ? srs->ha : srs->h).as<G2Affine>() + i, z.as<uint8_t>(), m);
      HIP_OK(hipMemcpyAsync(buf.data(), z.p, sz * (size_t)m, hipMemcpyDeviceToHost, st));
      HIP_OK(hipStreamSynchronize(st));
      ok = fwrite(buf.data(), sz, (size_t)m, f) == (size_t)m;
    }
  closer.f = nullptr;
  ok = (fclose(f) == 0) && ok;
  if (!ok) { set_error("sonic_srs_save_compressed: write to %s failed", path); return SONIC_ERR_INVALID_ARG; }
  API_END
}

// decompresses one vector of a compressed container on the device, in chunks, straight into its array; the verdicts and the infinity
// rule (inf_ok: the one slot that may hold infinity, or -2) are folded into the loaders' error bits in *herr
static void srs_zload_vector(hipStream_t st, const std::vector<uint8_t>& src, size_t zsz, long n, long inf_ok, int* herr,
                             const std::function<void(const uint8_t*, uint8_t*, long, long)>& enqueue) {
  const long CH = 1L << 18;
  const long cap = n < CH ? n : CH;
  DevBuf raw(zsz * (size_t)cap), fl((size_t)cap);
  std::vector<uint8_t> hfl((size_t)cap);
  for (long i = 0; i < n; i += CH) {
    const long m = n - i < CH ? n - i : CH;
    HIP_OK(hipMemcpyAsync(raw.p, &src[zsz * (size_t)i], zsz * (size_t)m, hipMemcpyHostToDevice, st));
    enqueue((const uint8_t*)raw.as<uint8_t>(), fl.as<uint8_t>(), i, m);
    HIP_OK(hipMemcpyAsync(hfl.data(), fl.p, (size_t)m, hipMemcpyDeviceToHost, st));
    HIP_OK(hipStreamSynchronize(st));
    for (long k = 0; k < m; k++) {
      *herr |= hfl[(size_t)k];
      if (!hfl[(size_t)k] && (src[zsz * (size_t)(i + k)] & 0x40) && i + k != inf_ok) *herr |= 8;      // an accepted encoding of infinity
    }
  }
}
static int srs_load_compressed(const char* path, sonic_srs_t** out) {
  SrsFile file;
  std::string why;
  const int frc = srs_zfile_read(path, file, why);
  if (frc) { set_error("sonic_srs_load: %s", why.c_str()); return frc == 1 ? SONIC_ERR_INVALID_ARG : SONIC_ERR_BAD_ENCODING; }
  std::lock_guard<std::mutex> g(call_mutex());
  hipStream_t st = default_stream();
  const int64_t d = file.d;
  const long n = 2 * d + 1;
  sonic_srs* s = srs_alloc(d);
  DevBuf err(4);
  int herr = 0;
  try {
    for (int b = 0; b < 2; b++)
      srs_zload_vector(st, b ? file.g1 : file.g0, 48, n, b ? (long)d : -2L, &herr, [&](const uint8_t* in, uint8_t* fl, long i, long m) {
        g1_decompress_enqueue(st, in, s->basis_mut(b) + i, nullptr, fl, m, false);          // (the subgroup walk is the shared tail's)
      });
    HIP_OK(hipMemcpyAsync(err.p, &herr, 4, hipMemcpyHostToDevice, st));
  } catch (...) { delete s; throw; }
  int rc = srs_finish_g1("sonic_srs_load", st, s, err, &s);
  if (rc) return rc;
  if (file.has_g2()) {
    DevBuf h0(sizeof(G2Affine) * n), h1(sizeof(G2Affine) * n);
    herr = 0;
    try {
      for (int b = 0; b < 2; b++)
        srs_zload_vector(st, b ? file.h1 : file.h0, 96, n, -2L, &herr, [&](const uint8_t* in, uint8_t* fl, long i, long m) {
          g2_decompress_enqueue(st, in, (b ? h1 : h0).as<G2Affine>() + i, nullptr, fl, m, true);
        });
      HIP_OK(hipMemcpyAsync(err.p, &herr, 4, hipMemcpyHostToDevice, st));
      rc = srs_attach_g2("sonic_srs_load", st, s, err, h0, h1);
    } catch (...) { delete s; throw; }
    if (rc) { delete s; return rc; }
  }
  *out = s;
  return SONIC_OK;
}

int sonic_srs_load(const char* path, sonic_srs_t** out) { return sonic_srs_load_on(-1, path, out); }
int sonic_srs_load_on(int device, const char* path, sonic_srs_t** out) {
  API_BEGIN_ON(device)
  if (!path || !out) return SONIC_ERR_INVALID_ARG;
  if (srs_file_is_compressed(path)) return srs_load_compressed(path, out);      // by its magic; everything else is srs_file_read's to judge
  SrsFile file;
  std::string why;
  const int frc = srs_file_read(path, file, why);             // header against the real file size before anything is allocated (srs_file.hpp)
  if (frc) { set_error("sonic_srs_load: %s", why.c_str()); return frc == 1 ? SONIC_ERR_INVALID_ARG : SONIC_ERR_BAD_ENCODING; }
  const int64_t d = file.d;
  const uint32_t flags = file.flags;
  std::vector<uint8_t>&b0 = file.g0, &b1 = file.g1, &h0 = file.h0, &h1 = file.h1;
  sonic_srs_t* s = nullptr;
  int rc = sonic_srs_from_points(d, b0.data(), b1.data(), &s);     // validates every point, rebuilds the window tables
  if (rc) return rc;
  if (flags & 1u) {
    rc = sonic_srs_set_g2_points(s, h0.data(), h1.data());
    if (rc) { sonic_srs_free(s); return rc; }
  }
  *out = s;
  API_END
}

// A replica of an SRS on another GPU of this process, copied device to device: both G1 bases with their window tables (so that the
// replica plans every MSM exactly like the original: sonic_prove_shared's ranks must agree on NB and W), the G2 half if present, the
// trapdoor if the G2 half has not been generated yet.  hipMemcpyPeer goes over xGMI where the GPUs are linked and through the host
// otherwise; nothing is validated again (the source was) and no table is rebuilt.
int sonic_srs_replicate(const sonic_srs_t* srs, int device, sonic_srs_t** out) {
  API_BEGIN_ON(device)
  if (!srs || !out) return SONIC_ERR_INVALID_ARG;
  DeviceCtx& ctx = current_ctx();
  std::lock_guard<std::mutex> g(ctx.call_mu);
  std::unique_ptr<sonic_srs> r(new sonic_srs());
  r->d = srs->d; r->geo = srs->geo; r->view_n = srs->view_n; r->device = ctx.dev;
  r->tab_c = srs->tab_c; r->tab_W = srs->tab_W; r->tab_endo = srs->tab_endo;
  r->g.alloc(srs->g.bytes); r->ga.alloc(srs->ga.bytes);
  HIP_OK(hipMemcpyPeer(r->g.p, ctx.dev, srs->g.p, srs->device, srs->g.bytes));
  HIP_OK(hipMemcpyPeer(r->ga.p, ctx.dev, srs->ga.p, srs->device, srs->ga.bytes));
  if (srs->ps.p) { r->ps.alloc(srs->ps.bytes); HIP_OK(hipMemcpyPeer(r->ps.p, ctx.dev, srs->ps.p, srs->device, srs->ps.bytes)); }
  if (srs->gs.p) { r->gs.alloc(srs->gs.bytes); HIP_OK(hipMemcpyPeer(r->gs.p, ctx.dev, srs->gs.p, srs->device, srs->gs.bytes)); }
  {
    std::lock_guard<std::mutex> g2(srs->g2_mu);
    if (srs->h.p) {
      r->h.alloc(srs->h.bytes); r->ha.alloc(srs->ha.bytes);
      HIP_OK(hipMemcpyPeer(r->h.p, ctx.dev, srs->h.p, srs->device, srs->h.bytes));
      HIP_OK(hipMemcpyPeer(r->ha.p, ctx.dev, srs->ha.p, srs->device, srs->ha.bytes));
    } else if (srs->have_trapdoor) {
      r->have_trapdoor = true; r->x_std = srs->x_std; r->alpha_std = srs->alpha_std;
    }
  }
  HIP_OK(hipDeviceSynchronize());
  *out = r.release();
  API_END
}

// ---- circuit-sized views (srs_view.hpp): the same d, the same Fiat-Shamir id, the same commitments and proofs, over copies of only the
// exponent windows a circuit of (n, Q) touches, with window tables, running sums and symmetric sums sized for those windows ------------
static int view_args_ok(const char* who, int64_t d, int64_t n, int64_t Q) {
  if (n < 1 || Q < 1) { set_error("%s: a circuit has n >= 1 and Q >= 1, got n = %ld, Q = %ld", who, (long)n, (long)Q); return SONIC_ERR_INVALID_ARG; }
  if (n > SRS_FILE_MAX_D || Q > SRS_FILE_MAX_D) { set_error("%s: n = %ld, Q = %ld is no circuit size", who, (long)n, (long)Q); return SONIC_ERR_INVALID_ARG; }
  const int64_t need = srs_view_d_needed(d, n);
  if (need) {
    set_error("%s: d = %ld is too small for a circuit of n = %ld: it needs d >= %ld (7n for the prover, 4n + 8 for the blinders of t)", who, (long)d, (long)n, (long)need);
    return SONIC_ERR_INVALID_ARG;
  }
  return SONIC_OK;
}
// the four G2 points of a view from their 192-byte encodings (basis-major), validated like every G2 half that is attached
static int view_attach_g2(const char* who, hipStream_t st, sonic_srs* v, const uint8_t* bytes) {
  DevBuf raw(192 * 4), err(4), h0(sizeof(G2Affine) * 2), h1(sizeof(G2Affine) * 2);
  HIP_OK(hipMemsetAsync(err.p, 0, 4, st));
  HIP_OK(hipMemcpyAsync(raw.p, bytes, 192 * 4, hipMemcpyHostToDevice, st));
  g2_points_from_bytes_enqueue(st, raw.as<uint8_t>(), h0.as<G2Affine>(), 2, err.as<int>());
  g2_points_from_bytes_enqueue(st, raw.as<uint8_t>() + 192 * 2, h1.as<G2Affine>(), 2, err.as<int>());
  return srs_attach_g2(who, st, v, err, h0, h1);
}

int sonic_srs_for_circuit(const sonic_srs_t* srs, int64_t n, int64_t Q, sonic_srs_t** out) {
  API_BEGIN_ON(srs_device(srs))
  if (!srs || !out) { set_error("sonic_srs_for_circuit: bad argument"); return SONIC_ERR_INVALID_ARG; }
  int rc = view_args_ok("sonic_srs_for_circuit", srs->d, n, Q);
  if (rc) return rc;
  const SrsGeometry geo = srs_view_geometry(srs->d, n, Q);
  if (!srs_held_ok("sonic_srs_for_circuit", srs, geo.lo0, geo.len0()) || !srs_held_ok("sonic_srs_for_circuit", srs, geo.lo1, geo.len1())) return SONIC_ERR_INVALID_ARG;
  // the G2 half the way a verifier asks for it (generated on first use where the source still has its trapdoor); a source that cannot
  // supply all four gives a view without one
  uint8_t g2[192 * 4];
  bool with_g2 = sonic_srs_has_g2(srs) != 0;
  const SrsViewG2 q = srs_view_g2(srs->d, n);
  for (int b = 0; b < 2 && with_g2; b++)
    for (int i = 0; i < 2 && with_g2; i++) with_g2 = sonic_srs_get_g2_points(srs, b, q.e[b][i], 1, g2 + 192 * (2 * b + i)) == SONIC_OK;
  std::lock_guard<std::mutex> g(call_mutex());
  hipStream_t st = default_stream();
  std::unique_ptr<sonic_srs> v(srs_alloc_view(srs->d, n, Q));
  const size_t pb = SONIC_SRS_POINT_BYTES;
  for (int b = 0; b < 2; b++) {            // table 0 of both bases, window by window (windows are contiguous in both handles)
    const char* from = srs->basis(b).p;
    char* to = v->basis_mut(b).p;
    HIP_OK(hipMemcpyAsync(to, from + pb * (size_t)srs->geo.slot(geo.lo0), pb * (size_t)geo.len0(), hipMemcpyDeviceToDevice, st));
    if (geo.two()) HIP_OK(hipMemcpyAsync(to + pb * (size_t)geo.len0(), from + pb * (size_t)srs->geo.slot(geo.lo1), pb * (size_t)geo.len1(), hipMemcpyDeviceToDevice, st));
  }
  srs_build_tables(st, v.get());          // (synchronises: the source may be freed from here on)
  if (with_g2) {
    rc = view_attach_g2("sonic_srs_for_circuit", st, v.get(), g2);
    if (rc) return rc;
  }
  *out = v.release();
  API_END
}

int sonic_srs_load_for_circuit(const char* path, int64_t n, int64_t Q, sonic_srs_t** out) { return sonic_srs_load_for_circuit_on(-1, path, n, Q, out); }
int sonic_srs_load_for_circuit_on(int device, const char* path, int64_t n, int64_t Q, sonic_srs_t** out) {
  API_BEGIN_ON(device)
  if (!path || !out) { set_error("sonic_srs_load_for_circuit: bad argument"); return SONIC_ERR_INVALID_ARG; }
  int rc = view_args_ok("sonic_srs_load_for_circuit", SRS_FILE_MAX_D, n, Q);          // (d is the file's to say: srs_view_file_read)
  if (rc) return rc;
  SrsViewFile file;
  std::string why;
  const int frc = srs_view_file_read(path, n, Q, file, why);       // header against the real file size, then only the windows' byte ranges
  if (frc) { set_error("sonic_srs_load_for_circuit: %s", why.c_str()); return frc == 1 || frc == 4 ? SONIC_ERR_INVALID_ARG : SONIC_ERR_BAD_ENCODING; }
  std::lock_guard<std::mutex> g(call_mutex());
  hipStream_t st = default_stream();
  const int64_t d = file.head.d;
  sonic_srs* s = srs_alloc_view(d, n, Q);
  const long npts = s->geo.npts(), hole = s->geo.centre();          // basis 1 has the empty slot e = 0 (SRS.hs:38); basis 0 has none
  DevBuf err(4);
  try {
    if (file.head.compressed) {
      int herr = 0;
      for (int b = 0; b < 2; b++)
        srs_zload_vector(st, file.g[b], 48, npts, b ? hole : -2L, &herr, [&](const uint8_t* in, uint8_t* fl, long i, long m) {
          g1_decompress_enqueue(st, in, s->basis_mut(b) + i, nullptr, fl, m, false);
        });
      HIP_OK(hipMemcpyAsync(err.p, &herr, 4, hipMemcpyHostToDevice, st));
      HIP_OK(hipStreamSynchronize(st));
    } else {
      DevBuf raw(96 * (size_t)npts);
      HIP_OK(hipMemsetAsync(err.p, 0, 4, st));
      for (int b = 0; b < 2; b++) {
        HIP_OK(hipMemcpyAsync(raw.p, file.g[b].data(), 96 * (size_t)npts, hipMemcpyHostToDevice, st));
        points_from_bytes_enqueue(st, raw.as<uint8_t>(), s->basis_mut(b), npts, err.as<int>(), b ? hole : -2L);
      }
      HIP_OK(hipStreamSynchronize(st));
    }
  } catch (...) { delete s; throw; }
  rc = srs_finish_g1("sonic_srs_load_for_circuit", st, s, err, &s);          // r P = O for every point read, then the tables
  if (rc) return rc;
  std::unique_ptr<sonic_srs> v(s);
  if (file.head.has_g2()) {
    if (file.head.compressed) {
      DevBuf h0(sizeof(G2Affine) * 2), h1(sizeof(G2Affine) * 2);
      int herr = 0;
      const std::vector<uint8_t> half[2] = {std::vector<uint8_t>(file.g2.begin(), file.g2.begin() + 192), std::vector<uint8_t>(file.g2.begin() + 192, file.g2.end())};
      for (int b = 0; b < 2; b++)
        srs_zload_vector(st, half[b], 96, 2, -2L, &herr, [&](const uint8_t* in, uint8_t* fl, long i, long m) {
          g2_decompress_enqueue(st, in, (b ? h1 : h0).as<G2Affine>() + i, nullptr, fl, m, true);
        });
      HIP_OK(hipMemcpyAsync(err.p, &herr, 4, hipMemcpyHostToDevice, st));
      HIP_OK(hipStreamSynchronize(st));
      rc = srs_attach_g2("sonic_srs_load_for_circuit", st, v.get(), err, h0, h1);
    } else {
      rc = view_attach_g2("sonic_srs_load_for_circuit", st, v.get(), file.g2.data());
    }
    if (rc) return rc;
  }
  *out = v.release();
  API_END
}

int sonic_srs_windows(const sonic_srs_t* srs, int64_t out[4]) {
  if (!srs || !out) return SONIC_ERR_INVALID_ARG;
  out[0] = srs->geo.lo0; out[1] = srs->geo.hi0; out[2] = srs->geo.lo1; out[3] = srs->geo.hi1;
  return SONIC_OK;
}
int sonic_srs_device_bytes(const sonic_srs_t* srs, size_t* out) {
  if (!srs || !out) return SONIC_ERR_INVALID_ARG;
  *out = srs->g.bytes + srs->ga.bytes + srs->ps.bytes + srs->gs.bytes;
  return SONIC_OK;
}

int sonic_srs_point_bytes(void) { return SONIC_SRS_POINT_BYTES; }

}  // extern "C"
