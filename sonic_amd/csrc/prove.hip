// Host orchestration of the Sonic prover on one MI355X: Sonic.Protocol.prove
// (src/Sonic/Protocol.hs:47-109) with Sonic.Signature.hscProve (src/Sonic/Signature.hs:38-72),
// plus the jobs behind commitPoly and openPoly (their C-ABI faces: poly_api.hip).
//
// Everything between "inputs in HBM" and "7+4Q window-sum slots + 3+2Q field elements in HBM" is
// device work queued with no host synchronisation: the `rnd` draws are explicit (transcript), so no
// step waits for a result.  The main stream builds the polynomials, a side stream the t(X,y) product,
// and the MSMs that depend on one polynomial run as one batched chain on an MSM lane.
// The host then runs the O(W) tails of the MSMs (msm_finish_host) and lays out the proof bytes.
//
// Each reference step is done once: the reference re-evaluates evalY 1 polyR' three times
// (Protocol.hs:63,79,80), evalY y tXY twice (:72,81) and evalY y_j sXY twice per j
// (Signature.hs:41,54).
#include "prover.hpp"
#include "witness_tree.hpp"

namespace sonic {

// How a batched group over large bucket sets (>= 2^18 buckets) that is not the proof's last reduces them by running sums.
// Until round 7 every K-bucket segment multiplied its run by its weight, a ~30-step double-and-add, and K = 64 was the shortest segment
// whose multiple was bearable (15 % of the kernel).  In the two-level form (msm.hip, k_bucket_segments<true>) a segment costs 2 K
// additions and its run 2 more in a small butterfly -- 2 + 2 / K per bucket -- so a short segment is cheap, and it halves the chain a
// wave walks before its slot is free for the accumulation beside it.  ms per streamed proof at n = 2^18, one box, alternating
// (profiles/r07_two_level_reduce.txt, block C): before 34.87; the multiple at K = 32 33.86; two-level at K = 64 / 32  34.84 / 33.46
// (block A / B, two-level: K = 128 38.1, K = 16 34.4).  So: two-level with K = 32 -- for jobs of up to 2^21 terms.  A single n = 2^20
// proof (jobs of up to 7n terms, four times the entries per bucket) measured 1 % SLOWER with either half of that change, so larger
// groups keep the multiple and K = 64, the path they had.  Only two sizes are measured: the bound sits between them.
// SONIC_PROVE_SEGMENT=K (8..1024) and SONIC_PROVE_TWO_LEVEL=0/1 override the two choices: the A/B knobs behind those tables, and how the
// tests reach both forms and the sums over few segments at a small size.  They are read per group and not once per process, because
// the tests switch them inside one process; that is two getenv calls per group, five groups per proof.
constexpr long PROVE_TWO_LEVEL_MAX_TERMS = 1L << 21;
constexpr long POOL_MAX_TERMS = 1L << 21;      // the largest job (T: 7n + 9 terms) of a handle that borrows the device's pooled streams (prover_new_impl)
static bool prove_two_level(const MsmPlan& pl, int k, bool last, long nmax) {
  if (last || k <= 1 || pl.NB < (1 << 18)) return false;
  const char* e = getenv("SONIC_PROVE_TWO_LEVEL");
  if (e && (e[0] == '0' || e[0] == '1') && !e[1]) return e[0] == '1';
  return nmax <= PROVE_TWO_LEVEL_MAX_TERMS;
}
static int prove_segment(const MsmPlan& pl, int k, bool last, bool two_level) {
  const bool big = pl.NB >= (1 << 18);
  if (last) return big ? 16 : 4;
  if (k <= 1) return big ? 8 : 4;
  if (!big) return 16;
  const char* e = getenv("SONIC_PROVE_SEGMENT");
  const int v = e ? atoi(e) : 0;
  return v >= 8 && v <= 1024 ? v : (two_level ? 32 : 64);
}

// commitPoly (CommitmentScheme.hs:20-33): F = sum_e c_e * A[e + d - max], A = alpha basis.
// `poly` dense over exponents [lo, lo+len).  Terms whose shifted exponent leaves [-d, d] or hits the
// e' = 0 hole are legal only if their coefficient is zero (the reference's normalised sparse form
// would not contain them); otherwise FLAG_SRS_INDEX (`index` panics, CommitmentScheme.hs:70-73).
// Queues the checks and returns the MSM that is left to run.
MsmJob commit_job(hipStream_t st, const sonic_srs* srs, const Fr* poly, long lo, long len, long maxm, MsmSlot* slot, int* d_flags) {
  const long d = srs->d, shift = d - maxm;
  long i0 = -d - shift - lo, i1 = d - shift - lo + 1;     // in-range i: lo + i + shift in [-d, d]
  if (i0 < 0) i0 = 0;
  if (i1 > len) i1 = len;
  if (i1 < i0) i1 = i0;
  const PointArray points = srs_job_points("commitPoly", srs, 1, lo + i0 + shift, i1 - i0);      // (a view refuses here, before any launch)
  flag_nonzero_enqueue(st, poly, i0, d_flags, FLAG_SRS_INDEX);
  flag_nonzero_enqueue(st, poly + i1, len - i1, d_flags, FLAG_SRS_INDEX);
  const long ih = -shift - lo;
  if (ih >= i0 && ih < i1) flag_nonzero_enqueue(st, poly + ih, 1, d_flags, FLAG_SRS_INDEX);
  return MsmJob{points, poly + i0, i1 - i0, slot};
}

// The MSMs that become ready together run as one batched kernel chain when the SRS has window tables (msm.hpp);
// otherwise one after the other.
void run_jobs(hipStream_t st, const sonic_srs* srs, MsmWorkspace& ws, const MsmJob* jobs, int k, bool last, bool exposed) {
  if (k <= 0) return;
  long nmax = 0;
  for (int j = 0; j < k; j++) nmax = std::max(nmax, jobs[j].n);
  MsmPlan pl = srs_msm_plan(srs, nmax);
  // Which groups reduce their buckets by the bit-sum butterfly: the group that finishes last, and every group when the caller knows
  // that little else runs beside it (`exposed`: a rank's share of a proof split over many GPUs); the others keep the running sums
  // over K-bucket segments.  The butterfly costs 2 additions per bucket and is one addition deep per level; the segments touch every
  // bucket once, are 2K additions deep and cost 2 + 2 / K in the two-level form (a run and a local total per segment, the runs reduced
  // by a small butterfly of their own: prove_two_level above) or 2 + a ~30-step multiple per segment, 2.35 at K = 64, where every
  // segment multiplies its run (larger groups, and the MSMs that run alone); profiles/r07_two_level_reduce.txt.
  // Butterfly in EVERY group, measured again in round 5 (same box, alternating, ms per proof): streamed 33.76 / 33.91 against
  // 33.67 / 33.76, one at a time 34.75 / 34.98 against 34.21 / 34.50, n = 2^20 127.6 / 127.5 against 126.6 / 127.2 -- not adopted.
  // Small bucket sets (<= 2^17, round 6): always the butterfly.  Their running sums are pure latency -- K = 16 segments and the 256-lane
  // window tree took 0.95 + 0.43 ms per group at 2^16 buckets, whatever ran beside them, against 0.12 + 0.12 ms for the butterfly
  // (profiles/r06_small_proofs.txt) -- and a small proof has little accumulation to hide 1.4 ms under.
  const bool tree = last || exposed || pl.NB <= (1 << 17);
  if (k > 1 && msm_can_batch(pl)) {
    // the group that finishes last reduces with nothing left to hide under: shortest chain instead of least work
    pl.two_level = prove_two_level(pl, k, last, nmax);
    msm_plan_set_segment(pl, prove_segment(pl, k, last, pl.two_level));
    pl.tree = tree;
    msm_enqueue_batch(st, ws, pl, jobs, k, true);
    return;
  }
  for (int j = 0; j < k; j++) {
    MsmPlan p1 = srs_msm_plan(srs, jobs[j].n);
    msm_plan_set_segment(p1, prove_segment(p1, 1, false, false));
    p1.tree = tree;
    msm_enqueue_batch(st, ws, p1, &jobs[j], 1, true);
  }
}

// f(z) for a dense Laurent f: D_e = c_e z^e, inclusive prefix sums, f(z) = last prefix.
static void eval_prefix_enqueue(hipStream_t st, Scratch& sc, const Fr* poly, long lo, long len, const Fr* zpair, Fr* d_fz) {
  sc.reserve(len);
  sc.scan.ensure(sizeof(Fr) * (len / 1024 + 2));
  poly_scale_powers_enqueue(st, poly, sc.D.as<Fr>(), len, lo, zpair, zpair + 1);
  poly_prefix_sum_enqueue(st, sc.D.as<Fr>(), len, sc.scan);
  HIP_OK(hipMemcpyAsync(d_fz, sc.D.as<Fr>() + (len - 1), sizeof(Fr), hipMemcpyDeviceToDevice, st));
}

// the MSM of a quotient q over exponents [lo, lo+len-2], plain basis; coefficients outside [-d, d] must be zero (FLAG_SRS_INDEX)
static MsmJob quotient_job(hipStream_t st, const sonic_srs* srs, const Fr* q, long lo, long len, MsmSlot* slot, int* d_flags) {
  const long d = srs->d, qn = len - 1;
  long i0 = -d - lo, i1 = d - lo + 1;
  if (i0 < 0) i0 = 0;
  if (i1 > qn) i1 = qn;
  if (i1 < i0) i1 = i0;
  const PointArray points = srs_job_points("openPoly", srs, 0, lo + i0, i1 - i0);
  flag_nonzero_enqueue(st, q, i0, d_flags, FLAG_SRS_INDEX);
  flag_nonzero_enqueue(st, q + i1, qn - i1, d_flags, FLAG_SRS_INDEX);
  return MsmJob{points, q + i0, i1 - i0, slot};
}

// openPoly (CommitmentScheme.hs:36-48).  Requires lo <= 0 <= lo+len-1 (callers extend the range to
// contain X^0, where `fX - monomial 0 fz` puts -f(z)).  Quotient exponents [lo, lo+len-2], plain basis.
// Queues evaluation + quotient and returns the MSM that is left to run (its scalars live in `sc` until then).
MsmJob open_job(hipStream_t st, const sonic_srs* srs, Scratch& sc, const Fr* poly, long lo, long len,
                       const Fr* zpair, Fr* d_fz, MsmSlot* slot, int* d_flags) {
  sc.reserve(len);
  eval_prefix_enqueue(st, sc, poly, lo, len, zpair, d_fz ? d_fz : sc.fz_discard.as<Fr>());
  poly_quotient_enqueue(st, sc.D.as<Fr>(), sc.q.as<Fr>(), len, lo, zpair, zpair + 1);
  return quotient_job(st, srs, sc.q.as<Fr>(), lo, len, slot, d_flags);
}

// openPoly at z = 0 of a polynomial without negative exponents (lo == 0): f(0) = c_0 and (f - c_0)/X is the coefficient
// array shifted down by one (CommitmentScheme.hs:43-44 with z = 0).  The prefix-sum form above multiplies by z^{-1-j} and
// cannot express it (0^-1 is not defined; k_fr_with_inverse returns 0 for it).
MsmJob open_job_at_zero(hipStream_t st, const sonic_srs* srs, const Fr* poly, long len, Fr* d_fz, MsmSlot* slot, int* d_flags) {
  const long d = srs->d;
  HIP_OK(hipMemcpyAsync(d_fz, poly, sizeof(Fr), hipMemcpyDeviceToDevice, st));
  const long qn = len - 1;                 // quotient exponents [0, len - 2]
  long i1 = d + 1;
  if (i1 > qn) i1 = qn;
  flag_nonzero_enqueue(st, poly + 1 + i1, qn - i1, d_flags, FLAG_SRS_INDEX);
  return MsmJob{srs_job_points("openPoly", srs, 0, 0, i1), poly + 1, i1, slot};
}

// openPoly for several openings over one exponent range as one batched set of launches (poly.hip, open_batch_enqueue); the jobs
// that are left to run come back in jobs_out, in the order of `ops`
struct PendingOpen { const Fr* poly; long lo, len; const Fr* zp; Fr* fz; MsmSlot* slot; long slot_index; Scratch* sc; };
// entry i of a batch: the opening of `poly` (len coefficients) at zp = {z, z^-1}, worked in `sc`, grown to fit; fz null: f(z) is not kept
static void open_batch_set(OpenBatch& b, int i, Scratch& sc, const Fr* poly, long len, const Fr* zp, Fr* fz) {
  sc.q.ensure(sizeof(Fr) * (len + 1));                   // (no D: the sweeps read the polynomial itself)
  sc.fz_discard.ensure(sizeof(Fr));
  sc.scan.ensure(sizeof(Fr) * open_sweep_entries(len));
  b.poly[i] = poly; b.q[i] = sc.q.as<Fr>(); b.tiles[i] = sc.scan.as<Fr>();
  b.zpair[i] = zp; b.fz[i] = fz ? fz : sc.fz_discard.as<Fr>();
}
static void open_jobs_batched(hipStream_t st, const sonic_srs* srs, const PendingOpen* ops, int k, int* d_flags, MsmJob* jobs_out) {
  for (int at = 0; at < k;) {
    int e = at;
    OpenBatch b;
    memset(&b, 0, sizeof b);
    while (e < k && e - at < OPEN_BATCH_MAX && ops[e].lo == ops[at].lo && ops[e].len == ops[at].len) {
      open_batch_set(b, e - at, *ops[e].sc, ops[e].poly, ops[e].len, ops[e].zp, ops[e].fz);
      e++;
    }
    b.k = e - at;
    const long lo = ops[at].lo, len = ops[at].len;
    open_batch_enqueue(st, b, lo, len);
    for (int i = at; i < e; i++) jobs_out[i] = quotient_job(st, srs, ops[i].sc->q.as<Fr>(), lo, len, ops[i].slot, d_flags);
    at = e;
  }
}

bool bytes_are_zero(const uint8_t* p, size_t n) { for (size_t i = 0; i < n; i++) if (p[i]) return false; return true; }

}  // namespace sonic

int upload_fr_mont(hipStream_t st, DevBuf& dst, const uint8_t* src, long count, int* d_flags) {
  dst.ensure(sizeof(Fr) * (count > 0 ? count : 1));
  if (count > 0) {
    HIP_OK(hipMemcpyAsync(dst.p, src, 32 * count, hipMemcpyHostToDevice, st));
    fr_to_mont_enqueue(st, dst.as<Fr>(), count, d_flags);
  }
  return 0;
}

int flags_to_status(int f, const char* who) {
  if (f & FLAG_BAD_ENCODING) { set_error("%s: non-canonical field element in input", who); return SONIC_ERR_BAD_ENCODING; }
  if (f & FLAG_SRS_INDEX) { set_error("%s: a non-zero coefficient needs an SRS element outside [-d, d] or the omitted g^alpha (index -1)", who); return SONIC_ERR_SRS_INDEX; }
  return SONIC_OK;
}

// the circuit of a handle: uploaded and brought to Montgomery form -- Q x n weights per matrix, or the sparse form (csr.hpp) laid out on
// the host: both orientations and the chunk table -- and Q constants.  A call hands its circuit over (prover_hand_over: p->pend), and
// prover_upload_circuit queues its upload: at once when a handle is made, inside the proof when a one-shot call re-uses a parked shell.
void prover_hand_over(sonic_prover_t* p, const CircuitView& c) {
  p->circuit_has_runs = circuit_runs_hint(c, RUN_TILE);
  p->pend.view = c;
  if (c.csr) csr_layout(c, p->pend.layout);
  p->pend.set = true;
}

static void upload_i32(hipStream_t st, DevBuf& dst, const std::vector<int32_t>& src) {
  dst.ensure(sizeof(int32_t) * (src.empty() ? 1 : src.size()));
  if (!src.empty()) HIP_OK(hipMemcpyAsync(dst.p, src.data(), sizeof(int32_t) * src.size(), hipMemcpyHostToDevice, st));
}
// (flags: non-canonical values.  The host buffers of p->pend are read until `st` has drained: the caller clears it after that)
static void prover_upload_circuit(sonic_prover_t* p, hipStream_t st, int* d_flags) {
  const CircuitView& c = p->pend.view;
  const long n = p->n, Q = p->Q;
  p->have_weights_digest_v2 = false;
  if (c.csr) {
    const CsrLayout& L = p->pend.layout;
    sonic_prover::CsrBufs& b = p->sp;
    upload_i32(st, b.row_ptr, L.row_ptr); upload_i32(st, b.col, L.col);
    upload_i32(st, b.col_ptr, L.col_ptr); upload_i32(st, b.row, L.row);
    upload_i32(st, b.chunk_row, L.chunk_row); upload_i32(st, b.chunk_begin, L.chunk_begin); upload_i32(st, b.row_chunk, L.row_chunk);
    upload_fr_mont(st, b.val, c.val, L.nnz, d_flags);
    upload_fr_mont(st, b.cval, L.cval.data(), L.nnz, d_flags);
    b.nnz = L.nnz;
    b.nchunks = (long)L.chunk_row.size();
    b.partial.ensure(sizeof(Fr) * (b.nchunks > 0 ? b.nchunks : 1));
    b.h_row_ptr = L.row_ptr;
  } else {
    upload_fr_mont(st, p->wL, c.wL, Q * n, d_flags);
    upload_fr_mont(st, p->wR, c.wR, Q * n, d_flags);
    upload_fr_mont(st, p->wO, c.wO, Q * n, d_flags);
  }
  upload_fr_mont(st, p->cs, c.cs, Q, d_flags);
  p->csr = c.csr;
  p->pend.set = false;
}

static int prover_load_circuit(sonic_prover* p, const CircuitView& c) {
  hipStream_t st = p->st;
  prover_hand_over(p, c);
  HIP_OK(hipMemsetAsync(p->flags.p, 0, 4, st));
  prover_upload_circuit(p, st, p->flags.as<int>());
  int f = read_flags(st, p->flags);          // (also: the pageable host buffers of the layout have been read when this returns)
  p->pend = sonic_prover::PendingCircuit();
  if (f) return flags_to_status(f, c.csr ? "sonic_prover_new_csr" : "sonic_prover_new");
  return SONIC_OK;
}

// s(X,y) / s(u,Y) of the handle's circuit, in whichever form it holds it
static void s_of_y_of(sonic_prover* p, hipStream_t st, const Fr* ypow, Fr* out) {
  if (p->csr) s_of_y_csc_enqueue(st, p->sp.col_ptr.as<int32_t>(), p->sp.row.as<int32_t>(), p->sp.cval.as<Fr>(), ypow, p->n, p->Q, out);
  else s_of_y_enqueue(st, p->wL.as<Fr>(), p->wR.as<Fr>(), p->wO.as<Fr>(), ypow, p->n, p->Q, out);
}
static void s_of_u_of(sonic_prover* p, hipStream_t st, const Fr* upow, Fr* out) {
  sonic_prover::CsrBufs& b = p->sp;
  if (p->csr) s_of_u_csr_enqueue(st, b.row_ptr.as<int32_t>(), b.col.as<int32_t>(), b.val.as<Fr>(), b.chunk_row.as<int32_t>(), b.chunk_begin.as<int32_t>(),
                                 b.nchunks, b.row_chunk.as<int32_t>(), upow, p->n, p->Q, out, b.partial.as<Fr>());
  else s_of_u_enqueue(st, p->wL.as<Fr>(), p->wR.as<Fr>(), p->wO.as<Fr>(), upow, p->n, p->Q, out, p->tmp);
}

extern "C" {

size_t sonic_proof_size(int64_t Q) { return ProofLayout{Q}.proof_bytes(); }

static int prover_new_entry(const char* who, const sonic_srs_t* srs, const CircuitView& c, sonic_prover_t** out) {
  API_BEGIN_ON(srs_device(srs))
  if (!srs || !c.cs || !out) { set_error("%s: bad argument (need n >= 1, Q >= 1)", who); return SONIC_ERR_INVALID_ARG; }
  int rc = prover_admits(who, srs, c);
  if (rc) return rc;
  return prover_new_impl(srs, c, out);
  API_END
}
int sonic_prover_new(const sonic_srs_t* srs, int64_t n, int64_t Q, const uint8_t* wL, const uint8_t* wR, const uint8_t* wO,
                     const uint8_t* cs, sonic_prover_t** out) {
  return prover_new_entry("sonic_prover_new", srs, dense_view(n, Q, wL, wR, wO, cs), out);
}
int sonic_prover_new_csr(const sonic_srs_t* srs, int64_t n, int64_t Q, const int64_t* row_ptr, const int64_t* col, const uint8_t* val,
                         const uint8_t* cs, sonic_prover_t** out) {
  return prover_new_entry("sonic_prover_new_csr", srs, csr_view(n, Q, row_ptr, col, val, cs), out);
}

}  // extern "C"

// the circuit's arguments, Protocol.hs:54-55, then the circuit's own checks (csr.hpp), in the order the entry points always had them
int prover_admits(const char* who, const sonic_srs* srs, const CircuitView& c) {
  if (circuit_args_ok(c) && srs->d < 7 * c.n) {
    set_error("Parameter d is not large enough: %ld should be greater than %ld", (long)srs->d, (long)(7 * c.n));
    return SONIC_ERR_D_TOO_SMALL;
  }
  // a view must hold the windows of this circuit (srs_view.hpp): refused here, not in the middle of a proof
  if (circuit_args_ok(c) && srs->is_view() && !srs_view_admits(who, srs, c.n, c.Q)) return SONIC_ERR_INVALID_ARG;
  return circuit_validate(who, c);
}

// (an admitted circuit)
int prover_new_impl(const sonic_srs_t* srs, const CircuitView& c, sonic_prover_t** out, bool own_streams) {
  const long n = c.n, Q = c.Q;
  // what a core proof reads of the transcript, the pairs, the slots and the evaluations: the counts of a proof without pairs.  The first
  // proof with a signature re-creates these buffers for Q pairs (ensure_signature_state)
  const ProofLayout L{0};
  static_assert(ProofLayout{0}.transcript_len() >= ProofLayout::core_transcript_len && ProofLayout{0}.n_pairs() == ProofLayout::core_n_pairs &&
                ProofLayout{0}.slots_total() >= ProofLayout::core_K && ProofLayout{0}.F() == ProofLayout::core_F, "a core proof's prefixes are ProofLayout{0}'s");
  for (long q = 0; c.csr && q < Q; q++) {
    Fr k; memcpy(k.l, c.cs + 32 * q, 32);
    if (!fp_is_canonical(k)) { set_error("sonic_prover_new_csr: non-canonical constant cs[%ld]", q); return SONIC_ERR_BAD_ENCODING; }
  }
  std::unique_ptr<sonic_prover> p(new sonic_prover());
  p->srs = srs; p->n = n; p->Q = Q;
  p->device = srs_device(srs);
  {
    const MsmPlan probe = srs_msm_plan(srs, 3 * n);
    p->small_plan = msm_can_batch(probe) && probe.NB <= (1 << 17);
  }
  p->use_graph = getenv("SONIC_PROVE_GRAPH") && atoi(getenv("SONIC_PROVE_GRAPH")) != 0;
  // the handle's streams: borrowed from the device's pool by role, or its own (prover.hpp, `pooled`)
  // Not the largest proofs.  At n = 2^20 (jobs of 7n terms) every group fills the chip for ~20 ms and the head and tail that the pool
  // orders are 3 % of a proof; what counts there is that one group's sort and reduction run under another's accumulation, a lane per
  // group, and a pool of 4 has two group streams: one proof at a time measured 122.2 ms pooled against 120.0 (n = 2^18: 34.0 against
  // 35.3).  As with PROVE_TWO_LEVEL_MAX_TERMS only these two sizes are measured, and the bound sits between them.  SONIC_STREAM_POOL=k,
  // k > 0, pools every size (the tests force the pool at small sizes either way: they are below the bound).
  const bool pool_size_ok = 7 * n + 9 <= POOL_MAX_TERMS || (getenv("SONIC_STREAM_POOL") && atoi(getenv("SONIC_STREAM_POOL")) > 0);
  p->pooled = !p->use_graph && !own_streams && pool_size_ok && device_prover_streams() > 0;
  auto mkstream = [&p](hipStream_t* s, PoolRole role, int k = 0) {
    if (p->pooled) *s = device_prover_stream(role, k);
    else HIP_OK(hipStreamCreateWithFlags(s, hipStreamNonBlocking));
  };
  mkstream(&p->st, PoolRole::HEAD);
  mkstream(&p->ts, PoolRole::NTT);
  p->tail = p->pooled ? device_prover_stream(PoolRole::TAIL) : p->st;
  hipStream_t st = p->st;
  EnqueueLock enq(p.get());      // (held to the end: the circuit's upload and the first memsets are queued and waited for here)
  p->flags.alloc(8);
  int rc_c = prover_load_circuit(p.get(), c);
  if (rc_c) return rc_c;
  // workspaces
  const long tlen = 7 * n + 9;
  int lg = 0;
  while ((1L << lg) < tlen) lg++;
  p->log2m = lg;
  p->ntt = &device_ntt_tables(lg);
  const long M = 1L << lg;
  p->fa.alloc(sizeof(Fr) * M); p->fb.alloc(sizeof(Fr) * M);
  p->r1.alloc(sizeof(Fr) * (3 * n + 5));
  p->sy0.alloc(sizeof(Fr) * (3 * n + 1));
  // (syj, ev_syj: the Q buffers of 3n + 1 elements and Q events of the signature's pairs are made by ensure_signature_state, on first use)
  p->su.alloc(sizeof(Fr) * (2 * n + Q + 1));
  p->pw.alloc(sizeof(Fr) * (3 * n + Q + 2));
  p->kpow.alloc(sizeof(Fr) * Q);
  p->S.alloc(sizeof(Fr) * L.transcript_len()); p->PAIRS.alloc(sizeof(Fr) * 2 * L.n_pairs());
  p->slots.alloc(sizeof(MsmSlot) * L.slots_total());
  p->pin_tr.alloc(32 * L.transcript_len()); p->pin_pairs.alloc(sizeof(Fr) * 2 * L.n_pairs());
  p->pin_slots.alloc(sizeof(MsmSlot) * L.slots_total()); p->pin_fr.alloc(32 * L.F());
  p->pin_flags.alloc(8); p->pin_root.alloc(32);
  p->h_tr = p->pin_tr.as<uint8_t>(); p->h_pairs = p->pin_pairs.as<Fr>(); p->h_slots = p->pin_slots.as<MsmSlot>(); p->h_fr = p->pin_fr.as<uint8_t>();
  p->h_flags = p->pin_flags.as<int>(); p->h_root = p->pin_root.as<uint32_t>();
  p->h_flags[0] = p->h_flags[1] = 0;
  // (the partial sums of k(y) over many blocks, where the default plan of this Q has any: an enqueue then allocates nothing)
  {
    const KOfYPlan kp = k_of_y_choose(Q);
    if (kp.blocks > 0) p->k_partial.alloc(sizeof(Fr) * (size_t)kp.blocks);
  }
  p->frout.alloc(sizeof(Fr) * L.F());
  p->frstd.alloc(sizeof(Fr) * L.F());
  HIP_OK(hipMemsetAsync(p->frout.p, 0, sizeof(Fr) * L.F(), st));
  HIP_OK(hipMemsetAsync(p->slots.p, 0, sizeof(MsmSlot) * L.slots_total(), st));      // W = 0: an empty sum until the slot's MSM has run
  memset(p->h_slots, 0, sizeof(MsmSlot) * L.slots_total());
  auto mkev = [](hipEvent_t* e) { HIP_OK(hipEventCreateWithFlags(e, hipEventDisableTiming)); };
  mkev(&p->ev_r1); mkev(&p->ev_sy0); mkev(&p->ev_t); mkev(&p->ev_su);
  mkev(&p->done); mkev(&p->ev_head); mkev(&p->ev_ts);
  // MSM workspaces and opening scratch grow on first use: every proof maps the same group of MSMs to the same lane
  if (p->small_plan) {
    const char* le = getenv("SONIC_FUSED_LANES");
    p->n_lanes = std::min(std::max(le ? atoi(le) : N_LANES, 1), N_LANES);      // (lane_at and pick divide by it)
  }
  for (int i = 0; i < p->n_lanes; i++) {
    Lane& l = p->lanes[i];
    // (the last lane in use carries the t group: prover.hpp, t_lane.  On a small-proof handle it only prepares the group's openings for
    // the chain, like the other lanes, and must not sit behind another handle's tail: a GROUP -- stream_pool.hpp -- and the one after
    // the last lane's, which at P = 4 is the group stream that the product does NOT share: there the lanes queued in front of it do not
    // wait for the product, so its openings start the moment the product ends.  On the product's stream, behind two other lanes, one
    // n = 2^14 proof at a time took 3.94 ms against 3.71)
    const bool t_lane = i == p->n_lanes - 1;
    if (t_lane && !p->small_plan) mkstream(&l.st, PoolRole::T_GROUP); else mkstream(&l.st, PoolRole::GROUP, t_lane ? i + 1 : i);
    mkev(&l.done);
    mkev(&l.prep);
  }
  if (p->small_plan) {
    // (the second chain stream is only used by proofs of more than MSM_MAX_JOBS MSMs: Q > 2)
    for (int c = 0; c < (ProofLayout{Q}.K() > MSM_MAX_JOBS ? 2 : 1); c++) {
      mkstream(&p->chain[c].st, PoolRole::CHAIN, c);
      mkev(&p->chain[c].done);
    }
  }
  HIP_OK(hipStreamSynchronize(st));
  *out = p.release();
  return SONIC_OK;
}

// The signature state (prover.hpp, have_signature_state), on first use: everything a proof with a signature needs beyond a core proof's
// prefixes.  The MSM slots 5 and above on the device and pinned on the host (5Q + 8 slots of sizeof(MsmSlot) = 12 304 bytes each: 6.2 GB
// twice for a compiled R1CS of m = 2^15), the transcript, pairs and evaluations beyond 8, 5 and 3 elements, and the per-pair buffers: Q
// buffers of 3n + 1 elements for the s(X, y_j) with the Q events that order their groups (32 Q (3n + 1) bytes).  Called by prove_enqueue,
// before anything of the proof is queued or captured, for every enqueue that is not a core proof's: the handle is never in flight here
// and nothing of an earlier proof is read afterwards, so the buffers are re-created, slots zeroed, as the constructor makes them.
// Everything is acquired first and handed to the handle at the end: a failed allocation frees what it had got and leaves the handle as
// it was, good for core proofs and for another try.
static int ensure_signature_state(sonic_prover_t* p) {
  if (p->have_signature_state) return SONIC_OK;
  const long n = p->n, Q = p->Q;
  const ProofLayout L{Q};
  const size_t each = sizeof(Fr) * (size_t)(3 * n + 1), slot_bytes = sizeof(MsmSlot) * (size_t)L.slots_total();
  DevBuf S, PAIRS, slots, frout, frstd;
  PinnedBuf tr, pairs, hslots, hfr;
  std::vector<DevBuf> syj;
  std::vector<hipEvent_t> ev;
  bool made = false;
  try {
    slots.alloc(slot_bytes);
    hslots.alloc(slot_bytes);
    S.alloc(sizeof(Fr) * (size_t)L.transcript_len()); PAIRS.alloc(sizeof(Fr) * 2 * (size_t)L.n_pairs());
    frout.alloc(sizeof(Fr) * (size_t)L.F()); frstd.alloc(sizeof(Fr) * (size_t)L.F());
    tr.alloc(32 * (size_t)L.transcript_len()); pairs.alloc(sizeof(Fr) * 2 * (size_t)L.n_pairs()); hfr.alloc(32 * (size_t)L.F());
    syj.resize((size_t)Q);
    for (auto& b : syj) b.alloc(each);
    ev.resize((size_t)Q, nullptr);
    for (auto& e : ev) HIP_OK(hipEventCreateWithFlags(&e, hipEventDisableTiming));
    p->slot_ran.reserve((size_t)L.slots_total());
    p->fr_valid.reserve((size_t)L.F());
    {
      EnqueueLock enq(p);
      HIP_OK(hipMemsetAsync(frout.p, 0, sizeof(Fr) * (size_t)L.F(), p->st));
      HIP_OK(hipMemsetAsync(slots.p, 0, slot_bytes, p->st));      // W = 0: an empty sum until the slot's MSM has run
      HIP_OK(hipStreamSynchronize(p->st));
    }
    memset(hslots.p, 0, slot_bytes);
    made = true;
  } catch (const HipFail&) {             // a device or pinned allocation, an event, a memset
  } catch (const std::bad_alloc&) {      // the host vectors themselves
  }
  if (!made) {
    for (hipEvent_t e : ev) if (e) (void)hipEventDestroy(e);
    (void)hipGetLastError();      // (the failed allocation must not surface as the next launch's error)
    set_error("prove: no room for the signature's state: %ld MSM slots of %zu bytes on the device and as many in pinned host memory (%.3f GB each), and Q = %ld "
              "device buffers of %zu bytes, %.3f GB in all (core proofs need none of it)",
              L.slots_total(), sizeof(MsmSlot), (double)slot_bytes / 1e9, Q, each, (double)Q * (double)each / 1e9);
    return SONIC_ERR_HIP;      // (the locals release what they hold)
  }
  p->S = std::move(S); p->PAIRS = std::move(PAIRS); p->slots = std::move(slots); p->frout = std::move(frout); p->frstd = std::move(frstd);
  p->pin_tr = std::move(tr); p->pin_pairs = std::move(pairs); p->pin_slots = std::move(hslots); p->pin_fr = std::move(hfr);
  p->h_tr = p->pin_tr.as<uint8_t>(); p->h_pairs = p->pin_pairs.as<Fr>(); p->h_slots = p->pin_slots.as<MsmSlot>(); p->h_fr = p->pin_fr.as<uint8_t>();
  p->syj = std::move(syj);
  p->ev_syj = std::move(ev);
  p->have_signature_state = true;
  return SONIC_OK;
}

extern "C" {

int sonic_prover_set_assignment(sonic_prover_t* p, const uint8_t* aL, const uint8_t* aR, const uint8_t* aO) {
  API_BEGIN_ON(p ? p->device : -1)
  if (!p || !aL || !aR || !aO) return SONIC_ERR_INVALID_ARG;
  std::lock_guard<std::mutex> g(p->mu);
  if (p->in_flight) { set_error("sonic_prover_set_assignment: a submitted proof is still reading the current assignment (collect it first)"); return SONIC_ERR_INVALID_ARG; }
  hipStream_t st = p->st;
  EnqueueLock enq(p);
  HIP_OK(hipMemsetAsync(p->flags.p, 0, 4, st));
  upload_fr_mont(st, p->aL, aL, p->n, p->flags.as<int>());
  upload_fr_mont(st, p->aR, aR, p->n, p->flags.as<int>());
  upload_fr_mont(st, p->aO, aO, p->n, p->flags.as<int>());
  int f = read_flags(st, p->flags);
  if (f) {
    // the handle's buffers now hold a partly converted assignment: it must not be proven with (a caller that ignores the status and
    // calls prove gets "no assignment set", not a proof of garbage)
    p->have_assignment = false;
    return flags_to_status(f, "sonic_prover_set_assignment");
  }
  p->have_assignment = true;
  p->assignment_changed();
  API_END
}

}  // extern "C"

// ---- the group queue: how a group of MSMs becomes a batch on a lane or on the proof's one chain ---------------------------------------
// The commitments / openings that depend on one polynomial form a group: it runs on the next MSM lane as soon as its input exists
// (event), as ONE batched MSM kernel chain -- or, fused, the lanes only prepare the openings and all jobs of the proof run as one chain
// (prover.hpp).  Results land in disjoint slots / frout entries.  One queue per enqueue; it also cuts every job down to this rank's
// piece of a shared proof and records what ran (slot_ran, fr_valid).
// (packing consecutive groups into ONE batched chain -- fewer, wider chains -- was measured in round 3 and removed in round 5: n = 2^18
// 35.9 / 38.9 ms streamed / one at a time packed against 35.0 / 35.9: the chains of one proof overlap less)
struct GroupQueue {
  sonic_prover_t* const p;
  const sonic_srs* const srs;
  const ProofLayout L;
  int* const flags; MsmSlot* const slots; Fr* const frout;      // the handle's error flags, MSM slots and evaluations (device)
  const SlotShare* const sh;                            // this rank's pieces of the MSMs (share_plan.hpp); nullptr: everything
  Lane* cur = nullptr;
  std::vector<PendingOpen> pend;                        // the openings of the group that is being assembled: evaluated and divided together when the group is flushed
  std::vector<std::function<void()>> after_flush;       // small MSMs that use the lane's workspace after the batch (stream order)
  std::vector<std::function<void()>> deferred_small;    // (fused proofs: the same, queued behind the proof's chain)
  enum Side { BESIDE_GROUP, BEHIND_CHAIN };

  explicit GroupQueue(sonic_prover_t* p_)
      : p(p_), srs(p_->srs), L{p_->Q}, flags(p_->flags.as<int>()), slots(p_->slots.as<MsmSlot>()), frout(p_->frout.as<Fr>()),
        sh(p_->share_world > 1 ? p_->share.row(p_->share_rank) : nullptr) {
    p->next_lane = 0;
    // (a core proof's enqueue marks slots 0 .. 4 and evaluations 0 .. 2 only, and its finish reads neither vector: nothing Q long)
    const ProofLayout V{p->core ? 0 : p->Q};
    p->slot_ran.assign((size_t)V.slots_total(), 0);
    p->fr_valid.assign((size_t)V.F(), 0);
  }
  bool on(int ph) const { return ((p->phases >> ph) & 1u) != 0; }
  bool own(long slot) const { return !sh || sh[slot].hi > sh[slot].lo; }
  bool first_piece(long slot) const { return !sh || (sh[slot].hi > sh[slot].lo && sh[slot].lo == 0); }
  // cuts the job down to this rank's term range and adds what is left of it to the group
  void push(MsmJob job, long slot) {
    if (sh) {
      long t0, t1;
      share_term_range(sh[slot], job.n, &t0, &t1);
      job.points = job.points + t0; job.scalars += t0; job.n = t1 - t0;
      if (job.n <= 0) return;
    }
    p->slot_ran[(size_t)slot] = 1;
    cur->jobs[cur->njobs++] = job;
  }
  void issue_opens() {
    if (pend.empty()) return;
    MsmJob oj[MSM_MAX_JOBS];
    open_jobs_batched(cur->st, srs, pend.data(), (int)pend.size(), flags, oj);
    for (size_t i = 0; i < pend.size(); i++) push(oj[i], pend[i].slot_index);
    pend.clear();
  }
  void flush(bool last = false) {
    if (!cur) return;
    issue_opens();
    if (p->fused) p->fused_jobs.insert(p->fused_jobs.end(), cur->jobs, cur->jobs + cur->njobs);      // run at the end, as one chain
    else run_jobs(cur->st, srs, cur->ws, cur->jobs, cur->njobs, last, /*exposed=*/p->share_world >= 4);
    cur->njobs = 0;
    // the small MSMs beside a group (Q-term sums): at once behind the group's chain -- or, when the proof is ONE chain, after that chain has
    // been queued: they are ~14 launches each whose results are only read at the very end, and on a stream the chain waits for they held its
    // start back by 0.8 ms (n = 2^16 streamed: profiles/r06_streamed_handover.txt)
    if (p->fused) deferred_small.insert(deferred_small.end(), after_flush.begin(), after_flush.end());
    else for (auto& f : after_flush) f();
    after_flush.clear();
  }
  void begin_group(hipEvent_t e) {
    flush();
    cur = &p->pick(e);
    cur->njobs = 0;
  }
  // the t group's lane (prover.hpp, t_lane) takes over without a flush; it waits for the product
  void begin_t_group(Lane& lane_t) {
    if (on(PH_T)) HIP_OK(hipStreamWaitEvent(lane_t.st, p->ev_t, 0));
    cur = &lane_t; cur->njobs = 0;
  }
  void make_room() { if (cur->njobs + (int)pend.size() == MSM_MAX_JOBS) flush(); }
  void commit(int ph, const Fr* poly, long lo, long len, long maxm, long slot) {
    if (!on(ph) || !own(slot)) return;
    make_room();
    push(commit_job(cur->st, srs, poly, lo, len, maxm, &slots[slot], flags), slot);
  }
  // commitPoly with the runs of equal coefficients taken out (S_j of a handle that is not prepared): the flag checks read the
  // coefficients themselves, the large MSM a copy with the uniform tiles zeroed, and a small MSM over gathered running sums -- on the
  // main stream, beside this lane's batch -- adds c (ps[b] - ps[a - 1]) per run
  void commit_runs(int ph, const Fr* poly, long lo, long len, long maxm, long j) {
    const long slot = L.S(j), Q = L.Q;
    if (!on(ph) || !own(slot)) return;
    make_room();
    MsmJob job = commit_job(cur->st, srs, poly, lo, len, maxm, &slots[slot], flags);
    const long ntiles = job.n / RUN_TILE;
    if (ntiles > 0) {
      if ((long)p->runs.size() < Q) p->runs.resize((size_t)Q);
      sonic_prover::RunBufs& rb = p->runs[(size_t)j];
      if (!rb.masked_ev) HIP_OK(hipEventCreateWithFlags(&rb.masked_ev, hipEventDisableTiming));
      rb.masked.ensure(sizeof(Fr) * job.n); rb.val.ensure(sizeof(Fr) * ntiles); rb.uniform.ensure(4 * ntiles);
      rb.scal.ensure(sizeof(Fr) * 2 * ntiles); rb.pts.ensure(sizeof(G1Affine) * 2 * ntiles);
      run_tiles_enqueue(cur->st, job.scalars, job.n, rb.masked.as<Fr>(), rb.val.as<Fr>(), rb.uniform.as<uint32_t>());
      HIP_OK(hipEventRecord(rb.masked_ev, cur->st));
      const long first = (long)((job.points.p - srs->basis(1).p) / (long)job.points.stride);
      sonic_prover::RunBufs* rbp = &rb;
      side([this, rbp, first, ntiles, j] {
        hipStream_t ms = p->st;
        HIP_OK(hipStreamWaitEvent(ms, rbp->masked_ev, 0));
        run_terms_enqueue(ms, rbp->val.as<Fr>(), rbp->uniform.as<uint32_t>(), ntiles, srs->prefix() + first, first, rbp->scal.as<Fr>(), rbp->pts.as<G1Affine>());
        msm_enqueue(ms, p->runs_ws, msm_plan(2 * ntiles), PointArray::packed(rbp->pts.as<G1Affine>()), rbp->scal.as<Fr>(), 2 * ntiles, true, &slots[L.S_extra(j)]);
      }, BEHIND_CHAIN);
      job.scalars = rb.masked.as<Fr>();
      p->slot_ran[(size_t)L.S_extra(j)] = 1;
    }
    push(job, slot);
  }
  // C = commitPoly(s(u,Y)) over the symmetric sums (prover.hpp, sym_on; never a piece of a shared proof): exponents 1 .. n as
  // c_i (A[i] + A[-i]) in the group, exponents n+1 .. n+Q as a Q-term MSM on the main stream (su was built there)
  void commit_sym(int ph, const Fr* su, long lo, long len, long n) {
    if (!on(ph) || !own(L.C())) return;
    const long d = srs->d;
    make_room();
    MsmJob job = commit_job(cur->st, srs, su, lo, len, d, &slots[L.C()], flags);      // (the index checks of the whole range)
    job.points = srs->sym() + 1; job.scalars = su + (n + 1); job.n = n; job.table_stride = srs->geo.sym_n();
    push(job, L.C());
    p->slot_ran[(size_t)L.C_extra()] = 1;
    side([this, su, n] { msm_enqueue(p->st, p->runs_ws, msm_plan(L.Q), srs->basis(1) + srs->geo.slot(n + 1), su + (2 * n + 1), L.Q, true, &slots[L.C_extra()]); }, BEHIND_CHAIN);
  }
  // fr: index of the evaluation in frout (-1: not reported); every rank with a piece of the opening computes it (the quotient
  // needs the prefix sums anyway), the rank whose piece starts at term 0 reports it
  void open(int ph, const Fr* poly, long lo, long len, const Fr* zp, long fr, long slot) {
    if (!on(ph) || !own(slot)) return;
    make_room();
    Scratch& sc = p->fused ? p->fused_scratch() : cur->sc[cur->njobs + (int)pend.size()];
    pend.push_back(PendingOpen{poly, lo, len, zp, fr >= 0 ? &frout[fr] : nullptr, &slots[slot], slot, &sc});
    if (fr >= 0 && first_piece(slot)) p->fr_valid[(size_t)fr] = 1;
  }
  // a small MSM whose result is only read at the very end.  BESIDE_GROUP: at once when the group has been flushed, else behind its batch;
  // BEHIND_CHAIN: at once, or (fused) once the proof's chain has been queued
  void side(std::function<void()> fn, Side when) {
    if (when == BEHIND_CHAIN ? !p->fused : cur->njobs == 0) fn();
    else (when == BEHIND_CHAIN ? deferred_small : after_flush).push_back(std::move(fn));
  }
  // the proof's chain(s): every lane has queued the openings of its groups by now; chunks of at most MSM_MAX_JOBS jobs (one chunk up to
  // Q = 2) on the two chain streams in turn so that two chunks overlap like two groups did
  void run_chains() {
    if (!p->fused || p->fused_jobs.empty()) return;
    for (int i = 0; i < p->n_lanes; i++) HIP_OK(hipEventRecord(p->lanes[i].prep, p->lanes[i].st));
    const int total = (int)p->fused_jobs.size();
    const int nchunks = (total + MSM_MAX_JOBS - 1) / MSM_MAX_JOBS, per = (total + nchunks - 1) / nchunks;
    for (int c = 0, at = 0; c < nchunks; c++, at += per) {
      Lane& cl = p->chain[c & 1];
      if (c < 2) for (int i = 0; i < p->n_lanes; i++) HIP_OK(hipStreamWaitEvent(cl.st, p->lanes[i].prep, 0));
      const int k = std::min(per, total - at);
      const MsmJob* jobs = &p->fused_jobs[(size_t)at];
      long nmax = 0;
      for (int j = 0; j < k; j++) nmax = std::max(nmax, jobs[j].n);
      MsmPlan pl = srs_msm_plan(srs, nmax);
      pl.tree = true;
      pl.accum_block = 128;      // (measured for this chain, n = 2^16 streamed: 128 lanes 9.19-9.27 ms, 256 9.46-9.49, 512 9.42-9.46)
      msm_enqueue_batch(cl.st, cl.ws, pl, jobs, k, true);
    }
    p->fused_jobs.clear();
  }
  void drain_deferred() {
    for (auto& f : deferred_small) f();
    deferred_small.clear();
  }
  // the tail stream (a handle with private streams: its main stream) waits for every stream that carried a part of the proof
  void join() {
    hipStream_t ms = p->tail;
    if (p->pooled) {
      HIP_OK(hipEventRecord(p->ev_head, p->st)); HIP_OK(hipStreamWaitEvent(ms, p->ev_head, 0));
      HIP_OK(hipEventRecord(p->ev_ts, p->ts)); HIP_OK(hipStreamWaitEvent(ms, p->ev_ts, 0));
    }
    for (int i = 0; i < p->n_lanes; i++) { Lane& l = p->lanes[i]; HIP_OK(hipEventRecord(l.done, l.st)); HIP_OK(hipStreamWaitEvent(ms, l.done, 0)); }
    if (p->fused) for (auto& l : p->chain) if (l.st) { HIP_OK(hipEventRecord(l.done, l.st)); HIP_OK(hipStreamWaitEvent(ms, l.done, 0)); }
  }
};

// What one enqueue of a proof works with besides the queue: the exponent ranges of its polynomials, the {v, v^-1} pairs of its
// evaluation points, and which polynomials and groups this rank has a piece of (all of them unless the proof is shared)
struct ProofPass {
  const long n, Q, d;
  const long r_lo, r_len, s_lo, s_len, t_lo, t_len, u_lo, u_len;
  const Fr* const PR;
  bool need_g0, need_T, need_su, need_j_any = false;
  std::vector<uint8_t> need_j;
  long last_j = -1;
  int last_group;                 // the group whose reduction nothing is left to hide under (the t group when this rank has a piece of it)
  bool g0_queued = false;
  const Fr* pair(long i) const { return PR + 2 * i; }
  ProofPass(sonic_prover_t* p, const GroupQueue& q)
      : n(p->n), Q(p->Q), d(p->srs->d), r_lo(ProofLayout::r_lo(n)), r_len(ProofLayout::r_len(n)), s_lo(ProofLayout::s_lo(n)), s_len(ProofLayout::s_len(n)),
        t_lo(ProofLayout::t_lo(n)), t_len(ProofLayout::t_len(n)), u_lo(ProofLayout::u_lo(n)), u_len(q.L.u_len(n)), PR(p->PAIRS.as<Fr>()), need_j(p->core ? 0 : (size_t)Q, 0) {
    const ProofLayout& L = q.L;
    need_su = !p->core && (q.own(L.C()) || q.own(L.Qv()));
    for (long j = 0; j < Q && !p->core; j++) {      // (a core proof has no signature: none of its groups)
      need_j[(size_t)j] = q.own(L.S(j)) || q.own(L.W(j)) || q.own(L.Wp(j));
      need_j_any = need_j_any || need_j[(size_t)j];
      if (need_j[(size_t)j]) last_j = j;
      need_su = need_su || q.own(L.Qj(j));
    }
    need_g0 = q.own(L.R) || q.own(L.Wa) || q.own(L.Wb);
    need_T = q.own(L.T) || q.own(L.Wt);
    last_group = need_T ? 3 : need_su ? 2 : need_j_any ? 1 : 0;
  }
};

// the group that needs nothing but r(X,1): R, (a, W_a), (b, W_b)
static void enqueue_group0(sonic_prover_t* p, GroupQueue& q, ProofPass& w) {
  if (!w.need_g0 || w.g0_queued) return;
  w.g0_queued = true;
  const ProofLayout& L = q.L;
  const Fr* r1 = p->r1.as<Fr>();
  q.begin_group(p->ev_r1);
  q.commit(PH_R, r1, w.r_lo, w.r_len, w.n, L.R);                                       // R            Protocol.hs:63
  q.open(PH_OPEN, r1, w.r_lo, w.r_len, w.pair(L.pZ), L.a, L.Wa);                       // (a, W_a)     :79
  q.open(PH_OPEN, r1, w.r_lo, w.r_len, w.pair(L.pYZ), L.b, L.Wb);                      // (b, W_b)     :80
  q.flush(w.last_group == 0);
}

// ---- all polynomials first (small kernels; queued behind a bucket accumulation they would each wait ~0.5 ms for CUs) ----
// (a polynomial is built in the pass that first knows its challenge -- every pass when phases == PH_ALL -- and stays in the
// handle's buffers for the later passes of sonic_prover_prove_fs: r(X,1) from the blinders, s(X,y) and t(X,y) from y, s(X,y_j)
// from y_j, s(u,Y) from u)
static void enqueue_polynomials(sonic_prover_t* p, GroupQueue& q, ProofPass& w) {
  const ProofLayout& L = q.L;
  const long n = w.n, Q = w.Q;
  hipStream_t ms = p->st;
  int* flags = q.flags;
  Fr *r1 = p->r1.as<Fr>(), *sy = p->sy0.as<Fr>(), *pw = p->pw.as<Fr>(), *fa = p->fa.as<Fr>(), *fb = p->fb.as<Fr>();
  auto ready = [&](hipEvent_t e) { HIP_OK(hipEventRecord(e, ms)); };
  // zkP_1: r'(X,1)                                                                   Protocol.hs:58-63
  if (p->pend_asg[0]) {
    upload_fr_mont(ms, p->aL, p->pend_asg[0], n, flags + 1);
    upload_fr_mont(ms, p->aR, p->pend_asg[1], n, flags + 1);
    upload_fr_mont(ms, p->aO, p->pend_asg[2], n, flags + 1);
    p->pend_asg[0] = nullptr;
    p->assignment_changed();
  }
  if (p->pend_wit.set) {
    // (a witness source: the handle's stream waits for the source's, then ONE launch checks, converts and writes the three arrays)
    for (DevBuf* a : {&p->aL, &p->aR, &p->aO}) a->ensure(sizeof(Fr) * (size_t)n);
    if (p->pend_wit.ready) HIP_OK(hipStreamWaitEvent(ms, p->pend_wit.ready, 0));
    witness_load_enqueue(p, ms, p->pend_wit.v, 1, p->aL.as<Fr>(), p->aR.as<Fr>(), p->aO.as<Fr>(), n, flags + 1);
    p->pend_wit.set = false;
    p->assignment_changed();
  }
  if (p->pend_cs) {
    upload_fr_mont(ms, p->cs, p->pend_cs, Q, flags + 1);
    p->pend_cs = nullptr;
  }
  if ((w.need_g0 || w.need_T) && q.on(PH_R)) build_r1_enqueue(ms, p->aL.as<Fr>(), p->aR.as<Fr>(), p->aO.as<Fr>(), p->S.as<Fr>(), n, r1);
  ready(p->ev_r1);
  // the group that needs nothing but r(X,1): queued here, ahead of the other polynomials, when this call's circuit is still on the host
  if (p->pend.set) {
    enqueue_group0(p, q, w);
    prover_upload_circuit(p, ms, flags + 1);
  }
  // s(X,y)                                                                           Protocol.hs:69-70
  if (w.need_T && q.on(PH_T)) {
    poly_scale_powers_enqueue(ms, nullptr, pw, 2 * n + Q + 1, -n, w.pair(L.pY), w.pair(L.pY) + 1);       // y^e, e in [-n, n+Q]
    s_of_y_of(p, ms, pw, sy);
    HIP_OK(hipMemcpyAsync(p->kpow.p, pw + (2 * n + 1), sizeof(Fr) * Q, hipMemcpyDeviceToDevice, ms));   // y^{n+1..n+Q} for k(y); pw is reused below
  }
  ready(p->ev_sy0);
  if (w.need_T && q.on(PH_T)) {
    // zkP_2: t(X,y) = r(X,1) * (r(X,y) + s(X,y)) - k(y), on its own stream          Protocol.hs:69-73, Constraints.hs:56-68
    hipStream_t ts = p->ts;
    const long M = 1L << p->log2m;
    HIP_OK(hipStreamWaitEvent(ts, p->ev_sy0, 0));          // ev_sy0 follows ev_r1 on the main stream
    t_operands_enqueue(ts, r1, w.r_len, w.r_lo, sy, w.s_lo - w.r_lo, w.s_len, w.pair(L.pY), fa, fb, M);     // fa = r(X,1), fb = r(X,y) + s(X,y), zero-padded
    ntt_forward_enqueue(ts, *p->ntt, fa, p->log2m);
    ntt_forward_enqueue(ts, *p->ntt, fb, p->log2m);
    ntt_inverse_of_product_enqueue(ts, *p->ntt, fa, fb, p->log2m);
    sub_k_of_y_enqueue(ts, fa + (0 - w.t_lo), p->cs.as<Fr>(), p->kpow.as<Fr>(), Q, flags, 0, p->k_plan, p->k_partial.as<Fr>());
    HIP_OK(hipEventRecord(p->ev_t, ts));
  }
  // hscProve: s(X, y_j), s(u, Y)                                                     Signature.hs:41,51
  // (no pair has a piece here -- a core proof, whose handle may not even have the pairs' buffers and events: no per-j work at all.  Nothing
  // waits for an ev_syj[j] but the group of a j that is needed)
  for (long j = 0; w.need_j_any && j < Q; j++) {
    if (w.need_j[(size_t)j] && q.on(PH_HSCS)) {
      poly_scale_powers_enqueue(ms, nullptr, pw, 2 * n + Q + 1, -n, w.pair(L.pYj(j)), w.pair(L.pYj(j)) + 1);
      // a prepared handle that has only a piece of S_j's diagonal part does not read s(X, y_j) itself
      if (!p->prepared || q.own(L.W(j)) || q.own(L.Wp(j))) s_of_y_of(p, ms, pw, p->syj[j].as<Fr>());
      if (p->prepared && q.own(L.S(j))) s_diag_part_enqueue(ms, pw, n, Q, p->diag[j].as<Fr>(), p->yq[j].as<Fr>());
    }
    ready(p->ev_syj[j]);
  }
  if (w.need_su && q.on(PH_HSCW)) {
    poly_scale_powers_enqueue(ms, nullptr, pw, 3 * n + 1, -n, w.pair(L.pU), w.pair(L.pU) + 1);           // u^e, e in [-n, 2n]
    s_of_u_of(p, ms, pw, p->su.as<Fr>());
  }
  ready(p->ev_su);
}

// T and W_t: the group whose polynomial is ready last
static void enqueue_t_group(sonic_prover_t* p, GroupQueue& q, const ProofPass& w, Lane& lane_t) {
  const ProofLayout& L = q.L;
  const Fr* t = p->fa.as<Fr>();                                                        // exponents [t_lo, t_lo + t_len)
  q.begin_t_group(lane_t);
  q.commit(PH_T, t, w.t_lo, w.t_len, w.d, L.T);                                        // T            Protocol.hs:73
  q.open(PH_OPEN, t, w.t_lo, w.t_len, w.pair(L.pZ), -1, L.Wt);                         // W_t          :81
  q.flush(true);
}

// ---- the MSM groups, largest first where its input allows: what the protocol commits to and opens ----
static void enqueue_groups(sonic_prover_t* p, GroupQueue& q, ProofPass& w) {
  const ProofLayout& L = q.L;
  const long n = w.n, Q = w.Q, d = w.d;
  MsmSlot* slots = q.slots;
  Fr* su = p->su.as<Fr>();
  Lane& lane_t = p->t_lane(p->ev_sy0);
  if (q.on(PH_OPEN) && q.first_piece(L.Wt)) {                                          // s(z,y)       :83  (reported by the rank that starts W_t)
    OpenBatch eb;
    memset(&eb, 0, sizeof eb);
    eb.k = 1;
    open_batch_set(eb, 0, lane_t.sc[MSM_MAX_JOBS - 1], p->sy0.as<Fr>(), w.s_len, w.pair(L.pZ), &q.frout[L.s]);
    open_batch_enqueue(lane_t.st, eb, w.s_lo, w.s_len, /*quotient=*/false);
    p->fr_valid[(size_t)L.s] = 1;
  }
  enqueue_group0(p, q, w);
  for (long j = 0; w.need_j_any && j < Q; j++) {
    if (!w.need_j[(size_t)j]) continue;
    Fr* syj = p->syj[j].as<Fr>();
    q.begin_group(p->ev_syj[j]);
    if (p->prepared) q.commit(PH_HSCS, p->diag[j].as<Fr>(), n + 1, n, d, L.S(j));      // S_j (diagonal part)   Signature.hs:42
    else if (p->runs_on) q.commit_runs(PH_HSCS, syj, w.s_lo, w.s_len, d, j);           // S_j, runs through the running sums   :42
    else q.commit(PH_HSCS, syj, w.s_lo, w.s_len, d, L.S(j));                           // S_j                   :42
    q.open(PH_HSCS, syj, w.s_lo, w.s_len, w.pair(L.pZj(j)), L.s_j(j), L.W(j));         // (s_j, W_j)    :43
    q.open(PH_HSCW, syj, w.s_lo, w.s_len, w.pair(L.pU), -1, L.Wp(j));                  // W'_j          :54
    q.flush(w.last_group == 1 && j == w.last_j);
    if (p->prepared && q.on(PH_HSCS) && q.first_piece(L.S(j))) {                       // sum_q y_j^{n+q} C_q, Q-term MSM
      Lane* ln = q.cur;
      p->slot_ran[(size_t)L.S_extra(j)] = 1;
      q.side([p, ln, j, Q, out = &slots[L.S_extra(j)]] {
        msm_enqueue(ln->st, ln->ws, p->cq_tab.p ? msm_plan_tables(Q, CQ_TAB_C, CQ_TAB_W, Q) : msm_plan(Q),
                    PointArray::packed(p->cq_tab.p ? p->cq_tab.as<G1Affine>() : p->cq.as<G1Affine>()), p->yq[j].as<Fr>(), Q, true, out);
      }, GroupQueue::BESIDE_GROUP);
    }
  }
  if (w.need_su) {
    q.begin_group(p->ev_su);
    if (p->sym_on) q.commit_sym(PH_HSCW, su, w.u_lo, w.u_len, n);                      // C             :52, over the symmetric sums
    else q.commit(PH_HSCW, su, w.u_lo, w.u_len, d, L.C());                             // C             :52
    for (long j = 0; j < Q; j++) q.open(PH_HSCW, su, w.u_lo, w.u_len, w.pair(L.pYj(j)), L.sp_j(j), L.Qj(j));   // (s'_j, Q_j) :55
    q.open(PH_QV, su, w.u_lo, w.u_len, w.pair(L.pV), -1, L.Qv());                      // Q_v           :63
  }
  q.flush(w.last_group == 2 && q.sh != nullptr);
  if (w.need_T) enqueue_t_group(p, q, w, lane_t);
  q.run_chains();
  q.drain_deferred();
}

// Everything between "inputs in HBM" and "window-sum slots + evaluations on the host", queued with no host synchronisation: what a
// captured hipGraph replays
// a pooled handle: the assignment of this call goes up on the handle's own upload stream, before the enqueue lock is taken (prover.hpp,
// `up`); it collects its flags in flags[1], which enqueue_proof then leaves alone
static void stage_assignment(sonic_prover_t* p) {
  if (!p->up) {
    HIP_OK(hipStreamCreateWithFlags(&p->up, hipStreamNonBlocking));
    HIP_OK(hipEventCreateWithFlags(&p->ev_up, hipEventDisableTiming));
  }
  int* flags = p->flags.as<int>();
  HIP_OK(hipMemsetAsync(flags + 1, 0, 4, p->up));
  upload_fr_mont(p->up, p->aL, p->pend_asg[0], p->n, flags + 1);
  upload_fr_mont(p->up, p->aR, p->pend_asg[1], p->n, flags + 1);
  upload_fr_mont(p->up, p->aO, p->pend_asg[2], p->n, flags + 1);
  HIP_OK(hipEventRecord(p->ev_up, p->up));
  p->pend_asg[0] = nullptr;
  p->assignment_changed();
  p->asg_staged = true;
}

static void enqueue_proof(sonic_prover_t* p) {
  const ProofLayout L{p->Q};
  hipStream_t st = p->st;
  int* flags = p->flags.as<int>();
  if (p->asg_staged) {
    HIP_OK(hipMemsetAsync(flags, 0, 4, st));
    HIP_OK(hipStreamWaitEvent(st, p->ev_up, 0));
    p->asg_staged = false;
  } else HIP_OK(hipMemsetAsync(flags, 0, 8, st));
  Fr* S = p->S.as<Fr>();
  // (a core proof: its six transcript elements and the five-pair prefix, whatever Q is)
  const long TL = p->core ? L.core_transcript_len : L.transcript_len(), NP = p->core ? L.core_n_pairs : L.n_pairs();
  HIP_OK(hipMemcpyAsync(S, p->h_tr, 32 * TL, hipMemcpyHostToDevice, st));
  fr_to_mont_enqueue(st, S, TL, flags);
  HIP_OK(hipMemcpyAsync(p->PAIRS.p, p->h_pairs, sizeof(Fr) * 2 * NP, hipMemcpyHostToDevice, st));
  GroupQueue q(p);
  ProofPass w(p, q);
  enqueue_polynomials(p, q, w);
  enqueue_groups(p, q, w);
  q.join();
  // the copy-out, behind the join on the tail stream (a pooled handle: not the stream the next proof's head is queued on)
  hipStream_t tl = p->tail;
  Fr* frstd = p->frstd.as<Fr>();
  const long F = p->core ? L.core_F : L.F();
  HIP_OK(hipMemcpyAsync(frstd, q.frout, sizeof(Fr) * F, hipMemcpyDeviceToDevice, tl));
  fr_from_mont_enqueue(tl, frstd, F);
  // (the side slots that this proof's modes fill: the second halves of the S_j, and of C; a core proof: the head's five slots)
  const long KS = p->core ? L.core_K : p->sym_on ? L.slots_total() : (p->prepared || p->runs_on) ? L.C_extra() : L.K();
  HIP_OK(hipMemcpyAsync(p->h_slots, q.slots, sizeof(MsmSlot) * KS, hipMemcpyDeviceToHost, tl));
  HIP_OK(hipMemcpyAsync(p->h_fr, frstd, 32 * F, hipMemcpyDeviceToHost, tl));
  HIP_OK(hipMemcpyAsync(p->h_flags, flags, 8, hipMemcpyDeviceToHost, tl));
  if (p->pooled) HIP_OK(hipEventRecord(p->done, tl));
}

// ---- the per-proof mode decisions ------------------------------------------------------------------------------------------------
static void decide_modes(sonic_prover_t* p) {
  // runs of equal coefficients in S_j go through the running sums of the alpha basis: not for a piece of a shared proof (its term
  // ranges cut the runs), and by default from n = 2^16 (measured, unprepared ms per proof with / without: n = 2^18 32.9 / 36.7,
  // 2^17 19.8 / 20.8, 2^16 12.2 / 12.3, 2^14 6.8 / 6.0 -- below, the extra launches cost more than the additions they save;
  // profiles/r05_runs_ab.txt).  SONIC_PROVE_RUNS=0: never (the plain 3n + 1-term MSM); =1: whenever there are 8 tiles (tests).
  {
    const char* re = getenv("SONIC_PROVE_RUNS");
    const int mode = re ? atoi(re) : -1;
    const bool size_ok = mode == 1 ? 3 * p->n + 1 >= 8 * RUN_TILE : p->n >= (1L << 16);
    p->runs_on = mode != 0 && size_ok && (mode == 1 || p->circuit_has_runs) && !p->prepared && p->share_world <= 1 && p->srs->prefix().p != nullptr;
  }
  {
    // by default from n = 2^17: the Q-term MSM's launches cost a small proof more than n additions save it (ms per proof streamed with /
    // without, profiles/r05_sym_ab.txt: n = 2^20 113.0-113.4 / 115.6-115.7, 2^18 31.35-31.6 / 31.95-32.0, 2^16 11.3-11.5 / 10.9-11.1,
    // 2^14 6.1-6.6 / 5.8-6.1).  SONIC_PROVE_SYM=0: never; =1: always (tests).  Not for a piece of a shared proof (the plan counts C's terms).
    const char* se = getenv("SONIC_PROVE_SYM");
    const int mode = se ? atoi(se) : -1;
    // (round 6, n = 2^16 again, where a proof is one chain now: with / without 9.20-9.25 / 9.08-9.15 ms streamed, 10.44-10.51 / 10.49-10.80
    // one at a time -- still no gain below 2^17; profiles/r06_ab_small_final.txt)
    p->sym_on = mode != 0 && (mode == 1 || p->n >= (1L << 17)) && p->share_world <= 1 && p->srs->sym().p != nullptr && p->n < p->srs->geo.sym_n();
  }
  {
    const MsmPlan probe = srs_msm_plan(p->srs, 3 * p->n);
    const char* fe = getenv("SONIC_PROVE_FUSED");
    const int mode = fe ? atoi(fe) : -1;
    p->fused = mode != 0 && p->small_plan && msm_can_batch(probe) && p->share_world <= 1;
    p->fused_jobs.clear();
    p->fused_sc_next = 0;
  }
  // k(y) in one block or over many (poly.hip, k_of_y_choose).  The partial sums are the handle's; under the default plan they exist since
  // the handle was made, so this grows them only when the knobs ask for more blocks -- here, before anything is queued or captured
  // (a handle that replays a captured proof keeps the plan and the buffer the capture holds)
  if (!p->graph) {
    p->k_plan = k_of_y_choose(p->Q);
    if (p->k_plan.blocks > 0) p->k_partial.ensure(sizeof(Fr) * (size_t)p->k_plan.blocks);
  }
}

// a shared proof's plan, computed when the share or the prepared state changed since the last one
static void share_replan_if_needed(sonic_prover_t* p) {
  if (p->share_world <= 1 || (p->share_planned && p->share_planned_prepared == p->prepared)) return;
  const long n = p->n, Q = p->Q;
  const MsmPlan mp = srs_msm_plan(p->srs, 3 * n);
  const ShareCosts costs = ShareCosts::from_env();
  p->share = share_plan(n, Q, p->prepared, p->share_world, mp.NB, mp.W, costs);
  // what the plan was computed from, as a 32-bit tag in the share header: the plan is a pure function of these, but NB and W come from
  // the rank's own SRS handle (window tables or not: free memory at SRS construction) and the cost constants from its environment --
  // ranks that disagree would report pieces that do not fit together, and sonic_proof_from_shares says so instead of "do not cover"
  uint64_t h = 1469598103934665603ull;
  auto mix = [&](uint64_t v) { for (int i = 0; i < 8; i++) { h ^= (v >> (8 * i)) & 0xff; h *= 1099511628211ull; } };
  auto mixd = [&](double d) { uint64_t v; memcpy(&v, &d, 8); mix(v); };
  mix((uint64_t)n); mix((uint64_t)Q); mix(p->prepared ? 1 : 0); mix((uint64_t)p->share_world); mix((uint64_t)mp.NB); mix((uint64_t)mp.W);
  mixd(costs.per_job_buckets); mixd(costs.r1); mixd(costs.sy); mixd(costs.su); mixd(costs.tprod);
  p->share_plan_tag = (int32_t)(uint32_t)(h ^ (h >> 32));
  p->share_planned = true; p->share_planned_prepared = p->prepared;
}

// {v, v^-1} for v = y, z, yz, u, v, y_1..y_Q, z_1..z_Q (Montgomery form), on the host with one shared inversion: the same
// values cost a proof 0.35 ms of single-thread Fermat inversions on the device before its first polynomial could be built.
// A non-canonical element is flagged by the device's conversion of the transcript; its pair here is then irrelevant.
// A core proof's transcript ends with z: its pairs are y, z and yz, and the five-pair prefix it uploads is completed with {1, 1} for u and
// v, which are never drawn (the values the padded transcript of earlier versions gave them; nothing reads them).
static void challenge_pairs_host(sonic_prover_t* p, const uint8_t* transcript) {
  const ProofLayout L{p->core ? 0 : p->Q};
  const long np = L.n_pairs();
  Fr small[2 * ProofLayout::core_n_pairs];
  std::vector<Fr> big(p->core ? 0 : 2 * (size_t)np);
  Fr* v = p->core ? small : big.data();
  Fr* pre = v + np;
  auto tr = [&](long k) { Fr a; memcpy(a.l, transcript + 32 * k, 32); return fp_to_mont(a); };
  v[L.pY] = tr(L.y); v[L.pZ] = tr(L.z); v[L.pYZ] = fp_mul(v[L.pY], v[L.pZ]);
  if (p->core) v[L.pU] = v[L.pV] = Fr::one();
  else { v[L.pU] = tr(L.u()); v[L.pV] = tr(L.v()); }
  for (long j = 0; j < L.Q; j++) { v[L.pYj(j)] = tr(L.y_j(j)); v[L.pZj(j)] = tr(L.z_j(j)); }
  Fr acc = Fr::one();
  for (long i = 0; i < np; i++) { pre[i] = acc; acc = fp_mul(acc, v[i].is_zero() ? Fr::one() : v[i]); }
  Fr inv = fp_inv(acc);
  for (long i = np - 1; i >= 0; i--) {
    p->h_pairs[2 * i] = v[i];
    if (v[i].is_zero()) { p->h_pairs[2 * i + 1] = v[i]; continue; }
    p->h_pairs[2 * i + 1] = fp_mul(inv, pre[i]);
    inv = fp_mul(inv, v[i]);
  }
}

// prove = prove_enqueue (queues the whole proof on the handle's streams, no host synchronisation) + prove_finish (waits, runs
// the host tails, lays out the bytes).  sonic_prover_prove runs them back to back; sonic_prover_submit / sonic_prover_collect
// expose the halves, so that ONE host thread can keep two handles busy: while it waits for and finishes proof i on one handle,
// proof i + 1 is already running on the other (its polynomial building and sorts fill the first proof's reduction tail).
// Both run under p->mu.
static int prove_enqueue(sonic_prover_t* p, const uint8_t* transcript) {
  API_BEGIN_ON(p->device)
  p->t_begin = std::chrono::steady_clock::now();
  const ProofLayout L{p->Q};
  hipStream_t st = p->st;
  // evaluation points feed `pow x e` with negative e (Utils.hs:18, poly's eval): x = 0 has no inverse
  // (p->core: `transcript` is the six elements of a core proof -- 4 blinders, y, z -- and nothing below reads past them)
  const long TL = p->core ? L.core_transcript_len : L.transcript_len();
  for (long k = L.n_blinders; k < TL; k++)
    if (bytes_are_zero(transcript + 32 * k, 32)) { set_error("prove: transcript element %ld is zero: Laurent evaluation at 0 divides by zero", k); return SONIC_ERR_INEXACT_DIVISION; }
  if (p->share_world > 1 && p->phases != PH_ALL) { set_error("prove: a shared proof runs with a caller-supplied transcript only"); return SONIC_ERR_INVALID_ARG; }
  // (every enqueue of a proof that HAS a signature: its whole-proof enqueue, its share, each of its Fiat-Shamir passes -- those before
  // PH_HSCS too, which still visit the pairs' groups; a core proof's enqueues never)
  if (!p->core) {
    const int rc_sig = ensure_signature_state(p);
    if (rc_sig) return rc_sig;
  }
  decide_modes(p);
  share_replan_if_needed(p);
  memcpy(p->h_tr, transcript, 32 * TL);
  challenge_pairs_host(p, transcript);
  // Launch-bound sizes replay the whole multi-stream enqueue as one hipGraph: captured on the second proof of a handle (the
  // first one grows the workspaces), every address in it is owned by the handle.
  const bool pending = p->pend.set || p->pend_asg[0] != nullptr || p->pend_wit.set || p->pend_cs != nullptr;
  const bool want_graph = p->use_graph && p->proofs_done >= 1 && !profiler().on && p->phases == PH_ALL && !pending;
  const bool replay = want_graph && p->graph != nullptr;
  const bool capturing = want_graph && !replay && !p->graph_tried;
  struct CaptureGuard {        // an error while capturing must not leave the stream in capture mode
    hipStream_t st; bool active = false;
    ~CaptureGuard() { if (active) { hipGraph_t g = nullptr; (void)hipStreamEndCapture(st, &g); if (g) (void)hipGraphDestroy(g); } }
  } capture{st};
  if (capturing) { p->graph_tried = true; HIP_OK(hipStreamBeginCapture(st, hipStreamCaptureModeRelaxed)); capture.active = true; }
  if (p->pooled && p->pend_asg[0]) stage_assignment(p);
  if (!replay) { EnqueueLock enq(p); enqueue_proof(p); }
  if (capturing) {
    hipGraph_t g = nullptr;
    capture.active = false;
    HIP_OK(hipStreamEndCapture(st, &g));
    hipError_t ge = hipGraphInstantiate(&p->graph, g, nullptr, nullptr, 0);
    (void)hipGraphDestroy(g);
    if (ge != hipSuccess) { p->graph = nullptr; set_error("prove: hipGraphInstantiate failed: %s", hipGetErrorString(ge)); return SONIC_ERR_HIP; }
  }
  if (replay || capturing) HIP_OK(hipGraphLaunch(p->graph, st));
  p->t_enq = std::chrono::steady_clock::now();
  API_END
}

// ---- one proof over several GPUs: the share a rank reports and how the shares become the proof ---------------------------------
// share = header (32 B) | K x {lo, hi} pieces (8 B each) | K x 192-B un-normalised partial sums (infinity where the rank has no
// piece) | (3 + 2Q) x 32-B evaluations a, b, s, s_j, s'_j (standard form; zeros unless reported) | (3 + 2Q) x int32 reported
namespace {
struct ShareHeader { uint32_t magic, version; int32_t rank, world; int64_t Q; int32_t flags, plan_tag; };
constexpr uint32_t SHARE_VERSION = 2;      // 2 (round 5): plan_tag in what was padding
constexpr uint32_t SHARE_MAGIC = 0x48534e53u;      // "SNSH"
G1XYZZ g1_sum(const G1XYZZ& a, const G1XYZZ& b) { return g1_add(a, b); }
}
extern "C" size_t sonic_proof_share_size(int64_t Q) {
  const size_t K = (size_t)ProofLayout{Q}.K(), F = (size_t)ProofLayout{Q}.F();
  return sizeof(ShareHeader) + K * 8 + K * 192 + F * 32 + F * 4;
}

// what both finishes open with: wait for the device, count the proof, say where the time went (SONIC_DEBUG_TIMING: returns whether it is set)
static bool await_proof(sonic_prover_t* p, bool share) {
  p->await_done();
  p->proofs_done++;
  if (!getenv("SONIC_DEBUG_TIMING")) return false;
  char who[32] = "prove";
  if (share) snprintf(who, sizeof who, "share %d/%d", p->share_rank, p->share_world);
  fprintf(stderr, "[sonic] %s: enqueue %.3f ms, then waited %.3f ms for the device\n", who,
          std::chrono::duration<double, std::milli>(p->t_enq - p->t_begin).count(),
          std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - p->t_enq).count());
  return true;
}

static int prove_finish_share(sonic_prover_t* p, uint8_t* out_share) {
  API_BEGIN_ON(p->device)
  const long Q = p->Q;
  const ProofLayout L{Q};
  const int K = (int)L.K(), F = (int)L.F();
  await_proof(p, /*share=*/true);
  const MsmSlot* hs = p->h_slots;
  memset(out_share, 0, sonic_proof_share_size(Q));
  ShareHeader h{SHARE_MAGIC, SHARE_VERSION, p->share_rank, p->share_world > 1 ? p->share_world : 1, Q, *p->h_flags, p->share_world > 1 ? p->share_plan_tag : 0};
  memcpy(out_share, &h, sizeof h);
  uint8_t* o = out_share + sizeof h;
  for (int i = 0; i < K; i++) {
    SlotShare s; s.lo = 0; s.hi = SHARE_ONE;
    if (p->share_world > 1) s = p->share.row(p->share_rank)[i];
    memcpy(o, &s.lo, 4); memcpy(o + 4, &s.hi, 4); o += 8;
  }
  // (a slot that did not run in this enqueue is the empty sum here, whatever an earlier proof left in it)
  std::vector<G1XYZZ> sums((size_t)L.slots_total());
  for (long i = 0; i < L.slots_total(); i++) sums[(size_t)i] = p->slot_ran[(size_t)i] ? msm_finish_host(hs[i]) : G1XYZZ::inf();
  fold_side_slots(L, p->prepared || p->runs_on, p->sym_on, sums.data(), sums.data() + K, g1_sum);
  memcpy(o, sums.data(), 192 * (size_t)K);
  o += 192 * (size_t)K;
  for (int i = 0; i < F; i++, o += 32) if (p->fr_valid[(size_t)i]) memcpy(o, p->h_fr + 32 * i, 32);
  for (int i = 0; i < F; i++, o += 4) { const int32_t v = p->fr_valid[(size_t)i]; memcpy(o, &v, 4); }
  API_END
}

// the shares of all ranks -> proof bytes.  Checks that the pieces of every MSM partition its term range and that every evaluation
// was reported; a rank's error flags (non-canonical input, SRS index, unsatisfied circuit) become the status, as in sonic_prove.
extern "C" int sonic_proof_from_shares(int64_t Q, int world, const uint8_t* shares, const uint8_t* transcript, uint8_t* out_proof) {
  try {
  if (Q < 1 || world < 1 || !shares || !transcript || !out_proof) return SONIC_ERR_INVALID_ARG;
  const int K = (int)ProofLayout{Q}.K(), F = (int)ProofLayout{Q}.F();
  const size_t sz = sonic_proof_share_size(Q);
  std::vector<const uint8_t*> by_rank((size_t)world, nullptr);
  int flags = 0;
  int32_t tag0 = 0;
  for (int r = 0; r < world; r++) {
    ShareHeader h;
    memcpy(&h, shares + sz * r, sizeof h);
    if (r == 0) tag0 = h.plan_tag;
    if (h.magic == SHARE_MAGIC && h.version == SHARE_VERSION && h.plan_tag != tag0) {
      set_error("sonic_proof_from_shares: the ranks planned the proof with different parameters (share %d: tag %08x, share 0: %08x) -- their SRS handles "
                "run different MSM plans (window tables built on one GPU and not on another?) or their SONIC_SHARE_COST_* environments differ", r, (unsigned)h.plan_tag, (unsigned)tag0);
      return SONIC_ERR_INVALID_ARG;
    }
    if (h.magic != SHARE_MAGIC || h.version != SHARE_VERSION || h.Q != Q || h.world != world || h.rank < 0 || h.rank >= world || by_rank[(size_t)h.rank]) {
      set_error("sonic_proof_from_shares: share %d is not one of %d distinct shares of a Q = %ld proof", r, world, (long)Q); return SONIC_ERR_INVALID_ARG; }
    by_rank[(size_t)h.rank] = shares + sz * r;
    flags |= h.flags;
  }
  if (flags) return flags_to_status(flags, "prove");
  std::vector<G1XYZZ> sums((size_t)K, G1XYZZ::inf());
  for (int i = 0; i < K; i++) {
    std::vector<std::pair<uint32_t, uint32_t>> pieces;
    for (int r = 0; r < world; r++) {
      const uint8_t* b = by_rank[(size_t)r] + sizeof(ShareHeader);
      uint32_t lo, hi;
      memcpy(&lo, b + 8 * i, 4); memcpy(&hi, b + 8 * i + 4, 4);
      if (hi <= lo) continue;
      pieces.push_back({lo, hi});
      G1XYZZ part;
      memcpy(&part, b + 8 * K + 192 * (size_t)i, 192);
      sums[(size_t)i] = g1_add(sums[(size_t)i], part);
    }
    std::sort(pieces.begin(), pieces.end());
    uint32_t at = 0;
    for (auto& pc : pieces) { if (pc.first != at) break; at = pc.second; }
    if (at != SHARE_ONE) { set_error("sonic_proof_from_shares: the pieces of MSM %d do not cover its terms exactly once", i); return SONIC_ERR_INVALID_ARG; }
  }
  std::vector<uint8_t> pts(96 * (size_t)K), frs(32 * (size_t)F);
  g1_canonical_bytes_host_batch(sums.data(), K, pts.data());
  for (int i = 0; i < F; i++) {
    bool got = false;
    for (int r = 0; r < world && !got; r++) {
      const uint8_t* b = by_rank[(size_t)r] + sizeof(ShareHeader) + 8 * (size_t)K + 192 * (size_t)K;
      int32_t v; memcpy(&v, b + 32 * (size_t)F + 4 * (size_t)i, 4);
      if (v) { memcpy(&frs[32 * (size_t)i], b + 32 * (size_t)i, 32); got = true; }
    }
    if (!got) { set_error("sonic_proof_from_shares: no share reports evaluation %d", i); return SONIC_ERR_INVALID_ARG; }
  }
  proof_layout(Q, pts.data(), frs.data(), transcript, out_proof);
  } catch (const std::exception& e) { set_error("%s", e.what()); return SONIC_ERR_HIP; }
  return SONIC_OK;
}

// host tails: with window tables a slot holds ONE window sum and there is nothing to fold; without them the Horner walks over <= 64
// window sums (255 doublings each) run on up to max_threads threads
static bool slots_folded(const MsmSlot* hs, long K) {
  for (long i = 0; i < K; i++) if (hs[i].W > 1 && hs[i].pad1 == 0) return false;
  return true;
}
// (round 7) a slot of the two-level running sums (pad1 == 3) is a ~14-step walk over bit sums, 35 us: the 13 of a large proof were
// 0.45 ms on one thread, which only a stream of proofs hides.  From eight such slots on they are folded on up to four threads (a
// thread costs about as much to start as one slot to fold).  Fewer, and the butterfly's own slots, stay on the caller's thread as before.
static void finish_slots_host(const MsmSlot* hs, long K, G1XYZZ* out, int max_threads) {
  long two_level = 0;
  for (long i = 0; i < K; i++) two_level += hs[i].pad1 == 3;
  const int nt = !slots_folded(hs, K) ? (int)std::min<long>(K, max_threads) : (two_level >= 8 ? std::min(4, max_threads) : 1);
  ThreadGroup th;
  for (int w = 1; w < nt; w++) th.emplace_back([=] { for (long i = w; i < K; i += nt) out[i] = msm_finish_host(hs[i]); });
  for (long i = 0; i < K; i += nt) out[i] = msm_finish_host(hs[i]);
}

static int prove_finish(sonic_prover_t* p, uint8_t* out_proof) {
  API_BEGIN_ON(p->device)
  const long Q = p->Q;
  const ProofLayout L{Q};
  const int K = (int)L.K();
  const uint8_t* transcript = p->h_tr;
  const bool timing = await_proof(p, /*share=*/false);
  const MsmSlot* hs = p->h_slots;
  const uint8_t* hfr_p = p->h_fr;
  const int hflags = *p->h_flags;
  if (p->h_flags[1]) { p->have_assignment = false; return flags_to_status(p->h_flags[1], "prove (circuit / assignment handed over with the call)"); }
  if (hflags) return flags_to_status(hflags, "prove");
  std::vector<uint8_t> pts(96 * (size_t)K);
  {
    // host tails (finish_slots_host).  One shared inversion normalises all results.
    auto t0 = std::chrono::steady_clock::now();
    std::vector<G1XYZZ> sums((size_t)K);
    // S_j = its slot + its side slot on a prepared handle (sum_q y_j^{n+q} C_q) and on one that takes the runs of equal coefficients
    // out (their small MSM over gathered running sums: per-window sums, a Horner walk).  The side slots persist over the passes of
    // sonic_prover_prove_fs: not tied to this pass's slot_ran; a slot whose MSM never ran is W = 0, the empty sum.
    const bool has_extra = p->prepared || p->runs_on;
    std::vector<G1XYZZ> side((size_t)(Q + 1), G1XYZZ::inf());      // the sums of the side slots: the S_j's, then C's
    const MsmSlot* hx = hs + L.S_extra(0);
    ThreadGroup th;
    // (the Q-term half of C is per-window sums: a Horner walk, on a thread of its own; so are the walks of the S_j's side slots, beside the main thread's tails)
    if (p->sym_on) th.emplace_back([&] { side[(size_t)Q] = msm_finish_host(hs[L.C_extra()]); });
    if (has_extra && !slots_folded(hx, Q)) th.emplace_back([&] { finish_slots_host(hx, Q, side.data(), 8); });
    else if (has_extra) finish_slots_host(hx, Q, side.data(), 1);
    finish_slots_host(hs, K, sums.data(), 16);
    th.join();
    fold_side_slots(L, has_extra, p->sym_on, sums.data(), side.data(), g1_sum);
    g1_canonical_bytes_host_batch(sums.data(), K, pts.data());
    if (timing) fprintf(stderr, "[sonic] host tails of %d MSMs: %.3f ms\n", K, std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count());
  }
  proof_layout(Q, pts.data(), hfr_p, transcript, out_proof);
  API_END
}

// the finish of a CORE proof: the five slots of the head on the caller's thread (no side slots, no thread group), one shared inversion
static int prove_finish_core(sonic_prover_t* p, uint8_t* out_proof) {
  API_BEGIN_ON(p->device)
  await_proof(p, /*share=*/false);
  const MsmSlot* hs = p->h_slots;
  if (p->h_flags[1]) { p->have_assignment = false; return flags_to_status(p->h_flags[1], "prove (circuit / assignment handed over with the call)"); }
  if (p->h_flags[0]) return flags_to_status(p->h_flags[0], "prove");
  G1XYZZ sums[ProofLayout::core_K];
  uint8_t pts[96 * ProofLayout::core_K];
  for (long i = 0; i < ProofLayout::core_K; i++) sums[i] = msm_finish_host(hs[i]);
  g1_canonical_bytes_host_batch(sums, (int)ProofLayout::core_K, pts);
  core_proof_layout(pts, p->h_fr, out_proof);
  API_END
}

extern "C" {

static int whole_proof_only(sonic_prover_t* p, const char* who) {
  if (p->share_world > 1) { set_error("%s: the handle runs one rank's share of a proof (sonic_prover_set_share): use collect_share / prove_share", who); return SONIC_ERR_INVALID_ARG; }
  return SONIC_OK;
}

// a Fiat-Shamir proof in flight (sonic_prover_submit_fs) is collected by sonic_prover_collect_fs only
static int fs_flight_refused(sonic_prover_t* p, const char* who) {
  if (p->fs_flight) { set_error("%s: the proof in flight was submitted with sonic_prover_submit_fs: collect it with sonic_prover_collect_fs", who); return SONIC_ERR_INVALID_ARG; }
  if (p->core_flight) { set_error("%s: the proof in flight was submitted with sonic_prover_submit_core: collect it with sonic_prover_collect_core", who); return SONIC_ERR_INVALID_ARG; }
  return SONIC_OK;
}

static int prove_args_ok(sonic_prover_t* p, const char* who) {
  if (!p->have_assignment) { set_error("%s: no assignment set", who); return SONIC_ERR_INVALID_ARG; }
  if (p->in_flight) { set_error("%s: a submitted proof has not been collected yet", who); return SONIC_ERR_INVALID_ARG; }
  return SONIC_OK;
}

// the tail of every prove call: queue the proof, then `finish` it into `out` (null: leave it in flight, sonic_prover_submit)
static int prove_run(sonic_prover_t* p, const uint8_t* transcript, int (*finish)(sonic_prover_t*, uint8_t*), uint8_t* out) {
  int rc = prove_enqueue(p, transcript);
  if (rc) {      // an enqueue that failed half way: let what was queued drain (a pooled handle: on every stream it may have queued on)
    if (p->st) (void)hipStreamSynchronize(p->st);
    if (p->pooled) {
      (void)hipStreamSynchronize(p->ts); (void)hipStreamSynchronize(p->tail);
      if (p->up) (void)hipStreamSynchronize(p->up);
      p->asg_staged = false;
      for (auto& l : p->lanes) if (l.st) (void)hipStreamSynchronize(l.st);
      for (auto& l : p->chain) if (l.st) (void)hipStreamSynchronize(l.st);
    }
    return rc;
  }
  return finish ? finish(p, out) : SONIC_OK;
}

int sonic_prover_prove(sonic_prover_t* p, const uint8_t* transcript, uint8_t* out_proof) {
  if (!p || !transcript || !out_proof) return SONIC_ERR_INVALID_ARG;
  std::lock_guard<std::mutex> g(p->mu);
  int rc = prove_args_ok(p, "sonic_prover_prove");
  if (!rc) rc = whole_proof_only(p, "sonic_prover_prove");
  if (!rc) rc = prove_run(p, transcript, prove_finish, out_proof);
  return rc;
}

// prove with the assignment of THIS call still in the caller's host buffers (uploaded inside the proof's queue: pend_asg) and its
// constants (pend_cs), either or both
int prove_with_statement(sonic_prover_t* p, const uint8_t* aL, const uint8_t* aR, const uint8_t* aO, const uint8_t* cs, const uint8_t* transcript,
                         uint8_t* out_proof) {
  std::lock_guard<std::mutex> g(p->mu);
  if (p->in_flight) { set_error("prove: a submitted proof has not been collected yet"); return SONIC_ERR_INVALID_ARG; }
  int rc = whole_proof_only(p, "prove");
  if (rc) return rc;
  if (!aL && !p->have_assignment) { set_error("prove: no assignment set"); return SONIC_ERR_INVALID_ARG; }
  if (aL) { p->pend_asg[1] = aR; p->pend_asg[2] = aO; p->pend_asg[0] = aL; }
  p->pend_cs = cs;
  rc = prove_run(p, transcript, prove_finish, out_proof);
  p->pend_asg[0] = nullptr;
  p->pend_cs = nullptr;
  if (aL) p->have_assignment = rc == SONIC_OK;          // (a failed call may have left a partly converted assignment behind)
  return rc;
}

// the same with the assignment of THIS call in a witness source (witness_src.hpp): block 0 of `w`, checked by the caller, read at the
// head of the proof's queue (pend_wit)
int prove_with_witness(sonic_prover_t* p, const WitnessView& w, hipEvent_t ready, const uint8_t* cs, const uint8_t* transcript, uint8_t* out_proof) {
  std::lock_guard<std::mutex> g(p->mu);
  if (p->in_flight) { set_error("prove: a submitted proof has not been collected yet"); return SONIC_ERR_INVALID_ARG; }
  int rc = whole_proof_only(p, "prove");
  if (rc) return rc;
  p->pend_wit.v = w; p->pend_wit.ready = ready; p->pend_wit.set = true;
  p->pend_cs = cs;
  rc = prove_run(p, transcript, prove_finish, out_proof);
  p->pend_wit.set = false;
  p->pend_cs = nullptr;
  p->have_assignment = rc == SONIC_OK;          // (a failed call may have left a refused assignment behind)
  return rc;
}

int sonic_prover_submit(sonic_prover_t* p, const uint8_t* transcript) {
  if (!p || !transcript) return SONIC_ERR_INVALID_ARG;
  std::lock_guard<std::mutex> g(p->mu);
  int rc = prove_args_ok(p, "sonic_prover_submit");
  if (!rc) rc = prove_run(p, transcript, nullptr, nullptr);
  if (!rc) p->in_flight = true;
  return rc;
}

int sonic_prover_collect(sonic_prover_t* p, uint8_t* out_proof) {
  if (!p || !out_proof) return SONIC_ERR_INVALID_ARG;
  std::lock_guard<std::mutex> g(p->mu);
  if (!p->in_flight) { set_error("sonic_prover_collect: nothing was submitted"); return SONIC_ERR_INVALID_ARG; }
  if (fs_flight_refused(p, "sonic_prover_collect")) return SONIC_ERR_INVALID_ARG;
  if (whole_proof_only(p, "sonic_prover_collect")) return SONIC_ERR_INVALID_ARG;
  p->in_flight = false;
  return prove_finish(p, out_proof);
}

// ---- core proofs (include/sonic_hip.h, "Core proofs") -----------------------------------------------------------------------------
// The same enqueue with the phase mask PH_CORE: build_r1, s(X, y), the NTT product, group 0, the t group and s(z, y); no MSM of the
// signature is queued and none of its polynomials built.  The enqueue reads the six transcript elements of the caller and nothing
// behind them (prove_enqueue, enqueue_proof): no host work that grows with Q, and the head's bytes are those of sonic_prover_prove for
// every transcript that starts with these six.
static int prove_core_run(sonic_prover_t* p, const uint8_t* transcript6, uint32_t phases, int (*finish)(sonic_prover_t*, uint8_t*), uint8_t* out) {
  p->phases = phases; p->core = true;
  const int rc = prove_run(p, transcript6, finish, out);
  p->phases = PH_ALL; p->core = false;
  return rc;
}

int sonic_prover_prove_core(sonic_prover_t* p, const uint8_t* transcript, uint8_t* out_proof) {
  if (!p || !transcript || !out_proof) return SONIC_ERR_INVALID_ARG;
  std::lock_guard<std::mutex> g(p->mu);
  int rc = prove_args_ok(p, "sonic_prover_prove_core");
  if (!rc) rc = whole_proof_only(p, "sonic_prover_prove_core");
  if (!rc) rc = prove_core_run(p, transcript, PH_CORE, prove_finish_core, out_proof);
  return rc;
}

int sonic_prover_submit_core(sonic_prover_t* p, const uint8_t* transcript) {
  if (!p || !transcript) return SONIC_ERR_INVALID_ARG;
  std::lock_guard<std::mutex> g(p->mu);
  int rc = prove_args_ok(p, "sonic_prover_submit_core");
  if (!rc) rc = whole_proof_only(p, "sonic_prover_submit_core");
  if (!rc) rc = prove_core_run(p, transcript, PH_CORE, nullptr, nullptr);
  if (!rc) { p->in_flight = true; p->core_flight = true; }
  return rc;
}

int sonic_prover_collect_core(sonic_prover_t* p, uint8_t* out_proof) {
  if (!p || !out_proof) return SONIC_ERR_INVALID_ARG;
  std::lock_guard<std::mutex> g(p->mu);
  if (!p->in_flight) { set_error("sonic_prover_collect_core: nothing was submitted"); return SONIC_ERR_INVALID_ARG; }
  if (!p->core_flight) { set_error("sonic_prover_collect_core: the proof in flight is not a core proof: collect it with the call that belongs to its submit"); return SONIC_ERR_INVALID_ARG; }
  p->in_flight = false; p->core_flight = false;
  return prove_finish_core(p, out_proof);
}

// a core proof with the constants of THIS call and, with w, its assignment from block 0 of a witness source (sonic_prove_batch_core_src)
int prove_core_with_witness(sonic_prover_t* p, const WitnessView* w, hipEvent_t ready, const uint8_t* cs, const uint8_t* transcript, uint8_t* out_proof) {
  std::lock_guard<std::mutex> g(p->mu);
  if (p->in_flight) { set_error("prove: a submitted proof has not been collected yet"); return SONIC_ERR_INVALID_ARG; }
  int rc = whole_proof_only(p, "prove");
  if (rc) return rc;
  if (!w && !p->have_assignment) { set_error("prove: no assignment set"); return SONIC_ERR_INVALID_ARG; }
  if (w) { p->pend_wit.v = *w; p->pend_wit.ready = ready; p->pend_wit.set = true; }
  p->pend_cs = cs;
  rc = prove_core_run(p, transcript, PH_CORE, prove_finish_core, out_proof);
  p->pend_wit.set = false;
  p->pend_cs = nullptr;
  if (w) p->have_assignment = rc == SONIC_OK;          // (a failed call may have left a refused assignment behind)
  return rc;
}

// ONE proof over `world` GPUs (SURVEY 8e "MSM-level parallelism"; BASELINE configs[3] as one n = 2^20 instance on 8 GPUs): every rank
// makes a handle for the same circuit and assignment, calls set_share(rank, world), and then submit + collect_share (or
// prove_share) with the same transcript; the shares are all-gathered (a few KB) and sonic_proof_from_shares turns them into the
// proof on every rank.  world <= 1 restores the whole proof.
int sonic_prover_set_share(sonic_prover_t* p, int rank, int world) {
  API_BEGIN_ON(p ? p->device : -1)
  if (!p || (world > 1 && (rank < 0 || rank >= world))) return SONIC_ERR_INVALID_ARG;
  std::lock_guard<std::mutex> g(p->mu);
  if (p->in_flight) { set_error("sonic_prover_set_share: a submitted proof has not been collected yet"); return SONIC_ERR_INVALID_ARG; }
  if (p->graph) { (void)hipGraphExecDestroy(p->graph); p->graph = nullptr; }
  p->graph_tried = false;
  p->share_rank = world > 1 ? rank : 0;
  p->share_world = world > 1 ? world : 0;
  p->share_planned = false;
  // slots and evaluations of pieces this rank no longer runs must not survive from an earlier proof
  EnqueueLock enq(p);
  // (a handle without the signature state holds a core proof's slots and evaluations only: ProofLayout{0}'s)
  const ProofLayout HL{p->have_signature_state ? p->Q : 0};
  HIP_OK(hipMemsetAsync(p->slots.p, 0, sizeof(MsmSlot) * HL.C_extra(), p->st));      // (all but C's side slot, which a share never fills)
  HIP_OK(hipMemsetAsync(p->frout.p, 0, sizeof(Fr) * HL.F(), p->st));
  HIP_OK(hipStreamSynchronize(p->st));
  API_END
}

int sonic_prover_collect_share(sonic_prover_t* p, uint8_t* out_share) {
  if (!p || !out_share) return SONIC_ERR_INVALID_ARG;
  std::lock_guard<std::mutex> g(p->mu);
  if (!p->in_flight) { set_error("sonic_prover_collect_share: nothing was submitted"); return SONIC_ERR_INVALID_ARG; }
  if (fs_flight_refused(p, "sonic_prover_collect_share")) return SONIC_ERR_INVALID_ARG;
  p->in_flight = false;
  return prove_finish_share(p, out_share);
}

int sonic_prover_prove_share(sonic_prover_t* p, const uint8_t* transcript, uint8_t* out_share) {
  if (!p || !transcript || !out_share) return SONIC_ERR_INVALID_ARG;
  std::lock_guard<std::mutex> g(p->mu);
  int rc = prove_args_ok(p, "sonic_prover_prove_share");
  if (!rc) rc = prove_run(p, transcript, prove_finish_share, out_share);
  return rc;
}

// what the plan gives a rank (host only): K = 7 + 4Q pieces {lo, hi} in units of 1 / 2^20 of each MSM's terms (slot order R, T,
// W_a, W_b, W_t, [S_j, W_j]_j, [W'_j, Q_j]_j, Q_v, C) and the modelled cost in MSM terms.  nb, w: buckets per set and windows of
// the MSM plan (sonic_msm_plan; 0, 0: the defaults of an SRS with window tables, 2^19 and 13).
int sonic_prove_share_plan(int64_t n, int64_t Q, int prepared, int world, int rank, int64_t nb, int w, uint32_t* out_lo_hi, double* out_cost) {
  if (n < 1 || Q < 1 || world < 1 || rank < 0 || rank >= world || !out_lo_hi) return SONIC_ERR_INVALID_ARG;
  const SharePlan pl = share_plan(n, Q, prepared != 0, world, nb > 0 ? nb : (1L << 19), w > 0 ? w : 13, ShareCosts::from_env());
  for (int i = 0; i < pl.K; i++) { out_lo_hi[2 * i] = pl.row(rank)[i].lo; out_lo_hi[2 * i + 1] = pl.row(rank)[i].hi; }
  if (out_cost) *out_cost = pl.cost[(size_t)rank];
  return SONIC_OK;
}

// ---- opt-in Fiat-Shamir transcript (fs.hpp) ----------------------------------------------------------------------
// The challenges of the reference are `rnd` draws made AFTER certain proof elements exist; as hashes of those elements they
// serialise the proof: R -> y -> T -> z -> openings -> y_j, z_j -> S_j.. -> u -> C.. -> v -> Q_v.  sonic_prover_prove_fs walks
// that chain in six passes over the same enqueue (prove_enqueue with one phase bit each): every MSM of the proof still runs
// exactly once and every polynomial is built once, in the pass that first knows its challenge (round 4; it was rebuilt in every pass
// before); between passes the host waits, reads the new elements' canonical bytes and hashes.  The caller-supplied transcript stays the default and fast path (one pass, no waits).
// the statement part of the transcript, once per circuit (circuit_digest, csr.hpp; its sparse twin is in verify.hip)
int sonic_fs_circuit_digest(int64_t n, int64_t Q, const uint8_t* wL, const uint8_t* wR, const uint8_t* wO, const uint8_t* cs, uint8_t out[32]) {
  return circuit_digest_checked("sonic_fs_circuit_digest", dense_view(n, Q, wL, wR, wO, cs), out);
}

int sonic_fs_challenges_v2(int64_t n, int64_t Q, int64_t d, const uint8_t circuit_digest[32], const uint8_t srs_id[32], const uint8_t* proof, uint8_t* out) {
  if (n < 1 || Q < 1 || d < 1 || !circuit_digest || !srs_id || !proof || !out) return SONIC_ERR_INVALID_ARG;
  fs_challenges_of_proof(n, Q, d, circuit_digest, srs_id, proof, out);
  return SONIC_OK;
}
// retired with round 3's prototype: round 4 put srs_id in the middle of the argument list under the same name, so a caller built against
// the older header passed its proof pointer where the srs id is read
int sonic_fs_challenges(int64_t, int64_t, int64_t, const uint8_t*, const uint8_t*, uint8_t*) {
  set_error("sonic_fs_challenges is retired (the transcript binds the SRS since round 4): use sonic_fs_challenges_v2, which takes the srs id");
  return SONIC_ERR_INVALID_ARG;
}

// witness digest v1: SHA-256 of the assignment's canonical bytes, once per set_assignment: the device copy is Montgomery, so a scratch
// copy is converted back and brought to the host
static void witness_digest_v1_ensure(sonic_prover_t* p) {
  if (p->have_witness_digest) return;
  const long n = p->n;
  EnqueueLock enq(p);
  DevBuf tmp(sizeof(Fr) * 3 * n);
  Fr* t3 = tmp.as<Fr>();
  HIP_OK(hipMemcpyAsync(t3, p->aL.p, sizeof(Fr) * n, hipMemcpyDeviceToDevice, p->st));
  HIP_OK(hipMemcpyAsync(t3 + n, p->aR.p, sizeof(Fr) * n, hipMemcpyDeviceToDevice, p->st));
  HIP_OK(hipMemcpyAsync(t3 + 2 * n, p->aO.p, sizeof(Fr) * n, hipMemcpyDeviceToDevice, p->st));
  fr_from_mont_enqueue(p->st, t3, 3 * n);
  std::vector<uint8_t> host(96 * (size_t)n);
  HIP_OK(hipMemcpyAsync(host.data(), t3, host.size(), hipMemcpyDeviceToHost, p->st));
  HIP_OK(hipStreamSynchronize(p->st));
  Sha256 h;
  h.update("sonic-hip/witness/v1", 20);
  h.update(host.data(), host.size());
  h.finish(p->witness_digest);
  p->have_witness_digest = true;
}

// witness digest v2 (fs.hpp): the tree runs on the GPU over the resident assignment (witness.hip), 32 bytes come back.  The two halves:
// queue (behind whatever uploads the assignment on the main stream) and, once the stream has drained, the 60-byte hash over the root.
static void witness_digest_v2_enqueue(sonic_prover_t* p) {
  if (p->have_witness_digest_v2) return;
  const uint32_t* root = witness_tree_enqueue(p->st, p->aL.as<Fr>(), p->aR.as<Fr>(), p->aO.as<Fr>(), p->n, p->wtree);
  HIP_OK(hipMemcpyAsync(p->h_root, root, 32, hipMemcpyDeviceToHost, p->st));
}
static void witness_digest_v2_finish(sonic_prover_t* p) {
  if (p->have_witness_digest_v2) return;
  uint8_t root[32];
  wt_digest_bytes(p->h_root, root);
  fs_witness_digest_v2(p->n, root, p->witness_digest_v2);
  p->have_witness_digest_v2 = true;
}
static void witness_digest_v2_ensure(sonic_prover_t* p) {
  if (p->have_witness_digest_v2) return;
  EnqueueLock enq(p);
  witness_digest_v2_enqueue(p);
  HIP_OK(hipStreamSynchronize(p->st));
  witness_digest_v2_finish(p);
}

// The six passes of a Fiat-Shamir proof: the blinders from `witness_digest` (v1 for the blocking call, v2 for the proofs in flight and the
// batches: the only difference between them), then PH_R .. PH_QV with the host's hashes in between.  The caller has checked the handle
// and holds it: p->mu, or the flight (in_flight, which refuses every other call).  out_transcript may be null.
// A CORE proof (core: fs.hpp, "core proofs") walks the first three passes of the same chain under its own label and ends there: out_proof
// gets its 576 bytes and out_transcript, where given, y and z (64 bytes).
static int prove_fs_walk(sonic_prover_t* p, const uint8_t circuit_digest[32], const uint8_t blinder_seed[32], const uint8_t witness_digest[32], uint8_t* out_proof,
                         uint8_t* out_transcript, bool core = false) {
  int rc;
  const long n = p->n, Q = p->Q, d = p->srs->d;
  const ProofLayout L{Q};
  // (a core proof: its six transcript elements and its 576 bytes, nothing Q long)
  const long TL = core ? L.core_transcript_len : L.transcript_len();
  std::vector<uint8_t> tr(32 * (size_t)TL, 0), pf(core ? L.core_proof_bytes() : sonic_proof_size(Q));
  uint8_t srs_id[32];
  if ((rc = sonic_fs_srs_id(p->srs, srs_id))) return rc;
  for (long k = 0; k < L.n_blinders; k++) fs_blinder(blinder_seed, circuit_digest, srs_id, witness_digest, (uint32_t)k, &tr[32 * k]);
  for (long k = L.n_blinders; k < TL; k++) tr[32 * k] = 1;               // not drawn yet: any invertible value (results that use it are not read)
  FsTranscript t;
  if (core) t.init(n, Q, d, circuit_digest, srs_id, FS_CORE_LABEL);
  else t.init(n, Q, d, circuit_digest, srs_id);
  auto pass = [&](int ph) {
    if (core) return prove_core_run(p, tr.data(), 1u << ph, prove_finish_core, pf.data());
    p->phases = 1u << ph;
    int r = prove_run(p, tr.data(), prove_finish, pf.data());
    p->phases = PH_ALL;
    return r;
  };
  const uint8_t* R = pf.data(), * T = R + 96, * open = R + 192;
  if ((rc = pass(PH_R))) return rc;
  t.absorb("R", R, 96);
  t.challenge("y", 0, &tr[32 * L.y]);
  if ((rc = pass(PH_T))) return rc;
  t.absorb("T", T, 96);
  t.challenge("z", 0, &tr[32 * L.z]);
  if ((rc = pass(PH_OPEN))) return rc;
  if (core) {
    memcpy(out_proof, pf.data(), L.core_proof_bytes());
    if (out_transcript) memcpy(out_transcript, &tr[32 * L.y], 64);
    return SONIC_OK;
  }
  const uint8_t* hscS = R + 576, * hscW = hscS + Q * 224, * Cc = hscW + Q * 224 + 96;
  t.absorb("open", open, 384);
  for (long j = 0; j < Q; j++) { t.challenge("yj", (uint32_t)j, &tr[32 * L.y_j(j)]); t.challenge("zj", (uint32_t)j, &tr[32 * L.z_j(j)]); }
  if ((rc = pass(PH_HSCS))) return rc;
  t.absorb("hscS", hscS, (size_t)Q * 224);
  t.challenge("u", 0, &tr[32 * L.u()]);
  if ((rc = pass(PH_HSCW))) return rc;
  {
    std::string w(reinterpret_cast<const char*>(Cc), 96);
    w.append(reinterpret_cast<const char*>(hscW), (size_t)Q * 224);
    t.absorb("hscW", reinterpret_cast<const uint8_t*>(w.data()), w.size());
  }
  t.challenge("v", 0, &tr[32 * L.v()]);
  if ((rc = pass(PH_QV))) return rc;
  memcpy(out_proof, pf.data(), pf.size());
  if (out_transcript) memcpy(out_transcript, tr.data(), tr.size());
  return SONIC_OK;
}

int sonic_prover_prove_fs(sonic_prover_t* p, const uint8_t circuit_digest[32], const uint8_t blinder_seed[32], uint8_t* out_proof,
                          uint8_t* out_transcript) {
  if (!p || !circuit_digest || !blinder_seed || !out_proof) return SONIC_ERR_INVALID_ARG;
  API_BEGIN_ON(p->device)
  std::lock_guard<std::mutex> g(p->mu);
  int rc = prove_args_ok(p, "sonic_prover_prove_fs");
  if (!rc) rc = whole_proof_only(p, "sonic_prover_prove_fs");
  if (rc) return rc;
  witness_digest_v1_ensure(p);
  return prove_fs_walk(p, circuit_digest, blinder_seed, p->witness_digest, out_proof, out_transcript);
  API_END
}

// the assignment of a Fiat-Shamir proof from block 0 of a witness source, checked by the caller: it goes up at once, with the tree of its
// digest queued right behind it, so that one wait serves both (the caller runs inside API_BEGIN_ON and holds p->mu)
static int fs_take_witness(sonic_prover_t* p, const WitnessView& w, hipEvent_t ready) {
  hipStream_t st = p->st;
  p->have_assignment = false;               // (until the source is known to be good)
  p->assignment_changed();
  for (DevBuf* a : {&p->aL, &p->aR, &p->aO}) a->ensure(sizeof(Fr) * (size_t)p->n);
  {
    EnqueueLock enq(p);
    if (ready) HIP_OK(hipStreamWaitEvent(st, ready, 0));
    HIP_OK(hipMemsetAsync(p->flags.p, 0, 4, st));
    witness_load_enqueue(p, st, w, 1, p->aL.as<Fr>(), p->aR.as<Fr>(), p->aO.as<Fr>(), p->n, p->flags.as<int>());
    witness_digest_v2_enqueue(p);
    const int f = read_flags(st, p->flags);
    if (f) return flags_to_status(f, "prove (assignment handed over with the call)");
  }
  witness_digest_v2_finish(p);
  p->have_assignment = true;
  return SONIC_OK;
}

// a core proof under its own Fiat-Shamir transcript (fs.hpp): three passes, the blinders from witness digest v2 as for the proofs in flight
int sonic_prover_prove_core_fs(sonic_prover_t* p, const uint8_t circuit_digest[32], const uint8_t blinder_seed[32], uint8_t* out_proof, uint8_t* out_yz) {
  if (!p || !circuit_digest || !blinder_seed || !out_proof) return SONIC_ERR_INVALID_ARG;
  API_BEGIN_ON(p->device)
  std::lock_guard<std::mutex> g(p->mu);
  int rc = prove_args_ok(p, "sonic_prover_prove_core_fs");
  if (!rc) rc = whole_proof_only(p, "sonic_prover_prove_core_fs");
  if (rc) return rc;
  witness_digest_v2_ensure(p);
  return prove_fs_walk(p, circuit_digest, blinder_seed, p->witness_digest_v2, out_proof, out_yz, /*core=*/true);
  API_END
}

int sonic_fs_core_challenges(int64_t n, int64_t Q, int64_t d, const uint8_t circuit_digest[32], const uint8_t srs_id[32], const uint8_t* proof, uint8_t* out_yz) {
  if (n < 1 || Q < 1 || d < 1 || !circuit_digest || !srs_id || !proof || !out_yz) return SONIC_ERR_INVALID_ARG;
  fs_core_challenges_of_proof(n, Q, d, circuit_digest, srs_id, proof, out_yz);
  return SONIC_OK;
}

// the same with the constants of THIS call and, with w, the assignment from block 0 of a witness source (sonic_prove_batch_core_fs_src)
int prove_core_fs_with_witness(sonic_prover_t* p, const WitnessView* w, hipEvent_t ready, const uint8_t* cs, const uint8_t circuit_digest[32],
                               const uint8_t blinder_seed[32], uint8_t* out_proof, uint8_t* out_yz) {
  API_BEGIN_ON(p->device)
  std::lock_guard<std::mutex> g(p->mu);
  if (p->in_flight) { set_error("prove: a submitted proof has not been collected yet"); return SONIC_ERR_INVALID_ARG; }
  int rc = whole_proof_only(p, "prove");
  if (rc) return rc;
  if (!w && !p->have_assignment) { set_error("prove: no assignment set"); return SONIC_ERR_INVALID_ARG; }
  if (w) {
    if ((rc = fs_take_witness(p, *w, ready))) return rc;
  } else witness_digest_v2_ensure(p);
  p->pend_cs = cs;
  rc = prove_fs_walk(p, circuit_digest, blinder_seed, p->witness_digest_v2, out_proof, out_yz, /*core=*/true);
  p->pend_cs = nullptr;
  return rc;
  API_END
}

int sonic_prover_witness_digest_v2(sonic_prover_t* p, uint8_t out[32]) {
  API_BEGIN_ON(p ? p->device : -1)
  if (!p || !out) { set_error("sonic_prover_witness_digest_v2: bad argument"); return SONIC_ERR_INVALID_ARG; }
  std::lock_guard<std::mutex> g(p->mu);
  int rc = prove_args_ok(p, "sonic_prover_witness_digest_v2");
  if (rc) return rc;
  witness_digest_v2_ensure(p);
  memcpy(out, p->witness_digest_v2, 32);
  API_END
}

// ---- one Fiat-Shamir proof in flight per handle --------------------------------------------------------------------------------
// submit_fs marks the handle in flight and hands the six passes to the handle's worker thread (prover.hpp, FsWorker); collect_fs waits
// for it.  Between the two, every call that an explicit-transcript flight refuses is refused (they all look at in_flight under p->mu),
// so the worker has the handle to itself without holding the mutex.
static int fs_job(sonic_prover_t* p, FsWorker& w) {
  API_BEGIN_ON(p->device)
  witness_digest_v2_ensure(p);
  return prove_fs_walk(p, w.circuit_digest, w.seed, p->witness_digest_v2, w.proof.data(), w.transcript.data());
  API_END
}
static void fs_worker_main(sonic_prover_t* p) {
  FsWorker& w = *p->fsw;
  std::unique_lock<std::mutex> lk(w.m);
  for (;;) {
    w.cv.wait(lk, [&] { return w.quit || (w.has_job && !w.done); });
    if (!(w.has_job && !w.done)) return;        // (quit: a job that was submitted is still walked to its end first)
    lk.unlock();
    int rc = SONIC_ERR_HIP;
    std::string err;
    try {
      rc = fs_job(p, w);
      if (rc) { char b[512]; sonic_last_error(b, sizeof b); err = b; }
    } catch (...) { rc = SONIC_ERR_HIP; err = "sonic_prover_submit_fs: the worker failed"; }      // (nothing may leave a thread's body: std::terminate)
    lk.lock();
    w.rc = rc; w.err = err; w.done = true;
    w.cv.notify_all();
  }
}

int sonic_prover_submit_fs(sonic_prover_t* p, const uint8_t circuit_digest[32], const uint8_t blinder_seed[32]) {
  API_BEGIN_ON(p ? p->device : -1)
  if (!p || !circuit_digest || !blinder_seed) { set_error("sonic_prover_submit_fs: bad argument"); return SONIC_ERR_INVALID_ARG; }
  std::lock_guard<std::mutex> g(p->mu);
  int rc = prove_args_ok(p, "sonic_prover_submit_fs");
  if (!rc) rc = whole_proof_only(p, "sonic_prover_submit_fs");
  if (rc) return rc;
  if (!p->fsw) {
    p->fsw.reset(new FsWorker());
    p->fsw->th = std::thread(fs_worker_main, p);
  }
  FsWorker& w = *p->fsw;
  {
    std::lock_guard<std::mutex> gw(w.m);
    memcpy(w.circuit_digest, circuit_digest, 32); memcpy(w.seed, blinder_seed, 32);
    w.proof.assign(sonic_proof_size(p->Q), 0);
    w.transcript.assign(32 * (size_t)ProofLayout{p->Q}.transcript_len(), 0);
    w.has_job = true; w.done = false; w.rc = SONIC_OK; w.err.clear();
  }
  p->in_flight = true; p->fs_flight = true;
  w.cv.notify_all();
  API_END
}

int sonic_prover_collect_fs(sonic_prover_t* p, uint8_t* out_proof, uint8_t* out_transcript) {
  API_BEGIN_ON(p ? p->device : -1)
  if (!p || !out_proof) { set_error("sonic_prover_collect_fs: bad argument"); return SONIC_ERR_INVALID_ARG; }
  std::lock_guard<std::mutex> g(p->mu);
  if (!p->in_flight) { set_error("sonic_prover_collect_fs: nothing was submitted"); return SONIC_ERR_INVALID_ARG; }
  if (!p->fs_flight) { set_error("sonic_prover_collect_fs: the proof in flight was submitted with a transcript (sonic_prover_submit): collect it with sonic_prover_collect"); return SONIC_ERR_INVALID_ARG; }
  FsWorker& w = *p->fsw;
  std::unique_lock<std::mutex> lk(w.m);
  w.cv.wait(lk, [&] { return w.done; });
  w.has_job = false;
  p->in_flight = false; p->fs_flight = false;
  if (w.rc) { set_error("%s", w.err.c_str()); return w.rc; }
  memcpy(out_proof, w.proof.data(), w.proof.size());
  if (out_transcript) memcpy(out_transcript, w.transcript.data(), w.transcript.size());
  API_END
}

// a Fiat-Shamir proof with the assignment and the constants of THIS call (sonic_prove_batch_fs).  The assignment goes up at once, not at
// the head of the first pass: its digest decides the blinders, so the tree is queued right behind the upload and one wait serves both.
int prove_fs_with_statement(sonic_prover_t* p, const uint8_t* aL, const uint8_t* aR, const uint8_t* aO, const uint8_t* cs, const uint8_t circuit_digest[32],
                            const uint8_t blinder_seed[32], uint8_t* out_proof, uint8_t* out_transcript) {
  API_BEGIN_ON(p->device)
  std::lock_guard<std::mutex> g(p->mu);
  if (p->in_flight) { set_error("prove: a submitted proof has not been collected yet"); return SONIC_ERR_INVALID_ARG; }
  int rc = whole_proof_only(p, "prove");
  if (rc) return rc;
  if (!aL && !p->have_assignment) { set_error("prove: no assignment set"); return SONIC_ERR_INVALID_ARG; }
  hipStream_t st = p->st;
  if (aL) {
    EnqueueLock enq(p);
    p->have_assignment = false;             // (until the upload is known to be good: a failed one leaves a partly converted assignment)
    p->assignment_changed();
    HIP_OK(hipMemsetAsync(p->flags.p, 0, 4, st));
    upload_fr_mont(st, p->aL, aL, p->n, p->flags.as<int>());
    upload_fr_mont(st, p->aR, aR, p->n, p->flags.as<int>());
    upload_fr_mont(st, p->aO, aO, p->n, p->flags.as<int>());
    witness_digest_v2_enqueue(p);
    const int f = read_flags(st, p->flags);
    if (f) return flags_to_status(f, "prove (assignment handed over with the call)");
    witness_digest_v2_finish(p);
    p->have_assignment = true;
  } else witness_digest_v2_ensure(p);
  p->pend_cs = cs;
  rc = prove_fs_walk(p, circuit_digest, blinder_seed, p->witness_digest_v2, out_proof, out_transcript);
  p->pend_cs = nullptr;
  return rc;
  API_END
}

// the same with the assignment in a witness source: block 0 of `w`, checked by the caller
int prove_fs_with_witness(sonic_prover_t* p, const WitnessView& w, hipEvent_t ready, const uint8_t* cs, const uint8_t circuit_digest[32],
                          const uint8_t blinder_seed[32], uint8_t* out_proof, uint8_t* out_transcript) {
  API_BEGIN_ON(p->device)
  std::lock_guard<std::mutex> g(p->mu);
  if (p->in_flight) { set_error("prove: a submitted proof has not been collected yet"); return SONIC_ERR_INVALID_ARG; }
  int rc = whole_proof_only(p, "prove");
  if (rc) return rc;
  if ((rc = fs_take_witness(p, w, ready))) return rc;
  p->pend_cs = cs;
  rc = prove_fs_walk(p, circuit_digest, blinder_seed, p->witness_digest_v2, out_proof, out_transcript);
  p->pend_cs = nullptr;
  return rc;
  API_END
}

// Circuit-only precomputation for handles that prove more than once: C_q = Commit(d, P_q), P_q the q-th constraint's
// weight polynomial.  Afterwards S_j = Commit(d, s(X, y_j)) (Signature.hs:42) is assembled as
// sum_q y_j^{n+q} C_q + Commit(d, diagonal part): the same group element from an n-term MSM instead of a 3n-term one.
int sonic_prover_prepare(sonic_prover_t* p) {
  API_BEGIN_ON(p ? p->device : -1)
  if (!p) return SONIC_ERR_INVALID_ARG;
  std::lock_guard<std::mutex> g(p->mu);
  if (p->prepared) return SONIC_OK;
  if (p->in_flight) { set_error("sonic_prover_prepare: a submitted proof has not been collected yet"); return SONIC_ERR_INVALID_ARG; }
  if (p->graph) { (void)hipGraphExecDestroy(p->graph); p->graph = nullptr; }     // a captured proof would not know the prepared path
  p->graph_tried = false;
  const long n = p->n, Q = p->Q, d = p->srs->d;
  int* flags = p->flags.as<int>();
  EnqueueLock enq(p);      // (to the end: the rows' MSMs are queued on the lanes and waited for here)
  HIP_OK(hipMemsetAsync(flags, 0, 4, p->st));
  HIP_OK(hipStreamSynchronize(p->st));
  DevBuf slots(sizeof(MsmSlot) * Q);
  std::vector<DevBuf> rows(p->csr ? 0 : std::min<long>(Q, N_LANES));
  for (auto& b : rows) b.alloc(sizeof(Fr) * (3 * n + 1));
  DevBuf terms_pts, terms_scal;
  if (p->csr) {
    // P_q's nnz_q terms only: rows q, Q + q, 2Q + q gathered as (alpha-basis point, value) pairs, one plain MSM each -- instead of the
    // 3n + 1-term MSM over a mostly-zero row.  Their exponents lie in [-n, 2n] without 0, inside [-d, d] (d >= 7n) and off the omitted
    // g^alpha: where the dense path's index checks never fire, and neither do these.  A row without entries commits to the point at
    // infinity (its slot stays the empty sum).
    const std::vector<int32_t>& rp = p->sp.h_row_ptr;
    const long nnz = p->sp.nnz;
    terms_pts.alloc(sizeof(G1Affine) * (nnz > 0 ? nnz : 1));
    terms_scal.alloc(sizeof(Fr) * (nnz > 0 ? nnz : 1));
    HIP_OK(hipMemsetAsync(slots.p, 0, sizeof(MsmSlot) * Q, p->st));
    HIP_OK(hipStreamSynchronize(p->st));
    const PointArray A = p->srs->basis(1) + p->srs->geo.centre();                   // the alpha basis at exponent 0
    long at = 0;
    for (long q = 0; q < Q; q++) {
      const int32_t seg[6] = {rp[q], rp[q + 1] - rp[q], rp[Q + q], rp[Q + q + 1] - rp[Q + q], rp[2 * Q + q], rp[2 * Q + q + 1] - rp[2 * Q + q]};
      const long cnt = (long)seg[1] + seg[3] + seg[5];
      if (cnt == 0) continue;
      Lane& l = p->lane_at((int)(q % N_LANES));
      G1Affine* pts = terms_pts.as<G1Affine>() + at;
      Fr* scal = terms_scal.as<Fr>() + at;
      csr_row_terms_enqueue(l.st, p->sp.col.as<int32_t>(), p->sp.val.as<Fr>(), seg, n, A, pts, scal);
      msm_enqueue(l.st, l.ws, msm_plan(cnt), PointArray::packed(pts), scal, cnt, true, slots.as<MsmSlot>() + q);
      at += cnt;
    }
  }
  for (long q = 0; q < Q && !p->csr; q++) {
    Lane& l = p->lane_at((int)(q % N_LANES));
    Fr* row = rows[q % N_LANES].as<Fr>();
    weight_row_poly_enqueue(l.st, p->wL.as<Fr>(), p->wR.as<Fr>(), p->wO.as<Fr>(), n, q, row);
    MsmJob job = commit_job(l.st, p->srs, row, -n, 3 * n + 1, d, slots.as<MsmSlot>() + q, flags);
    run_jobs(l.st, p->srs, l.ws, &job, 1);
  }
  for (int i = 0; i < p->n_lanes; i++) HIP_OK(hipStreamSynchronize(p->lanes[i].st));
  std::vector<MsmSlot> hs(Q);
  HIP_OK(hipMemcpy(hs.data(), slots.p, sizeof(MsmSlot) * Q, hipMemcpyDeviceToHost));
  int hflags = 0;
  HIP_OK(hipMemcpy(&hflags, flags, 4, hipMemcpyDeviceToHost));
  if (hflags) return flags_to_status(hflags, "sonic_prover_prepare");
  std::vector<G1Affine> cq(Q);
  {
    std::vector<G1XYZZ> sums((size_t)Q);
    finish_slots_host(hs.data(), Q, sums.data(), 16);
    g1_batch_affine_host(sums.data(), Q, cq.data());
  }
  p->cq.alloc(sizeof(G1Affine) * Q);
  HIP_OK(hipMemcpy(p->cq.p, cq.data(), sizeof(G1Affine) * Q, hipMemcpyHostToDevice));
  if (Q <= CQ_TAB_MAX_Q) {
    // tab[w * Q + q] = 2^shift(w) C_q: 255 doublings per C_q, once per circuit, on the host
    std::vector<G1XYZZ> tx((size_t)CQ_TAB_W * Q);
    ThreadGroup th;
    const int nt = (int)std::min<long>(Q, 16);
    for (int t = 0; t < nt; t++)
      th.emplace_back([&, t] {
        for (long q = t; q < Q; q += nt) {
          G1XYZZ a = G1XYZZ::from_affine(cq[q]);
          tx[q] = a;
          for (int w = 1; w < CQ_TAB_W; w++) {
            for (int k = 0; k < msm_even_width(CQ_TAB_W, w - 1); k++) a = g1_dbl(a);
            tx[(size_t)w * Q + q] = a;
          }
        }
      });
    for (auto& x : th) x.join();
    std::vector<G1Affine> tab(tx.size());
    g1_batch_affine_host(tx.data(), (long)tx.size(), tab.data());
    p->cq_tab.alloc(sizeof(G1Affine) * tab.size());
    HIP_OK(hipMemcpy(p->cq_tab.p, tab.data(), sizeof(G1Affine) * tab.size(), hipMemcpyHostToDevice));
  }
  p->diag.resize(Q); p->yq.resize(Q);
  for (auto& b : p->diag) b.alloc(sizeof(Fr) * n);
  for (auto& b : p->yq) b.alloc(sizeof(Fr) * Q);
  // (the rows' MSMs ran in slots of this call's own; the side slots of the S_j that a prepared proof fills belong to the signature state)
  p->prepared = true;
  API_END
}

void sonic_prover_free(sonic_prover_t* p) {
  if (!p) return;
  try { DeviceScope scope(p->device); delete p; } catch (const HipFail&) { delete p; }
}

// The device memory the handle owns at this moment: every DevBuf of the handle, the workspaces and opening scratch of its lanes and
// chains included, as the sizes they were allocated with.  Not counted: what the handle borrows -- the SRS, the device's shared NTT
// tables and pooled streams -- and the temporaries of a call (prepare, hscProve, aggregate), which are gone when it returns.
int sonic_prover_device_bytes(sonic_prover_t* p, int64_t* out) {
  API_BEGIN_ON(p ? p->device : -1)
  if (!p || !out) { set_error("sonic_prover_device_bytes: bad argument"); return SONIC_ERR_INVALID_ARG; }
  std::lock_guard<std::mutex> g(p->mu);
  size_t total = 0;
  auto add = [&total](const DevBuf& b) { total += b.bytes; };
  auto add_ws = [&](const MsmWorkspace& w) {
    for (const DevBuf* b : {&w.count, &w.off, &w.digits, &w.entries, &w.buckets, &w.segres, &w.scan_tmp, &w.order, &w.heavy_meta, &w.heavy_partial, &w.endo_scalars,
                            &w.g2_nchunk, &w.g2_chunk_off, &w.g2_scan_tmp, &w.g2_partial, &w.g2_buckets, &w.g2_segres, &w.g2_sum_tmp, &w.g2_wsum}) add(*b);
  };
  auto add_sc = [&](const Scratch& s) { for (const DevBuf* b : {&s.D, &s.q, &s.scan, &s.fz_discard}) add(*b); };
  auto add_lane = [&](const Lane& l) { add_ws(l.ws); for (const Scratch& s : l.sc) add_sc(s); };
  for (const DevBuf* b : {&p->wL, &p->wR, &p->wO, &p->cs, &p->aL, &p->aR, &p->aO, &p->S, &p->PAIRS, &p->r1, &p->sy0, &p->su, &p->pw, &p->kpow, &p->fa, &p->fb, &p->slots,
                          &p->frout, &p->flags, &p->tmp, &p->wit_raw, &p->frstd, &p->cq, &p->cq_tab, &p->wtree, &p->wdtree, &p->k_partial}) add(*b);
  const sonic_prover::CsrBufs& sp = p->sp;
  for (const DevBuf* b : {&sp.row_ptr, &sp.col, &sp.val, &sp.col_ptr, &sp.row, &sp.cval, &sp.chunk_row, &sp.chunk_begin, &sp.row_chunk, &sp.partial}) add(*b);
  for (const DevBuf* b : {&p->stm.stage, &p->stm.partial, &p->stm.out, &p->stm.gates}) add(*b);
  for (const Lane& l : p->lanes) add_lane(l);
  for (const Lane& l : p->chain) add_lane(l);
  add_ws(p->runs_ws);
  for (const auto& r : p->runs) for (const DevBuf* b : {&r.masked, &r.val, &r.uniform, &r.scal, &r.pts}) add(*b);
  for (const auto& s : p->fused_sc) add_sc(*s);
  for (const std::vector<DevBuf>* v : {&p->syj, &p->diag, &p->yq}) for (const DevBuf& b : *v) add(b);
  *out = (int64_t)total;
  API_END
}

// The pinned host memory the handle owns at this moment, as the sizes it was allocated with: the staging of the transcript, the pairs,
// the MSM slots and the evaluations (a core proof's prefixes until the signature state exists), the flags and the digest root.  Not
// counted: pageable memory (the host vectors of the handle) and the temporaries of a call.
int sonic_prover_host_bytes(sonic_prover_t* p, int64_t* out) {
  API_BEGIN_ON(p ? p->device : -1)
  if (!p || !out) { set_error("sonic_prover_host_bytes: bad argument"); return SONIC_ERR_INVALID_ARG; }
  std::lock_guard<std::mutex> g(p->mu);
  size_t total = 0;
  for (const PinnedBuf* b : {&p->pin_tr, &p->pin_pairs, &p->pin_slots, &p->pin_fr, &p->pin_flags, &p->pin_root}) total += b->bytes;
  *out = (int64_t)total;
  API_END
}

// hscProve :: SRS -> BiVLaurent Fr -> [(Fr, Fr)] -> m HscProof (Signature.hs:32-72) on its own, for the s(X,Y) of the handle's
// circuit (Constraints.hs:34-53) and ANY number m of (y_j, z_j) pairs -- inside prove() m is the number of linear constraints,
// the reference's own test of the sub-protocol (test/Test/Signature.hs:20-36) draws them freely.  u, v are hscProve's two `rnd`
// draws (:48, :60).  Not the hot path (prove() runs these MSMs interleaved with the rest of the proof): one group after the
// other on the handle's main stream, same kernels.  out: [S_j, s_j, W_j]_j, [s'_j, W'_j, Q_j]_j, Q_v, C, u, v.
size_t sonic_hsc_proof_size(int64_t m) { return (size_t)((2 + 4 * m) * 96 + (2 + 2 * m) * 32); }

int sonic_prover_hsc_prove(sonic_prover_t* p, int64_t m, const uint8_t* yzs, const uint8_t u[32], const uint8_t v[32], uint8_t* out) {
  API_BEGIN_ON(p ? p->device : -1)
  if (!p || m < 0 || (m > 0 && !yzs) || !u || !v || !out) return SONIC_ERR_INVALID_ARG;
  std::lock_guard<std::mutex> g(p->mu);
  if (p->in_flight) { set_error("sonic_prover_hsc_prove: a submitted proof has not been collected yet"); return SONIC_ERR_INVALID_ARG; }
  const long n = p->n, Q = p->Q, d = p->srs->d;
  for (long k = 0; k < 2 * m; k++)
    if (bytes_are_zero(yzs + 32 * k, 32)) { set_error("hscProve: y_j / z_j number %ld is zero: Laurent evaluation at 0 divides by zero", k); return SONIC_ERR_INEXACT_DIVISION; }
  if (bytes_are_zero(u, 32) || bytes_are_zero(v, 32)) { set_error("hscProve: u or v is zero"); return SONIC_ERR_INEXACT_DIVISION; }
  hipStream_t st = p->st;
  EnqueueLock enq(p);      // (to the end: everything is queued on the main stream and waited for here)
  const sonic_srs* srs = p->srs;
  const long NS = 2 * m + 2;                                   // scalars: y_1..y_m, z_1..z_m, u, v
  const long K = 4 * m + 2;                                    // MSMs
  DevBuf S(sizeof(Fr) * NS), PR(sizeof(Fr) * 2 * NS), slots(sizeof(MsmSlot) * K), frout(sizeof(Fr) * (2 * m + 1)), flags(4);
  DevBuf pw(sizeof(Fr) * (3 * n + Q + 2)), su(sizeof(Fr) * (2 * n + Q + 1)), sy(sizeof(Fr) * (3 * n + 1));
  int* fl = flags.as<int>();
  HIP_OK(hipMemsetAsync(fl, 0, 4, st));
  {
    std::vector<uint8_t> h(32 * (size_t)NS);
    for (long j = 0; j < m; j++) { memcpy(&h[32 * j], yzs + 64 * j, 32); memcpy(&h[32 * (m + j)], yzs + 64 * j + 32, 32); }
    memcpy(&h[32 * (2 * m)], u, 32); memcpy(&h[32 * (2 * m + 1)], v, 32);
    HIP_OK(hipMemcpyAsync(S.p, h.data(), h.size(), hipMemcpyHostToDevice, st));
    HIP_OK(hipStreamSynchronize(st));
  }
  fr_to_mont_enqueue(st, S.as<Fr>(), NS, fl);
  fr_with_inverse_enqueue(st, S.as<Fr>(), (int)NS, PR.as<Fr>());
  const Fr* P0 = PR.as<Fr>();
  auto pY = [&](long j) { return P0 + 2 * j; };
  auto pZ = [&](long j) { return P0 + 2 * (m + j); };
  const Fr *pU = P0 + 2 * (2 * m), *pV = P0 + 2 * (2 * m + 1);
  MsmSlot* sl = slots.as<MsmSlot>();
  Fr* fo = frout.as<Fr>();
  Lane& lane = p->lane_at(0);
  const long s_lo = -n, s_len = 3 * n + 1, u_lo = -n, u_len = 2 * n + Q + 1;
  // slots: S_j = 3j, W_j = 3j + 1, W'_j = 3j + 2;  Q_j = 3m + j;  Q_v = 4m;  C = 4m + 1.   frout: s_j = j, s'_j = m + j
  for (long j = 0; j < m; j++) {                                                       // Signature.hs:40-45, 54
    poly_scale_powers_enqueue(st, nullptr, pw.as<Fr>(), 2 * n + Q + 1, -n, pY(j), pY(j) + 1);
    s_of_y_of(p, st, pw.as<Fr>(), sy.as<Fr>());
    MsmJob jobs[3];
    jobs[0] = commit_job(st, srs, sy.as<Fr>(), s_lo, s_len, d, &sl[3 * j], fl);
    jobs[1] = open_job(st, srs, lane.sc[1], sy.as<Fr>(), s_lo, s_len, pZ(j), &fo[j], &sl[3 * j + 1], fl);
    jobs[2] = open_job(st, srs, lane.sc[2], sy.as<Fr>(), s_lo, s_len, pU, nullptr, &sl[3 * j + 2], fl);
    run_jobs(st, srs, lane.ws, jobs, 3);
  }
  poly_scale_powers_enqueue(st, nullptr, pw.as<Fr>(), 3 * n + 1, -n, pU, pU + 1);      // u^e, e in [-n, 2n]       :51
  s_of_u_of(p, st, pw.as<Fr>(), su.as<Fr>());
  {
    MsmJob jobs[MSM_MAX_JOBS];
    int k = 0;
    auto flush = [&] { run_jobs(st, srs, lane.ws, jobs, k); k = 0; };
    jobs[k++] = commit_job(st, srs, su.as<Fr>(), u_lo, u_len, d, &sl[4 * m + 1], fl);                               // C    :52
    for (long j = 0; j < m; j++) {                                                                                    // Q_j  :55
      if (k == MSM_MAX_JOBS) flush();
      jobs[k] = open_job(st, srs, lane.sc[k], su.as<Fr>(), u_lo, u_len, pY(j), &fo[m + j], &sl[3 * m + j], fl);
      k++;
    }
    if (k == MSM_MAX_JOBS) flush();
    jobs[k] = open_job(st, srs, lane.sc[k], su.as<Fr>(), u_lo, u_len, pV, &fo[2 * m], &sl[4 * m], fl);               // Q_v  :63
    k++;
    flush();
  }
  fr_from_mont_enqueue(st, fo, 2 * m + 1);
  std::vector<MsmSlot> hs((size_t)K);
  std::vector<uint8_t> hfr(32 * (size_t)(2 * m + 1));
  HIP_OK(hipMemcpyAsync(hs.data(), sl, sizeof(MsmSlot) * K, hipMemcpyDeviceToHost, st));
  HIP_OK(hipMemcpyAsync(hfr.data(), fo, hfr.size(), hipMemcpyDeviceToHost, st));
  int hflags = read_flags(st, flags);
  if (hflags) return flags_to_status(hflags, "hscProve");
  std::vector<uint8_t> pts(96 * (size_t)K);
  {
    std::vector<G1XYZZ> sums((size_t)K);
    finish_slots_host(hs.data(), K, sums.data(), 16);
    g1_canonical_bytes_host_batch(sums.data(), (int)K, pts.data());
  }
  uint8_t* o = out;
  auto putG = [&](long i) { memcpy(o, &pts[96 * (size_t)i], 96); o += 96; };
  auto putF = [&](const uint8_t* b) { memcpy(o, b, 32); o += 32; };
  for (long j = 0; j < m; j++) { putG(3 * j); putF(&hfr[32 * j]); putG(3 * j + 1); }                 // hscS
  for (long j = 0; j < m; j++) { putF(&hfr[32 * (m + j)]); putG(3 * j + 2); putG(3 * m + j); }       // hscW
  putG(4 * m); putG(4 * m + 1); putF(u); putF(v);                                                   // Qv, C, u, v
  API_END
}

}  // extern "C"
