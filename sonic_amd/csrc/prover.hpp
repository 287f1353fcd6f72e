// What the translation units of the prover share (prove.hip: one proof on one handle; prove_multi.hip: the one-shot call and the calls that
// take several handles; poly_api.hip: commitPoly / openPoly / hscProve on caller-supplied polynomials, NTT and dense product): the handle,
// its lanes, the opening scratch, and the helpers that turn a polynomial into the MSM that commits to it or opens it.  Internal: included
// by those three files only (hence the using-directive below).
#pragma once
#include <string.h>
#include <algorithm>
#include <chrono>
#include <condition_variable>
#include <functional>
#include <memory>
#include <thread>
#include <numeric>
#include <string>
#include <vector>
#include "srs_handle.hpp"
#include "poly.hpp"
#include "fs.hpp"
#include "share_plan.hpp"
#include "csr.hpp"
#include "witness_src.hpp"
#include "k_of_y_plan.hpp"
#include "proof_layout.hpp"


namespace sonic {


enum { FLAG_BAD_ENCODING = 1, FLAG_SRS_INDEX = 2 };
// phases of a proof = the points at which the reference's prover draws (Protocol.hs:58,66,76,84-85; Signature.hs:48,60): what can be
// computed once the draws up to there are known
enum { PH_R = 1,      // R                                   (blinders)
       PH_T = 2,      // T                                   (+ y)
       PH_OPEN = 3,   // a, W_a, b, W_b, W_t, s              (+ z)
       PH_HSCS = 4,   // S_j, s_j, W_j                       (+ y_j, z_j)
       PH_HSCW = 5,   // C, s'_j, W'_j, Q_j                  (+ u)
       PH_QV = 6,     // Q_v                                 (+ v)
       PH_ALL = 0x7e,
       PH_CORE = 0x0e };      // R, T and the openings: all of a core proof (include/sonic_hip.h, "Core proofs")
// Buckets per running-sum segment inside prove().  More buckets per segment = fewer small scalar multiplications (less work),
// fewer = shorter dependent chains.  Batched groups hide their chains under other groups' accumulation, so they take the
// work-optimal end; the group that finishes last has nothing left to hide under and takes a short chain.  Measured
// (ms per proof, batched / last): n = 2^18 (2^19 buckets): 16/8 45.9, 32/8 44.3, 64/8 43.2, 64/16 42.6, 64/32 43.7, 128/16 44.6;
// n = 2^16 (2^16 buckets): 4/4 15.7, 8/4 15.1, 16/4 14.95, 16/8 15.1; n = 2^14: 4/4 7.2, 8/4 6.7, 16/4 6.6.
// window tables of the per-circuit commitments C_q (sonic_prover_prepare): 29 windows of 9 / 8 bits over 256 shared buckets
constexpr int CQ_TAB_W = 29, CQ_TAB_C = 9;
constexpr long CQ_TAB_MAX_Q = 1L << 16;
// (sonic_prover_device_bytes, prove.hip, lists these buffers by name: a buffer added here must be added there)
struct Scratch {
  DevBuf D, q, scan, fz_discard;
  void reserve(long len) { D.ensure(sizeof(Fr) * (len + 1)); q.ensure(sizeof(Fr) * (len + 1)); fz_discard.ensure(sizeof(Fr)); }
};

// (prove.hip)
MsmJob commit_job(hipStream_t st, const sonic_srs* srs, const Fr* poly, long lo, long len, long maxm, MsmSlot* slot, int* d_flags);
void run_jobs(hipStream_t st, const sonic_srs* srs, MsmWorkspace& ws, const MsmJob* jobs, int k, bool last = false, bool exposed = true);
MsmJob open_job(hipStream_t st, const sonic_srs* srs, Scratch& sc, const Fr* poly, long lo, long len,
                       const Fr* zpair, Fr* d_fz, MsmSlot* slot, int* d_flags);
MsmJob open_job_at_zero(hipStream_t st, const sonic_srs* srs, const Fr* poly, long len, Fr* d_fz, MsmSlot* slot, int* d_flags);
bool bytes_are_zero(const uint8_t* p, size_t n);

}  // namespace sonic

using namespace sonic;

// pinned host memory of a handle, counted by sonic_prover_host_bytes as the size it was allocated with (DevBuf's twin)
struct PinnedBuf {
  void* p = nullptr; size_t bytes = 0;
  PinnedBuf() {}
  PinnedBuf(const PinnedBuf&) = delete; PinnedBuf& operator=(const PinnedBuf&) = delete;
  PinnedBuf& operator=(PinnedBuf&& o) noexcept { if (this != &o) { release(); p = o.p; bytes = o.bytes; o.p = nullptr; o.bytes = 0; } return *this; }
  ~PinnedBuf() { release(); }
  void alloc(size_t n) { release(); HIP_OK(hipHostMalloc(&p, n, hipHostMallocDefault)); bytes = n; }
  void release() { if (p) { (void)hipHostFree(p); p = nullptr; bytes = 0; } }
  template <class T> T* as() const { return reinterpret_cast<T*>(p); }
};

// One MSM "lane": its own stream, bucket workspace and opening scratch.  The MSMs of a proof that depend on the same
// polynomial form a group (R, W_a, W_b | T, W_t | S_j, W_j, W'_j | C, Q_j.., Q_v) that runs on one lane as ONE batched
// kernel chain (msm_enqueue_batch); different groups run on different lanes so that one group's sort and reduction
// phases run under another's accumulation.
struct Lane {
  hipStream_t st = nullptr;
  hipEvent_t done = nullptr;
  hipEvent_t prep = nullptr;     // fused proofs: the lane's openings (evaluation, quotient) are queued; the proof's ONE chain waits for it
  MsmWorkspace ws;
  Scratch sc[MSM_MAX_JOBS];       // one per opening of the group in flight (grown on first use)
  MsmJob jobs[MSM_MAX_JOBS];
  int njobs = 0;
};
constexpr int N_LANES = 6;

// One Fiat-Shamir proof in flight (sonic_prover_submit_fs / collect_fs): the host thread that walks the six passes for the handle while the
// submitting thread goes on -- it waits for the device between passes, runs the host tails and hashes, so another handle's kernels fill
// the GPU meanwhile.  Made on the first submit_fs, joined when the handle is freed.  `m` guards everything below it.
struct FsWorker {
  std::thread th;
  std::mutex m;
  std::condition_variable cv;
  bool has_job = false, done = false, quit = false;
  uint8_t circuit_digest[32], seed[32];
  int rc = 0;
  std::string err;                             // the job's error text: set_error is per thread, collect_fs hands it to its caller
  std::vector<uint8_t> proof, transcript;
};

// Every DevBuf below -- directly, in CsrBufs, StatementBufs, RunBufs, the lanes and chains, the vectors -- is counted by
// sonic_prover_device_bytes (prove.hip), which names them one by one: a device buffer added to the handle must be added to that list,
// or the handle under-reports what it owns.
struct sonic_prover {
  const sonic_srs* srs = nullptr;
  int device = 0;                            // the SRS's GPU: the handle's streams, buffers and every call on it live there
  long n = 0, Q = 0;
  hipStream_t st = nullptr;
  hipStream_t ts = nullptr;                  // the t(X,y) product (NTT) runs beside the hscProve polynomials
  // Where the streams come from (stream_pool.hpp).  pooled: st, ts, tail, every Lane::st and chain[].st are BORROWED from the device's
  // pool, picked by role (HEAD, NTT, TAIL, GROUP(i) / T_GROUP, CHAIN(c)) -- shared with every other pooled handle on the device and
  // never destroyed here.  Not pooled (SONIC_STREAM_POOL=0, the default when the pool is off, and SONIC_PROVE_GRAPH=1 handles: a
  // capture on a shared stream would take the other handle's work with it): private streams, and tail == st.
  // Workspaces, scratch and events are the handle's own either way.
  bool pooled = false;
  hipStream_t tail = nullptr;                // the join over the lanes and the copy-out of a proof's results
  // pooled: recorded on `tail` behind a proof's last copy.  The caller waits for THIS (await_done): synchronising a shared stream
  // would also wait for whatever another handle has queued on it since.
  hipEvent_t done = nullptr;
  hipEvent_t ev_head = nullptr, ev_ts = nullptr;      // pooled: the ends of this proof's work on st and ts, which tail waits for
  // pooled: the assignment of THIS call (pend_asg, 6.3 MB at n = 2^16) goes up on a stream of the handle's own, queued BEFORE the enqueue
  // lock is taken, and the head waits for ev_up: a pageable upload blocks its host thread, and on the shared head stream under the lock
  // it held up the other handle's thread and head as well (sonic_prove_batch with per-proof assignments: 11.5 against 10.9 ms per proof)
  hipStream_t up = nullptr;
  hipEvent_t ev_up = nullptr;
  bool asg_staged = false;
  // blocks until the proof queued last has left the device.  (The calls off the hot path -- set_assignment, prepare, hscProve, ... --
  // still synchronise the stream they queued on: they hold the enqueue lock meanwhile, so nothing newer can be on it.)
  void await_done() { if (pooled) HIP_OK(hipEventSynchronize(done)); else HIP_OK(hipStreamSynchronize(st)); }
  bool have_assignment = false;
  DevBuf wL, wR, wO, cs, aL, aR, aO;        // Montgomery, resident across proofs
  // the circuit in sparse form (sonic_prover_new_csr, sonic_prove_csr; csr.hpp): the 3Q stacked rows and their column-major copy, int32
  // indices and Montgomery values, plus the chunks of s(u,Y)'s row sums.  `csr` says which form the kernels read (wL, wR, wO or these);
  // a parked one-shot shell switches with the circuit of each call.
  bool csr = false;
  struct CsrBufs {
    DevBuf row_ptr, col, val, col_ptr, row, cval, chunk_row, chunk_begin, row_chunk, partial;
    long nnz = 0, nchunks = 0;
    std::vector<int32_t> h_row_ptr;           // (prepare: the entry ranges of the rows of each P_q)
  } sp;
  Lane lanes[N_LANES];
  // lanes in use (always >= 1): all six by default; SONIC_FUSED_LANES=k (small-proof handles): k of them.  Six, although a fused proof's
  // lanes only prepare openings: side by side those finish sooner than queued behind each other on fewer streams
  int n_lanes = N_LANES;
  // fused proofs (below): the proof's ONE chain runs on a stream of its own, so that the lanes can queue the next proof's openings
  // beside it instead of behind its accumulation
  Lane chain[2];
  bool small_plan = false;                   // decided when the handle is made: the SRS plans 2^17 buckets or fewer for this n
  int next_lane = 0;
  const NttTables* ntt = nullptr;            // the device's shared tables for 2^log2m points (device_ntt_tables)
  DevBuf S, PAIRS, r1, sy0, su, pw, kpow, fa, fb, slots, frout, flags, tmp;
  std::vector<DevBuf> syj;
  // sonic_prover_prepare: Commit(P_q) per constraint row (affine, Montgomery) and per-j scalar buffers
  // pinned host staging (fixed addresses: the whole enqueue of a proof can be captured once and replayed as a hipGraph).  The pointers
  // below are views of these buffers, set where they are allocated (prove.hip: prover_new_impl, ensure_signature_state)
  PinnedBuf pin_tr, pin_pairs, pin_slots, pin_fr, pin_flags, pin_root;
  uint8_t* h_tr = nullptr;
  Fr* h_pairs = nullptr;         // {v, v^-1} of the evaluation points, computed on the host (prove_enqueue)
  MsmSlot* h_slots = nullptr;
  uint8_t* h_fr = nullptr;
  int* h_flags = nullptr;                  // [0] the proof's flags, [1] those of a circuit uploaded inside the proof (pend)
  // the circuit of THIS call, still in the caller's host buffers (prover_hand_over; a sparse one laid out on the host beside it).  When a
  // handle is made it is uploaded at once; a one-shot call into a parked shell (sonic_prove, sonic_prove_csr) leaves it to prove_enqueue,
  // which uploads it after it has queued the group of MSMs that needs the assignment only (R, W_a, W_b), so the weights cross PCIe
  // under those kernels instead of in front of the proof
  struct PendingCircuit { bool set = false; CircuitView view = {}; CsrLayout layout; } pend;
  // the same for the ASSIGNMENT of this call (round 6: sonic_prove_batch with per-proof assignments, sonic_prove): uploaded at the head of
  // the proof's own queue instead of by a sonic_prover_set_assignment that waits for the device before the proof may even be queued -- beside
  // another handle's accumulation that wait was ~1 ms per proof (config5: 99 against 113 proofs/s, profiles/r06_bench.json)
  const uint8_t* pend_asg[3] = {nullptr, nullptr, nullptr};
  // and for the CONSTANTS of this call (sonic_prove_batch_statements: one statement per proof): Q canonical field elements, checked by the
  // caller, uploaded into `cs` in place at the same point of the queue -- k(y) reads them on the transform's stream, which waits for the
  // main stream's polynomials anyway
  const uint8_t* pend_cs = nullptr;
  // and for an assignment that comes from a witness source (witness_src.hpp; sonic_prove_batch_src): the block of this proof, read at the
  // same point of the queue by the one launch of k_witness_ingest -- a device source where it lies, a host source through wit_raw.  `ready`
  // (may be null) is the event recorded on the source's stream when the call was entered: the handle's stream waits for it first
  struct PendingWitness { bool set = false; WitnessView v; hipEvent_t ready = nullptr; } pend_wit;
  DevBuf wit_raw;                            // a host source's bytes as they are: 3 x n elements (statement.hip: 3 x a chunk of assignments)
  // sonic_prover_eval_constraints (statement.hip): the staging buffer of the assignments of one chunk, the partial sums, the results
  struct StatementBufs { DevBuf stage, partial, out, gates; } stm;
  // runs of equal coefficients in the S_j of a handle that is not prepared (poly.hip, k_run_tiles): per j the masked copy of s(X, y_j),
  // the tile records and the (scalar, running-sum point) slots of the small MSM that stands for the runs; its sum lands in the side
  // slot S_extra(j) (proof_layout.hpp), where a prepared handle keeps sum_q y_j^{n+q} C_q, and the host adds it the same way
  // The small MSM runs on the handle's MAIN stream, which has built all polynomials by then and only waits for the lanes: behind the
  // batch of the lane that reads the masked copy its ~13 short launches and the chained sums of its per-window buckets added 0.6-1.3 ms
  // to a proof's latency; a stream of its own (two more streams per handle than the 8 hardware queues the runtime is given) cost
  // 1-5 ms per streamed proof.
  struct RunBufs {
    DevBuf masked, val, uniform, scal, pts;
    hipEvent_t masked_ev = nullptr;
  };
  MsmWorkspace runs_ws;
  std::vector<RunBufs> runs;
  bool runs_on = false;
  // does this circuit HAVE runs?  Sampled on the host from the weights as they are handed over (circuit_runs_hint): a circuit without
  // repeated rows would pay the masked copy, the tile scan and a small MSM per S_j and get nothing back (measured with
  // uniformly random weights at n = 2^18: profiles/r06_runs_dense_ab.txt).  A hint only: the path is exact for any input.
  bool circuit_has_runs = true;
  // C = commitPoly(s(u, Y)) through the SRS's symmetric sums (srs.hip, srs_build_sym): s(u, Y) has the same coefficient at Y^i and Y^-i
  // (i <= n), so n terms over A[i] + A[-i] and a Q-term MSM for Y^{n+1} .. Y^{n+Q} stand for its 2n + Q + 1 terms; the Q-term sum lands
  // in the side slot C_extra() and the host adds it
  bool sym_on = false;
  // Small proofs (round 6): ALL the MSMs of a proof as ONE batched kernel chain.  With 2^16 shared buckets and fewer (c <= 18: d < 2^20,
  // n <= 2^16) a group of two or three MSMs is 2048-3072 one-thread-per-bucket waves -- one round of the chip's 2048 wave slots, half
  // empty on its second -- and a proof is five such chains whose sorts, heavy-bucket launches and reductions (each ~15 launches of
  // 5-20 us, plus ~1.4 ms of latency-bound running sums) queue behind each other's accumulation for wave slots: n = 2^14 measured 5.5 ms
  // per proof for 1.8 ms of additions at the full-chip rate, n = 2^16 11.1 ms for 7.2 (profiles/r06_small_proofs.txt).  Fused, the lanes
  // only prepare the openings (evaluation, prefix sums, quotient: they still run side by side); their jobs are collected here and run as
  // one chain of up to MSM_MAX_JOBS jobs on the t lane: one sort, ONE accumulation launch that keeps every wave slot filled until its
  // tail, one butterfly over all bucket sets.  Larger plans (2^19 buckets per set) fill the chip per group and keep the lanes
  // (packing their groups was measured slower in round 3).  SONIC_PROVE_FUSED=0: never; =1 is the same as unset: only handles whose
  // plan is small (small_plan) have chain streams, so only they fuse.
  bool fused = false;
  std::vector<MsmJob> fused_jobs;
  std::vector<std::unique_ptr<Scratch>> fused_sc;      // one per opening of the proof: a quotient lives until the chain has read it
  size_t fused_sc_next = 0;
  Scratch& fused_scratch() {
    if (fused_sc_next == fused_sc.size()) fused_sc.emplace_back(new Scratch());
    return *fused_sc[fused_sc_next++];
  }
  // SONIC_PROVE_GRAPH=1 (read when the handle is made): capture the enqueue of the second proof and replay it.  Off by default: in round 3
  // the replay of a ~220-node, 7-stream proof was slower than the direct launches (n = 2^10: 9.0 vs 4.9 ms per proof, n = 2^14: 9.6 vs 6.5);
  // with one chain per proof (round 6) it is 4-8 % faster streamed from one host thread (n = 2^14: 3.18 vs 3.47 ms), 5-20 % slower one at a
  // time, and no faster through sonic_prove_batch at BASELINE configs[4] (profiles/r06_ab_graph.txt).
  bool use_graph = false;
  hipGraphExec_t graph = nullptr;
  bool graph_tried = false;
  long proofs_done = 0;
  bool in_flight = false;                    // between sonic_prover_submit and sonic_prover_collect, or submit_fs and collect_fs
  bool fs_flight = false;                    // the proof in flight is a Fiat-Shamir one: fsw walks it, and only collect_fs ends it
  bool core_flight = false;                  // the proof in flight is a core proof (sonic_prover_submit_core): only collect_core ends it
  // The enqueue in progress belongs to a CORE proof: the groups of the signature are not even visited (their commits and openings would
  // all return at once: 4Q empty jobs and Q + 1 lane hand-overs at Q = 64), and only the slots 0 .. 4 and the evaluations a, b, s come
  // back.  Set around prove_run by the core calls, under p->mu or the flight; a full proof never sees it.
  bool core = false;
  std::unique_ptr<FsWorker> fsw;
  // Which steps of the proof an enqueue runs (bit = phase; PH_ALL normally).  The Fiat-Shamir mode (sonic_prover_prove_fs) proves in
  // six passes, each running exactly the MSMs whose challenges have become known: results of earlier passes stay in `slots` / `frout`.
  uint32_t phases = 0x7e;
  DevBuf frstd;                              // frout in standard form (frout itself stays Montgomery across passes)
  std::chrono::steady_clock::time_point t_begin, t_enq;
  bool prepared = false;
  DevBuf cq;
  // window tables of the C_q (CQ_TAB_W x Q points, table w = 2^shift(w) C_q): their Q-term MSM then shares one bucket set and
  // leaves ONE window sum like every other MSM of a proof, instead of 64 that the host folds with 255 doublings (126 us each)
  DevBuf cq_tab;
  std::vector<DevBuf> diag, yq;
  hipEvent_t ev_r1 = nullptr, ev_sy0 = nullptr, ev_t = nullptr, ev_su = nullptr;
  std::vector<hipEvent_t> ev_syj;
  int log2m = 0;
  std::mutex mu;
  // ONE proof over several GPUs (sonic_prover_set_share, share_plan.hpp): this handle runs rank share_rank's pieces of the proof's
  // MSMs and reports un-normalised partial sums (sonic_prover_collect_share); share_world <= 1: the whole proof
  int share_rank = 0, share_world = 0;
  SharePlan share;
  bool share_planned_prepared = false, share_planned = false;
  int32_t share_plan_tag = 0;                // hash of the plan's inputs (share header: ranks must have planned alike)
  std::vector<uint8_t> slot_ran;             // per slot, side slots included: the last enqueue queued an MSM for it
  std::vector<uint8_t> fr_valid;             // per evaluation: the last enqueue computed it
  uint8_t witness_digest[32] = {0};          // SHA-256 of the assignment (Fiat-Shamir blinders, fs.hpp), made on first use
  bool have_witness_digest = false;
  // witness digest v2 (fs.hpp): the SHA-256 tree over the resident assignment, computed by the GPU (witness.hip) into `wtree` (all levels,
  // grown on first use; the root comes back through the pinned h_root), cached until the assignment changes
  uint8_t witness_digest_v2[32] = {0};
  bool have_witness_digest_v2 = false;
  DevBuf wtree;
  uint32_t* h_root = nullptr;
  void assignment_changed() { have_witness_digest = false; have_witness_digest_v2 = false; }
  // weights digest v2 (fs.hpp): the SHA-256 tree over the entries of the resident CSR (weights_digest.hip) into `wdtree`, the root through
  // h_root as well; cached until the circuit changes (prover_upload_circuit)
  uint8_t weights_digest_v2[32] = {0};
  bool have_weights_digest_v2 = false;
  DevBuf wdtree;
  // The signature state: everything a proof WITH a signature needs and a core proof does not.  A handle is made with S, PAIRS, slots,
  // frout, frstd and their pinned twins (h_tr, h_pairs, h_slots, h_fr) sized for a core proof -- the counts of ProofLayout{0}: 8 transcript
  // elements, 5 pairs, 8 slots, 3 evaluations -- and without the per-pair buffers: s(X, y_j) for each of the Q pairs (syj: Q buffers of
  // 3n + 1 elements) and the events that order their groups (ev_syj).  ensure_signature_state (prove.hip) re-creates the former at the
  // sizes of ProofLayout{Q} (5Q + 8 slots of sizeof(MsmSlot) bytes on the device and pinned, 8 + 2Q, 5 + 2Q, 3 + 2Q elements) and makes
  // the latter, on the first enqueue whose proof has a signature; a handle that only ever makes core proofs, aggregates, digests or
  // constraint evaluations never has it.  slot_ran and fr_valid are as long as the enqueue's own layout.
  bool have_signature_state = false;
  // k(y) over many blocks (poly.hip, k_of_y_plan.hpp): the plan of the enqueue in progress (decide_modes) and the blocks' partial sums
  KOfYPlan k_plan;
  DevBuf k_partial;
  // Lane N_LANES-1 carries the t(X,y) group (the largest, ready last); the other groups alternate over the rest, which
  // balances the point additions per lane (Q = 2: 55M / 51M / 48M) while one lane's sort and reduction phases run under
  // another lane's accumulation.  Streams beyond the 4 hardware queues would serialise behind each other.
  Lane& lane_at(int i) { return lanes[i % n_lanes]; }      // (prepare, hscProve: any lane)
  Lane& pick(hipEvent_t ready) {
    Lane& l = lanes[next_lane];
    next_lane = (next_lane + 1) % (n_lanes > 1 ? n_lanes - 1 : 1);
    (void)hipStreamWaitEvent(l.st, ready, 0);
    return l;
  }
  Lane& t_lane(hipEvent_t ready) {
    Lane& l = lanes[n_lanes - 1];
    (void)hipStreamWaitEvent(l.st, ready, 0);
    return l;
  }
  ~sonic_prover() {
    if (fsw) {      // a proof in flight is walked to its end first: it uses everything below
      { std::lock_guard<std::mutex> g(fsw->m); fsw->quit = true; }
      fsw->cv.notify_all();
      if (fsw->th.joinable()) fsw->th.join();
    }
    if (pooled) {
      // the streams are the pool's and go on serving other handles: wait for this handle's OWN events -- the end of its last proof and
      // of its lanes (an event that was never recorded counts as complete) -- and only then let the members below release the buffers
      if (done) (void)hipEventSynchronize(done);
      for (auto& l : lanes) if (l.done) (void)hipEventSynchronize(l.done);
      for (auto& l : chain) if (l.done) (void)hipEventSynchronize(l.done);
      for (hipEvent_t e : {ev_head, ev_ts, ev_up}) if (e) (void)hipEventSynchronize(e);
    }
    if (up) (void)hipStreamDestroy(up);
    if (ev_up) (void)hipEventDestroy(ev_up);
    for (auto& l : lanes) { if (l.st && !pooled) (void)hipStreamDestroy(l.st); if (l.done) (void)hipEventDestroy(l.done); if (l.prep) (void)hipEventDestroy(l.prep); }
    for (auto& l : chain) { if (l.st && !pooled) (void)hipStreamDestroy(l.st); if (l.done) (void)hipEventDestroy(l.done); if (l.prep) (void)hipEventDestroy(l.prep); }
    for (auto& r : runs) if (r.masked_ev) (void)hipEventDestroy(r.masked_ev);
    for (hipEvent_t e : {ev_r1, ev_sy0, ev_t, ev_su, done, ev_head, ev_ts}) if (e) (void)hipEventDestroy(e);
    for (hipEvent_t e : ev_syj) if (e) (void)hipEventDestroy(e);
    if (st && !pooled) (void)hipStreamDestroy(st);
    if (ts && !pooled) (void)hipStreamDestroy(ts);
    if (graph) (void)hipGraphExecDestroy(graph);
  }
};

// Held by every call that queues work for a pooled handle, for as long as it queues (a proof or a share, each Fiat-Shamir pass, prepare,
// set_assignment / set_witness, hscProve, a new handle's circuit upload): the device's enqueue lock, so that all pool streams see the
// handles' work in one order (the argument: internal.hpp, DeviceCtx::enqueue_mu).  Nothing for a handle with private streams -- the
// one-shot shells among them (prove_multi.hip).  Taken inside the call's device scope, never while another EnqueueLock is held by the
// same thread.
struct EnqueueLock {
  std::unique_lock<std::mutex> l;
  explicit EnqueueLock(const sonic_prover* p) { if (p->pooled) l = std::unique_lock<std::mutex>(current_ctx().enqueue_mu); }
};

// (prove.hip)
int upload_fr_mont(hipStream_t st, DevBuf& dst, const uint8_t* src, long count, int* d_flags);
int flags_to_status(int f, const char* who);
// (defined inside prove.hip's extern "C" block, not exported) prove with the assignment and the constants of THIS call still in the
// caller's host buffers (cs: Q canonical field elements, or null: the handle's; aL, aR, aO all null: the resident assignment)
extern "C" int prove_with_statement(sonic_prover_t* p, const uint8_t* aL, const uint8_t* aR, const uint8_t* aO, const uint8_t* cs, const uint8_t* transcript,
                                    uint8_t* out_proof);
// the same for a Fiat-Shamir proof (sonic_prove_batch_fs): the six passes over witness digest v2; out_transcript may be null
extern "C" int prove_fs_with_statement(sonic_prover_t* p, const uint8_t* aL, const uint8_t* aR, const uint8_t* aO, const uint8_t* cs, const uint8_t circuit_digest[32],
                                       const uint8_t blinder_seed[32], uint8_t* out_proof, uint8_t* out_transcript);
// the same two with the assignment read from block 0 of a witness source (sonic_prove_batch_src, sonic_prove_batch_fs_src); `ready` as in
// sonic_prover::PendingWitness
extern "C" int prove_with_witness(sonic_prover_t* p, const WitnessView& w, hipEvent_t ready, const uint8_t* cs, const uint8_t* transcript, uint8_t* out_proof);
extern "C" int prove_fs_with_witness(sonic_prover_t* p, const WitnessView& w, hipEvent_t ready, const uint8_t* cs, const uint8_t circuit_digest[32],
                                     const uint8_t blinder_seed[32], uint8_t* out_proof, uint8_t* out_transcript);
// the two for a CORE proof (sonic_prove_batch_core_src, sonic_prove_batch_core_fs_src): w null: the resident assignment; transcript: 6 x 32;
// out_proof: 576 bytes; out_yz (64 bytes) may be null
extern "C" int prove_core_with_witness(sonic_prover_t* p, const WitnessView* w, hipEvent_t ready, const uint8_t* cs, const uint8_t* transcript, uint8_t* out_proof);
extern "C" int prove_core_fs_with_witness(sonic_prover_t* p, const WitnessView* w, hipEvent_t ready, const uint8_t* cs, const uint8_t circuit_digest[32],
                                          const uint8_t blinder_seed[32], uint8_t* out_proof, uint8_t* out_yz);
// (witness_src.hip) a source checked against the rules of include/sonic_hip.h ("Witness sources"), the host's half and the device's;
// nb blocks of a checked source brought into three planes of Montgomery elements (block b at plane + b * out_stride), by ONE launch --
// a host source goes through p->wit_raw first; and the event that orders a device source
namespace sonic {
int witness_view_of(const char* who, const sonic_witness_src_t* src, long n, long B, WitnessView* out);
int witness_on_device_of(const char* who, const WitnessView& v, long n, long B, int device);
void witness_load_enqueue(sonic_prover* p, hipStream_t st, const WitnessView& v, long nb, Fr* oL, Fr* oR, Fr* oO, long out_stride, int* d_err);
struct WitnessReady {
  hipEvent_t ev = nullptr;
  WitnessReady() {}
  WitnessReady(const WitnessReady&) = delete;
  WitnessReady& operator=(const WitnessReady&) = delete;
  void record(const WitnessView& v);      // on v.hip_stream, if it names one (the current device must be the stream's)
  ~WitnessReady() { if (ev) (void)hipEventDestroy(ev); }
};
}
// (witness.hip) queues the SHA-256 tree of witness digest v2 over the Montgomery arrays into `tree` (grown to fit); returns where the
// root's eight state words will be
namespace sonic { const uint32_t* witness_tree_enqueue(hipStream_t st, const Fr* aL, const Fr* aR, const Fr* aO, long n, DevBuf& tree); }
// (prove.hip) what sonic_prover_new[_csr] and the one-shot calls share: the checks of a circuit against an SRS, a handle for an admitted
// circuit, and the hand-over of the next call's circuit to a handle that exists (uploaded inside its next proof)
int prover_admits(const char* who, const sonic_srs* srs, const CircuitView& c);
// (own_streams: the handle makes private streams whatever the device's pool says -- the shells of the one-shot calls, below)
int prover_new_impl(const sonic_srs_t* srs, const CircuitView& c, sonic_prover_t** out, bool own_streams = false);
void prover_hand_over(sonic_prover_t* p, const CircuitView& c);

