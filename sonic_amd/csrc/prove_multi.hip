// The calls that wrap whole proofs around the handle of prove.hip: the reference's own call shape with everything handed over per call
// (sonic_prove: src/Sonic/Protocol.hs:47-52; parked shells), many statements over several SRS replicas (sonic_prove_many), ONE proof shared
// by several handles (sonic_prove_shared) and a batch of proofs over several handles (sonic_prove_batch: `mapM prove`).
#include "prover.hpp"

// prove :: SRS -> Assignment Fr -> ArithCircuit Fr -> m (Proof, RndOracle) with the reference's own shape: everything handed over per
// call (Protocol.hs:47-52).  A handle costs streams, events, ~20 workspace allocations that grow on the first proof and the twiddle
// tables -- tens of milliseconds against a 32-ms proof -- so the device parks the shell of a finished one-shot call and the next call
// with the same SRS handle and (n, Q) only uploads its circuit and assignment into it (round 5; bench.py `one_shot`).  Several host
// threads inside sonic_prove on one GPU each take a parked shell or make one; at most ONE_SHOT_SHELLS stay parked per device.
namespace {
constexpr size_t ONE_SHOT_SHELLS = 4;
}
namespace sonic {
void drop_one_shot_of(const sonic_srs* s) {
  DeviceCtx& c = current_ctx();
  std::vector<OneShotShell*> gone;
  {
    std::lock_guard<std::mutex> g(c.one_shot_mu);
    for (size_t i = 0; i < c.one_shot.size();) {
      OneShotShell* sh = static_cast<OneShotShell*>(c.one_shot[i]);
      if (sh->srs == s) { gone.push_back(sh); c.one_shot.erase(c.one_shot.begin() + (long)i); } else i++;
    }
  }
  for (OneShotShell* sh : gone) { delete sh->p; delete sh; }
}
}
extern "C" {
// frees the parked one-shot shells of every device this process has used (or of one device: device >= 0).  A parked shell holds all the
// workspaces of a proof of its shape -- several GB at n = 2^20 -- until another shape evicts it or its SRS is freed; a host that has
// finished a burst of sonic_prove / sonic_prove_many calls gives the memory back with this.  Returns the number of shells freed.
int sonic_one_shot_trim(int device) {
  int freed = 0;
  try {
    int ndev = 0;
    if (sonic_device_count(&ndev) != SONIC_OK) return 0;
    for (int d = 0; d < ndev; d++) {
      if (device >= 0 && d != device) continue;
      DeviceScope scope(d);
      DeviceCtx& c = scope.ctx();
      std::vector<void*> gone;
      { std::lock_guard<std::mutex> g(c.one_shot_mu); gone.swap(c.one_shot); }
      for (void* v : gone) { OneShotShell* sh = static_cast<OneShotShell*>(v); delete sh->p; delete sh; freed++; }
    }
  } catch (const HipFail&) {}
  return freed;
}

}  // extern "C"

// the newest parked shell of this SRS and shape, taken out of the list (nullptr: none)
static OneShotShell* take_shell(DeviceCtx& ctx, const sonic_srs* srs, long n, long Q) {
  std::lock_guard<std::mutex> g(ctx.one_shot_mu);
  for (size_t i = ctx.one_shot.size(); i-- > 0;) {                 // newest first
    OneShotShell* c = static_cast<OneShotShell*>(ctx.one_shot[i]);
    if (c->srs == srs && c->p->n == n && c->p->Q == Q) { ctx.one_shot.erase(ctx.one_shot.begin() + (long)i); return c; }
  }
  return nullptr;
}
// the oldest parked shell makes room
static void park_shell(DeviceCtx& ctx, OneShotShell* sh) {
  OneShotShell* evict = nullptr;
  {
    std::lock_guard<std::mutex> g(ctx.one_shot_mu);
    if (ctx.one_shot.size() >= ONE_SHOT_SHELLS) { evict = static_cast<OneShotShell*>(ctx.one_shot.front()); ctx.one_shot.erase(ctx.one_shot.begin()); }
    ctx.one_shot.push_back(sh);
  }
  if (evict) { delete evict->p; delete evict; }
}

// sonic_prove and sonic_prove_csr.  The parked shells are shared by both: a shell holds whichever form of circuit its last call handed
// over (sonic_prover::csr) and switches with the upload of the next call's, so dense and sparse calls of one (n, Q) alternate over the
// same shells.  The circuit is checked before a shell is taken (a sparse one is validated here, once per call); into a parked shell it is
// handed over on the host (the runs hint; a sparse one's transpose) and uploaded inside the proof, behind the group of MSMs that needs the
// assignment only.
static int one_shot_prove(const char* who, const sonic_srs_t* srs, const CircuitView& c, const uint8_t* aL, const uint8_t* aR, const uint8_t* aO,
                          const uint8_t* transcript, uint8_t* out_proof) {
  API_BEGIN_ON(srs_device(srs))
  if (!srs || !c.cs || !aL || !aR || !aO || !transcript || !out_proof) { set_error("%s: bad argument (need n >= 1, Q >= 1)", who); return SONIC_ERR_INVALID_ARG; }
  int rc = prover_admits(who, srs, c);
  if (rc) return rc;
  DeviceCtx& ctx = current_ctx();
  OneShotShell* sh = take_shell(ctx, srs, c.n, c.Q);
  if (sh) prover_hand_over(sh->p, c);
  else {
    // A shell keeps streams of its own, pool or not: a one-shot proof's head carries the call's circuit and assignment (50 MB at n = 2^18),
    // and on the pool's shared head stream that upload sits in front of every other handle's next proof -- and of the other thread's
    // call in sonic_prove_many.  Measured with pooled shells, n = 2^18 on 4 queues: 36.5 ms per call against 34.8
    // (profiles/r13_stream_pool.txt).
    sonic_prover_t* p = nullptr;
    rc = prover_new_impl(srs, c, &p, /*own_streams=*/true);
    if (rc) return rc;
    sh = new OneShotShell{srs, p};
  }
  rc = prove_with_statement(sh->p, aL, aR, aO, /*cs=*/nullptr, transcript, out_proof);
  sh->p->pend = sonic_prover::PendingCircuit();       // (a call that failed before its upload: the caller's buffers end with the call)
  park_shell(ctx, sh);        // (also after a failed call: the next one loads its own circuit and assignment)
  return rc;
  API_END
}

extern "C" {

int sonic_prove(const sonic_srs_t* srs, int64_t n, int64_t Q, const uint8_t* wL, const uint8_t* wR, const uint8_t* wO,
                const uint8_t* cs, const uint8_t* aL, const uint8_t* aR, const uint8_t* aO, const uint8_t* transcript,
                uint8_t* out_proof) {
  return one_shot_prove("sonic_prove", srs, dense_view(n, Q, wL, wR, wO, cs), aL, aR, aO, transcript, out_proof);
}

// the same with sparse gate weights (csr.hpp)
int sonic_prove_csr(const sonic_srs_t* srs, int64_t n, int64_t Q, const int64_t* row_ptr, const int64_t* col, const uint8_t* val,
                    const uint8_t* cs, const uint8_t* aL, const uint8_t* aR, const uint8_t* aO, const uint8_t* transcript, uint8_t* out_proof) {
  return one_shot_prove("sonic_prove_csr", srs, csr_view(n, Q, row_ptr, col, val, cs), aL, aR, aO, transcript, out_proof);
}

// mapM (\(assignment, circuit) -> prove srs assignment circuit) over K INDEPENDENT statements of one shape (n, Q), spread over the SRS
// replicas -- one per GPU -- with two host threads per replica (statement i on thread i mod 2 n_srs; two one-shot calls in flight per
// GPU stream it: one call's upload and host tail under the other's kernels).  BASELINE's "batch of 64 independent proofs streamed over 8
// GPUs" with every proof its own circuit and witness; no collective.  Returns the first non-zero status in list order; all are attempted.
int sonic_prove_many(const sonic_srs_t* const* srs, int n_srs, int64_t n, int64_t Q, const sonic_statement_t* statements, int64_t K,
                     uint8_t* out_proofs, int* out_status) {
  if (!srs || n_srs < 1 || n_srs > 512 || n < 1 || Q < 1 || K < 0 || (K > 0 && (!statements || !out_proofs))) return SONIC_ERR_INVALID_ARG;
  for (int i = 0; i < n_srs; i++) if (!srs[i]) return SONIC_ERR_INVALID_ARG;
  const size_t psz = sonic_proof_size(Q);
  const int T = 2 * n_srs;
  std::vector<int> status((size_t)K, SONIC_OK);
  std::vector<std::string> errs((size_t)T);
  auto body = [&](int t) {
    const sonic_srs_t* s = srs[t % n_srs];
    for (int64_t i = t; i < K; i += T) {
      int rc = SONIC_ERR_HIP;
      try {
        const sonic_statement_t& st = statements[i];
        rc = sonic_prove(s, n, Q, st.wL, st.wR, st.wO, st.cs, st.aL, st.aR, st.aO, st.transcript, out_proofs + psz * (size_t)i);
        if (rc && errs[(size_t)t].empty()) { char b[512]; sonic_last_error(b, sizeof b); errs[(size_t)t] = b; }
      } catch (...) { rc = SONIC_ERR_HIP; }                            // (nothing may leave a thread's body: std::terminate)
      status[(size_t)i] = rc;
    }
  };
  {
    ThreadGroup th;
    for (int t = 1; t < T && t < K; t++) th.emplace_back(body, t);
    body(0);
    for (auto& x : th) x.join();
  }
  if (out_status) for (int64_t i = 0; i < K; i++) out_status[i] = status[(size_t)i];
  for (int64_t i = 0; i < K; i++)
    if (status[(size_t)i]) {
      const int t = (int)(i % T);
      set_error("sonic_prove_many, statement %ld (device %d): %s", (long)i, srs_device(srs[t % n_srs]), errs[(size_t)t].c_str());
      return status[(size_t)i];
    }
  return SONIC_OK;
}

// ---- N GPUs from ONE host process: one proof shared by several handles, a batch of proofs over several handles ------------------
// (include/sonic_hip.h).  One host thread per handle; a handle carries its device, so the threads need no set-up of their own.
int sonic_prover_device(const sonic_prover_t* p) { return p ? p->device : -1; }

int sonic_prove_shared(sonic_prover_t* const* provers, int world, const uint8_t* transcript, uint8_t* out_proof) {
  if (!provers || world < 1 || world > 1024 || !transcript || !out_proof) return SONIC_ERR_INVALID_ARG;
  for (int r = 0; r < world; r++) {
    if (!provers[r]) return SONIC_ERR_INVALID_ARG;
    if (provers[r]->n != provers[0]->n || provers[r]->Q != provers[0]->Q) { set_error("sonic_prove_shared: handle %d proves another circuit shape (n, Q) than handle 0", r); return SONIC_ERR_INVALID_ARG; }
    for (int q = 0; q < r; q++) if (provers[q] == provers[r]) { set_error("sonic_prove_shared: handle %d appears twice (one handle runs one share at a time)", r); return SONIC_ERR_INVALID_ARG; }
  }
  if (world == 1) {
    // one handle: the whole proof (a handle left in share mode by an earlier call goes back first)
    if (provers[0]->share_world > 1) { int rc = sonic_prover_set_share(provers[0], 0, 1); if (rc) return rc; }
    return sonic_prover_prove(provers[0], transcript, out_proof);
  }
  const long Q = provers[0]->Q;
  const size_t ssz = sonic_proof_share_size(Q);
  std::vector<uint8_t> shares(ssz * (size_t)world);
  std::vector<int> rcs((size_t)world, SONIC_OK);
  std::vector<std::string> errs((size_t)world);
  auto body = [&](int r) {
    sonic_prover_t* p = provers[r];
    int rc = SONIC_OK;
    try {
      bool placed;
      { std::lock_guard<std::mutex> g(p->mu); placed = p->share_world == world && p->share_rank == r; }
      if (!placed) rc = sonic_prover_set_share(p, r, world);          // (clears the slots of pieces the handle no longer runs; once per change)
      if (!rc) rc = sonic_prover_prove_share(p, transcript, &shares[ssz * (size_t)r]);
      if (rc) { char b[512]; sonic_last_error(b, sizeof b); errs[(size_t)r] = b; }
    } catch (...) { rc = SONIC_ERR_HIP; }                            // (nothing may leave a thread's body: std::terminate)
    rcs[(size_t)r] = rc;
  };
  {
    ThreadGroup th;
    for (int r = 1; r < world; r++) th.emplace_back(body, r);
    body(0);                                                       // the calling thread is rank 0's
    for (auto& t : th) t.join();
  }
  for (int r = 0; r < world; r++)
    if (rcs[(size_t)r]) { set_error("sonic_prove_shared, rank %d (device %d): %s", r, provers[r]->device, errs[(size_t)r].c_str()); return rcs[(size_t)r]; }
  return sonic_proof_from_shares(Q, world, shares.data(), transcript, out_proof);
}

// sonic_prove_batch (cs == null), sonic_prove_batch_statements (cs: K x Q constants, proof i's uploaded at the head of its own queue) and
// sonic_prove_batch_fs (fs: the circuit digests and blinder seeds in place of transcripts; the transcripts come back)
struct BatchFs { const uint8_t *circuit_digests, *blinder_seeds; uint8_t* out_transcripts; };
static int prove_batch_impl(const char* who, sonic_prover_t* const* provers, int n_provers, int64_t K, const uint8_t* aL, const uint8_t* aR, const uint8_t* aO,
                            const uint8_t* cs, const uint8_t* transcripts, uint8_t* out_proofs, int* out_status, const BatchFs* fs = nullptr,
                            const sonic_witness_src_t* src = nullptr, bool from_src = false, bool core = false) {
  if (!provers || n_provers < 1 || n_provers > 1024 || K < 0 || (K > 0 && (!(fs ? fs->circuit_digests && fs->blinder_seeds : transcripts != nullptr) || !out_proofs))) return SONIC_ERR_INVALID_ARG;
  const bool per_proof = aL || aR || aO;
  if (per_proof && !(aL && aR && aO)) { set_error("%s: aL, aR, aO must be given together (or all NULL: the handles' resident assignments)", who); return SONIC_ERR_INVALID_ARG; }
  for (int i = 0; i < n_provers; i++) {
    if (!provers[i]) return SONIC_ERR_INVALID_ARG;
    if (provers[i]->n != provers[0]->n || provers[i]->Q != provers[0]->Q) { set_error("%s: handle %d proves another circuit shape (n, Q) than handle 0", who, i); return SONIC_ERR_INVALID_ARG; }
    if (provers[i]->share_world > 1) { set_error("%s: handle %d runs one rank's share of a proof (sonic_prover_set_share)", who, i); return SONIC_ERR_INVALID_ARG; }
    for (int q = 0; q < i; q++) if (provers[q] == provers[i]) { set_error("%s: handle %d appears twice", who, i); return SONIC_ERR_INVALID_ARG; }
  }
  const long n = provers[0]->n, Q = provers[0]->Q;
  // a witness source (sonic_prove_batch_src, sonic_prove_batch_fs_src): checked once, against every handle's GPU, before anything is
  // queued; the event that orders a device source is recorded here, at entry, and every handle's stream waits for it
  WitnessView wv;
  WitnessReady ready;
  if (from_src && K > 0) {
    int rc = witness_view_of(who, src, n, K, &wv);
    if (rc) return rc;
    try {
      DeviceScope scope(provers[0]->device);
      for (int i = 0; i < n_provers && !rc; i++) rc = witness_on_device_of(who, wv, n, K, provers[i]->device);
      if (!rc) ready.record(wv);
    } catch (const HipFail& f) { return f.code; }
    if (rc) return rc;
  }
  // (core proofs: 576 bytes each, 6 transcript elements in, and y, z where a Fiat-Shamir batch gives the transcripts back)
  const size_t psz = core ? ProofLayout::core_proof_bytes() : sonic_proof_size(Q), tsz = core ? (fs ? 64 : 32 * (size_t)ProofLayout::core_transcript_len) : 32 * (size_t)(8 + 2 * Q);
  const size_t asz = 32 * (size_t)n, ksz = 32 * (size_t)Q;
  std::vector<int> status((size_t)K, SONIC_OK);
  std::vector<std::string> errs((size_t)n_provers);
  std::vector<int64_t> first_bad((size_t)n_provers, -1);
  auto body = [&](int h) {
    for (int64_t i = h; i < K; i += n_provers) {
      int rc = SONIC_OK;
      try {
        // (the constants are checked here, before anything of proof i is queued: its status, and the handle keeps the constants it has)
        for (long q = 0; cs && q < Q && !rc; q++) {
          Fr k;
          memcpy(k.l, cs + ksz * (size_t)i + 32 * (size_t)q, 32);
          if (!fp_is_canonical(k)) { set_error("%s: cs[%ld] of proof %ld is not a canonical field element", who, q, (long)i); rc = SONIC_ERR_BAD_ENCODING; }
        }
        const uint8_t *aLi = per_proof ? aL + asz * (size_t)i : nullptr, *aRi = per_proof ? aR + asz * (size_t)i : nullptr, *aOi = per_proof ? aO + asz * (size_t)i : nullptr;
        const uint8_t* csi = cs ? cs + ksz * (size_t)i : nullptr;
        uint8_t* out = out_proofs + psz * (size_t)i;
        WitnessView blk;
        if (rc) {}      // (refused above)
        else if (core && fs) rc = prove_core_fs_with_witness(provers[h], from_src ? &(blk = wv.block(i)) : nullptr, ready.ev, csi, fs->circuit_digests + 32 * (size_t)i,
                                                             fs->blinder_seeds + 32 * (size_t)i, out, fs->out_transcripts ? fs->out_transcripts + tsz * (size_t)i : nullptr);
        else if (core) rc = prove_core_with_witness(provers[h], from_src ? &(blk = wv.block(i)) : nullptr, ready.ev, csi, transcripts + tsz * (size_t)i, out);
        else if (from_src && fs) rc = prove_fs_with_witness(provers[h], wv.block(i), ready.ev, csi, fs->circuit_digests + 32 * (size_t)i, fs->blinder_seeds + 32 * (size_t)i, out,
                                                            fs->out_transcripts ? fs->out_transcripts + tsz * (size_t)i : nullptr);
        else if (from_src) rc = prove_with_witness(provers[h], wv.block(i), ready.ev, csi, transcripts + tsz * (size_t)i, out);
        else if (fs) rc = prove_fs_with_statement(provers[h], aLi, aRi, aOi, csi, fs->circuit_digests + 32 * (size_t)i, fs->blinder_seeds + 32 * (size_t)i, out,
                                                  fs->out_transcripts ? fs->out_transcripts + tsz * (size_t)i : nullptr);
        else if (cs || per_proof) rc = prove_with_statement(provers[h], aLi, aRi, aOi, csi, transcripts + tsz * (size_t)i, out);
        else rc = sonic_prover_prove(provers[h], transcripts + tsz * (size_t)i, out);
        if (rc && first_bad[(size_t)h] < 0) { first_bad[(size_t)h] = i; char b[512]; sonic_last_error(b, sizeof b); errs[(size_t)h] = b; }
      } catch (...) { rc = SONIC_ERR_HIP; }                          // (nothing may leave a thread's body: std::terminate)
      status[(size_t)i] = rc;
    }
  };
  {
    ThreadGroup th;
    for (int h = 1; h < n_provers && h < K; h++) th.emplace_back(body, h);
    body(0);
    for (auto& t : th) t.join();
  }
  if (out_status) for (int64_t i = 0; i < K; i++) out_status[i] = status[(size_t)i];
  for (int64_t i = 0; i < K; i++)
    if (status[(size_t)i]) {
      const int h = (int)(i % n_provers);
      set_error("%s, proof %ld (handle %d, device %d): %s", who, (long)i, h, provers[h]->device, errs[(size_t)h].c_str());
      return status[(size_t)i];
    }
  return SONIC_OK;
}


int sonic_prove_batch(sonic_prover_t* const* provers, int n_provers, int64_t K, const uint8_t* aL, const uint8_t* aR, const uint8_t* aO,
                      const uint8_t* transcripts, uint8_t* out_proofs, int* out_status) {
  return prove_batch_impl("sonic_prove_batch", provers, n_provers, K, aL, aR, aO, nullptr, transcripts, out_proofs, out_status);
}

int sonic_prove_batch_statements(sonic_prover_t* const* provers, int n_provers, int64_t K, const uint8_t* aL, const uint8_t* aR, const uint8_t* aO,
                                 const uint8_t* cs, const uint8_t* transcripts, uint8_t* out_proofs, int* out_status) {
  try { DeviceScope probe(-1); } catch (const HipFail& f) { return f.code; }      // (no device: SONIC_ERR_NO_DEVICE whatever the arguments are)
  if (K > 0 && !cs) { set_error("sonic_prove_batch_statements: cs is NULL (sonic_prove_batch proves with the handles' constants)"); return SONIC_ERR_INVALID_ARG; }
  return prove_batch_impl("sonic_prove_batch_statements", provers, n_provers, K, aL, aR, aO, cs, transcripts, out_proofs, out_status);
}

int sonic_prove_batch_fs(sonic_prover_t* const* provers, int n_provers, int64_t K, const uint8_t* aL, const uint8_t* aR, const uint8_t* aO, const uint8_t* cs,
                         const uint8_t* circuit_digests, const uint8_t* blinder_seeds, uint8_t* out_proofs, uint8_t* out_transcripts, int* out_status) {
  try { DeviceScope probe(-1); } catch (const HipFail& f) { return f.code; }      // (no device: SONIC_ERR_NO_DEVICE whatever the arguments are)
  const BatchFs fs{circuit_digests, blinder_seeds, out_transcripts};
  return prove_batch_impl("sonic_prove_batch_fs", provers, n_provers, K, aL, aR, aO, cs, nullptr, out_proofs, out_status, &fs);
}

// the two batch calls over a witness source (include/sonic_hip.h, "Witness sources"): proof i reads block i of each vector
int sonic_prove_batch_src(sonic_prover_t* const* provers, int n_provers, int64_t K, const sonic_witness_src_t* src, const uint8_t* cs, const uint8_t* transcripts,
                          uint8_t* out_proofs, int* out_status) {
  try { DeviceScope probe(-1); } catch (const HipFail& f) { return f.code; }      // (no device: SONIC_ERR_NO_DEVICE whatever the arguments are)
  return prove_batch_impl("sonic_prove_batch_src", provers, n_provers, K, nullptr, nullptr, nullptr, cs, transcripts, out_proofs, out_status, nullptr, src, true);
}

int sonic_prove_batch_fs_src(sonic_prover_t* const* provers, int n_provers, int64_t K, const sonic_witness_src_t* src, const uint8_t* cs, const uint8_t* circuit_digests,
                             const uint8_t* blinder_seeds, uint8_t* out_proofs, uint8_t* out_transcripts, int* out_status) {
  try { DeviceScope probe(-1); } catch (const HipFail& f) { return f.code; }      // (no device: SONIC_ERR_NO_DEVICE whatever the arguments are)
  const BatchFs fs{circuit_digests, blinder_seeds, out_transcripts};
  return prove_batch_impl("sonic_prove_batch_fs_src", provers, n_provers, K, nullptr, nullptr, nullptr, cs, nullptr, out_proofs, out_status, &fs, src, true);
}

// the two for core proofs (include/sonic_hip.h, "Core proofs"): the same per-handle routine with the core mask; src NULL: the resident assignments
int sonic_prove_batch_core_src(sonic_prover_t* const* provers, int n_provers, int64_t K, const sonic_witness_src_t* src, const uint8_t* cs, const uint8_t* transcripts,
                               uint8_t* out_proofs, int* out_status) {
  try { DeviceScope probe(-1); } catch (const HipFail& f) { return f.code; }      // (no device: SONIC_ERR_NO_DEVICE whatever the arguments are)
  return prove_batch_impl("sonic_prove_batch_core_src", provers, n_provers, K, nullptr, nullptr, nullptr, cs, transcripts, out_proofs, out_status, nullptr, src, src != nullptr, true);
}

int sonic_prove_batch_core_fs_src(sonic_prover_t* const* provers, int n_provers, int64_t K, const sonic_witness_src_t* src, const uint8_t* cs, const uint8_t* circuit_digests,
                                  const uint8_t* blinder_seeds, uint8_t* out_proofs, uint8_t* out_yz, int* out_status) {
  try { DeviceScope probe(-1); } catch (const HipFail& f) { return f.code; }      // (no device: SONIC_ERR_NO_DEVICE whatever the arguments are)
  const BatchFs fs{circuit_digests, blinder_seeds, out_yz};
  return prove_batch_impl("sonic_prove_batch_core_fs_src", provers, n_provers, K, nullptr, nullptr, nullptr, cs, nullptr, out_proofs, out_status, &fs, src, src != nullptr, true);
}

}  // extern "C"
