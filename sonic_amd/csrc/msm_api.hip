// The stand-alone MSM entry points of the C ABI (include/sonic_hip.h): sonic_msm_g1 over caller-supplied points, MSM lanes over an SRS
// handle (submit / collect, the blocking forms on pooled lanes), the bucket-exchange entry points, one MSM over several GPUs of the
// process (msm_multi) and the host-side sums of partial results.  The kernels and plans: msm.hip, msm.hpp.
#include <string.h>
#include <condition_variable>
#include <memory>
#include <string>
#include <vector>
#include "srs_handle.hpp"

using namespace sonic;

extern "C" {

int sonic_msm_set_window(int c) { msm_set_window_override(c); return SONIC_OK; }

int sonic_msm_plan(const sonic_srs_t* srs, int64_t n, int* window_bits, int* windows, int* bucket_sets) {
  if (!srs || n < 0) return SONIC_ERR_INVALID_ARG;
  if (n >= MSM_MAX_TERMS) { set_error("MSM of %ld terms: at most 2^31 - 1 (entry encoding)", (long)n); return SONIC_ERR_INVALID_ARG; }
  MsmPlan pl = srs_msm_plan(srs, n);
  if (window_bits) *window_bits = pl.c;
  if (windows) *windows = pl.W;
  if (bucket_sets) *bucket_sets = pl.Wb;
  return SONIC_OK;
}

int sonic_msm_g1(const uint8_t* points, const uint8_t* scalars, int64_t n, uint8_t out_g1[96]) {
  API_BEGIN
  if (n < 0 || !out_g1 || (n > 0 && (!points || !scalars))) return SONIC_ERR_INVALID_ARG;
  CallLease lease;
  hipStream_t st = lease.st();
  const long m = n > 0 ? n : 1;
  DevBuf raw(96 * m), pts(sizeof(G1Affine) * m), sc(32 * m), err(4);
  HIP_OK(hipMemsetAsync(err.p, 0, 4, st));
  if (n > 0) {
    HIP_OK(hipMemcpyAsync(raw.p, points, 96 * n, hipMemcpyHostToDevice, st));
    HIP_OK(hipMemcpyAsync(sc.p, scalars, 32 * n, hipMemcpyHostToDevice, st));
    points_from_bytes_enqueue(st, raw.as<uint8_t>(), PointArrayMut{pts.as<char>(), (uint32_t)sizeof(G1Affine)}, (long)n, err.as<int>(), -1L);
    fr_check_enqueue(st, sc.as<Fr>(), n, err.as<int>());
  }
  const int herr = read_flags(st, err);
  if (herr) { set_error("sonic_msm_g1: non-canonical input or point not on curve"); return SONIC_ERR_BAD_ENCODING; }
  msm_blocking(st, lease.ws(), msm_plan(n > 0 ? n : 1, /*fold=*/false), PointArray::packed(pts.as<G1Affine>()), sc.as<Fr>(), n, false, out_g1, nullptr);
  API_END
}

// ---- the same MSM in two halves, on a lane of its own (stream + bucket workspace + pinned result slot): submit queues scalar
// check, sort, accumulation and reduction and returns; collect waits, finishes on the host.  Two lanes used in turn keep the
// chip busy across consecutive MSMs: the sort and the (latency-bound) reduction of one run under the accumulation of the other.
struct sonic_msm_lane {
  int device = 0;                // the GPU the lane's stream and workspace live on; it serves SRS handles of that device
  hipStream_t st = nullptr;
  MsmWorkspace ws;
  DevBuf slot, err;
  MsmSlot* h_slot = nullptr;
  int* h_err = nullptr;
  int Wb = 0;
  bool in_flight = false;
  bool own_stream = true;        // false: the lane runs on a stream the caller owns (sonic_msm_lane_new_on_stream)
  // sonic_msm_g1_srs_multi keeps a pooled lane's exchange buffers across calls: this rank's scalar slice (host-scalar form), its full
  // bucket set, the slices it pulled from its peers, its device-side result
  DevBuf x_scalars, x_buckets, x_slices, x_part;
  std::mutex mu;
  ~sonic_msm_lane() {
    if (st) { (void)hipStreamSynchronize(st); if (own_stream) (void)hipStreamDestroy(st); }
    if (h_slot) (void)hipHostFree(h_slot);
    if (h_err) (void)hipHostFree(h_err);
  }
};

// own_stream: the lane makes (and later destroys) its stream; otherwise it runs on caller_stream, which may be the null stream
static sonic_msm_lane* lane_make(bool own_stream, hipStream_t caller_stream) {
  std::unique_ptr<sonic_msm_lane> l(new sonic_msm_lane());
  l->device = current_ctx().dev;
  l->own_stream = own_stream;
  if (own_stream) HIP_OK(hipStreamCreateWithFlags(&l->st, hipStreamNonBlocking));
  else l->st = caller_stream;
  l->slot.alloc(sizeof(MsmSlot));
  l->err.alloc(4);
  HIP_OK(hipHostMalloc((void**)&l->h_slot, sizeof(MsmSlot), hipHostMallocDefault));
  HIP_OK(hipHostMalloc((void**)&l->h_err, 4, hipHostMallocDefault));
  return l.release();
}
int sonic_msm_lane_new(sonic_msm_lane_t** out) { return sonic_msm_lane_new_on(-1, out); }
int sonic_msm_lane_new_on(int device, sonic_msm_lane_t** out) {
  API_BEGIN_ON(device)
  if (!out) return SONIC_ERR_INVALID_ARG;
  *out = lane_make(true, nullptr);
  API_END
}
// A lane on a stream the caller owns -- e.g. torch.cuda.current_stream().cuda_stream, so that the lane's kernels, the caller's
// RCCL collectives on the bucket / partial buffers and the caller's copies are ordered by the stream and need no host
// synchronisation in between.  The stream must outlive the lane.
int sonic_msm_lane_new_on_stream(void* hip_stream, sonic_msm_lane_t** out) {
  // the lane lives on the stream's device (the null stream belongs to whatever device is current: the default device then)
  int sdev = -1;
  if (hip_stream && hipStreamGetDevice(static_cast<hipStream_t>(hip_stream), &sdev) != hipSuccess) { (void)hipGetLastError(); sdev = -1; }
  API_BEGIN_ON(sdev)
  if (!out) return SONIC_ERR_INVALID_ARG;
  *out = lane_make(false, static_cast<hipStream_t>(hip_stream));
  API_END
}
void sonic_msm_lane_free(sonic_msm_lane_t* l) {
  if (!l) return;
  try { DeviceScope scope(l->device); delete l; } catch (const HipFail&) { delete l; }
}
// a lane and an SRS handle meet in one call: both must live on the same GPU
static bool same_device(const sonic_msm_lane_t* l, const sonic_srs_t* srs, const char* who) {
  if (l->device == srs->device) return true;
  set_error("%s: the lane lives on device %d, the SRS on device %d", who, l->device, srs->device);
  return false;
}

static int msm_submit_common(sonic_msm_lane_t* l, const sonic_srs_t* srs, int basis, int64_t e0, const void* d_scalars, int64_t n, void* d_partial_out);
int sonic_msm_submit(sonic_msm_lane_t* l, const sonic_srs_t* srs, int basis, int64_t e0, const void* d_scalars, int64_t n) {
  return msm_submit_common(l, srs, basis, e0, d_scalars, n, nullptr);
}
// the same with the un-normalised 192-byte sum ALSO left in device memory (d_partial_out), queued on the lane's stream: the
// operand of a cross-rank all-gather that never visits the host.  Only plans that leave one window sum (window tables) can do
// that -- others need the host's Horner fold -- SONIC_ERR_INVALID_ARG otherwise (use sonic_msm_collect's out_partial then).
int sonic_msm_submit_dev_v2(sonic_msm_lane_t* l, const sonic_srs_t* srs, int basis, int64_t e0, const void* d_scalars, int64_t n, void* d_partial_out,
                            size_t out_bytes) {
  if (!d_partial_out) return SONIC_ERR_INVALID_ARG;
  if (out_bytes < sizeof(MsmSlot)) { set_error("sonic_msm_submit_dev_v2: the result takes %zu bytes of device memory (SONIC_G1_DEV_PARTIAL_BYTES), the buffer has %zu", sizeof(MsmSlot), out_bytes); return SONIC_ERR_INVALID_ARG; }
  return msm_submit_common(l, srs, basis, e0, d_scalars, n, d_partial_out);
}
// Retired symbols keep their OLD prototypes and refuse: up to round 3 these wrote 192 bytes to d_partial_out, since round 4 the result
// is SONIC_G1_DEV_PARTIAL_BYTES (12304) -- a caller built against the old header must get an error, not 12 KB written over its 192-byte
// buffer.  The _v2 forms take the buffer's size.
int sonic_msm_submit_dev(sonic_msm_lane_t*, const sonic_srs_t*, int, int64_t, const void*, int64_t, void*) {
  set_error("sonic_msm_submit_dev is retired (its result grew from 192 to %d bytes): use sonic_msm_submit_dev_v2, which takes the buffer size", SONIC_G1_DEV_PARTIAL_BYTES);
  return SONIC_ERR_INVALID_ARG;
}
static int msm_submit_common(sonic_msm_lane_t* l, const sonic_srs_t* srs, int basis, int64_t e0, const void* d_scalars, int64_t n, void* d_partial_out) {
  API_BEGIN_ON(l ? l->device : -1)
  if (!l || !srs || n < 0 || (n > 0 && !d_scalars) || (basis != 0 && basis != 1)) return SONIC_ERR_INVALID_ARG;
  if (!same_device(l, srs, "sonic_msm_submit")) return SONIC_ERR_INVALID_ARG;
  if (n > 0 && !srs_range_ok("msm over SRS", srs, e0, n)) return SONIC_ERR_SRS_INDEX;
  if (n > 0 && !srs_held_ok("msm over SRS", srs, e0, n)) return SONIC_ERR_INVALID_ARG;
  std::lock_guard<std::mutex> g(l->mu);
  if (l->in_flight) { set_error("sonic_msm_submit: the lane's previous MSM has not been collected"); return SONIC_ERR_INVALID_ARG; }
  hipStream_t st = l->st;
  const Fr* dsc = static_cast<const Fr*>(d_scalars);
  HIP_OK(hipMemsetAsync(l->err.p, 0, 4, st));
  fr_check_enqueue(st, dsc, n, l->err.as<int>());
  MsmPlan pl = srs_msm_plan(srs, n);
  pl.accum_block = 64;           // a lane's MSM runs alone or beside other lanes' MSMs, not inside a proof (msm.hpp)
  msm_enqueue(st, l->ws, pl, srs->basis(basis) + srs->geo.slot(e0), dsc, n, false, l->slot.as<MsmSlot>());
  l->Wb = pl.Wb;
  if (d_partial_out) HIP_OK(hipMemcpyAsync(d_partial_out, l->slot.p, sizeof(MsmSlot), hipMemcpyDeviceToDevice, st));
  HIP_OK(hipMemcpyAsync(l->h_slot, l->slot.p, sizeof(MsmSlot), hipMemcpyDeviceToHost, st));
  HIP_OK(hipMemcpyAsync(l->h_err, l->err.p, 4, hipMemcpyDeviceToHost, st));
  l->in_flight = true;
  API_END
}

int sonic_msm_collect(sonic_msm_lane_t* l, uint8_t* out_g1, uint8_t* out_partial) {
  API_BEGIN_ON(l ? l->device : -1)
  if (!l) return SONIC_ERR_INVALID_ARG;
  std::lock_guard<std::mutex> g(l->mu);
  if (!l->in_flight) { set_error("sonic_msm_collect: nothing was submitted"); return SONIC_ERR_INVALID_ARG; }
  l->in_flight = false;
  HIP_OK(hipStreamSynchronize(l->st));
  if (*l->h_err) { set_error("msm over SRS: non-canonical scalar"); return SONIC_ERR_BAD_ENCODING; }
  G1XYZZ sum = msm_finish_host(*l->h_slot);
  if (out_g1) g1_canonical_bytes_host(sum, out_g1);
  if (out_partial) memcpy(out_partial, &sum, sizeof sum);
  API_END
}

// a lane of the current device's pool (made on first need; workspaces and buffers stay with it), handed back when the holder dies
struct PooledLane {
  DeviceCtx& ctx;
  sonic_msm_lane_t* lane = nullptr;
  explicit PooledLane(DeviceCtx& c) : ctx(c) {
    {
      std::lock_guard<std::mutex> g(ctx.pool_mu);
      if (!ctx.lanes.empty()) { lane = static_cast<sonic_msm_lane_t*>(ctx.lanes.back()); ctx.lanes.pop_back(); }
    }
    if (!lane) {
      int rc = sonic_msm_lane_new_on(ctx.dev, &lane);
      if (rc) throw HipFail{rc};
    }
  }
  ~PooledLane() { if (lane) { std::lock_guard<std::mutex> g(ctx.pool_mu); ctx.lanes.push_back(lane); } }
  PooledLane(const PooledLane&) = delete;
  PooledLane& operator=(const PooledLane&) = delete;
};

// the blocking entry points run on one shared lane (pinned result slot, one host synchronisation per call)
static int msm_srs_common(const sonic_srs_t* srs, int basis, int64_t e0, const void* d_scalars, const uint8_t* h_scalars,
                          int64_t n, uint8_t* out96, uint8_t* out192) {
  API_BEGIN_ON(srs_device(srs))
  if (!srs || n < 0 || (basis != 0 && basis != 1)) return SONIC_ERR_INVALID_ARG;
  // a lane per call from the device's pool (the blocking MSMs of different host threads run side by side)
  PooledLane pooled(current_ctx());
  sonic_msm_lane_t* lane = pooled.lane;
  DevBuf sc;
  const void* dsc = d_scalars;
  if (h_scalars && n > 0) {
    sc.alloc(32 * n);
    HIP_OK(hipMemcpyAsync(sc.p, h_scalars, 32 * n, hipMemcpyHostToDevice, lane->st));
    dsc = sc.p;
  }
  if (n > 0 && !dsc) return SONIC_ERR_INVALID_ARG;
  int rc = sonic_msm_submit(lane, srs, basis, e0, dsc, n);
  if (rc) { (void)hipStreamSynchronize(lane->st); return rc; }       // (the upload of `sc` may still be in flight)
  return sonic_msm_collect(lane, out96, out192);       // waits for the stream: `sc` may go out of scope afterwards
  API_END
}

int sonic_msm_g1_srs(const sonic_srs_t* srs, int basis, int64_t e0, const uint8_t* scalars, int64_t n, uint8_t out_g1[96]) {
  return msm_srs_common(srs, basis, e0, nullptr, scalars, n, out_g1, nullptr);
}
int sonic_msm_g1_srs_dev(const sonic_srs_t* srs, int basis, int64_t e0, const void* d_scalars, int64_t n, uint8_t out_g1[96]) {
  return msm_srs_common(srs, basis, e0, d_scalars, nullptr, n, out_g1, nullptr);
}
int sonic_msm_g1_srs_partial_dev(const sonic_srs_t* srs, int basis, int64_t e0, const void* d_scalars, int64_t n, uint8_t out_partial[192]) {
  return msm_srs_common(srs, basis, e0, d_scalars, nullptr, n, nullptr, out_partial);
}

// ---- one MSM over several GPUs, sharded by BUCKET range (strong scaling) ----------------------------------------------------
// Every rank sorts and accumulates its term range into a full bucket set; the ranks exchange bucket ranges (all-to-all of
// slice_len x 192 B per pair); each rank adds the slices it received and reduces its range with the range's weights; the
// 192-byte partials are gathered and added as in the term-range scheme.  The reduction of the shared buckets -- which a
// term-range shard repeats in full on every rank -- is divided by the number of ranks this way.
int sonic_msm_exchange_layout(const sonic_srs_t* srs, int world, int64_t* n_buckets, int64_t* slice_len) {
  if (!srs || world < 1 || !n_buckets || !slice_len) return SONIC_ERR_INVALID_ARG;
  if (srs->tab_W <= 1 || srs->tab_endo) { set_error("bucket exchange needs the full window tables of the SRS (one shared bucket set per MSM)"); return SONIC_ERR_INVALID_ARG; }
  const int64_t NB = 1LL << (srs->tab_c - 1);
  int64_t S = (NB + world - 1) / world;
  S = (S + MSM_SLICE_QUANTUM - 1) / MSM_SLICE_QUANTUM * MSM_SLICE_QUANTUM;
  *n_buckets = NB;
  *slice_len = S;
  return SONIC_OK;
}

int sonic_msm_accumulate_dev(sonic_msm_lane_t* l, const sonic_srs_t* srs, int basis, int64_t e0, const void* d_scalars, int64_t n,
                             void* d_buckets, int64_t capacity) {
  API_BEGIN_ON(l ? l->device : -1)
  if (!l || !srs || n < 0 || (n > 0 && !d_scalars) || (basis != 0 && basis != 1) || !d_buckets) return SONIC_ERR_INVALID_ARG;
  if (!same_device(l, srs, "sonic_msm_accumulate_dev")) return SONIC_ERR_INVALID_ARG;
  if (n > 0 && !srs_range_ok("msm over SRS", srs, e0, n)) return SONIC_ERR_SRS_INDEX;
  if (n > 0 && !srs_held_ok("msm over SRS", srs, e0, n)) return SONIC_ERR_INVALID_ARG;
  if (srs->tab_W <= 1 || srs->tab_endo) { set_error("sonic_msm_accumulate_dev needs the full window tables of the SRS"); return SONIC_ERR_INVALID_ARG; }
  const int64_t NB = 1LL << (srs->tab_c - 1);
  if (capacity < NB) { set_error("sonic_msm_accumulate_dev: room for %ld buckets, the plan has %ld", (long)capacity, (long)NB); return SONIC_ERR_INVALID_ARG; }
  std::lock_guard<std::mutex> g(l->mu);
  hipStream_t st = l->st;
  const Fr* dsc = static_cast<const Fr*>(d_scalars);
  HIP_OK(hipMemsetAsync(l->err.p, 0, 4, st));
  fr_check_enqueue(st, dsc, n, l->err.as<int>());
  // always over the tables (a term-range share may be small against the bucket set; every rank must fill the SAME buckets)
  MsmPlan pl = msm_plan_tables(n > 0 ? n : 1, srs->tab_c, srs->tab_W, srs->geo.npts());
  pl.accum_block = 64;
  MsmJob job{srs->basis(basis) + srs->geo.slot(e0), dsc, (long)n, nullptr};
  msm_enqueue_batch(st, l->ws, pl, &job, 1, false, static_cast<G1XYZZ*>(d_buckets));
  if (capacity > NB) HIP_OK(hipMemsetAsync(static_cast<G1XYZZ*>(d_buckets) + NB, 0, sizeof(G1XYZZ) * (size_t)(capacity - NB), st));   // padding = infinity
  HIP_OK(hipMemcpyAsync(l->h_err, l->err.p, 4, hipMemcpyDeviceToHost, st));
  API_END
}

int sonic_msm_reduce_slices_dev(sonic_msm_lane_t*, const sonic_srs_t*, const void*, int, int64_t, int64_t, void*) {
  set_error("sonic_msm_reduce_slices_dev is retired (its result grew from 192 to %d bytes): use sonic_msm_reduce_slices_dev_v2, which takes the buffer size", SONIC_G1_DEV_PARTIAL_BYTES);
  return SONIC_ERR_INVALID_ARG;
}
int sonic_msm_reduce_slices_dev_v2(sonic_msm_lane_t* l, const sonic_srs_t* srs, const void* d_slices, int k, int64_t slice_len, int64_t bucket_base,
                                   void* d_partial_out, size_t out_bytes) {
  API_BEGIN_ON(l ? l->device : -1)
  if (!l || !srs || !d_slices || k < 1 || !d_partial_out || slice_len < 1 || bucket_base < 0) return SONIC_ERR_INVALID_ARG;
  if (out_bytes < sizeof(MsmSlot)) { set_error("sonic_msm_reduce_slices_dev_v2: the result takes %zu bytes of device memory (SONIC_G1_DEV_PARTIAL_BYTES), the buffer has %zu", sizeof(MsmSlot), out_bytes); return SONIC_ERR_INVALID_ARG; }
  if (!same_device(l, srs, "sonic_msm_reduce_slices_dev_v2")) return SONIC_ERR_INVALID_ARG;
  if (slice_len % MSM_SLICE_QUANTUM || bucket_base % MSM_SLICE_QUANTUM) { set_error("sonic_msm_reduce_slices_dev: slice length and base must be multiples of %ld (sonic_msm_exchange_layout)", (long)MSM_SLICE_QUANTUM); return SONIC_ERR_INVALID_ARG; }
  std::lock_guard<std::mutex> g(l->mu);
  hipStream_t st = l->st;
  msm_reduce_slices_enqueue(st, l->ws, static_cast<const G1XYZZ*>(d_slices), k, slice_len, bucket_base, srs->tab_c, l->slot.as<MsmSlot>());
  HIP_OK(hipMemcpyAsync(d_partial_out, l->slot.p, sizeof(MsmSlot), hipMemcpyDeviceToDevice, st));
  API_END
}

// waits for what the lane has queued (accumulate / reduce / submit_dev) and reports a non-canonical scalar
int sonic_msm_lane_sync(sonic_msm_lane_t* l) {
  API_BEGIN_ON(l ? l->device : -1)
  if (!l) return SONIC_ERR_INVALID_ARG;
  std::lock_guard<std::mutex> g(l->mu);
  HIP_OK(hipStreamSynchronize(l->st));
  if (*l->h_err) { *l->h_err = 0; set_error("msm over SRS: non-canonical scalar"); return SONIC_ERR_BAD_ENCODING; }
  API_END
}

// ---- ONE MSM over several GPUs of this process (include/sonic_hip.h, "N GPUs from ONE host process") -------------------------------
// One host thread per replica; thread r owns a lane on srs[r]'s GPU.  mode 0: every GPU a whole MSM over its term range, the host adds
// the partial sums.  mode 1: every GPU accumulates its term range into a full bucket set, waits for the others at a host barrier, pulls
// ITS bucket range from every peer (hipMemcpyPeerAsync on its own lane's stream: xGMI is point to point, the world - 1 pulls of a GPU
// run on world - 1 links), adds the slices, reduces 1/world of the buckets and reports its device-side result; the host adds those.
namespace {
struct HostBarrier {
  std::mutex mu; std::condition_variable cv; int n, waiting = 0, phase = 0;
  explicit HostBarrier(int n_) : n(n_) {}
  void wait() {
    std::unique_lock<std::mutex> l(mu);
    const int ph = phase;
    if (++waiting == n) { waiting = 0; phase++; cv.notify_all(); return; }
    cv.wait(l, [&] { return phase != ph; });
  }
};
}
static int msm_multi(const sonic_srs_t* const* srs, int world, int basis, const int64_t* e0, const void* const* d_scalars, const uint8_t* const* h_scalars,
                     const int64_t* n, int mode, uint8_t out_g1[96]) {
  if (!srs || world < 1 || world > 64 || !out_g1 || (basis != 0 && basis != 1) || (mode != 0 && mode != 1)) return SONIC_ERR_INVALID_ARG;
  for (int r = 0; r < world; r++) {
    if (!srs[r] || n[r] < 0 || (n[r] > 0 && !(d_scalars ? d_scalars[r] : (const void*)h_scalars[r]))) return SONIC_ERR_INVALID_ARG;
    if (srs[r]->d != srs[0]->d) { set_error("sonic_msm_g1_srs_multi: replica %d has d = %ld, replica 0 d = %ld", r, (long)srs[r]->d, (long)srs[0]->d); return SONIC_ERR_INVALID_ARG; }
  }
  int64_t NB = 0, S = 0;
  if (mode == 1 && world > 1) {
    for (int r = 0; r < world; r++) {
      int64_t nb_r = 0, s_r = 0;
      int rc = sonic_msm_exchange_layout(srs[r], world, &nb_r, &s_r);
      if (rc) return rc;
      if (r == 0) { NB = nb_r; S = s_r; }
      else if (nb_r != NB || s_r != S) { set_error("sonic_msm_g1_srs_multi: replica %d runs another MSM plan than replica 0 (window tables differ)", r); return SONIC_ERR_INVALID_ARG; }
    }
  }
  const bool exchange = mode == 1 && world > 1;
  std::vector<int> rcs((size_t)world, SONIC_OK);
  std::vector<std::string> errs((size_t)world);
  std::vector<G1XYZZ> partial((size_t)world, G1XYZZ::inf());
  std::vector<uint8_t> blobs(exchange ? sizeof(MsmSlot) * (size_t)world : 0);
  std::vector<void*> bucket_ptr((size_t)world, nullptr);       // each rank's full bucket set (mode 1), read by its peers
  HostBarrier bar(world);
  auto body = [&](int r) {
    int rc = SONIC_OK;
    const int dev = srs[r]->device;
    bool at_barrier_1 = false, at_barrier_2 = false;
    auto fail = [&](int code) { rc = code; char b[512]; sonic_last_error(b, sizeof b); errs[(size_t)r] = b; };
    try {
      DeviceScope scope(dev);
      PooledLane pooled(current_ctx());          // the device's pooled lanes keep their workspaces and exchange buffers from call to call
      sonic_msm_lane_t* lane = pooled.lane;
      do {
        const void* sc = d_scalars ? d_scalars[r] : nullptr;
        if (!d_scalars && n[r] > 0) {
          lane->x_scalars.ensure(32 * (size_t)n[r]);
          HIP_OK(hipMemcpyAsync(lane->x_scalars.p, h_scalars[r], 32 * (size_t)n[r], hipMemcpyHostToDevice, lane->st));
          sc = lane->x_scalars.p;
        }
        if (!exchange) {
          uint8_t part[192];
          if ((rc = sonic_msm_submit(lane, srs[r], basis, e0[r], sc, n[r])) || (rc = sonic_msm_collect(lane, nullptr, part))) { fail(rc); (void)hipStreamSynchronize(lane->st); break; }
          memcpy(&partial[(size_t)r], part, 192);
          break;
        }
        const size_t cap = (size_t)world * (size_t)S;
        lane->x_buckets.ensure(cap * sizeof(G1XYZZ)); lane->x_slices.ensure(cap * sizeof(G1XYZZ)); lane->x_part.ensure(sizeof(MsmSlot));
        if ((rc = sonic_msm_accumulate_dev(lane, srs[r], basis, e0[r], sc, n[r], lane->x_buckets.p, (int64_t)cap)) || (rc = sonic_msm_lane_sync(lane))) fail(rc);
        if (rc) (void)hipStreamSynchronize(lane->st);
        bucket_ptr[(size_t)r] = rc ? nullptr : lane->x_buckets.p;
        bar.wait(); at_barrier_1 = true;                           // every rank's buckets are complete (or it has failed)
        bool all = true;
        for (int q = 0; q < world; q++) all = all && bucket_ptr[(size_t)q] != nullptr;
        if (all) {
          try {
            // direct reads over xGMI where the GPUs are linked: ask once per pair (a runtime that refuses, or has it on already, still
            // copies -- staged -- so the answer is not an error here)
            for (int q = 0; q < world; q++)
              if (srs[q]->device != dev) { if (hipDeviceEnablePeerAccess(srs[q]->device, 0) != hipSuccess) (void)hipGetLastError(); }
            for (int q = 0; q < world; q++)                        // slice r of rank q -> slot q of my [world][S] buffer
              HIP_OK(hipMemcpyPeerAsync(lane->x_slices.as<G1XYZZ>() + (size_t)q * S, dev, static_cast<const G1XYZZ*>(bucket_ptr[(size_t)q]) + (size_t)r * S,
                                        srs[q]->device, (size_t)S * sizeof(G1XYZZ), lane->st));
          } catch (const HipFail& f) { fail(f.code); }
          if (!rc && ((rc = sonic_msm_reduce_slices_dev_v2(lane, srs[r], lane->x_slices.p, world, S, (int64_t)r * S, lane->x_part.p, sizeof(MsmSlot))) ||
                      (rc = sonic_msm_lane_sync(lane)))) fail(rc);
          if (!rc) {
            try { HIP_OK(hipMemcpy(&blobs[sizeof(MsmSlot) * (size_t)r], lane->x_part.p, sizeof(MsmSlot), hipMemcpyDeviceToHost)); } catch (const HipFail& f) { fail(f.code); }
          }
        } else if (!rc) { rc = -1; errs[(size_t)r] = "a peer rank failed before the bucket exchange"; }      // (secondary: the peer's own status is the call's)
        (void)hipStreamSynchronize(lane->st);
        bar.wait(); at_barrier_2 = true;                           // nobody re-uses its buckets while a peer still reads them
      } while (false);
    } catch (const HipFail& f) { fail(f.code); }
    catch (const std::exception& e) { rc = SONIC_ERR_HIP; errs[(size_t)r] = e.what(); }       // (nothing may leave a thread's body: std::terminate)
    catch (...) { rc = SONIC_ERR_HIP; errs[(size_t)r] = "unknown exception"; }
    if (exchange) { if (!at_barrier_1) bar.wait(); if (!at_barrier_2) bar.wait(); }
    rcs[(size_t)r] = rc;
  };
  if (world == 1) body(0);
  else {
    ThreadGroup th;
    for (int r = 0; r < world; r++) th.emplace_back(body, r);
    for (auto& t : th) t.join();
  }
  for (int pass = 0; pass < 2; pass++)               // a rank's own failure first; "a peer failed" only if nothing else explains it
    for (int r = 0; r < world; r++)
      if (pass == 0 ? rcs[(size_t)r] > 0 : rcs[(size_t)r] != 0) {
        set_error("sonic_msm_g1_srs_multi, rank %d (device %d): %s", r, srs[r]->device, errs[(size_t)r].c_str());
        return rcs[(size_t)r] > 0 ? rcs[(size_t)r] : SONIC_ERR_HIP;
      }
  if (exchange) return sonic_g1_sum_dev_partials(blobs.data(), world, out_g1);
  G1XYZZ acc = G1XYZZ::inf();
  for (int r = 0; r < world; r++) acc = g1_add(acc, partial[(size_t)r]);
  g1_canonical_bytes_host(acc, out_g1);
  return SONIC_OK;
}

int sonic_msm_g1_srs_multi_dev(const sonic_srs_t* const* srs, int world, int basis, const int64_t* e0, const void* const* d_scalars, const int64_t* n, int mode,
                               uint8_t out_g1[96]) {
  if (!e0 || !d_scalars || !n) return SONIC_ERR_INVALID_ARG;
  try { return msm_multi(srs, world, basis, e0, d_scalars, nullptr, n, mode, out_g1); }
  catch (const std::exception& e) { set_error("%s", e.what()); return SONIC_ERR_HIP; }
}
int sonic_msm_g1_srs_multi(const sonic_srs_t* const* srs, int world, int basis, int64_t e0, const uint8_t* scalars, int64_t n, int mode, uint8_t out_g1[96]) {
  if (world < 1 || world > 64 || n < 0 || (n > 0 && !scalars)) return SONIC_ERR_INVALID_ARG;
  std::vector<int64_t> e((size_t)world), cnt((size_t)world);
  std::vector<const uint8_t*> hs((size_t)world);
  for (int r = 0; r < world; r++) {                              // contiguous term ranges, as even as possible
    const int64_t lo = n * r / world, hi = n * (r + 1) / world;
    e[(size_t)r] = e0 + lo; cnt[(size_t)r] = hi - lo; hs[(size_t)r] = scalars + 32 * (size_t)lo;
  }
  try { return msm_multi(srs, world, basis, e.data(), nullptr, hs.data(), cnt.data(), mode, out_g1); }
  catch (const std::exception& e2) { set_error("%s", e2.what()); return SONIC_ERR_HIP; }
}

// the device-side partials of sonic_msm_submit_dev / sonic_msm_reduce_slices_dev (SONIC_G1_DEV_PARTIAL_BYTES each: what the bulk kernels
// leave of an MSM, a handful of points the host folds) -> their sum, normalised
static_assert(sizeof(MsmSlot) == SONIC_G1_DEV_PARTIAL_BYTES, "SONIC_G1_DEV_PARTIAL_BYTES is the size of a device-side MSM result");
int sonic_g1_sum_dev_partials(const uint8_t* blobs, int k, uint8_t out_g1[96]) {
  if (!blobs || k < 1 || !out_g1) return SONIC_ERR_INVALID_ARG;
  G1XYZZ acc = G1XYZZ::inf();
  std::unique_ptr<MsmSlot> s(new MsmSlot());
  for (int i = 0; i < k; i++) {
    memcpy(s.get(), blobs + sizeof(MsmSlot) * (size_t)i, sizeof(MsmSlot));
    if (s->W < 0 || s->W > MSM_MAX_WINDOWS || (s->pad1 == 1 && s->W >= MSM_MAX_WINDOWS) || (s->pad1 == 2 && s->W >= MSM_MAX_WINDOWS - MSM_ENDO_SLOT_OFFSET) || (s->pad1 == 3 && (s->W >= MSM_MAX_WINDOWS || s->pad0 < 1 || (s->pad0 & (s->pad0 - 1)))) || s->pad1 < 0 || s->pad1 > 3 || s->c < 0 || s->c > 32) { set_error("sonic_g1_sum_dev_partials: blob %d is not a device-side MSM result", i); return SONIC_ERR_INVALID_ARG; }
    acc = g1_add(acc, msm_finish_host(*s));
  }
  g1_canonical_bytes_host(acc, out_g1);
  return SONIC_OK;
}

int sonic_g1_sum_partials(const uint8_t* partials, int k, uint8_t out_g1[96]) {
  if (!partials || k < 1 || !out_g1) return SONIC_ERR_INVALID_ARG;
  G1XYZZ acc = G1XYZZ::inf();
  for (int i = 0; i < k; i++) { G1XYZZ p; memcpy(&p, partials + sizeof(G1XYZZ) * i, sizeof p); acc = g1_add(acc, p); }
  g1_canonical_bytes_host(acc, out_g1);
  return SONIC_OK;
}

}  // extern "C"
