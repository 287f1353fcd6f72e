// The helper of helped verification (include/sonic_hip.h, "Helped verification"): ONE signature of correct
// computation -- an HscProof with m = K, Signature.hs:38-72 -- over the (y_k, z_k) of K core proofs, for the s(X, Y) of the handle's
// circuit, with u and v drawn from the aggregate's own transcript (fs.hpp, "helped verification").  It is the throughput form of what
// sonic_prover_hsc_prove does one pair at a time on one stream:
//
//   pass 1   per tile of up to AGG_TILE pairs: the tile's power tables in ONE launch, its polynomials s(X, y_j) in ONE launch (on a
//            prepared handle also the diagonal parts and the vectors y_j^{n+1+q}), then S_j and (s_j, W_j) of the whole tile as ONE
//            chain of up to MSM_MAX_JOBS jobs.  Tiles are dealt over the handle's lanes, so that one tile's sort and reduction run
//            under another's accumulation.                                                        host: u = H(.. S_j, s_j, W_j ..)
//   pass 2   s(u, Y) and C once; per tile W'_j and (s'_j, Q_j) as one chain of 2 x AGG_TILE jobs.  The polynomials of pass 1 are
//            kept when K (3n + 1) 32 bytes fit AGG_KEEP_BUDGET and recomputed per tile otherwise.  host: v = H(.. C, s'_j, W'_j, Q_j ..)
//   pass 3   Q_v.
//
// Device memory is bounded by the budget and the lanes, not by K: a lane holds one tile's tables, polynomials and window-sum slots, and
// the slots of a finished tile go to pinned host memory behind it on the lane's stream.
#include "prover.hpp"

namespace sonic {

constexpr int AGG_TILE = 8;                          // pairs per polynomial launch; 2 x AGG_TILE = MSM_MAX_JOBS jobs per chain
static_assert(2 * AGG_TILE == MSM_MAX_JOBS, "a tile's two MSMs per pair fill one batched chain");
// pass 2 reads s(X, y_j) again.  Keeping all K of them costs K (3n + 1) 32 bytes (n = 2^18, K = 64: 1.6 GB); above this they are
// recomputed tile by tile instead, which reads the circuit once more per tile.  SONIC_AGG_KEEP=0 / 1 forces either.
constexpr size_t AGG_KEEP_BUDGET = (size_t)4 << 30;

// workgroups of a launch over `items` gates: as poly.hip's elementwise launches (few fat workgroups for short arrays)
static unsigned agg_grid(long items) {
  const long full = ceil_div(items, 256L);
  return (unsigned)(items <= (1L << 19) && full > 64 ? 64 : (full > 0 ? full : 1));
}

// The J power tables of a tile in one launch: out[j * len + i] = y_j^(e0 + i), y_j = pairs[stride j], its inverse pairs[stride j + 1]; blockIdx.y = j.
// PER elements per thread, strided by the block, as k_scale_powers.
__global__ __launch_bounds__(256) void k_agg_powers(const Fr* __restrict__ pairs, int stride, Fr* __restrict__ out, long len, long e0, int PER) {
  const long base = (long)blockIdx.x * (256 * PER) + threadIdx.x;
  if (base >= len) return;
  const Fr x = pairs[stride * blockIdx.y], xinv = pairs[stride * blockIdx.y + 1];
  Fr* o = out + (long)blockIdx.y * len;
  const long e = e0 + base;
  Fr p = e >= 0 ? fp_pow_u64(x, (uint64_t)e) : fp_pow_u64(xinv, (uint64_t)(-e));
  const Fr step = fp_pow_u64(x, 256);
#pragma unroll 1
  for (int k = 0; k < PER; k++) {
    const long i = base + (long)k * 256;
    if (i >= len) break;
    o[i] = p;
    p = fp_mul(p, step);
  }
}

// what the two polynomial kernels of a tile read and write: J <= AGG_TILE pairs
//   pw[j * pw_len + e + n] = y_j^e, e in [-n, n + Q]
//   sy[j * (3n + 1) + e + n] = the coefficient of X^e in s(X, y_j), e in [-n, 2n]           (Constraints.hs:39-49, as k_s_of_y)
//   diag[j * n + i - 1] = -(y_j^i + y_j^-i), yq[j * Q + q] = y_j^{n+1+q}                     (null on a handle that is not prepared)
struct AggTile {
  const Fr* pw; long pw_len;
  Fr* sy; Fr* diag; Fr* yq;
  long n, Q; int J;
};

// the part of gate i every form shares: X^{i+n} takes the diagonal terms; and the prepared handle's copy of them
__device__ __forceinline__ void agg_store_wo(const AggTile& t, int j, long i, const Fr& w) {
  const Fr* pw = t.pw + (long)j * t.pw_len;
  const Fr dg = fp_add(pw[t.n + i], pw[t.n - i]);
  t.sy[(long)j * (3 * t.n + 1) + 2 * t.n + i] = fp_sub(w, dg);
  if (t.diag) t.diag[(long)j * t.n + i - 1] = fp_neg(dg);
}
__device__ __forceinline__ void agg_tail(const AggTile& t) {
  // X^0 of every polynomial, and the Q powers a prepared handle multiplies the C_q by
  for (long k = (long)blockIdx.x * 256 + threadIdx.x; k < (long)t.J * (t.Q + 1); k += (long)gridDim.x * 256) {
    const int j = (int)(k / (t.Q + 1));
    const long q = k - (long)j * (t.Q + 1);
    if (q == t.Q) t.sy[(long)j * (3 * t.n + 1) + t.n] = Fr::zero();
    else if (t.yq) t.yq[(long)j * t.Q + q] = t.pw[(long)j * t.pw_len + 2 * t.n + 1 + q];
  }
}

// Dense weights.  blockIdx.y = matrix (wL, wR, wO): a thread holds AGG_TILE running sums -- one per pair, not one triple per pair,
// which would be 24 field elements = 192 registers before the product's own -- and reads its weight ONCE for the whole tile.  The
// powers y_j^{n+1+q} are the same address for every lane.
__global__ __launch_bounds__(256) void k_agg_s_of_y(const Fr* __restrict__ wL, const Fr* __restrict__ wR, const Fr* __restrict__ wO, AggTile t) {
  const int m = blockIdx.y;
  const Fr* __restrict__ w = m == 0 ? wL : (m == 1 ? wR : wO);
  const long n = t.n, Q = t.Q, slen = 3 * n + 1;
  for (long i = (long)blockIdx.x * 256 + threadIdx.x + 1; i <= n; i += (long)gridDim.x * 256) {
    Fr acc[AGG_TILE];
#pragma unroll
    for (int j = 0; j < AGG_TILE; j++) acc[j] = Fr::zero();
    for (long q = 0; q < Q; q++) {
      const Fr x = w[q * n + i - 1];
      const Fr* yq = t.pw + 2 * n + 1 + q;
#pragma unroll
      for (int j = 0; j < AGG_TILE; j++) if (j < t.J) acc[j] = fp_add(acc[j], fp_mul(x, yq[(long)j * t.pw_len]));
    }
#pragma unroll
    for (int j = 0; j < AGG_TILE; j++) {
      if (j >= t.J) continue;
      if (m == 0) t.sy[(long)j * slen + n - i] = acc[j];
      else if (m == 1) t.sy[(long)j * slen + n + i] = acc[j];
      else agg_store_wo(t, j, i, acc[j]);
    }
  }
  if (m == 0) agg_tail(t);
}

// Sparse weights, over the column-major copy (csr.hpp: the entries of gate i, rows ascending -- so wL's entries come first, then wR's,
// then wO's).  One thread per gate walks its column ONCE for the whole tile with AGG_TILE running sums, and hands them over whenever the
// matrix changes.  The powers are gathered per entry: from LDS when the tile's J x Q of them fit `stage` bytes of it, else through L2.
__device__ __forceinline__ int agg_matrix(int r, int Q) { return r >= 2 * Q ? 2 : (r >= Q ? 1 : 0); }
__global__ __launch_bounds__(256) void k_agg_s_of_y_csc(const int32_t* __restrict__ col_ptr, const int32_t* __restrict__ row, const Fr* __restrict__ val, AggTile t, int stage) {
  extern __shared__ uint32_t agg_lds[];
  const long n = t.n, slen = 3 * n + 1;
  const int Q = (int)t.Q;
  const Fr* yq = t.pw + 2 * n + 1;      // y_j^{n+1+q} at yq[j * ystride + q]
  long ystride = t.pw_len;
  if (stage) {
    Fr* sh = reinterpret_cast<Fr*>(agg_lds);
    for (int k = threadIdx.x; k < t.J * Q; k += 256) sh[k] = yq[(long)(k / Q) * t.pw_len + k % Q];
    __syncthreads();
    yq = sh;
    ystride = Q;
  }
  for (long i = (long)blockIdx.x * 256 + threadIdx.x + 1; i <= n; i += (long)gridDim.x * 256) {
    Fr acc[AGG_TILE];
#pragma unroll
    for (int j = 0; j < AGG_TILE; j++) acc[j] = Fr::zero();
    int cur = 0;
    auto hand_over = [&](int upto) {      // the sums of matrices cur .. upto - 1: the first holds what was gathered, the others nothing
      for (; cur < upto; cur++) {
#pragma unroll
        for (int j = 0; j < AGG_TILE; j++) {
          if (j >= t.J) continue;
          if (cur == 0) t.sy[(long)j * slen + n - i] = acc[j];
          else if (cur == 1) t.sy[(long)j * slen + n + i] = acc[j];
          else agg_store_wo(t, j, i, acc[j]);
          acc[j] = Fr::zero();
        }
      }
    };
    const int k1 = col_ptr[i];
    for (int k = col_ptr[i - 1]; k < k1; k++) {
      const int r = row[k], m = agg_matrix(r, Q);
      if (m != cur) hand_over(m);
      const Fr x = val[k];
      const Fr* y = yq + (r - m * Q);
#pragma unroll
      for (int j = 0; j < AGG_TILE; j++) if (j < t.J) acc[j] = fp_add(acc[j], fp_mul(x, y[(long)j * ystride]));
    }
    hand_over(3);
  }
  agg_tail(t);
}

namespace {

constexpr size_t AGG_CSC_LDS = 48 * 1024;

int agg_scale_per(long n) {      // elements per thread of a power table (poly.hip, scale_per)
  long per = n / (256L * 64L);
  if (per > 32) per = 32;
  if (per < 2) per = 2;
  return (int)per;
}

// what a lane holds for the tile it works on
struct AggLane {
  DevBuf pw, sy, diag, yq, slots;
  bool used = false;
};

// the tile's power tables and polynomials, queued on `st`; the {y_j, y_j^-1} are 4 elements apart ({z_j, z_j^-1} lie between)
void agg_tile_polys(sonic_prover* p, hipStream_t st, const Fr* ypairs, int J, AggLane& a, Fr* sy, bool want_diag) {
  const long n = p->n, Q = p->Q, pw_len = 2 * n + Q + 1;
  const int per = agg_scale_per(pw_len);
  LAUNCH(k_agg_powers, dim3((unsigned)ceil_div(pw_len, 256L * per), (unsigned)J), 256, 0, st, ypairs, 4, a.pw.as<Fr>(), pw_len, -n, per);
  AggTile t{a.pw.as<Fr>(), pw_len, sy, want_diag ? a.diag.as<Fr>() : nullptr, want_diag ? a.yq.as<Fr>() : nullptr, n, Q, J};
  if (p->csr) {
    const size_t lds = sizeof(Fr) * (size_t)J * (size_t)Q;
    const int stage = lds <= AGG_CSC_LDS ? 1 : 0;
    LAUNCH(k_agg_s_of_y_csc, agg_grid(n), 256, stage ? (unsigned)lds : 0u, st, (const int32_t*)p->sp.col_ptr.as<int32_t>(), (const int32_t*)p->sp.row.as<int32_t>(),
           (const Fr*)p->sp.cval.as<Fr>(), t, stage);
  } else {
    LAUNCH(k_agg_s_of_y, dim3(agg_grid(n), 3), 256, 0, st, (const Fr*)p->wL.as<Fr>(), (const Fr*)p->wR.as<Fr>(), (const Fr*)p->wO.as<Fr>(), t);
  }
}

void agg_s_of_u(sonic_prover* p, hipStream_t st, const Fr* upow, Fr* out) {
  sonic_prover::CsrBufs& b = p->sp;
  if (p->csr) s_of_u_csr_enqueue(st, b.row_ptr.as<int32_t>(), b.col.as<int32_t>(), b.val.as<Fr>(), b.chunk_row.as<int32_t>(), b.chunk_begin.as<int32_t>(),
                                 b.nchunks, b.row_chunk.as<int32_t>(), upow, p->n, p->Q, out, b.partial.as<Fr>());
  else s_of_u_enqueue(st, p->wL.as<Fr>(), p->wR.as<Fr>(), p->wO.as<Fr>(), upow, p->n, p->Q, out, p->tmp);
}

// pinned host memory, released with the call
struct PinnedSlots {
  MsmSlot* p = nullptr;
  explicit PinnedSlots(size_t count) { HIP_OK(hipHostMalloc(reinterpret_cast<void**>(&p), sizeof(MsmSlot) * count, hipHostMallocDefault)); memset(p, 0, sizeof(MsmSlot) * count); }
  ~PinnedSlots() { if (p) (void)hipHostFree(p); }
  PinnedSlots(const PinnedSlots&) = delete;
  PinnedSlots& operator=(const PinnedSlots&) = delete;
};

// Whatever happens, nothing of the call is left running when its buffers go: the main stream and every lane drained
struct AggDrain {
  sonic_prover* p;
  ~AggDrain() {
    for (int i = 0; i < p->n_lanes; i++) (void)hipStreamSynchronize(p->lanes[i].st);
    (void)hipStreamSynchronize(p->st);
  }
};

// the host tails of `count` slots on up to four threads (a slot over window tables is one short walk)
void agg_finish_slots(const MsmSlot* hs, size_t count, G1XYZZ* out) {
  const int nt = (int)std::min<size_t>(4, count / 32 + 1);
  ThreadGroup th;
  for (int w = 1; w < nt; w++) th.emplace_back([=] { for (size_t i = (size_t)w; i < count; i += (size_t)nt) out[i] = msm_finish_host(hs[i]); });
  for (size_t i = 0; i < count; i += (size_t)nt) out[i] = msm_finish_host(hs[i]);
}

int agg_keep(size_t bytes) {
  const char* e = getenv("SONIC_AGG_KEEP");
  if (e && (e[0] == '0' || e[0] == '1') && !e[1]) return e[0] == '1';
  return bytes <= AGG_KEEP_BUDGET;
}

}  // namespace
}  // namespace sonic

extern "C" {

int sonic_prover_aggregate_core(sonic_prover_t* p, const uint8_t weights_digest[32], int64_t K, const uint8_t* yz, uint8_t* out) {
  API_BEGIN_ON(p ? p->device : -1)
  if (!p || !weights_digest || K < 1 || K > (1L << 24) || !yz || !out) { set_error("sonic_prover_aggregate_core: bad argument (need K >= 1 pairs)"); return SONIC_ERR_INVALID_ARG; }
  std::lock_guard<std::mutex> g(p->mu);
  if (p->in_flight) { set_error("sonic_prover_aggregate_core: a submitted proof has not been collected yet"); return SONIC_ERR_INVALID_ARG; }
  if (p->share_world > 1) { set_error("sonic_prover_aggregate_core: the handle runs one rank's share of a proof (sonic_prover_set_share)"); return SONIC_ERR_INVALID_ARG; }
  for (long k = 0; k < 2 * K; k++)
    if (bytes_are_zero(yz + 32 * k, 32)) { set_error("sonic_prover_aggregate_core: %s of pair %ld is zero: Laurent evaluation at 0 divides by zero", k & 1 ? "z" : "y", k >> 1); return SONIC_ERR_INEXACT_DIVISION; }
  const sonic_srs* srs = p->srs;
  const long n = p->n, Q = p->Q, d = srs->d;
  const long s_lo = -n, s_len = 3 * n + 1, u_lo = -n, u_len = 2 * n + Q + 1, pw_len = 2 * n + Q + 1;
  const AggLayout A{K};
  uint8_t srs_id[32];
  int rc = sonic_fs_srs_id(srs, srs_id);
  if (rc) return rc;
  FsTranscript tr;
  fs_agg_begin(tr, n, Q, d, weights_digest, srs_id, K, yz);

  hipStream_t st = p->st;
  EnqueueLock enq(p);      // (to the end: the lanes are queued on and waited for here)
  const bool prepared = p->prepared;
  const int n_lanes = p->n_lanes;
  const long tiles = (K + AGG_TILE - 1) / AGG_TILE;
  const bool keep = agg_keep(sizeof(Fr) * (size_t)K * (size_t)s_len);
  // scalars: y_k at 2k, z_k at 2k + 1, then u, v; PR holds {x, x^-1} of each
  const long NS = 2 * K + 2;
  DevBuf S(sizeof(Fr) * NS), PR(sizeof(Fr) * 2 * NS), frout(sizeof(Fr) * (2 * K)), flags(4), sy_all, su(sizeof(Fr) * u_len), upw(sizeof(Fr) * s_len), one_slot(sizeof(MsmSlot) * 2);
  std::vector<AggLane> al((size_t)n_lanes);
  if (keep) sy_all.alloc(sizeof(Fr) * (size_t)K * (size_t)s_len);
  // host side of the slots, by field: S_k at k, W_k at K + k, S_k's side slot at 2K + k, W'_k at 3K + k, Q_k at 4K + k; then C, Q_v
  const size_t NSLOT = 5 * (size_t)K + 2;
  PinnedSlots hs(NSLOT);
  AggDrain drain{p};
  int* fl = flags.as<int>();
  Fr* fo = frout.as<Fr>();                      // s_k at k, s'_k at K + k
  const Fr* P0 = PR.as<Fr>();
  auto pY = [&](long k) { return P0 + 2 * (2 * k); };
  auto pZ = [&](long k) { return P0 + 2 * (2 * k + 1); };
  const Fr *pU = P0 + 2 * (2 * K), *pV = P0 + 2 * (2 * K + 1);
  hipEvent_t ready = p->ev_su;                  // (no proof is in flight: the handle's events are free)

  HIP_OK(hipMemsetAsync(fl, 0, 4, st));
  HIP_OK(hipMemcpyAsync(S.p, yz, 64 * (size_t)K, hipMemcpyHostToDevice, st));
  fr_to_mont_enqueue(st, S.as<Fr>(), 2 * K, fl);
  fr_with_inverse_enqueue(st, S.as<Fr>(), (int)(2 * K), PR.as<Fr>());
  HIP_OK(hipEventRecord(ready, st));

  auto lane_begin = [&](long tile) -> int {
    const int li = (int)(tile % n_lanes);
    AggLane& a = al[(size_t)li];
    if (!a.used) {
      a.used = true;
      a.pw.alloc(sizeof(Fr) * (size_t)AGG_TILE * (size_t)pw_len);
      if (!keep) a.sy.alloc(sizeof(Fr) * (size_t)AGG_TILE * (size_t)s_len);
      if (prepared) { a.diag.alloc(sizeof(Fr) * (size_t)AGG_TILE * (size_t)n); a.yq.alloc(sizeof(Fr) * (size_t)AGG_TILE * (size_t)Q); }
      a.slots.alloc(sizeof(MsmSlot) * 3 * AGG_TILE);
      HIP_OK(hipStreamWaitEvent(p->lanes[li].st, ready, 0));
      HIP_OK(hipMemsetAsync(a.slots.p, 0, sizeof(MsmSlot) * 3 * AGG_TILE, p->lanes[li].st));      // W = 0: an empty sum until a slot's MSM has run
    }
    return li;
  };
  // the end of a pass: the main stream behind every lane, then the host behind the main stream
  auto join = [&] {
    for (int li = 0; li < n_lanes; li++) {
      if (!al[(size_t)li].used) continue;
      HIP_OK(hipEventRecord(p->lanes[li].done, p->lanes[li].st));
      HIP_OK(hipStreamWaitEvent(st, p->lanes[li].done, 0));
    }
    return read_flags(st, flags);
  };
  // a tile's slots land on the host behind the tile, on its lane: J slots of one field, those of the pairs k0 .. k0 + J - 1
  auto slots_home = [&](hipStream_t ls, const MsmSlot* dev, long k0, int J, int field) {
    HIP_OK(hipMemcpyAsync(hs.p + field * K + k0, dev, sizeof(MsmSlot) * (size_t)J, hipMemcpyDeviceToHost, ls));
  };

  // ---- pass 1: S_j, (s_j, W_j) ----
  for (long tile = 0; tile < tiles; tile++) {
    const long k0 = tile * AGG_TILE;
    const int J = (int)std::min<long>(AGG_TILE, K - k0);
    const int li = lane_begin(tile);
    Lane& lane = p->lanes[li];
    AggLane& a = al[(size_t)li];
    hipStream_t ls = lane.st;
    Fr* sy = keep ? sy_all.as<Fr>() + (size_t)k0 * (size_t)s_len : a.sy.as<Fr>();
    MsmSlot* sl = a.slots.as<MsmSlot>();
    agg_tile_polys(p, ls, pY(k0), J, a, sy, prepared);
    MsmJob jobs[MSM_MAX_JOBS];
    for (int j = 0; j < J; j++) {
      const Fr* syj = sy + (size_t)j * (size_t)s_len;
      jobs[j] = prepared ? commit_job(ls, srs, a.diag.as<Fr>() + (size_t)j * (size_t)n, n + 1, n, d, &sl[j], fl)      // S_j, diagonal part   Signature.hs:42
                         : commit_job(ls, srs, syj, s_lo, s_len, d, &sl[j], fl);                                      // S_j
      jobs[J + j] = open_job(ls, srs, lane.sc[J + j], syj, s_lo, s_len, pZ(k0 + j), &fo[k0 + j], &sl[AGG_TILE + j], fl);   // (s_j, W_j)   :43
    }
    run_jobs(ls, srs, lane.ws, jobs, 2 * J);
    slots_home(ls, sl, k0, J, 0);
    slots_home(ls, sl + AGG_TILE, k0, J, 1);
    if (prepared) {                                                                                                   // sum_q y_j^{n+q} C_q, Q-term MSMs
      for (int j = 0; j < J; j++)
        msm_enqueue(ls, lane.ws, p->cq_tab.p ? msm_plan_tables(Q, CQ_TAB_C, CQ_TAB_W, Q) : msm_plan(Q),
                    PointArray::packed(p->cq_tab.p ? p->cq_tab.as<G1Affine>() : p->cq.as<G1Affine>()), a.yq.as<Fr>() + (size_t)j * (size_t)Q, Q, true, &sl[2 * AGG_TILE + j]);
      slots_home(ls, sl + 2 * AGG_TILE, k0, J, 2);
    }
  }
  int hflags = join();
  if (hflags) return flags_to_status(hflags, "sonic_prover_aggregate_core");

  // the host tails of a pass and its evaluations, then the bytes the transcript absorbs
  std::vector<uint8_t> hfr(32 * (size_t)(2 * K));
  std::vector<G1XYZZ> sums(NSLOT);
  std::vector<uint8_t> pts(96 * NSLOT);
  auto fr_home = [&](long from, long count) {
    fr_from_mont_enqueue(st, fo + from, count);
    HIP_OK(hipMemcpyAsync(&hfr[32 * (size_t)from], fo + from, 32 * (size_t)count, hipMemcpyDeviceToHost, st));
    HIP_OK(hipStreamSynchronize(st));
  };
  fr_home(0, K);
  agg_finish_slots(hs.p, (prepared ? 3 : 2) * (size_t)K, sums.data());
  if (prepared) for (long k = 0; k < K; k++) sums[(size_t)k] = g1_add(sums[(size_t)k], sums[2 * (size_t)K + (size_t)k]);
  g1_canonical_bytes_host_batch(sums.data(), (int)(2 * K), pts.data());
  for (long k = 0; k < K; k++) {
    uint8_t* o = out + A.hscS() + 224 * (size_t)k;
    memcpy(o, &pts[96 * (size_t)k], 96); memcpy(o + 96, &hfr[32 * (size_t)k], 32); memcpy(o + 128, &pts[96 * (size_t)(K + k)], 96);
  }
  uint8_t u[32], v[32];
  fs_agg_u(tr, K, out + A.hscS(), u);

  // ---- pass 2: C, W'_j, (s'_j, Q_j) ----
  HIP_OK(hipMemcpyAsync(S.as<Fr>() + 2 * K, u, 32, hipMemcpyHostToDevice, st));
  fr_to_mont_enqueue(st, S.as<Fr>() + 2 * K, 1, fl);
  fr_with_inverse_enqueue(st, S.as<Fr>() + 2 * K, 1, PR.as<Fr>() + 2 * (2 * K));
  poly_scale_powers_enqueue(st, nullptr, upw.as<Fr>(), s_len, -n, pU, pU + 1);                 // u^e, e in [-n, 2n]       Signature.hs:51
  agg_s_of_u(p, st, upw.as<Fr>(), su.as<Fr>());
  HIP_OK(hipEventRecord(ready, st));
  for (int li = 0; li < n_lanes; li++) if (al[(size_t)li].used) HIP_OK(hipStreamWaitEvent(p->lanes[li].st, ready, 0));
  {
    Lane& lane = p->lanes[0];                                                                  // C                        :52
    MsmJob job = commit_job(lane.st, srs, su.as<Fr>(), u_lo, u_len, d, one_slot.as<MsmSlot>(), fl);
    run_jobs(lane.st, srs, lane.ws, &job, 1);
    HIP_OK(hipMemcpyAsync(hs.p + 5 * K, one_slot.p, sizeof(MsmSlot), hipMemcpyDeviceToHost, lane.st));
  }
  for (long tile = 0; tile < tiles; tile++) {
    const long k0 = tile * AGG_TILE;
    const int J = (int)std::min<long>(AGG_TILE, K - k0);
    const int li = lane_begin(tile);
    Lane& lane = p->lanes[li];
    AggLane& a = al[(size_t)li];
    hipStream_t ls = lane.st;
    Fr* sy = keep ? sy_all.as<Fr>() + (size_t)k0 * (size_t)s_len : a.sy.as<Fr>();
    MsmSlot* sl = a.slots.as<MsmSlot>();
    if (!keep) agg_tile_polys(p, ls, pY(k0), J, a, sy, false);
    MsmJob jobs[MSM_MAX_JOBS];
    for (int j = 0; j < J; j++) {
      jobs[j] = open_job(ls, srs, lane.sc[j], sy + (size_t)j * (size_t)s_len, s_lo, s_len, pU, nullptr, &sl[j], fl);                       // W'_j         :54
      jobs[J + j] = open_job(ls, srs, lane.sc[J + j], su.as<Fr>(), u_lo, u_len, pY(k0 + j), &fo[K + k0 + j], &sl[AGG_TILE + j], fl);       // (s'_j, Q_j)  :55
    }
    run_jobs(ls, srs, lane.ws, jobs, 2 * J);
    slots_home(ls, sl, k0, J, 3);
    slots_home(ls, sl + AGG_TILE, k0, J, 4);
  }
  hflags = join();
  if (hflags) return flags_to_status(hflags, "sonic_prover_aggregate_core");
  fr_home(K, K);
  agg_finish_slots(hs.p + 3 * K, 2 * (size_t)K + 1, sums.data());      // W'_k, Q_k and C: one inversion normalises them
  g1_canonical_bytes_host_batch(sums.data(), (int)(2 * K + 1), pts.data());
  for (long k = 0; k < K; k++) {
    uint8_t* o = out + A.hscW() + 224 * (size_t)k;
    memcpy(o, &hfr[32 * (size_t)(K + k)], 32); memcpy(o + 32, &pts[96 * (size_t)k], 96); memcpy(o + 128, &pts[96 * (size_t)(K + k)], 96);
  }
  memcpy(out + A.C(), &pts[96 * (2 * (size_t)K)], 96);
  fs_agg_v(tr, K, out + A.C(), out + A.hscW(), v);

  // ---- pass 3: Q_v ----
  {
    Lane& lane = p->lanes[0];
    hipStream_t ls = lane.st;
    HIP_OK(hipMemcpyAsync(S.as<Fr>() + 2 * K + 1, v, 32, hipMemcpyHostToDevice, ls));
    fr_to_mont_enqueue(ls, S.as<Fr>() + 2 * K + 1, 1, fl);
    fr_with_inverse_enqueue(ls, S.as<Fr>() + 2 * K + 1, 1, PR.as<Fr>() + 2 * (2 * K + 1));
    MsmJob job = open_job(ls, srs, lane.sc[0], su.as<Fr>(), u_lo, u_len, pV, nullptr, one_slot.as<MsmSlot>() + 1, fl);      // Q_v          :63
    run_jobs(ls, srs, lane.ws, &job, 1, /*last=*/true);
    HIP_OK(hipMemcpyAsync(hs.p + 5 * K + 1, one_slot.as<MsmSlot>() + 1, sizeof(MsmSlot), hipMemcpyDeviceToHost, ls));
  }
  hflags = join();
  if (hflags) return flags_to_status(hflags, "sonic_prover_aggregate_core");
  g1_canonical_bytes_host(msm_finish_host(hs.p[5 * K + 1]), out + A.Qv());
  memcpy(out + A.u(), u, 32);
  memcpy(out + A.v(), v, 32);
  API_END
}

// ---- the transcript of an aggregate and the digest of a helped batch (fs.hpp); host only, no device ----
int sonic_fs_weights_digest(const uint8_t midstate[SONIC_FS_MIDSTATE_SIZE], uint8_t out[32]) {
  if (!midstate || !out) { set_error("sonic_fs_weights_digest: bad argument"); return SONIC_ERR_INVALID_ARG; }
  fs_weights_digest(midstate, out);
  return SONIC_OK;
}
int sonic_fs_aggregate_challenges(int64_t n, int64_t Q, int64_t d, const uint8_t weights_digest[32], const uint8_t srs_id[32], int64_t K, const uint8_t* yz,
                                  const uint8_t* aggregate, uint8_t out_uv[64]) {
  if (n < 1 || Q < 1 || d < 1 || !weights_digest || !srs_id || K < 1 || !yz || !aggregate || !out_uv) { set_error("sonic_fs_aggregate_challenges: bad argument"); return SONIC_ERR_INVALID_ARG; }
  fs_aggregate_challenges(n, Q, d, weights_digest, srs_id, K, yz, aggregate, out_uv);
  return SONIC_OK;
}
int sonic_verify_core_helped_digest(int64_t n, int64_t Q, int64_t d, const uint8_t weights_digest[32], const uint8_t srs_id[32], int64_t K, const uint8_t* proofs,
                                    const uint8_t* yz, const uint8_t* cs, const uint8_t* aggregate, uint8_t out[32]) {
  if (n < 1 || Q < 1 || d < 1 || !weights_digest || !srs_id || K < 1 || !proofs || !yz || !cs || !aggregate || !out) { set_error("sonic_verify_core_helped_digest: bad argument"); return SONIC_ERR_INVALID_ARG; }
  fs_core_helped_digest(n, Q, d, weights_digest, srs_id, K, proofs, yz, cs, aggregate, out);
  return SONIC_OK;
}

}  // extern "C"
