// Cross-translation-unit declarations inside libsonic_hip.so.
#pragma once
#include <atomic>
#include <exception>
#include "common.hpp"
#include "g1.hpp"
#include "msm.hpp"
#include "stream_pool.hpp"

struct sonic_srs;
struct sonic_prover;

namespace sonic {

struct NttTables;

// ---- devices (device.hip) ---------------------------------------------------------------------------------------------------------
// One host process may drive every GPU of the node (round 5): each handle -- SRS, prover, MSM lane -- is bound to the device it was
// made on, and what used to be process-wide state (the default stream, the mutex of the state-changing calls, the leased call
// contexts, the pool of blocking-MSM lanes, the twiddle tables and scratch of the stand-alone NTT entry points, per-device kernel
// attributes) lives in a DeviceCtx per ordinal.  Every entry point opens a DeviceScope: it makes the handle's device the calling
// thread's HIP device (hipSetDevice is per thread) for the duration of the call and puts the previous one back afterwards.
struct CallCtx;
struct DeviceCtx {
  int dev = -1;
  hipStream_t stream = nullptr;          // the device's default stream for the serialised (state-changing) calls; pool stream 0
  // the prover's stream pool (stream_pool.hpp): made on first use under pool_mu, non-blocking streams that live as long as the process.
  // prover_streams < 0: not asked yet; 0: no pool (SONIC_STREAM_POOL=0, or the default), handles make private streams
  int prover_streams = -1;
  hipStream_t prover_stream[POOL_MAX] = {};
  // The enqueue lock.  Every call that queues work for a pooled handle holds it while it queues (prover.hpp, EnqueueLock), so all pool
  // streams see the proofs of all handles in ONE order.  Why two handles can never wait for each other: a stream runs in order, and
  // hipStreamWaitEvent waits for a record that was queued BEFORE the wait, so every wait points backwards in that one order -- to work
  // of the same proof (its roles are queued HEAD, NTT, GROUPs, T_GROUP, CHAINs, TAIL, each waiting only for earlier ones) or of a proof
  // queued earlier.  The first unfinished item of the order therefore never waits for anything unfinished, whatever shares its stream:
  // by induction everything drains.  That holds for sonic_prove_batch's thread per handle too: the lock makes their enqueues one order.
  // Without the lock two threads could interleave their proofs differently on different streams; still no cycle (a wait always points at
  // something already queued), but proof B's head could sit behind proof A's groups on one stream and in front of them on another.
  std::mutex enqueue_mu;
  std::mutex call_mu;                    // SRS construction, the lazy G2 half, the shared NTT tables of the stand-alone entry points
  std::mutex pool_mu;
  std::vector<CallCtx*> pool;            // leased call contexts (CallLease)
  std::vector<void*> lanes;              // idle lanes of the blocking MSM entry points (sonic_msm_lane*, under pool_mu)
  NttTables* ntt = nullptr;              // sonic_ntt_fr / sonic_poly_mul_fr[_dev] (under call_mu)
  DevBuf mul_a, mul_b, mul_flags;        // scratch of sonic_poly_mul_fr_dev (under call_mu)
  std::atomic<int> sort_staged{-1};      // msm.hip: the LDS-staged sort passes got their dynamic-LDS attribute on this device (-1: not asked yet)
  std::atomic<int> ntt_big{-1};          // ntt.hip: the same for the 128-KB block of k_ntt_wide_big
  // twiddle tables of the prover handles, one set per transform size, shared by every handle on the device and never freed (64 + 64 MB
  // at 2^21 points: two streaming handles used to hold one copy each) (under pool_mu)
  std::map<int, NttTables*> prover_ntt;
  // the idle prover shells the one-shot sonic_prove keeps for later calls with the same SRS and circuit shape (prove.hip): at most
  // ONE_SHOT_SHELLS, the oldest goes when another is parked
  std::mutex one_shot_mu;
  std::vector<void*> one_shot;
};
const NttTables& device_ntt_tables(int log2n);          // of the current device; built on first use (blocks until they are complete)
void drop_one_shot_of(const sonic_srs* s);              // an SRS handle is going away: the parked one-shot shells over it go first
struct OneShotShell { const sonic_srs* srs; sonic_prover* p; };      // an entry of DeviceCtx::one_shot (prove.hip)
void unlink_one_shot_of(const sonic_srs* s);            // the same when no device scope can be opened: the shells are forgotten (leaked), never matched again
// dev < 0: the process's default device (sonic_init, else LOCAL_RANK % device count, else 0).  Throws HipFail{SONIC_ERR_NO_DEVICE}
// without a GPU -- the library has no CPU fallback -- and HipFail{SONIC_ERR_INVALID_ARG} for an ordinal the node does not have.
class DeviceScope {
 public:
  explicit DeviceScope(int dev = -1);
  ~DeviceScope();
  DeviceScope(const DeviceScope&) = delete;
  DeviceScope& operator=(const DeviceScope&) = delete;
  DeviceCtx& ctx() const { return *ctx_; }
 private:
  DeviceCtx* ctx_;
  DeviceCtx* prev_ctx_;
  int prev_dev_;
};
DeviceCtx& current_ctx();                 // the innermost DeviceScope of the calling thread
int default_device_ordinal();             // -1 before the first call that needed a device
inline hipStream_t default_stream() { return current_ctx().stream; }
// the current device's prover stream pool: its size (0: none), made on first use; stream i < size
int device_prover_streams();
inline hipStream_t device_prover_stream(PoolRole role, int k = 0) {
  DeviceCtx& c = current_ctx();
  return c.prover_stream[pool_stream_of(role, k, c.prover_streams)];
}
// serialises the calls that CHANGE shared state on the current device; the read-only entry points over an SRS (commitPoly, openPoly,
// hscProve, the blocking MSMs, srs_get_points) run on a leased context instead
inline std::mutex& call_mutex() { return current_ctx().call_mu; }
// A stream + MSM workspace of its own for the duration of one call: read-only calls on a shared SRS are re-entrant.
// Contexts are pooled per device and grow with the number of host threads that are inside the library at once.
struct CallCtx { hipStream_t st = nullptr; MsmWorkspace ws; };
class CallLease {
 public:
  CallLease();
  ~CallLease();
  CallLease(const CallLease&) = delete;
  CallLease& operator=(const CallLease&) = delete;
  hipStream_t st() const { return c_->st; }
  MsmWorkspace& ws() const { return c_->ws; }
 private:
  CallCtx* c_;
  DeviceCtx* owner_;
};

// ---- the entry-point wrapper ------------------------------------------------------------------------------------------------------
// Every entry point that touches a device runs inside a DeviceScope: API_BEGIN on the default device, API_BEGIN_ON(dev) on a handle's.
// Host-only entry points open with API_HOST_BEGIN: the same tail, no scope (it names nothing of the device: verify.hip is also built as
// plain C++).  API_END closes either with `return SONIC_OK`; API_CATCH is the tail alone, for bodies whose every path returns.
#define API_BEGIN_ON(dev) try { ::sonic::DeviceScope _scope(dev);
#define API_BEGIN API_BEGIN_ON(-1)
#define API_HOST_BEGIN try {
#define API_CATCH                                                               \
  } catch (const ::sonic::HipFail& f) { return f.code; }                        \
  catch (const std::exception& e) { ::sonic::set_error("%s", e.what()); return SONIC_ERR_HIP; }
#define API_END API_CATCH return SONIC_OK;

// ---- the SRS handle, opaque (srs_api.hip) -----------------------------------------------------------------------------------------
// The handle is a type in srs_handle.hpp for the code that works on its device side.  These two stay functions over the forward
// declaration because the verifier's host path (verify.hip, verify_host.hpp, and this header with them) is also compiled as plain C++
// under ASan / UBSan against a stand-in `struct sonic_srs` that supplies its own pair (tests/host/san_verify.cpp).
int64_t srs_d(const sonic_srs* s);
// the handle's Fiat-Shamir id (fs.hpp), made once by `make` and kept in the handle
int srs_cached_id(const sonic_srs* s, int (*make)(const sonic_srs*, uint8_t*), uint8_t out[32]);

// ---- encodings at the boundary (encoding.hip) -------------------------------------------------------------------------------------
void fr_to_mont_enqueue(hipStream_t st, Fr* d, long n, int* d_err);
void fr_from_mont_enqueue(hipStream_t st, Fr* d, long n);
void fr_check_enqueue(hipStream_t st, const Fr* d, long n, int* d_err);
// 96-byte canonical encodings -> Montgomery affine points; *d_err collects bits 1 non-canonical, 2 off the curve, 8 infinity at an index
// other than inf_ok (-1: accepted everywhere, -2: nowhere)
void points_from_bytes_enqueue(hipStream_t st, const uint8_t* d_in96, PointArrayMut out, long n, int* d_err, long inf_ok);
void points_subgroup_check_enqueue(hipStream_t st, PointArray in, long n, int* d_err);      // bit 4: a point outside the order-r subgroup
void points_to_bytes_enqueue(hipStream_t st, PointArray in, uint8_t* d_out96, long n);
int read_flags(hipStream_t st, DevBuf& flags);      // the error bits the stream's kernels have collected in a device word; waits for the stream
void msm_blocking(hipStream_t st, MsmWorkspace& ws, const MsmPlan& pl, PointArray d_pts, const Fr* d_sc, long n, bool mont,
                  uint8_t* out96, uint8_t* out_partial192);
struct G2Affine;
// G2 half (srs_g2.hip)
void srs_generate_g2(hipStream_t st, long d, const Fr& x_std, const Fr& alpha_std, G2Affine* h0, G2Affine* h1);
void g2_points_to_bytes_enqueue(hipStream_t st, const G2Affine* in, uint8_t* d_out, long n);
void g2_points_from_bytes_enqueue(hipStream_t st, const uint8_t* d_in, G2Affine* out, long n, int* d_err);
// updatable SRS (srs_g2.hip): sum_i rho[i] * pts[i] for the 128-bit randomizers of the structure check, as the 192 bytes of the header's G2
// layout; and a contribution to both G2 bases, o0[i] = x^e * h0[i], o1[i] = alpha x^e * h1[i] (Montgomery scalars).  Both wait for the stream.
void g2_weighted_sum(hipStream_t st, const G2Affine* pts, const Fr* d_rho, long n, uint8_t out192[192]);
void srs_scale_g2(hipStream_t st, long d, const G2Affine* h0, const G2Affine* h1, const Fr& x, const Fr& xinv, const Fr& alpha, G2Affine* o0, G2Affine* o1);

// compressed point encodings (compress.hip; the format: compress.hpp).  One thread per point; d_in at multiples of 48 / 96 bytes.
// decompress: out (may be {nullptr}) gets the Montgomery affine point, d_bytes (may be null) its canonical 96 / 192 bytes, d_flags one
// verdict per point: 0 accepted, else bits 1 malformed, 2 off the curve, 4 outside the subgroup (only with check_subgroup); a refused
// point is written as infinity.
void g1_decompress_enqueue(hipStream_t st, const uint8_t* d_in48, PointArrayMut out, uint8_t* d_bytes96, uint8_t* d_flags, long n, bool check_subgroup);
void g2_decompress_enqueue(hipStream_t st, const uint8_t* d_in96, G2Affine* out, uint8_t* d_bytes192, uint8_t* d_flags, long n, bool check_subgroup);
void g1_compress_enqueue(hipStream_t st, PointArray in, uint8_t* d_out48, long n);
void g2_compress_enqueue(hipStream_t st, const G2Affine* in, uint8_t* d_out96, long n);
// k_g1_validate (verify_batch.hip): 96-byte encodings -> affine points and flags, 1 = what load_g1 accepts
void g1_validate_enqueue(hipStream_t st, const uint8_t* d_in96, G1Affine* out, uint8_t* d_flags, long n);
// k_g1_subgroup (verify_batch.hip), k_g2_subgroup (srs_g2.hip): encodings -> one verdict per point, 0 accepted, else 1 non-canonical, 2 off
// the curve, 4 outside the subgroup by the test `method` names (SONIC_SUBGROUP_DEFAULT / SONIC_SUBGROUP_WALK)
void g1_subgroup_enqueue(hipStream_t st, const uint8_t* d_in96, uint8_t* d_flags, long n, int method);
void g2_subgroup_enqueue(hipStream_t st, const uint8_t* d_in192, uint8_t* d_flags, long n, int method);

// weights digest v2 (weights_digest.hip; fs.hpp): queues the SHA-256 tree over a resident CSR of R = 3Q rows and nnz entries (int32
// indices, Montgomery values) into `tree` (grown to fit); returns where the root's eight state words will be
const uint32_t* weights_tree_enqueue(hipStream_t st, const int32_t* row_ptr, const int32_t* col, const Fr* val, long R, long nnz, DevBuf& tree);

// NTT (ntt.hip).  Data in Montgomery form, in place.  forward: natural -> bit-reversed;
// inverse: bit-reversed -> natural, scaled by 1/n.
struct NttTables {
  int log2n = 0;
  DevBuf fwd, inv;    // stage-major twiddles, 2^log2n entries each: [2^L - 2^(L-s) + j] = w^(+-j 2^s), j < 2^(L-1-s) (Montgomery; ntt.hip)
  DevBuf ninv;        // (2^k)^-1, k = 0..32
  void ensure(hipStream_t st, int log2n);
};
void ntt_forward_enqueue(hipStream_t st, const NttTables& tw, Fr* d, int log2n);
void ntt_inverse_enqueue(hipStream_t st, const NttTables& tw, Fr* d, int log2n);
void ntt_inverse_of_product_enqueue(hipStream_t st, const NttTables& tw, Fr* d, const Fr* other, int log2n);
void fr_pointwise_mul_enqueue(hipStream_t st, Fr* a, const Fr* b, long n);
void fr_scale_enqueue(hipStream_t st, Fr* a, long n, const Fr* d_s);
void fr_bitrev_permute_enqueue(hipStream_t st, Fr* d, int log2n);

// polynomial kernels (poly.hip); all Fr arrays Montgomery, dense over an exponent range
// out[i] = in[i] * x^(e0 + i)
void poly_scale_powers_enqueue(hipStream_t st, const Fr* in, Fr* out, long n, long e0, const Fr* d_x, const Fr* d_xinv);
// inclusive prefix sums in Fr, in place; tmp >= ceil(n/1024)+1 Fr
void poly_prefix_sum_enqueue(hipStream_t st, Fr* d, long n, DevBuf& tmp);
// quotient of (f - f(z)) / (X - z) from d = f_e z^e and its prefix sums P (see poly.hip)
void poly_quotient_enqueue(hipStream_t st, const Fr* prefix, Fr* q, long n, long lo, const Fr* d_z, const Fr* d_zinv);

}  // namespace sonic
