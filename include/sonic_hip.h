/* sonic_hip.h -- C ABI of libsonic_hip.so, the MI355X-native Sonic prover hot path.
 *
 * The reference (sdiehl/sonic, Haskell) has no FFI: its public surface is the exposed modules of
 * sonic.cabal:31-37.  Each entry point below names the Haskell function it stands in for; a
 * `foreign import ccall` shim over these symbols re-creates Sonic.SRS /
 * Sonic.CommitmentScheme / Sonic.Protocol 1:1.
 *
 * Value encodings (standard form, never Montgomery):
 *   Fr  : 32 bytes little-endian integer < r
 *   G1  : 96 bytes  x || y, each 48 bytes little-endian < q; the point at infinity (`mempty`) is
 *         96 zero bytes ((0,0) is not on y^2 = x^3 + 4)
 *   sparse Laurent polynomial (poly's VLaurent as `GHC.Exts.toList` yields it,
 *         CommitmentScheme.hs:33,48): n_terms exponents (int64) + n_terms Fr coefficients;
 *         exponents need not be sorted, repeated exponents are summed, zero coefficients allowed
 *   gate weights wL, wR, wO (Bulletproofs GateWeights, lists of Q rows of n): dense Q x n
 *         row-major Fr
 *   gate weights as CSR (the `_csr` entry points, round 7): the three matrices stacked as ONE
 *         compressed-sparse-row matrix of 3Q rows -- rows 0..Q-1 are wL, Q..2Q-1 wR, 2Q..3Q-1 wO --
 *         over columns 0..n-1 (column i = gate i + 1 of the reference):
 *           const int64_t* row_ptr   3Q + 1 entries, row_ptr[0] == 0, non-decreasing;
 *                                    nnz = row_ptr[3Q] <= 2^31 - 1
 *           const int64_t* col       nnz entries in [0, n), strictly increasing within each row
 *                                    (canonical CSR: sorted, no duplicates)
 *           const uint8_t* val       nnz x 32-byte canonical Fr; explicit zeros are allowed
 *         col / val may be NULL when nnz = 0; cs stays dense (Q Fr).  A structural violation
 *         returns SONIC_ERR_INVALID_ARG with a message that names the row, a non-canonical value
 *         SONIC_ERR_BAD_ENCODING.  Every `_csr` call gives the bytes its dense counterpart gives for
 *         the densified matrices.
 *   transcript: the prover's `rnd` draws made explicit, in draw order (Protocol.hs:58,66,76,
 *         84-85; Signature.hs:48,60):  c_{n+1..n+4}, y, z, y_1..y_Q, z_1..z_Q, u, v  = 8 + 2Q Fr
 *   proof: record order of `Proof` (Protocol.hs:28-38) then `HscProof` (Signature.hs:22-29):
 *         R, T, a, Wa, b, Wb, Wt, s, [S_j, s_j, W_j]_j, [s'_j, W'_j, Q_j]_j, Qv, C, u, v
 *         = (7+4Q)*96 + (5+2Q)*32 bytes
 *
 * Errors: the reference panics (Protocol.hs:55, CommitmentScheme.hs:70-73) or hits `fromJust`
 * (CommitmentScheme.hs:44); here every function returns a status and never aborts the process.
 * sonic_last_error() gives the thread's last message.  There is no CPU fallback: without a HIP
 * device every call returns SONIC_ERR_NO_DEVICE.
 *
 * Threading: an SRS handle is immutable after construction and may be shared; a prover handle
 * owns its stream and workspace and serves one call at a time.
 *
 * Devices (round 5): one host process may drive every GPU of the node.  Every handle -- SRS, prover, MSM lane -- lives on the GPU it
 * was made on (the *_on constructors name it; the others use the default device: sonic_init, else LOCAL_RANK, else 0) and every
 * call on a handle runs there, whatever the calling thread's current HIP device is (which the call leaves as it found it).
 * sonic_prove_shared / sonic_prove_batch / sonic_msm_g1_srs_multi run ONE call over handles on several GPUs with one host thread
 * per device inside the library: no launcher, no torch, no RCCL.
 *
 * ABI version: sonic_abi_version().  An entry point whose argument list or buffer sizes change gets a NEW symbol (…_v2); the old
 * symbol keeps its old prototype and returns SONIC_ERR_INVALID_ARG, so that a caller built against an older header gets a status
 * instead of a memory overwrite.
 */
#ifndef SONIC_HIP_H
#define SONIC_HIP_H
#include <stddef.h>
#include <stdint.h>

#if defined(__GNUC__)
#pragma GCC visibility push(default)
#endif
#ifdef __cplusplus
extern "C" {
#endif

enum {
  SONIC_OK = 0,
  SONIC_ERR_D_TOO_SMALL = 1,      /* Protocol.hs:54-55  "Parameter d is not large enough" */
  SONIC_ERR_SRS_INDEX = 2,        /* CommitmentScheme.hs:70-73 "... is not long enough", incl. the
                                     e' = 0 hole of the alpha basis (index -1) */
  SONIC_ERR_BAD_ENCODING = 3,     /* non-canonical Fr / Fq, point not on the curve */
  SONIC_ERR_INEXACT_DIVISION = 4, /* CommitmentScheme.hs:44 fromJust; also z = 0 with negative exponents */
  SONIC_ERR_HIP = 5,
  SONIC_ERR_NO_DEVICE = 6,
  SONIC_ERR_INVALID_ARG = 7
};

#define SONIC_FR_BYTES 32
#define SONIC_G1_BYTES 96
#define SONIC_G1_PARTIAL_BYTES 192   /* un-normalised XYZZ accumulator exchanged between ranks */
/* what the bulk kernels leave of an MSM in DEVICE memory: a header and up to 64 points that the host folds in microseconds (window sums
 * of a Horner walk, or the bit sums of the round-4 bucket reduction) -- the operand of the cross-rank all-gather that never visits the
 * host (sonic_msm_submit_dev, sonic_msm_reduce_slices_dev), summed by sonic_g1_sum_dev_partials */
#define SONIC_G1_DEV_PARTIAL_BYTES 12304

typedef struct sonic_srs sonic_srs_t;
typedef struct sonic_prover sonic_prover_t;
typedef struct sonic_verifier sonic_verifier_t;

/* ---- library ---- */
#define SONIC_ABI_VERSION 7
/* the SONIC_ABI_VERSION the library was built as; no device needed.  History: 5 = round 5 (devices; sonic_msm_submit_dev_v2,
 * sonic_msm_reduce_slices_dev_v2 and sonic_fs_challenges_v2 replace the symbols whose meaning changed in round 4; share format 2);
 * 6 = round 6 (additions only: sonic_prove_batch fuses the proofs of a handle group, sonic_one_shot_trim);
 * 7 = round 7 (additions only: gate weights as CSR -- sonic_prover_new_csr, sonic_prove_csr, sonic_fs_circuit_digest_csr,
 * sonic_verify_csr, sonic_verify_fs_csr); still 7, additions only: the batched verifier -- sonic_verifier_new[_csr], sonic_verifier_free,
 * sonic_verifier_device, sonic_verifier_verify_batch, sonic_verifier_verify_fs_batch, sonic_verifier_eval_s, sonic_g1_validate,
 * sonic_verify_batch_randomizers; still 7, additions only: the compressed encodings -- sonic_g1_compress, sonic_g1_decompress,
 * sonic_g2_compress, sonic_g2_decompress, sonic_proof_size_compressed, sonic_proof_compress, sonic_proof_decompress,
 * sonic_verifier_verify_batch_z, sonic_verifier_verify_fs_batch_z, sonic_srs_save_compressed; still 7, additions only: one circuit, many
 * statements -- sonic_prover_eval_constraints, sonic_prover_set_constants, sonic_prove_batch_statements, sonic_fs_circuit_midstate[_csr],
 * sonic_fs_circuit_digest_resume, sonic_verifier_verify_batch_cs, sonic_verifier_verify_fs_batch_cs, sonic_verify_batch_digest_v2;
 * still 7, additions only: Fiat-Shamir proofs in flight -- sonic_prover_witness_digest_v2, sonic_prover_submit_fs,
 * sonic_prover_collect_fs, sonic_prove_batch_fs; still 7, additions only: witness sources -- sonic_witness_src_t, sonic_prover_set_witness,
 * sonic_prover_eval_constraints_src, sonic_prove_batch_src, sonic_prove_batch_fs_src; still 7, additions only: core proofs --
 * sonic_prover_prove_core, sonic_prover_submit_core, sonic_prover_collect_core, sonic_prover_prove_core_fs, sonic_fs_core_challenges,
 * sonic_prove_batch_core_src, sonic_prove_batch_core_fs_src, sonic_verify_core[_csr], sonic_verify_core_fs[_csr],
 * sonic_verifier_verify_core_batch, sonic_verifier_verify_core_fs_batch, sonic_verify_core_batch_digest, sonic_core_proof_compress,
 * sonic_core_proof_decompress; still 7, additions only: helped verification -- sonic_fs_weights_digest, sonic_fs_aggregate_challenges,
 * sonic_prover_aggregate_core, sonic_verifier_verify_core_batch_helped, sonic_verifier_verify_core_fs_batch_helped,
 * sonic_verify_core_helped_digest; still 7, additions only: the updatable SRS -- sonic_srs_check, sonic_srs_update, sonic_srs_verify_update;
 * still 7, additions only: the G2 sums -- sonic_msm_g2, sonic_msm_g2_srs[_dev], sonic_msm_g2_walk_max; subgroup membership --
 * sonic_g1_subgroup_check, sonic_g2_subgroup_check; pairings -- sonic_pairing_check; the opening chain alone -- sonic_open_batch_dense;
 * still 7, additions only: circuits with Q ~ n -- sonic_fs_weights_digest_v2_csr, sonic_fs_circuit_digest_v2, sonic_prover_weights_digest_v2,
 * sonic_verifier_weights_digest_v2, sonic_verifier_new_digest, sonic_verifier_digest_kind, sonic_prover_device_bytes,
 * sonic_prover_host_bytes */
int sonic_abi_version(void);
int sonic_init(int device_ordinal);                 /* choose the DEFAULT GPU (first call wins) and make it the thread's HIP device; idempotent */
int sonic_device_count(int* out);                   /* GPUs this process can see; SONIC_ERR_NO_DEVICE (and 0) without one */
int sonic_last_error(char* buf, size_t cap);        /* copies the calling thread's last message */
int sonic_device_sync(void);
/* HIP_VERSION the library was compiled against / hipRuntimeGetVersion of the runtime mapped into this process (major * 10^7 +
 * minor * 10^5 + patch).  A process holds ONE HIP runtime; when another component loaded its own first (a PyTorch-ROCm wheel), the
 * two differ and the caller may want to know.  No device needed. */
int sonic_hip_versions(int* build, int* runtime);

/* ---- Sonic.SRS ---- */
/* SRS.new :: Int -> Fr -> Fr -> SRS  (SRS.hs:27-43).  Generates, on the GPU, the G1 halves the
 * prover reads: basis 0 = g^{x^e}, basis 1 = g^{alpha x^e}, e in [-d, d]; slot e = 0 of basis 1 is
 * empty (g^alpha is not shared, SRS.hs:38).  gNegativeX[k] = basis0[-(k+1)], gPositiveX[k] =
 * basis0[k], gNegativeAlphaX[k] = basis1[-(k+1)], gPositiveAlphaX[k] = basis1[k+1]. */
int sonic_srs_new(int64_t d, const uint8_t x[32], const uint8_t alpha[32], sonic_srs_t** out);
/* the same on a named GPU (SURVEY 8b proposed `sonic_srs_new(d, x, alpha, n_gpus)`: one replica per device, made by one call each --
 * the calls may run on different host threads at once).  device < 0: the default device. */
int sonic_srs_new_on(int device, int64_t d, const uint8_t x[32], const uint8_t alpha[32], sonic_srs_t** out);
/* the record constructor `SRS{..}`: caller-supplied points, (2d+1) * 96 bytes per basis.  Every point is checked to be
 * canonical, on the curve and in the prime-order subgroup G1 (r P = O, as the powers of a generator are): MSMs over an
 * SRS rely on it (scalars above r/2 run as r - s on the negated point).  SONIC_ERR_BAD_ENCODING otherwise. */
int sonic_srs_from_points(int64_t d, const uint8_t* basis0, const uint8_t* basis1, sonic_srs_t** out);
int sonic_srs_from_points_on(int device, int64_t d, const uint8_t* basis0, const uint8_t* basis1, sonic_srs_t** out);
/* a replica of `srs` on another GPU of this process: the G1 bases and their window tables are copied device to device
 * (hipMemcpyPeer; no re-validation, no table rebuild), the G2 half if the handle holds it; a handle that could still generate its
 * G2 half hands its trapdoor on to the replica as well.  The replica runs the same MSM plans as the original (same tables), which
 * sonic_prove_shared relies on. */
int sonic_srs_replicate(const sonic_srs_t* srs, int device, sonic_srs_t** out);
void sonic_srs_free(sonic_srs_t* srs);
int64_t sonic_srs_d(const sonic_srs_t* srs);        /* srsD */
int sonic_srs_device(const sonic_srs_t* srs);       /* the GPU the handle lives on (-1 for NULL) */
/* srsPairing = e(g, h^alpha) (SRS.hs:21,42), the one record field that is neither a vector nor d: 576 bytes, the Fq12 element as
 * its twelve Fq coefficients c[i][j][k] (i: the Fq6 half of Fq12 = Fq6[w]/(w^2 - v), j: the Fq2 coefficient of Fq6 = Fq2[v]/(v^3 - (1 + u)),
 * k: real / imaginary part), 48-byte little-endian each -- the layout of oracle/pairing.py's nested tuples flattened.  Host pairing
 * (pairing.hpp) of the generator with hPositiveAlphaX[0]; needs the G2 half. */
int sonic_srs_pairing(const sonic_srs_t* srs, uint8_t out[576]);
/* basis: 0 = g^{x^e}, 1 = g^{alpha x^e} (the four reference vectors, SRS.hs:33-39); diagnostics: b + 2w = window table w of basis b,
 * SONIC_BASIS_ALPHA_PREFIX = the running sums of the alpha basis, entry e = sum of g^{alpha x^k} over k in [-d, e] (what a run of equal
 * coefficients is committed with: DESIGN.md section 4),
 * SONIC_BASIS_ALPHA_SYM = the symmetric sums g^{alpha x^e} + g^{alpha x^-e}, e in [1, d] (what hscProve's C is committed with) */
#define SONIC_BASIS_ALPHA_PREFIX 1000
#define SONIC_BASIS_ALPHA_SYM 1001
int sonic_srs_get_points(const sonic_srs_t* srs, int basis, int64_t e0, int64_t n, uint8_t* out);
/* the G2 half (SRS.hs:35-36,40-41): basis 0 = h^{x^e}, basis 1 = h^{alpha x^e}, e in [-d, d]; hNegativeX[k] = basis0[-(k+1)],
 * hPositiveX[k] = basis0[k], hPositiveAlphaX[k] = basis1[k], hNegativeAlphaX[k] = basis1[-(k+1)].  G2 encoding: 192 bytes
 * x.c0 || x.c1 || y.c0 || y.c1 (48-byte little-endian each, x = c0 + c1 u), infinity = zeros.  A handle made by
 * sonic_srs_new generates it on the GPU on first use and then forgets x and alpha; other handles have it only after
 * sonic_srs_set_g2_points or a load from a file that carries it (SONIC_ERR_INVALID_ARG otherwise). */
int sonic_srs_get_g2_points(const sonic_srs_t* srs, int basis, int64_t e0, int64_t n, uint8_t* out);
/* attaches caller-supplied G2 vectors, (2d+1) * 192 bytes per basis, checked like the G1 side (canonical, on the twist,
 * r P = O); the prover never reads them, the verifier reads three elements (CommitmentScheme.hs:58-68). */
int sonic_srs_set_g2_points(sonic_srs_t* srs, const uint8_t* basis0, const uint8_t* basis1);
/* on-disk SRS (the reference has no persistence): "SONICSRS", u32 version = 2, u32 flags (bit 0: G2 half present), i64 d,
 * the two G1 bases as (2d+1) x 96 canonical bytes each, then -- with_g2 != 0 -- the two G2 bases as (2d+1) x 192 bytes
 * each.  Loading validates every point like sonic_srs_from_points / sonic_srs_set_g2_points; version-1 files (G1 only)
 * still load.  A file never holds x or alpha.  with_g2: 0 = G1 only, 1 = with the G2 half (SONIC_ERR_INVALID_ARG if the handle
 * has none), 2 = with the G2 half if the handle has it (sonic_srs_has_g2).  (ABI note: the with_g2 argument was added in
 * round 2; callers built against the two-argument prototype must be recompiled.)  Infinity is rejected in every SRS input
 * (from_points except the omitted g^alpha slot, set_g2_points, load): no power of a generator is the identity. */
int sonic_srs_save(const sonic_srs_t* srs, const char* path, int with_g2);
/* 1 if the handle holds the G2 half or can still generate it (made by sonic_srs_new and not yet used), else 0 */
int sonic_srs_has_g2(const sonic_srs_t* srs);
/* sonic_srs_load[_on] takes either container, told apart by the magic: the one above, or the compressed one below */
int sonic_srs_load(const char* path, sonic_srs_t** out);
int sonic_srs_load_on(int device, const char* path, sonic_srs_t** out);
/* the compressed container, half the size: "SONICSRZ", u32 version = 1, u32 flags (bit 0: G2 half present), i64 d, the two G1 bases as
 * (2d+1) x 48 bytes each, then -- with_g2 as for sonic_srs_save -- the two G2 bases as (2d+1) x 96 bytes each, every point in the
 * compressed encoding ("Compressed encodings" below); slot e = 0 of basis 1 (the omitted g^alpha) is the encoding of infinity.  Loading
 * decompresses on the GPU and then validates exactly as the uncompressed container's load does.  A container of its own rather than a
 * version 3 of SONICSRS, so that every reader of that format keeps refusing what it does not know. */
int sonic_srs_save_compressed(const sonic_srs_t* srs, const char* path, int with_g2);

/* ---- circuit-sized views of a universal string (additions under ABI 7) ----
 * A VIEW is a second kind of sonic_srs_t: the same d, the same Fiat-Shamir id, the same commitments and proofs as the string it was made
 * from, but it holds only the exponent windows a circuit of (n, Q) touches,
 *     low   [-4n - 8, max(3n, n + Q)]     both G1 bases
 *     high  [d - 3n - 4, d]               (R is committed with max = n; only the alpha basis is read there)
 * merged into one window where they touch, with window tables, running sums and symmetric sums sized for those windows and a window
 * width chosen as for a string of d = 8n.  It owns copies of all it holds: the source may be freed.  Its G2 half is exactly what the
 * verifiers fetch -- basis 0 at exponents n - d and 0, basis 1 at 0 and 1 -- asked of the source the way a verifier asks (generated on
 * first use where the source still has its trapdoor); a source that cannot supply them gives a view without a G2 half.
 * n < 1, Q < 1, d < 7n or d < 4n + 8: SONIC_ERR_INVALID_ARG.  The source may itself be a view whose windows contain the new ones.
 * Every entry point that takes an SRS takes a view.  Asking a view for an exponent inside [-d, d] that it does not hold -- an MSM or
 * polynomial whose (dense) exponent range leaves a window or crosses the gap, sonic_srs_get_points, a G2 element other than its four, a
 * prover or verifier for a circuit whose windows the view's do not contain (refused when the handle is made; a smaller circuit, n' <= n
 * and n' + Q' <= max(3n, n + Q), passes for the prover; a verifier needs h^{x^{n' - d}} and so n' = n) -- is SONIC_ERR_INVALID_ARG with
 * the range and the windows in sonic_last_error, decided on the host before anything is launched; never a wrong point.  Exponents outside
 * [-d, d] keep SONIC_ERR_SRS_INDEX.  sonic_srs_save*, sonic_srs_set_g2_points refuse a view: it is not a reference string.
 * sonic_srs_for_circuit makes the view on the source's GPU, device to device.  sonic_srs_load_for_circuit[_on] reads only the windows'
 * byte ranges (and the four G2 points where the file has a G2 half) of either container, after the header has been checked against the
 * file's real size, and validates what it read as sonic_srs_load does. */
int sonic_srs_for_circuit(const sonic_srs_t* srs, int64_t n, int64_t Q, sonic_srs_t** out);
int sonic_srs_load_for_circuit(const char* path, int64_t n, int64_t Q, sonic_srs_t** out);
int sonic_srs_load_for_circuit_on(int device, const char* path, int64_t n, int64_t Q, sonic_srs_t** out);
/* lo0, hi0, lo1, hi1: the exponent windows a handle holds; one window (every whole string: [-d, d]): lo1 = 1, hi1 = 0 */
int sonic_srs_windows(const sonic_srs_t* srs, int64_t out[4]);
/* device memory of the G1 side: both bases with their window tables, the running sums, the symmetric sums */
int sonic_srs_device_bytes(const sonic_srs_t* srs, size_t* out);

/* ---- Sonic.CommitmentScheme ---- */
/* commitPoly :: SRS -> Int -> VLaurent Fr -> G1  (CommitmentScheme.hs:20-33) */
int sonic_commit_poly(const sonic_srs_t* srs, int64_t max, int64_t n_terms, const int64_t* exps,
                      const uint8_t* coeffs, uint8_t out_g1[96]);
/* openPoly :: SRS -> Fr -> VLaurent Fr -> (Fr, G1)  (CommitmentScheme.hs:36-48) */
int sonic_open_poly(const sonic_srs_t* srs, const uint8_t z[32], int64_t n_terms, const int64_t* exps,
                    const uint8_t* coeffs, uint8_t out_fz[32], uint8_t out_g1[96]);

/* ---- the kernels behind them, exposed for parity tests and the MSM benchmark ---- */
/* foldl' (\acc (P, v) -> acc <> P `mul` v) mempty  (the fold at CommitmentScheme.hs:26-29, 45-48).  Points only have to be
 * on the curve: s P is the literal multiple (no use of r P = O), also for cofactor points such as (0, 2). */
int sonic_msm_g1(const uint8_t* points, const uint8_t* scalars, int64_t n, uint8_t out_g1[96]);
/* same over an SRS slice e0 .. e0+n-1 of one basis; scalars on the host */
int sonic_msm_g1_srs(const sonic_srs_t* srs, int basis, int64_t e0, const uint8_t* scalars, int64_t n,
                     uint8_t out_g1[96]);
/* scalars already resident in HBM (canonical 32-byte Fr, device pointer) */
int sonic_msm_g1_srs_dev(const sonic_srs_t* srs, int basis, int64_t e0, const void* d_scalars, int64_t n,
                         uint8_t out_g1[96]);
/* one rank's share of a range-sharded MSM: the un-normalised partial sum */
int sonic_msm_g1_srs_partial_dev(const sonic_srs_t* srs, int basis, int64_t e0, const void* d_scalars,
                                 int64_t n, uint8_t out_partial[192]);
/* ---- the same sums over G2 (the twist): a bucket-method MSM of its own (ABI 7 additions) ----
 * Encodings are those of sonic_srs_get_g2_points: 192 bytes x.c0 || x.c1 || y.c0 || y.c1, little-endian, canonical; the result at
 * infinity is 192 zero bytes.  n = 0 gives infinity and launches nothing.  Blocking; re-entrant as the G1 forms are.
 *
 * sonic_msm_g2: caller-supplied points.  Every point must be canonical and on the twist y^2 = x^3 + 4(u + 1), else
 * SONIC_ERR_BAD_ENCODING (so is a scalar that is not < r).  An all-zero encoding is accepted as the point at infinity, the neutral
 * element of the sum (no point of the twist has x = y = 0).  The order-r subgroup is NOT tested -- the twist has a large cofactor and a
 * subgroup walk per point would cost more than the sum -- and the result is the literal sum_i s_i P_i for any point of the twist, as
 * sonic_msm_g1's is for any point of the curve: (r - 1) P is r - 1 times P, not -P.  A caller who needs the test runs
 * sonic_g2_subgroup_check over the points first.
 *
 * sonic_msm_g2_srs[_dev]: the sum over exponents e0 .. e0+n-1 of a basis of the handle's G2 half (0: h^{x^e}, 1: h^{alpha x^e}), scalars
 * on the host or resident in HBM (canonical 32-byte Fr).  A handle made by sonic_srs_new generates the half on first use; one without
 * a G2 half is SONIC_ERR_INVALID_ARG.  A range outside [-d, d] is SONIC_ERR_SRS_INDEX.  A view holds four G2 elements and serves
 * n = 1 at one of them; any other range is SONIC_ERR_INVALID_ARG with the range in sonic_last_error, never a wrong point. */
int sonic_msm_g2(const uint8_t* points /* n x 192 */, const uint8_t* scalars /* n x 32 */, int64_t n, uint8_t out_g2[192]);
int sonic_msm_g2_srs(const sonic_srs_t* srs, int basis, int64_t e0, const uint8_t* scalars, int64_t n, uint8_t out_g2[192]);
int sonic_msm_g2_srs_dev(const sonic_srs_t* srs, int basis, int64_t e0, const void* d_scalars, int64_t n, uint8_t out_g2[192]);
/* the longest run of additions one thread of the G2 bucket accumulation makes (longer buckets are cut into chunks); for tests */
int sonic_msm_g2_walk_max(void);
/* the same fold (CommitmentScheme.hs:26-29, 45-48 over an SRS slice, as sonic_msm_g1_srs_dev) in two halves on a lane of its
 * own (stream, bucket workspace, pinned result): submit queues it and returns,
 * collect waits and finishes it (out_g1: 96 canonical bytes, out_partial: 192-byte un-normalised sum; either may be NULL).
 * One MSM in flight per lane; two lanes used in turn stream MSMs with the sort and the reduction of one under the
 * accumulation of the other.  d_scalars: canonical 32-byte Fr resident in HBM, untouched until collect. */
typedef struct sonic_msm_lane sonic_msm_lane_t;
int sonic_msm_lane_new(sonic_msm_lane_t** out);
int sonic_msm_lane_new_on(int device, sonic_msm_lane_t** out);      /* a lane serves SRS handles of its own GPU (SONIC_ERR_INVALID_ARG otherwise) */
void sonic_msm_lane_free(sonic_msm_lane_t* lane);
int sonic_msm_submit(sonic_msm_lane_t* lane, const sonic_srs_t* srs, int basis, int64_t e0, const void* d_scalars, int64_t n);
int sonic_msm_collect(sonic_msm_lane_t* lane, uint8_t* out_g1, uint8_t* out_partial);
/* a lane on a stream the caller owns (e.g. the stream its RCCL collectives are ordered on); the stream must outlive the lane */
int sonic_msm_lane_new_on_stream(void* hip_stream, sonic_msm_lane_t** out);
/* sonic_msm_submit that also leaves the un-normalised result (SONIC_G1_DEV_PARTIAL_BYTES) in device memory, queued on the lane's stream:
 * the operand of a cross-rank all-gather that never visits the host.  out_bytes: the size of d_partial_out, checked against
 * SONIC_G1_DEV_PARTIAL_BYTES.  (sonic_msm_submit_dev, which wrote 192 bytes up to round 3 and 12304 in round 4 under one name, is
 * retired: the symbol still links and returns SONIC_ERR_INVALID_ARG.) */
int sonic_msm_submit_dev_v2(sonic_msm_lane_t* lane, const sonic_srs_t* srs, int basis, int64_t e0, const void* d_scalars, int64_t n,
                            void* d_partial_out, size_t out_bytes);
int sonic_msm_submit_dev(sonic_msm_lane_t* lane, const sonic_srs_t* srs, int basis, int64_t e0, const void* d_scalars, int64_t n,
                         void* d_partial_out);      /* retired: SONIC_ERR_INVALID_ARG */
/* ONE MSM strong-scaled over `world` GPUs by sharding its BUCKETS (the fold of CommitmentScheme.hs:25-29 / 45-48 split twice: by term
 * range for the accumulation, by bucket range for the reduction):
 *   layout      n_buckets of the shared bucket set and the slice length S (a multiple of 16384, world * S >= n_buckets)
 *   accumulate  sort + bucket accumulation of this rank's terms into d_buckets (capacity >= world * S entries of 192 B; the
 *               padding is cleared), queued on the lane's stream
 *   -- the caller exchanges slices: all-to-all, rank r receives entries [r S, (r+1) S) of every rank, laid out [world][S] --
 *   reduce      element-wise curve addition of the k slices, then sum_i (bucket_base + i + 1) * slice[i]: SONIC_G1_DEV_PARTIAL_BYTES in
 *               device memory (gathered and added like the term-range partials), queued on the lane's stream
 *   sync        waits for the lane, reports a non-canonical scalar */
int sonic_msm_exchange_layout(const sonic_srs_t* srs, int world, int64_t* n_buckets, int64_t* slice_len);
int sonic_msm_accumulate_dev(sonic_msm_lane_t* lane, const sonic_srs_t* srs, int basis, int64_t e0, const void* d_scalars, int64_t n,
                             void* d_buckets, int64_t capacity);
int sonic_msm_reduce_slices_dev_v2(sonic_msm_lane_t* lane, const sonic_srs_t* srs, const void* d_slices, int k, int64_t slice_len,
                                   int64_t bucket_base, void* d_partial_out, size_t out_bytes);
int sonic_msm_reduce_slices_dev(sonic_msm_lane_t* lane, const sonic_srs_t* srs, const void* d_slices, int k, int64_t slice_len,
                                int64_t bucket_base, void* d_partial_out);      /* retired like sonic_msm_submit_dev: SONIC_ERR_INVALID_ARG */
int sonic_msm_lane_sync(sonic_msm_lane_t* lane);
/* curve addition of k partials (RCCL has no such reduction op) + normalisation */
int sonic_g1_sum_partials(const uint8_t* partials, int k, uint8_t out_g1[96]);
/* the same for k device-side results of SONIC_G1_DEV_PARTIAL_BYTES each (host only) */
int sonic_g1_sum_dev_partials(const uint8_t* blobs, int k, uint8_t out_g1[96]);
/* in-place radix-2 NTT over Fr, natural order in and out; omega = 7^((r-1)/2^log2n); 0 <= log2n <= 28 (SONIC_ERR_INVALID_ARG beyond) */
int sonic_ntt_fr(uint8_t* data, int log2n, int inverse);
/* dense product of two coefficient arrays (the `*` at Constraints.hs:61): out has na+nb-1 Fr */
int sonic_poly_mul_fr(const uint8_t* a, int64_t na, const uint8_t* b, int64_t nb, uint8_t* out);
/* the opening chain of prove() on caller-supplied dense polynomials, without the MSM: k (1 .. 16) openings over ONE exponent range
 * [lo, lo + len), lo <= 0 <= lo + len - 1.  polys: k pointers to len canonical Fr each (coefficient of X^(lo + i) at i; equal pointers are
 * allowed and share one device array); zs: k points, none zero (SONIC_ERR_INEXACT_DIVISION).  out_fz: the k values f_k(z_k); out_q (used
 * when quotient != 0): k pointers to len - 1 Fr each, the coefficients of (f_k(X) - f_k(z_k)) / (X - z_k) over [lo, lo + len - 2].
 * chunk: coefficients per GPU thread, 0 = what prove() takes at this length; 2 .. 16 force one (tests of the tile edges at small sizes) */
int sonic_open_batch_dense(int k, const uint8_t* const* polys, int64_t lo, int64_t len, const uint8_t* zs, int quotient, int chunk,
                           uint8_t* out_fz, uint8_t* const* out_q);
/* the same with operands and result resident in HBM (device pointers to canonical Fr; d_out: na + nb - 1 elements) */
int sonic_poly_mul_fr_dev(const void* d_a, int64_t na, const void* d_b, int64_t nb, void* d_out);
/* bytes between consecutive points of an SRS basis / window table in HBM (128: one HBM line per 96-byte point); what a bucket walk
 * reads per (term, window) by design */
int sonic_srs_point_bytes(void);
/* MSM tuning knob for tests: window bits c = 4 .. 16 (0 = automatic).  Process-wide, not thread-safe.  Honoured
 * by the G1 MSMs (which then run without the window tables), by the G2 MSM (sonic_msm_g2, sonic_msm_g2_srs, sonic_msm_g2_srs_dev: every
 * slab at that c instead of floor(log2 n) - 4) and by the G2 sums of sonic_srs_check, whose 129-bit plan then has ceil(129 / c) windows */
int sonic_msm_set_window(int c);
/* what an n-term MSM over this SRS will run as: window bits, number of windows, and bucket sets
 * (1 = all windows share one bucket set over the precomputed window tables, else one set per window) */
int sonic_msm_plan(const sonic_srs_t* srs, int64_t n, int* window_bits, int* windows, int* bucket_sets);

/* ---- Sonic.Protocol / Sonic.Signature ---- */
size_t sonic_proof_size(int64_t Q);
/* prove :: SRS -> Assignment Fr -> ArithCircuit Fr -> m (Proof, RndOracle)  (Protocol.hs:47-109),
 * including hscProve (Signature.hs:38-72).  n = length aL, Q = length wL. */
int sonic_prove(const sonic_srs_t* srs, int64_t n, int64_t Q, const uint8_t* wL, const uint8_t* wR,
                const uint8_t* wO, const uint8_t* cs, const uint8_t* aL, const uint8_t* aR,
                const uint8_t* aO, const uint8_t* transcript, uint8_t* out_proof);
/* sonic_prove parks the shell of a finished call (streams, workspaces of a proof of that shape, twiddle tables: several GB at n = 2^20)
 * for the next call with the same SRS handle and (n, Q); at most four per GPU stay parked, and freeing an SRS frees the shells over it.
 * sonic_one_shot_trim frees the parked shells now -- of one GPU, or of all (device < 0) -- and returns how many there were. */
int sonic_one_shot_trim(int device);
/* the same split so that circuit and assignment stay resident in HBM across proofs */
int sonic_prover_new(const sonic_srs_t* srs, int64_t n, int64_t Q, const uint8_t* wL, const uint8_t* wR,
                     const uint8_t* wO, const uint8_t* cs, sonic_prover_t** out);
/* the same handle from gate weights as CSR (format above).  The handle keeps the rows and their column-major transpose in HBM
 * (O(nnz + n), int32 indices): s(X,y), s(u,Y) and sonic_prover_prepare then cost O(nnz + n) per constraint set instead of O(Q n).
 * Every operation on a prover handle accepts it -- set_assignment, prepare, prove, submit / collect, prove_fs, hsc_prove, set_share /
 * prove_share, sonic_prove_batch, sonic_prove_shared -- with the bytes a dense handle of the densified circuit gives. */
int sonic_prover_new_csr(const sonic_srs_t* srs, int64_t n, int64_t Q, const int64_t* row_ptr, const int64_t* col, const uint8_t* val,
                         const uint8_t* cs, sonic_prover_t** out);
/* sonic_prove with gate weights as CSR.  It shares the parked shells of sonic_prove: a shell holds the form of its last call's circuit,
 * and dense and CSR calls of one (n, Q) may alternate. */
int sonic_prove_csr(const sonic_srs_t* srs, int64_t n, int64_t Q, const int64_t* row_ptr, const int64_t* col, const uint8_t* val,
                    const uint8_t* cs, const uint8_t* aL, const uint8_t* aR, const uint8_t* aO, const uint8_t* transcript,
                    uint8_t* out_proof);
int sonic_prover_set_assignment(sonic_prover_t* p, const uint8_t* aL, const uint8_t* aR, const uint8_t* aO);
/* optional, once per handle: commits the Q constraint-row polynomials of sPoly (Constraints.hs:34-53), after which every
 * S_j = commitPoly(s(X, y_j)) (Signature.hs:42) costs an n-term MSM instead of a 3n-term one.  Same proof bytes. */
int sonic_prover_prepare(sonic_prover_t* p);
int sonic_prover_prove(sonic_prover_t* p, const uint8_t* transcript, uint8_t* out_proof);
/* prove (Protocol.hs:47-109) in two halves: submit queues the whole proof on the handle's streams and returns without waiting for the GPU;
 * collect waits for it, finishes it on the host and writes the bytes (prove = submit + collect).  One proof in flight per
 * handle.  A host thread that alternates between two handles -- submit(A, t0), submit(B, t1), collect(A), submit(A, t2),
 * collect(B), ... -- streams proofs with the next proof's start-up under the previous proof's tail (the reference's
 * `mapM prove` over a list of statements; BASELINE config "batch of independent proofs, throughput mode"). */
int sonic_prover_submit(sonic_prover_t* p, const uint8_t* transcript);
int sonic_prover_collect(sonic_prover_t* p, uint8_t* out_proof);
void sonic_prover_free(sonic_prover_t* p);

/* ---- ONE proof over several GPUs ----
 * The 7 + 4Q commitments and openings of prove + hscProve (Protocol.hs:63,73,79-81; Signature.hs:40-45,51-57,63) are independent
 * sums once the transcript is known.  Every rank (one process per GPU) makes a handle for the same circuit and assignment over its
 * replica of the SRS and calls set_share(rank, world): the handle then builds only the polynomials its pieces read and runs a
 * contiguous piece of the proof's MSMs laid end to end (a cut inside an MSM splits its term range), balanced by a cost model
 * (sonic_amd/csrc/share_plan.hpp).  submit + collect_share (or prove_share) with the SAME transcript on every rank yield one share
 * per rank -- un-normalised 192-byte partial sums per MSM, the evaluations the rank computed, its error flags: sonic_proof_share_size
 * bytes; the caller all-gathers them (RCCL / any transport) and sonic_proof_from_shares lays out the proof, byte-identical to
 * sonic_prover_prove on one GPU.  world <= 1 restores the whole proof.  Not available for sonic_prover_prove_fs (the Fiat-Shamir
 * chain serialises the MSMs). */
int sonic_prover_set_share(sonic_prover_t* p, int rank, int world);
size_t sonic_proof_share_size(int64_t Q);
int sonic_prover_prove_share(sonic_prover_t* p, const uint8_t* transcript, uint8_t* out_share);
int sonic_prover_collect_share(sonic_prover_t* p, uint8_t* out_share);       /* after sonic_prover_submit */
/* shares: world x sonic_proof_share_size(Q) bytes in any rank order; host only.  Fails with SONIC_ERR_INVALID_ARG unless the pieces
 * of every MSM cover its terms exactly once and every evaluation is reported; a rank's error flags become the status sonic_prove
 * would have returned. */
int sonic_proof_from_shares(int64_t Q, int world, const uint8_t* shares, const uint8_t* transcript, uint8_t* out_proof);
/* the plan itself (host only): out_lo_hi = 7 + 4Q pairs {lo, hi} in units of 1 / 2^20 of each MSM's terms, slot order R, T, W_a,
 * W_b, W_t, [S_j, W_j]_j, [W'_j, Q_j]_j, Q_v, C; out_cost (may be NULL): the rank's modelled cost in MSM terms.  nb, w: buckets per
 * set and windows of the MSM plan (0, 0: 2^19 and 13, an SRS with window tables at d >= 2^21). */
int sonic_prove_share_plan(int64_t n, int64_t Q, int prepared, int world, int rank, int64_t nb, int w, uint32_t* out_lo_hi, double* out_cost);

/* ---- N GPUs from ONE host process (round 5) ----
 * The reference's prove is one pure call in one process (Protocol.hs:47-52); these keep it that way on a node of GPUs.  Each takes an
 * array of handles that live on the GPUs to use (one SRS replica per device: sonic_srs_new_on / sonic_srs_replicate; the same device
 * may appear more than once, which is how the tests drive them on a one-GPU box) and runs one host thread per handle inside the
 * library.  Nothing here needs torch, RCCL or a launcher; sonic_amd/distributed.py keeps the one-process-per-GPU form over RCCL.
 *
 *   sonic_prove_shared    ONE proof over `world` prover handles of the same circuit and assignment: handle r runs rank r's share
 *                         (sonic_prover_set_share is applied by the call), the 3.3-KB shares are combined on the host
 *                         (sonic_proof_from_shares).  Same bytes as sonic_prover_prove on one GPU.
 *   sonic_prove_batch     K proofs of ONE circuit over n_provers handles (`mapM (prove srs asg_i circuit)`; for K statements with their own
 *                         circuits see sonic_prove_many): proof i goes to handle i % n_provers, each handle proves its share of the
 *                         list in order on a thread of its own; no collective.  Two handles per GPU stream that GPU's proofs (one
 *                         proof's host tail under the next proof's kernels).  aL, aR, aO: K x n x 32 bytes each, or all NULL to keep
 *                         every handle's resident assignment; transcripts: K x (8 + 2Q) x 32; out_proofs: K x sonic_proof_size(Q);
 *                         out_status (may be NULL): K statuses.  Returns the first non-zero status in list order (all proofs are
 *                         attempted).
 *   sonic_msm_g1_srs_multi        ONE MSM sum_i s_i B[e0 + i] over `world` SRS replicas, scalars on the host (n x 32 bytes);
 *   sonic_msm_g1_srs_multi_dev    the same with rank r's slice resident on srs[r]'s GPU: e0[r], d_scalars[r], n[r].
 *                         mode 0 = by term range: every GPU runs a whole MSM over its slice, the host adds the `world` partial sums
 *                         (CommitmentScheme.hs:25-29 is a fold over independent terms); mode 1 = by bucket range (strong scaling):
 *                         every GPU accumulates its slice into a full bucket set, the GPUs pull their bucket range from each other
 *                         (hipMemcpyPeerAsync: the all-to-all of sonic_msm_exchange_layout), each reduces 1/world of the buckets;
 *                         needs the full window tables on every replica.
 *   sonic_prove_many      K INDEPENDENT statements of one shape (n, Q) -- every proof its own circuit, assignment and transcript, as host
 *                         buffers: `mapM (uncurry (prove srs))` -- spread over the SRS replicas with two host threads per replica, each
 *                         making one-shot sonic_prove calls (the device parks the handles' shells between calls).  out_proofs: K x
 *                         sonic_proof_size(Q); out_status (may be NULL): K statuses; returns the first non-zero one in list order. */
typedef struct sonic_statement {
  const uint8_t *wL, *wR, *wO, *cs;      /* ArithCircuit: Q x n weights each, Q constants */
  const uint8_t *aL, *aR, *aO;           /* Assignment: n each */
  const uint8_t* transcript;             /* 8 + 2Q draws */
} sonic_statement_t;
int sonic_prove_many(const sonic_srs_t* const* srs, int n_srs, int64_t n, int64_t Q, const sonic_statement_t* statements, int64_t K,
                     uint8_t* out_proofs, int* out_status);
int sonic_prove_shared(sonic_prover_t* const* provers, int world, const uint8_t* transcript, uint8_t* out_proof);
int sonic_prove_batch(sonic_prover_t* const* provers, int n_provers, int64_t K, const uint8_t* aL, const uint8_t* aR, const uint8_t* aO,
                      const uint8_t* transcripts, uint8_t* out_proofs, int* out_status);
int sonic_msm_g1_srs_multi(const sonic_srs_t* const* srs, int world, int basis, int64_t e0, const uint8_t* scalars, int64_t n, int mode,
                           uint8_t out_g1[96]);
int sonic_msm_g1_srs_multi_dev(const sonic_srs_t* const* srs, int world, int basis, const int64_t* e0, const void* const* d_scalars,
                               const int64_t* n, int mode, uint8_t out_g1[96]);
int sonic_prover_device(const sonic_prover_t* p);   /* the GPU a prover handle lives on (its SRS's); -1 for NULL */

/* ---- opt-in Fiat-Shamir transcript ----
 * The reference draws its challenges with `rnd` (Protocol.hs:58,66,76,84-85; Signature.hs:48,60) and hands y, z, (y_j, z_j) to the
 * verifier as RndOracle.  In this mode each draw is instead SHA-256 of everything that precedes it, in that order (exact
 * definition: sonic_amd/csrc/fs.hpp): the proof carries its own challenges.  It serialises the
 * proof (R -> y -> T -> z -> ...: six waits for the GPU instead of one), so the explicit transcript above stays the default.
 *   circuit_digest  SHA-256 of (n, Q, wL, wR, wO, cs): computed once per circuit
 *   srs_id          SHA-256 of d and the four G1 elements g^x, g^{alpha x}, g^{1/x}, g^{alpha/x}: binds the transcript to ONE reference
 *                   string (round 4; the round-3 transcript bound only d)
 *   prove_fs        blinder_seed: the prover's secret randomness (32 bytes).  The four blinders are derived from the seed AND the
 *                   circuit digest, the srs id and a digest of the assignment (RFC 6979 style, round 4), so one seed may serve
 *                   several statements; a seed must still never be disclosed;
 *                   out_transcript (may be NULL): the 8 + 2Q values the proof was made with, in sonic_prove's transcript order --
 *                   sonic_prover_prove on them reproduces the proof byte for byte.  This call blocks through all six passes; one proof in
 *                   flight per handle, batches over several handles and the assignment's digest on the GPU: "Fiat-Shamir proofs in flight"
 *                   below (sonic_prover_submit_fs / collect_fs, sonic_prove_batch_fs)
 *   fs_challenges   what a proof determines: y, z, y_1..y_Q, z_1..z_Q, u, v (32 bytes each)
 *   verify_fs       recomputes them, requires the proof's own u, v to match, then verify (Protocol.hs:111-130) */
int sonic_fs_circuit_digest(int64_t n, int64_t Q, const uint8_t* wL, const uint8_t* wR, const uint8_t* wO, const uint8_t* cs, uint8_t out[32]);
/* the same digest from gate weights as CSR: host only, no device needed.  The rows are hashed as the dense bytes they stand for
 * (32 zero bytes per absent entry), so the digest equals sonic_fs_circuit_digest of the densified matrices and a proof made on
 * either form verifies under either.  This costs O(Q n) hashing, once per circuit. */
int sonic_fs_circuit_digest_csr(int64_t n, int64_t Q, const int64_t* row_ptr, const int64_t* col, const uint8_t* val, const uint8_t* cs,
                                uint8_t out[32]);
int sonic_prover_prove_fs(sonic_prover_t* p, const uint8_t circuit_digest[32], const uint8_t blinder_seed[32], uint8_t* out_proof,
                          uint8_t* out_transcript);
int sonic_fs_srs_id(const sonic_srs_t* srs, uint8_t out[32]);
int sonic_fs_challenges_v2(int64_t n, int64_t Q, int64_t d, const uint8_t circuit_digest[32], const uint8_t srs_id[32], const uint8_t* proof, uint8_t* out);
/* retired (round 3's prototype, without srs_id; round 4 changed the argument list under this name): SONIC_ERR_INVALID_ARG */
int sonic_fs_challenges(int64_t n, int64_t Q, int64_t d, const uint8_t circuit_digest[32], const uint8_t* proof, uint8_t* out);
int sonic_verify_fs(const sonic_srs_t* srs, int64_t n, int64_t Q, const uint8_t* wL, const uint8_t* wR, const uint8_t* wO,
                    const uint8_t* cs, const uint8_t* proof, int* accepted);
int sonic_verify_fs_csr(const sonic_srs_t* srs, int64_t n, int64_t Q, const int64_t* row_ptr, const int64_t* col, const uint8_t* val,
                        const uint8_t* cs, const uint8_t* proof, int* accepted);       /* gate weights as CSR */

/* hscProve :: SRS -> BiVLaurent Fr -> [(Fr, Fr)] -> m HscProof  (Signature.hs:32-72) on its own, for the s(X,Y) of the handle's
 * circuit (Constraints.hs:34-53) and any number m of (y_j, z_j) pairs (yzs: m x 64 bytes); u, v are its two `rnd` draws.
 * out (sonic_hsc_proof_size(m) bytes): [S_j, s_j, W_j]_j, [s'_j, W'_j, Q_j]_j, Q_v, C, u, v -- the HscProof part of a proof. */
size_t sonic_hsc_proof_size(int64_t m);
int sonic_prover_hsc_prove(sonic_prover_t* p, int64_t m, const uint8_t* yzs, const uint8_t u[32], const uint8_t v[32], uint8_t* out);

/* hscProve with the reference's own signature (Signature.hs:32-37): ANY sparse bivariate Laurent polynomial
 * s(X,Y) = sum_i coeffs[i] X^{x_exps[i]} Y^{y_exps[i]} (terms in any order, repeated exponent pairs are summed), m pairs (y_j, z_j),
 * the two `rnd` draws u, v.  Same output layout as sonic_prover_hsc_prove.  An evaluation point may be zero only if the
 * polynomial has no negative power of that variable (`pow 0 e`, e < 0, divides by zero in the reference). */
int sonic_hsc_prove_poly(const sonic_srs_t* srs, int64_t n_terms, const int64_t* x_exps, const int64_t* y_exps, const uint8_t* coeffs,
                         int64_t m, const uint8_t* yzs, const uint8_t u[32], const uint8_t v[32], uint8_t* out);

/* ---- the verifier side of the API (host CPU; outside the accelerated path) ---- */
/* pcV :: SRS -> Int -> G1 -> Fr -> (Fr, G1) -> Bool  (CommitmentScheme.hs:51-68); *accepted = 0 / 1 */
int sonic_pc_v(const sonic_srs_t* srs, int64_t max, const uint8_t commitment[96], const uint8_t z[32], const uint8_t v[32],
               const uint8_t w[96], int* accepted);
/* verify :: SRS -> ArithCircuit Fr -> Proof -> Fr -> Fr -> [(Fr, Fr)] -> Bool  (Protocol.hs:111-130), including
 * hscVerify (Signature.hs:74-90).  yzs = Q pairs y_j || z_j (64 bytes each), i.e. rndOracleYZs. */
int sonic_verify(const sonic_srs_t* srs, int64_t n, int64_t Q, const uint8_t* wL, const uint8_t* wR, const uint8_t* wO,
                 const uint8_t* cs, const uint8_t* proof, const uint8_t y[32], const uint8_t z[32], const uint8_t* yzs, int* accepted);
/* the same with gate weights as CSR: s(u, v) costs O(nnz + n) on the host instead of O(Q n) */
int sonic_verify_csr(const sonic_srs_t* srs, int64_t n, int64_t Q, const int64_t* row_ptr, const int64_t* col, const uint8_t* val,
                     const uint8_t* cs, const uint8_t* proof, const uint8_t y[32], const uint8_t z[32], const uint8_t* yzs, int* accepted);

/* hscVerify :: SRS -> BiVLaurent Fr -> [(Fr, Fr)] -> HscProof -> Bool  (Signature.hs:74-90) for the s(X,Y) of a circuit */
int sonic_hsc_verify(const sonic_srs_t* srs, int64_t n, int64_t Q, const uint8_t* wL, const uint8_t* wR, const uint8_t* wO,
                     int64_t m, const uint8_t* yzs, const uint8_t* hsc, int* accepted);

/* hscVerify (Signature.hs:74-90) for any sparse bivariate Laurent polynomial, the counterpart of sonic_hsc_prove_poly */
int sonic_hsc_verify_poly(const sonic_srs_t* srs, int64_t n_terms, const int64_t* x_exps, const int64_t* y_exps, const uint8_t* coeffs,
                          int64_t m, const uint8_t* yzs, const uint8_t* hsc, int* accepted);

/* ---- the batched verifier: K proofs for one circuit folded into ONE pairing product (device: point validation, s(u, v), the G1 sums) ----
 * A pcV check i = (max_i, F_i, z_i, v_i, W_i) holds iff e(W_i, h^{alpha x}) e(g^{v_i} W_i^{-z_i}, h^alpha) = e(F_i, h^{x^{max_i - d}}).  With
 * non-zero 128-bit randomizers rho_i, over all 4 + 3Q checks of all K proofs, the fold accepts iff
 *     e(sum rho_i W_i, h^{alpha x}) e((sum rho_i v_i) g - sum (rho_i z_i) W_i, h^alpha) prod_m e(-sum_{max_i = m} rho_i F_i, h^{x^{m-d}}) = 1
 * -- four Miller loops and one final exponentiation whatever K and Q are; a batch with a false equation passes with probability <= 2^-128.
 * rho_i = the first 16 bytes (little-endian) of SHA-256("sonic-hip/batch/v1" || seed || D || le64 i), 0 replaced by 1, where i = k (3Q + 4) +
 * (the check's index in sonic_verify's order) and D = SHA-256("sonic-hip/batch-digest/v1" || le64 n || le64 Q || le64 d || circuit digest ||
 * srs id || le64 K || K x (proof bytes || its challenges)): D binds everything the verdict depends on.
 *
 * The handle holds the circuit in device memory (as CSR, whichever form it is made from), the four G2 elements, the circuit digest, a
 * stream and an MSM workspace on the SRS's device.  It borrows the SRS, which must outlive it.  One call at a time per handle (calls on
 * one handle serialise); any number of handles may share an SRS.  Errors of construction are those of sonic_verify for the same circuit and SRS. */
int sonic_verifier_new(const sonic_srs_t* srs, int64_t n, int64_t Q, const uint8_t* wL, const uint8_t* wR, const uint8_t* wO, const uint8_t* cs,
                       sonic_verifier_t** out);
int sonic_verifier_new_csr(const sonic_srs_t* srs, int64_t n, int64_t Q, const int64_t* row_ptr, const int64_t* col, const uint8_t* val,
                           const uint8_t* cs, sonic_verifier_t** out);
void sonic_verifier_free(sonic_verifier_t* v);
int sonic_verifier_device(const sonic_verifier_t* v);
/* proofs: K x sonic_proof_size(Q) bytes.  challenges: K blocks of (2 + 2Q) Fr: y, z, then Q pairs (y_j, z_j) -- sonic_verify's arguments, proof
 * by proof.  seed: 32 bytes, or NULL (the library draws them from the operating system).  *all_accepted = 1 iff every proof is well-formed
 * and the fold over all of them holds.  each (K bytes, or NULL): per-proof verdicts -- all ones when *all_accepted; otherwise every
 * well-formed proof is folded on its own.  A MALFORMED PROOF (a non-canonical field element, a point off the curve or outside the
 * subgroup; also u = 0 or v = 0) IS A REJECTED PROOF, NOT A FAILED CALL: SONIC_OK, each[k] = 0, sonic_last_error names the first one --
 * unlike sonic_verify, so that one hostile proof cannot hide the verdicts of the others.  K < 1 or K (4Q + 7) > 2^26: SONIC_ERR_INVALID_ARG. */
int sonic_verifier_verify_batch(sonic_verifier_t* v, int64_t K, const uint8_t* proofs, const uint8_t* challenges, const uint8_t seed[32],
                                int* all_accepted, uint8_t* each);
/* Fiat-Shamir form: the challenges are recomputed per proof as sonic_verify_fs does; a proof whose own u, v are not its transcript's is rejected */
int sonic_verifier_verify_fs_batch(sonic_verifier_t* v, int64_t K, const uint8_t* proofs, const uint8_t seed[32], int* all_accepted, uint8_t* each);
/* the two kernels on their own.  eval_s: s(u_k, v_k) of the handle's circuit for K pairs (uv: K x 64 bytes, out: K x 32); a pair with u = 0 or
 * v = 0 gets 32 bytes of 0xff and the call returns SONIC_ERR_INEXACT_DIVISION after the other values are written.  g1_validate: flags[i] = 1
 * iff points[i] is what the host verifier accepts (canonical; infinity, or on the curve and in the order-r subgroup). */
int sonic_verifier_eval_s(sonic_verifier_t* v, int64_t K, const uint8_t* uv, uint8_t* out);
int sonic_g1_validate(const uint8_t* points, int64_t n, uint8_t* flags);
/* host only, no device: rho_0 .. rho_{count-1} of a batch with digest D (out: count x 16 bytes, little-endian) */
int sonic_verify_batch_randomizers(const uint8_t seed[32], const uint8_t batch_digest[32], int64_t count, uint8_t* out);

/* ---- Subgroup membership (ABI 7 additions) ----
 * Every point that enters the library is tested for membership of the order-r subgroup, and these two calls run that test on its own,
 * on the GPU, one thread per point.  The criteria: a finite point P of the curve is in G1 iff phi(P) = lambda P, with phi(x, y) =
 * (beta x, y), beta a cube root of unity in Fq and lambda = z^2 - 1 for the BLS parameter z = -0xd201000000010000 (phi^2 + phi + 1 = 0
 * on the whole curve and lambda^2 + lambda + 1 = r, so phi(P) = lambda P forces r P = O); a finite point P of the twist is in G2 iff
 * psi(P) = z P, with psi = twist . Frobenius . untwist, psi(x, y) = (conj(x) (1 + u)^(-(q-1)/3), conj(y) (1 + u)^(-(q-1)/2)) (psi^2 -
 * (z + 1) psi + q = 0 on the whole twist, so psi(P) = z P forces (q - z) P = O, and q - z = h1 r with h1 prime to the twist's cofactor).
 * Both walks are short -- z^2 has 128 bits, |z| has 64 -- where the definition, r P = O by double-and-add, walks 255.
 *
 * points: n encodings, 96 bytes as sonic_g1_validate reads them, 192 bytes as sonic_srs_get_g2_points writes them.  flags[i] = 0 for an
 * accepted point -- the all-zero encoding is the point at infinity and is accepted -- otherwise the error bits of the loaders: 1 a
 * non-canonical coordinate, 2 off the curve or twist, 4 outside the subgroup.  method: SONIC_SUBGROUP_DEFAULT is the endomorphism test,
 * the one every loader, validator and decompressor of the library runs; SONIC_SUBGROUP_WALK is the definition, kept for differential
 * tests and A/B measurements -- the two give the same flags on every input.  The call returns SONIC_OK whatever the verdicts are; n = 0 is
 * SONIC_OK and launches nothing; a NULL pointer with n > 0, n < 0, n > 2^26 (the bound of the batched verifier's validation stage) or an
 * unknown method is SONIC_ERR_INVALID_ARG. */
#define SONIC_SUBGROUP_DEFAULT 0   /* the endomorphism test */
#define SONIC_SUBGROUP_WALK    1   /* [r]P == O by double-and-add: the definition */
int sonic_g1_subgroup_check(const uint8_t* points96,  int64_t n, int method, uint8_t* flags);
int sonic_g2_subgroup_check(const uint8_t* points192, int64_t n, int method, uint8_t* flags);

/* ---- Pairing (ABI 7 additions) ----
 * Products of pairings checked in groups: the equations of KZG openings, of batches of BLS signatures, of the links of an SRS
 * ceremony.  The pairing is the verifier's own (one copy of the formulas for the host and the device, so both give the same bytes):
 * the ate Miller loop over |z| and the exponent 3 (q^12 - 1) / r.
 *
 * n_pairs pairs (g1: 96 bytes each, g2: 192 bytes each, the encodings of sonic_msm_g1 / sonic_msm_g2; all zeros is the point at
 * infinity, and a pair with one contributes 1), cut into n_groups groups: group g is pairs [group_end[g-1], group_end[g]), group_end
 * non-decreasing, group_end[n_groups-1] == n_pairs; an empty group's product is 1.
 * verdict[g]: 0 the product of the group's pairings is one; 1 it is not; otherwise the OR over the group's points of
 * 2 non-canonical, 4 off the curve / twist, 8 outside the subgroup (such a group's product is not computed).
 * gt (may be NULL): n_groups x 576 bytes, the value in the layout of sonic_srs_pairing -- e^3 of the textbook ate pairing,
 * since the exponent is 3 (q^12 - 1) / r; zeros for a group with a bad point.
 *
 * Every point is validated (canonical, on the curve, in the order-r subgroup), by the device's validators or the host's.  A bad point
 * is a verdict, not an error: the call returns SONIC_OK whatever the verdicts are.  SONIC_ERR_INVALID_ARG: a NULL array that is needed,
 * n_pairs or n_groups outside 0 .. 2^26, a group_end that decreases or does not end at n_pairs, an unknown `where`.  n_pairs == 0 with
 * n_groups empty groups is valid: verdict 0 for each.
 *
 * where: SONIC_PAIRING_HOST runs on up to 16 host threads, SONIC_PAIRING_GPU on the default device (one thread per pair, then one per
 * group), SONIC_PAIRING_AUTO by the library's rule: the device from the number of groups upward at which it was measured to win
 * (256 groups; README, "Pairing").  The environment's SONIC_PAIRING_GPU, read per call, overrides the rule -- 0: AUTO is the
 * host, 1: AUTO is the device -- and does the same for the per-proof verdicts of the batched verifiers (`each` after a failed fold).
 * AUTO decides by size alone and, like every device call of the library, does not fall back: where it picks the device and the process
 * has none, the call returns SONIC_ERR_NO_DEVICE (a HIP failure: SONIC_ERR_HIP).  SONIC_PAIRING_HOST is the one form that needs no GPU. */
#define SONIC_PAIRING_AUTO 0   /* the library's rule */
#define SONIC_PAIRING_HOST 1   /* pairing.hpp on host threads */
#define SONIC_PAIRING_GPU  2   /* the kernels of pairing.hip */
int sonic_pairing_check(const uint8_t* g1, const uint8_t* g2, int64_t n_pairs, const int64_t* group_end, int64_t n_groups,
                        int where, uint8_t* verdict, uint8_t* gt);

/* ---- Compressed encodings ----
 * The compressed form of the Zcash / IETF pairing-friendly-curves serialization, the default wire format of other BLS12-381 libraries.
 * Every existing entry point keeps its 96- / 192-byte little-endian encodings; these convert, and the `_z` verifier calls and the
 * compressed SRS container consume the compressed form directly.
 *
 * G1, 48 bytes: x as a 381-bit BIG-endian integer, three flag bits in byte 0:
 *   0x80  compression bit, always set (clear: malformed)
 *   0x40  infinity bit: infinity is exactly 0xc0 followed by 47 zero bytes (any other pattern with 0x40 set: malformed)
 *   0x20  sign bit: 1 iff y > (q - 1)/2 as an integer
 * Malformed also when, the flags masked, x >= q.  "Not on the curve" when x^3 + 4 is not a square.
 * G2, 96 bytes: x.c1 first, 48 big-endian bytes carrying the flags, then x.c0, 48 big-endian bytes (its three top bits zero).  Sign bit:
 * y.c1 > (q - 1)/2 when y.c1 != 0, otherwise y.c0 > (q - 1)/2; infinity and compression bits as for G1.  The uncompressed side is the
 * 192-byte layout of sonic_srs_get_g2_points: x.c0 || x.c1 || y.c0 || y.c1, little-endian.
 * The G1 generator is 97f1d3a7 3197d794 2695638c 4fa9ac0f c3688c4f 9774b905 a14e3a3f 171bac58 6c55e83f f97a1aef fb3af00a db22c6bb.
 *
 * Bulk conversion on the GPU, one thread per point; n = 0 is SONIC_OK.  decompress: flags[i] = 0 for an accepted point, otherwise the error
 * bits of the SRS loaders -- 1 malformed, 2 not on the curve, 4 outside the order-r subgroup (tested only when check_subgroup != 0) -- and
 * the refused point is written as infinity (zeros); the call returns SONIC_OK for well-formed arguments whatever the verdicts are, unless
 * flags == NULL: then the first refused point makes it SONIC_ERR_BAD_ENCODING.  compress: g1 input is validated as sonic_g1_validate does,
 * g2 input as sonic_srs_set_g2_points does (infinity allowed); a refused point -> SONIC_ERR_BAD_ENCODING. */
int sonic_g1_compress(const uint8_t* points96, int64_t n, uint8_t* out48);
int sonic_g1_decompress(const uint8_t* in48, int64_t n, int check_subgroup, uint8_t* out96, uint8_t* flags);
int sonic_g2_compress(const uint8_t* points192, int64_t n, uint8_t* out96);
int sonic_g2_decompress(const uint8_t* in96, int64_t n, int check_subgroup, uint8_t* out192, uint8_t* flags);
/* one proof, on the host, no device needed.  A compressed proof is the proof's record order with every 96-byte point replaced by its 48
 * bytes and the field elements untouched: (7 + 4Q) * 48 + (5 + 2Q) * 32 bytes.  compress validates the points as sonic_verify does
 * (canonical, on the curve, in the subgroup); decompress refuses a malformed, off-curve or out-of-subgroup point and a non-canonical field
 * element: SONIC_ERR_BAD_ENCODING either way. */
size_t sonic_proof_size_compressed(int64_t Q);
int sonic_proof_compress(int64_t Q, const uint8_t* proof, uint8_t* out);
int sonic_proof_decompress(int64_t Q, const uint8_t* proof_z, uint8_t* out_proof);
/* the batched verifier over K compressed proofs (K x sonic_proof_size_compressed(Q) bytes): decompression is the validation stage on the
 * GPU, and everything else -- the batch digest D, the Fiat-Shamir challenges, the checks -- reads the uncompressed bytes rebuilt from it.
 * A compressed proof is the same proof: for any proofs p and seed, verify_batch_z(compress(p)) gives the all_accepted and each of
 * verify_batch(p).  A malformed or off-curve compressed point rejects its own proof and changes no other verdict. */
int sonic_verifier_verify_batch_z(sonic_verifier_t* v, int64_t K, const uint8_t* proofs_z, const uint8_t* challenges, const uint8_t seed[32],
                                  int* all_accepted, uint8_t* each);
int sonic_verifier_verify_fs_batch_z(sonic_verifier_t* v, int64_t K, const uint8_t* proofs_z, const uint8_t seed[32], int* all_accepted, uint8_t* each);

/* ---- One circuit, many statements ----
 * In the reference a statement is (ArithCircuit, Assignment) with cs = wL.aL + wR.aR + wO.aO (test/Test/Reference.hs:138): the gate weights
 * are the program, the constants are the public inputs and change with every proof.  A prover handle and a verifier handle take cs when they
 * are made; these calls let ONE resident circuit -- its device layout, its prepared rows (sonic_prover_prepare), s(X,y), s(u,Y): all functions
 * of the weights only -- serve proofs of many statements.  cs enters the prover in one Q-term sum (k(y)), the verifier in the same sum, and
 * the Fiat-Shamir circuit digest as its last bytes.
 *
 * eval_constraints  the constants B assignments satisfy under the handle's weights, on the GPU (dense handle: three Q x n matrix-vector
 *                   products over Fr; CSR handle: one sparse product over the 3Q stacked rows), and the multiplication gates they break.
 *                   aL, aR, aO: B x n x 32 canonical bytes each; all three NULL: B must be 1 and the handle's resident assignment is read
 *                   (none set: SONIC_ERR_INVALID_ARG, as sonic_prover_prove).  out_cs: B x Q x 32 bytes, out_cs[b][q] = sum_i wL[q,i] aL_b[i]
 *                   + wR[q,i] aR_b[i] + wO[q,i] aO_b[i].  out_gates (may be NULL): B x 2 int64, {the number of i with aL_b[i] aR_b[i] !=
 *                   aO_b[i], the smallest such i (0-based) or -1}.  A non-canonical input: SONIC_ERR_BAD_ENCODING (the outputs are then
 *                   undefined); B < 1 or B n > 2^26: SONIC_ERR_INVALID_ARG; a handle with a proof in flight: SONIC_ERR_INVALID_ARG, as
 *                   sonic_prover_set_assignment.  The handle's own assignment and constants are left as they are.  Assignments are staged
 *                   through the device in chunks, so B is not bounded by device memory.
 * set_constants     overwrites the handle's cs (Q x 32 canonical bytes) in place: the assignment, the prepared rows, the share mode, parked
 *                   state and a proof graph captured under SONIC_PROVE_GRAPH=1 all stay.  A proof in flight: SONIC_ERR_INVALID_ARG, as
 *                   sonic_prover_set_assignment; a non-canonical cs: SONIC_ERR_BAD_ENCODING and the old constants stay.
 * prove_batch_statements   sonic_prove_batch with proof i's constants (cs: K x Q x 32) uploaded at the head of proof i's own queue, as its
 *                   assignment is: no device wait of its own.  Everything else as sonic_prove_batch: proof i on handle i % n_provers, all
 *                   proofs attempted, the first non-zero status returned; a proof whose assignment does not satisfy its constants gets
 *                   SONIC_ERR_SRS_INDEX, one with a non-canonical constant SONIC_ERR_BAD_ENCODING before anything of it is queued.  AFTER
 *                   THE CALL EACH HANDLE HOLDS THE CONSTANTS (and, when assignments are given, the assignment) OF THE LAST PROOF IT RAN.
 * fs_circuit_midstate[_csr], fs_circuit_digest_resume   host only, no device.  The midstate is the SHA-256 state after
 *                   "sonic-hip/circuit/v1" || le64 n || le64 Q || wL || wR || wO: SONIC_FS_MIDSTATE_SIZE bytes -- the chaining value (8 x le32),
 *                   the 64 bytes of the pending block (zero behind the pending ones), le64 length, le64 Q (sonic_amd/csrc/fs.hpp).
 *                   resume(midstate(W), cs) == sonic_fs_circuit_digest[_csr](W, cs) byte for byte, for every cs, at Q x 32 bytes of hashing;
 *                   dense and CSR midstates of the same matrices are equal.  resume refuses a midstate whose length is not 36 + 96 Q n for
 *                   its Q (SONIC_ERR_INVALID_ARG) and a non-canonical cs (SONIC_ERR_BAD_ENCODING).  sonic_prover_prove_fs takes the digest
 *                   from its caller: after set_constants, pass the resumed one. */
#define SONIC_FS_MIDSTATE_SIZE 112
int sonic_prover_eval_constraints(sonic_prover_t* p, int64_t B, const uint8_t* aL, const uint8_t* aR, const uint8_t* aO, uint8_t* out_cs,
                                  int64_t* out_gates);
int sonic_prover_set_constants(sonic_prover_t* p, const uint8_t* cs);
int sonic_prove_batch_statements(sonic_prover_t* const* provers, int n_provers, int64_t K, const uint8_t* aL, const uint8_t* aR, const uint8_t* aO,
                                 const uint8_t* cs, const uint8_t* transcripts, uint8_t* out_proofs, int* out_status);
int sonic_fs_circuit_midstate(int64_t n, int64_t Q, const uint8_t* wL, const uint8_t* wR, const uint8_t* wO, uint8_t out[SONIC_FS_MIDSTATE_SIZE]);
int sonic_fs_circuit_midstate_csr(int64_t n, int64_t Q, const int64_t* row_ptr, const int64_t* col, const uint8_t* val,
                                  uint8_t out[SONIC_FS_MIDSTATE_SIZE]);
int sonic_fs_circuit_digest_resume(const uint8_t midstate[SONIC_FS_MIDSTATE_SIZE], const uint8_t* cs, uint8_t out[32]);
/* The batched verifier with proof k checked against the handle's weights and ITS OWN constants cs_k (cs: K x Q x 32 bytes).  compressed: 0 =
 * proofs of sonic_proof_size(Q) bytes, 1 = of sonic_proof_size_compressed(Q) bytes (the `_z` forms' input).  Everything else -- challenges,
 * seed, all_accepted, each, the size limits -- as sonic_verifier_verify_batch / _fs_batch; the Fiat-Shamir form derives proof k's challenges
 * from resume(the handle's midstate, cs_k).  A non-canonical cs_k makes proof k a rejected, malformed proof, not a failed call.  The
 * randomizers bind the constants: rho_i is derived as above from
 *     D = SHA-256("sonic-hip/batch-digest/v2" || le64 n || le64 Q || le64 d || the handle's circuit digest || srs id || le64 K ||
 *                 K x (proof bytes || its challenges || cs_k))
 * (for compressed = 1 the rebuilt uncompressed proof bytes).  With every cs_k equal to the handle's constants the verdicts are those of
 * sonic_verifier_verify_batch.  sonic_verify_batch_digest_v2 is D on its own: host only, no device (challenges: K blocks of 2 + 2Q). */
int sonic_verifier_verify_batch_cs(sonic_verifier_t* v, int64_t K, const uint8_t* proofs, int compressed, const uint8_t* challenges,
                                   const uint8_t* cs, const uint8_t seed[32], int* all_accepted, uint8_t* each);
int sonic_verifier_verify_fs_batch_cs(sonic_verifier_t* v, int64_t K, const uint8_t* proofs, int compressed, const uint8_t* cs,
                                      const uint8_t seed[32], int* all_accepted, uint8_t* each);
int sonic_verify_batch_digest_v2(int64_t n, int64_t Q, int64_t d, const uint8_t circuit_digest[32], const uint8_t srs_id[32], int64_t K,
                                 const uint8_t* proofs, const uint8_t* challenges, const uint8_t* cs, uint8_t out[32]);

/* ---- Fiat-Shamir proofs in flight ----
 * The Fiat-Shamir prover beside sonic_prover_prove_fs, which stays as it is: one proof in flight per handle, batches over several handles,
 * and the digest of the assignment computed by the GPU.  A proof made here verifies like any other (sonic_verify_fs and the batched
 * verifier see no difference); its BLINDERS differ from sonic_prover_prove_fs's for the same seed, because they are derived from
 *   witness digest v2 = SHA-256("sonic-hip/witness/v2" || le64 n || root), root = a SHA-256 tree over the canonical bytes of aL || aR || aO
 *                   with 1024-byte leaves and 32 digests per node, every message opened by a 64-byte header that names the leaf or the level
 *                   and node (exact definition: sonic_amd/csrc/fs.hpp).  The GPU hashes the handle's resident assignment where it lies; 32
 *                   bytes come back.  Cached per assignment: set_assignment, an assignment handed over with a proof (batches, the
 *                   one-shot calls) and a failed upload invalidate it.
 *   witness_digest_v2  that digest of the resident assignment (SONIC_ERR_INVALID_ARG: none set, or a proof in flight)
 *   submit_fs       checks what sonic_prover_prove_fs checks (an assignment is set, nothing in flight, not one rank's share), marks the
 *                   handle in flight and hands the six passes to a host thread the handle owns (made on first use, joined by
 *                   sonic_prover_free, which therefore returns only after a proof in flight has ended).  Returns without waiting for the
 *                   device: one host thread keeps several handles busy, each handle's waits and hashes under the others' kernels.
 *   collect_fs      waits for that proof; out_transcript (may be NULL) as for prove_fs.  Its status is the proof's, and its message
 *                   becomes the calling thread's last error.  SONIC_ERR_INVALID_ARG with nothing in flight, or when the flight was
 *                   submitted with a transcript (sonic_prover_submit); sonic_prover_collect / collect_share refuse a Fiat-Shamir flight
 *                   the same way, and either leaves the flight as it is.  While a Fiat-Shamir proof is in flight every call that a
 *                   transcript flight refuses is refused (set_assignment, set_constants, prepare, set_share, eval_constraints, any prove
 *                   or submit).
 *   prove_batch_fs  sonic_prove_batch_statements' shape and rules (proof i on handle i % n_provers, one host thread per handle, all K
 *                   attempted, the first non-zero status in list order returned, out_status per proof) with a circuit digest and a
 *                   blinder seed per proof in place of a transcript: circuit_digests[i] = sonic_fs_circuit_digest_resume(midstate, cs_i).
 *                   aL, aR, aO: K x n x 32 each, or all NULL (the resident assignments); cs: K x Q x 32, or NULL (the handles'
 *                   constants); out_transcripts: K x (8 + 2Q) x 32, may be NULL. */
int sonic_prover_witness_digest_v2(sonic_prover_t* p, uint8_t out[32]);
int sonic_prover_submit_fs(sonic_prover_t* p, const uint8_t circuit_digest[32], const uint8_t blinder_seed[32]);
int sonic_prover_collect_fs(sonic_prover_t* p, uint8_t* out_proof, uint8_t* out_transcript);
int sonic_prove_batch_fs(sonic_prover_t* const* provers, int n_provers, int64_t K, const uint8_t* aL, const uint8_t* aR, const uint8_t* aO,
                         const uint8_t* cs, const uint8_t* circuit_digests, const uint8_t* blinder_seeds, uint8_t* out_proofs,
                         uint8_t* out_transcripts, int* out_status);

/* ---- Witness sources ----
 * Where an assignment comes from, as ONE description that every prover entry point below accepts: host or device memory, 32-byte
 * canonical Fr or signed 64-bit integers, aO given or derived on the GPU.  The calls above that take three host buffers of n x 32
 * canonical bytes stay as they are; for the same values these give the same bytes (proofs, constants, witness digests).
 *
 * Memory and alignment.  A device source with kind SONIC_WIT_FR32: the three pointers are 32-byte aligned and stride is a multiple of
 * 32; with kind SONIC_WIT_I64: 8-byte aligned, stride a multiple of 8.  A host source: any alignment.  stride, where it is not 0, is at
 * least n * element size.  The source is only read, and it must stay unchanged until the call returns; every call here is blocking.
 *
 * Ordering.  With a non-NULL hip_stream the library records an event on that stream at entry, and the handle's stream (each handle's,
 * in a batch) waits on that event before it reads the source.  With NULL the caller states that the data is complete.  The library
 * never makes the caller's stream wait.
 *
 * Devices.  A device source must lie on the GPU of every handle that reads it (checked with hipPointerGetAttributes): a mismatch is
 * SONIC_ERR_INVALID_ARG with a message that names both devices, and so is a host pointer passed with on_device = 1.  No peer copy is made.
 *
 * A device source is read where it lies, by one launch that checks, converts to Montgomery form and, with aO == NULL, multiplies; a host
 * source is copied into a staging buffer of the handle first (8 n bytes per vector for SONIC_WIT_I64) and read by the same launch.
 *
 *   set_witness     sonic_prover_set_assignment from a source.  A proof in flight, or a description that breaks a rule above:
 *                   SONIC_ERR_INVALID_ARG, before anything is launched and with the resident assignment left as it is.  A non-canonical
 *                   SONIC_WIT_FR32 element: SONIC_ERR_BAD_ENCODING, and the handle then has no assignment.  The witness digests are
 *                   recomputed on their next use, as after set_assignment.
 *   eval_constraints_src   sonic_prover_eval_constraints over B assignments of a source (B n <= 2^26; assignment b is block b of each
 *                   vector).  With aO == NULL no gate can break: out_gates is {0, -1} for every assignment.
 *   prove_batch_src   sonic_prove_batch_statements' shape and rules with proof i's assignment read from block i of the source, converted
 *                   at the head of proof i's own queue: no device wait of its own.  cs: K x Q x 32, or NULL (the handles' constants).
 *                   A proof with a non-canonical element gets SONIC_ERR_BAD_ENCODING in out_status; the others are unaffected.
 *   prove_batch_fs_src   the same for sonic_prove_batch_fs. */
#define SONIC_WIT_FR32 0   /* 32-byte little-endian canonical Fr per element (what set_assignment takes) */
#define SONIC_WIT_I64  1   /* int64_t per element; v >= 0 is v, v < 0 is r - |v| (INT64_MIN is r - 2^63) */
typedef struct sonic_witness_src {
  const void *aL, *aR, *aO;  /* aO == NULL: the library sets aO[i] = aL[i] * aR[i] in Fr */
  int32_t kind;              /* SONIC_WIT_*; one kind for all three vectors */
  int32_t on_device;         /* 0: host memory; 1: memory of the GPU the handle lives on */
  int64_t stride;            /* bytes from assignment b to b + 1 within each vector, in batched calls; 0 = packed (n * element size) */
  void*   hip_stream;        /* on_device only: the stream whose work produces the data, or NULL */
} sonic_witness_src_t;
int sonic_prover_set_witness(sonic_prover_t* p, const sonic_witness_src_t* src);
int sonic_prover_eval_constraints_src(sonic_prover_t* p, int64_t B, const sonic_witness_src_t* src, uint8_t* out_cs, int64_t* out_gates);
int sonic_prove_batch_src(sonic_prover_t* const* provers, int n_provers, int64_t K, const sonic_witness_src_t* src, const uint8_t* cs,
                          const uint8_t* transcripts, uint8_t* out_proofs, int* out_status);
int sonic_prove_batch_fs_src(sonic_prover_t* const* provers, int n_provers, int64_t K, const sonic_witness_src_t* src, const uint8_t* cs,
                             const uint8_t* circuit_digests, const uint8_t* blinder_seeds, uint8_t* out_proofs, uint8_t* out_transcripts,
                             int* out_status);

/* ---- Core proofs ----
 * A second proof form beside the reference-shaped one, which stays byte for byte what it is.
 *
 * Why.  `verify` (Protocol.hs:119-126) reads the proof's s in one place, t = a (b + s) - k(y), and the embedded HscProof is made at pairs
 * (y_j, z_j) drawn independently of (y, z): nothing that sonic_verify* or the batched verifier checks ties s to s(z, y).  Whoever picks
 * r(X) and t'(X) freely, opens them honestly and SOLVES the head equation for s satisfies every check for any statement, with any honest
 * signature of the same circuit appended.  That is the reference's behaviour; a deployed verifier must close it.
 *
 * A CORE proof is the head and nothing else -- R, T, a, W_a, b, W_b, W_t, s: 5 points and 3 field elements, SONIC_CORE_PROOF_SIZE bytes
 * whatever Q is -- and its verifier is Sonic's unhelped one: it evaluates s(z, y) itself (O(nnz + n); the batched verifier on the GPU),
 * REJECTS a proof whose s differs, and checks the three pcV equations of the head.  The head of a full proof is a core proof, so an
 * existing proof is checked soundly by sonic_verify_core over its first 576 bytes with its own y, z (a Fiat-Shamir proof's:
 * sonic_fs_challenges_v2).
 *
 * Prover.  The same kernel chain with the signature's jobs left out: 5 MSMs instead of 7 + 4Q.
 *   prove_core      transcript: 6 x 32 bytes (the blinders c_{n+1..n+4}, y, z).  For every transcript t of a full proof,
 *                   prove_core(t[0:6]) is the first 576 bytes of sonic_prover_prove(t): prepared or not, dense or CSR, over an SRS view.
 *                   A handle may alternate core and full proofs.  A handle in share mode: SONIC_ERR_INVALID_ARG.
 *   submit_core / collect_core   one proof in flight per handle, as sonic_prover_submit / collect.  sonic_prover_collect, collect_share and
 *                   collect_fs on a core flight are SONIC_ERR_INVALID_ARG and leave the flight as it is; so is collect_core on a
 *                   transcript or Fiat-Shamir flight, or on nothing.
 *   prove_core_fs   the Fiat-Shamir form, three passes; blinders from witness digest v2 as sonic_prover_submit_fs's.  The transcript has a
 *                   label of its own, so that a core proof can never be replayed as the head of a full one:
 *                     st0 = SHA256("sonic-hip/fs-core/v1" || le64 n || le64 Q || le64 d || circuit digest || srs id)
 *                     absorb("R", R) -> y = challenge("y", 0);   absorb("T", T) -> z = challenge("z", 0)
 *                   (absorb / challenge: sonic_amd/csrc/fs.hpp).  out_yz: y || z, 64 bytes, may be NULL.
 *   fs_core_challenges   y || z of a core proof, recomputed on the host; no device needed.
 *   prove_batch_core_src / prove_batch_core_fs_src   sonic_prove_batch_src's / _fs_src's shape and rules (proof i on handle i % n_provers, all
 *                   attempted, the first non-zero status returned).  src NULL: the handles' resident assignments.  cs: K x Q x 32 or
 *                   NULL; transcripts: K x 192; out_proofs: K x 576; out_yz: K x 64, may be NULL.
 *
 * Verifiers.
 *   verify_core[_csr]   one proof on the host, like sonic_verify: *accepted = 0 when the proof's s is not s(z, y) or an equation fails.
 *                   y = 0 or z = 0: SONIC_ERR_INEXACT_DIVISION.  verify_core_fs[_csr] recomputes y, z first.
 *   verifier_verify_core_batch / _core_fs_batch   K core proofs on a sonic_verifier_t handle: the 5K points validated (compressed = 1:
 *                   decompressed) on the GPU, s(z_k, y_k) by the kernel that evaluates s(u_k, v_k) for full proofs, the 3K checks folded
 *                   into the same four Miller loops.  yz: K x 64; cs: K x Q x 32, or NULL (the handle's constants for every proof).
 *                   A proof whose s is not s(z_k, y_k), a malformed proof (a non-canonical cs_k included) and one with y_k or z_k zero
 *                   are REJECTED proofs, not failed calls: each[k] = 0, the others' verdicts stand, sonic_last_error names the first.
 *                   Randomizers as sonic_verify_batch_randomizers' over
 *                     D = SHA-256("sonic-hip/batch-digest/core/v1" || le64 n || le64 Q || le64 d || circuit digest || srs id || le64 K ||
 *                                 K x (576 proof bytes || y_k || z_k || cs_k))
 *                   with check index 3k + i; compressed proofs are hashed as their rebuilt uncompressed bytes.
 *   verify_core_batch_digest   that D on its own; no device needed. */
#define SONIC_CORE_PROOF_SIZE 576
#define SONIC_CORE_PROOF_SIZE_COMPRESSED 336
int sonic_prover_prove_core(sonic_prover_t* p, const uint8_t* transcript, uint8_t* out_proof);
int sonic_prover_submit_core(sonic_prover_t* p, const uint8_t* transcript);
int sonic_prover_collect_core(sonic_prover_t* p, uint8_t* out_proof);
int sonic_prover_prove_core_fs(sonic_prover_t* p, const uint8_t circuit_digest[32], const uint8_t blinder_seed[32], uint8_t* out_proof, uint8_t* out_yz);
int sonic_fs_core_challenges(int64_t n, int64_t Q, int64_t d, const uint8_t circuit_digest[32], const uint8_t srs_id[32], const uint8_t* proof, uint8_t* out_yz);
int sonic_prove_batch_core_src(sonic_prover_t* const* provers, int n_provers, int64_t K, const sonic_witness_src_t* src, const uint8_t* cs,
                               const uint8_t* transcripts, uint8_t* out_proofs, int* out_status);
int sonic_prove_batch_core_fs_src(sonic_prover_t* const* provers, int n_provers, int64_t K, const sonic_witness_src_t* src, const uint8_t* cs,
                                  const uint8_t* circuit_digests, const uint8_t* blinder_seeds, uint8_t* out_proofs, uint8_t* out_yz, int* out_status);
int sonic_verify_core(const sonic_srs_t* srs, int64_t n, int64_t Q, const uint8_t* wL, const uint8_t* wR, const uint8_t* wO, const uint8_t* cs,
                      const uint8_t* proof, const uint8_t y[32], const uint8_t z[32], int* accepted);
int sonic_verify_core_csr(const sonic_srs_t* srs, int64_t n, int64_t Q, const int64_t* row_ptr, const int64_t* col, const uint8_t* val,
                          const uint8_t* cs, const uint8_t* proof, const uint8_t y[32], const uint8_t z[32], int* accepted);
int sonic_verify_core_fs(const sonic_srs_t* srs, int64_t n, int64_t Q, const uint8_t* wL, const uint8_t* wR, const uint8_t* wO, const uint8_t* cs,
                         const uint8_t* proof, int* accepted);
int sonic_verify_core_fs_csr(const sonic_srs_t* srs, int64_t n, int64_t Q, const int64_t* row_ptr, const int64_t* col, const uint8_t* val,
                             const uint8_t* cs, const uint8_t* proof, int* accepted);
int sonic_verifier_verify_core_batch(sonic_verifier_t* v, int64_t K, const uint8_t* proofs, int compressed, const uint8_t* yz, const uint8_t* cs,
                                     const uint8_t seed[32], int* all_accepted, uint8_t* each);
int sonic_verifier_verify_core_fs_batch(sonic_verifier_t* v, int64_t K, const uint8_t* proofs, int compressed, const uint8_t* cs,
                                        const uint8_t seed[32], int* all_accepted, uint8_t* each);
int sonic_verify_core_batch_digest(int64_t n, int64_t Q, int64_t d, const uint8_t circuit_digest[32], const uint8_t srs_id[32], int64_t K,
                                   const uint8_t* proofs, const uint8_t* yz, const uint8_t* cs, uint8_t out[32]);
int sonic_core_proof_compress(const uint8_t* proof, uint8_t* out);
int sonic_core_proof_decompress(const uint8_t* proof_z, uint8_t* out_proof);

/* ---- Helped verification: one aggregate signature for K core proofs (ABI 7, additions only) ----
 * A core proof carries no signature of correct computation, so its verifier evaluates s(z_k, y_k) itself: O(nnz + n) per proof.  Sonic's
 * helped mode moves that cost to an untrusted HELPER, which proves all K values s(z_k, y_k) with ONE signature (Signature.hs:38-72 with
 * m = K), after which a verifier needs s(u, v) at one point per batch.
 *
 * The aggregate for K pairs (y_k, z_k) is exactly an HscProof with m = K in the layout sonic_prover_hsc_prove writes --
 * [S_j, s_j, W_j]_j, [s'_j, W'_j, Q_j]_j, Q_v, C, u, v: sonic_hsc_proof_size(K) bytes -- so sonic_hsc_verify(m = K) accepts a correct one
 * and sonic_prover_hsc_prove(K, yzs, u, v) reproduces it byte for byte.  Its s_k is s(z_k, y_k): proof k's s must equal it.
 * u and v are not the helper's to choose.  They come from a transcript with a label of its own (absorb / challenge: sonic_amd/csrc/fs.hpp):
 *     st0 = SHA256("sonic-hip/fs-agg/v1" || le64 n || le64 Q || le64 d || weights digest || srs id)
 *     absorb("pairs", le64 K || K x (y_k || z_k))
 *     absorb("hscS", [S_j || s_j || W_j]_j)          -> u = challenge("u", 0)
 *     absorb("hscW", C || [s'_j || W'_j || Q_j]_j)   -> v = challenge("v", 0)
 * u follows every S_j, s_j, W_j and v follows C and every s'_j, W'_j, Q_j: a helper that knew u before it committed S_j (or v before C)
 * could commit to a polynomial that agrees with s at that one point only.
 * s(X, Y) depends on the gate weights only, and one circuit serves many statements with their own constants, so the transcript binds
 *     weights digest = SHA256("sonic-hip/weights/v1" || the SONIC_FS_MIDSTATE_SIZE bytes of sonic_fs_circuit_midstate[_csr])
 * and not the circuit digest, which ends in cs.
 *
 *   fs_weights_digest          that digest from a midstate (the bytes are hashed as they are); no device needed.
 *   fs_aggregate_challenges    u || v (64 bytes) that the bytes of an aggregate determine; no device needed.  yz: K x 64, y_k || z_k.
 *   prover_aggregate_core      the helper, on a prover handle (dense or CSR, prepared or not, over an SRS view too; no assignment needed).
 *                   Blocking; three passes with a host hash between them: S_j, s_j, W_j -> u -> C, s'_j, W'_j, Q_j -> v -> Q_v.  The
 *                   polynomials s(X, y_j) of up to 8 pairs come from one launch that reads the circuit once, their 16 MSMs run as one
 *                   chain, and the tiles of 8 are dealt over the handle's lanes.  Pass 2 reads the polynomials of pass 1 again: they are
 *                   kept when K (3n + 1) 32 bytes fit 4 GiB and recomputed per tile otherwise (SONIC_AGG_KEEP=0 / 1 forces either), so
 *                   device memory is bounded by that budget, not by K.  out: sonic_hsc_proof_size(K) bytes.
 *                   A zero y_k or z_k: SONIC_ERR_INEXACT_DIVISION before anything is launched.  A proof in flight, a handle in share
 *                   mode, K < 1: SONIC_ERR_INVALID_ARG (a flight stays intact).  A non-canonical y_k or z_k: SONIC_ERR_BAD_ENCODING.
 *   verifier_verify_core_batch_helped / _core_fs_batch_helped   K core proofs and the aggregate over their (y_k, z_k) on a sonic_verifier_t
 *                   handle (the _fs form recomputes y_k, z_k per proof as sonic_verifier_verify_core_fs_batch does).  proofs, compressed, yz,
 *                   cs, seed, all_accepted, each: as sonic_verifier_verify_core_batch's; aggregate: sonic_hsc_proof_size(K) bytes.  Steps:
 *                     1. the proofs' 5K points (compressed = 1: decompressed) and the aggregate's 4K + 2 points are validated on the GPU;
 *                     2. u, v are recomputed from the transcript: the aggregate's own must match, and neither may be zero;
 *                     3. proof k's s must equal the aggregate's s_k, as bytes;
 *                     4. s(u, v) is evaluated ONCE (where the unhelped batch evaluates s(z_k, y_k) K times);
 *                     5. the 3K checks of the heads and the 3K + 1 of the signature are folded into the same four Miller loops, under
 *                        randomizers derived from the digest D below: check index 3k + i for the heads, 3K + (position in the
 *                        signature's list: S_j at z_j, S_j at u, C at y_j for j = 0 .., then C at v) for the signature.
 *                   Verdicts: a bad input is a rejected proof, not a failed call.  An aggregate that is malformed, whose u, v are not
 *                   its transcript's, or whose global check (C at v against s(u, v)) fails rejects EVERY proof: each[k] = 0 for all k, and
 *                   sonic_last_error names the aggregate.  Otherwise proof k is accepted iff it is well-formed, its s equals s_k, its
 *                   three head checks hold and the three signature checks of j = k hold: when the whole fold fails, the global check is
 *                   folded alone, then each k's six checks alone, and the others' verdicts stand.
 *                   The handle computes the weights digest from what it holds, once, on the first helped call.
 *   verify_core_helped_digest  the digest a helped batch derives its randomizers from (as sonic_verify_batch_randomizers'); no device needed:
 *                     D = SHA-256("sonic-hip/batch-digest/helped/v1" || le64 n || le64 Q || le64 d || weights digest || srs id || le64 K ||
 *                                 K x (576 proof bytes || y_k || z_k || cs_k) || aggregate bytes) */
int sonic_fs_weights_digest(const uint8_t midstate[SONIC_FS_MIDSTATE_SIZE], uint8_t out[32]);
int sonic_fs_aggregate_challenges(int64_t n, int64_t Q, int64_t d, const uint8_t weights_digest[32], const uint8_t srs_id[32], int64_t K, const uint8_t* yz,
                                  const uint8_t* aggregate, uint8_t out_uv[64]);
int sonic_prover_aggregate_core(sonic_prover_t* p, const uint8_t weights_digest[32], int64_t K, const uint8_t* yz, uint8_t* out);
int sonic_verifier_verify_core_batch_helped(sonic_verifier_t* v, int64_t K, const uint8_t* proofs, int compressed, const uint8_t* yz, const uint8_t* cs,
                                            const uint8_t* aggregate, const uint8_t seed[32], int* all_accepted, uint8_t* each);
int sonic_verifier_verify_core_fs_batch_helped(sonic_verifier_t* v, int64_t K, const uint8_t* proofs, int compressed, const uint8_t* cs,
                                               const uint8_t* aggregate, const uint8_t seed[32], int* all_accepted, uint8_t* each);
int sonic_verify_core_helped_digest(int64_t n, int64_t Q, int64_t d, const uint8_t weights_digest[32], const uint8_t srs_id[32], int64_t K,
                                    const uint8_t* proofs, const uint8_t* yz, const uint8_t* cs, const uint8_t* aggregate, uint8_t out[32]);

/* ---- Updatable SRS: check a string, contribute to it, verify a contribution (ABI 7, additions only) ----
 * Notation: G0[e] = basis 0, G1[e] = basis 1 (slot e = 0 empty), H0[e], H1[e] the G2 bases, e in [-d, d]; g, h the fixed generators.
 * All three calls take whole strings: a circuit-sized view is SONIC_ERR_INVALID_ARG.
 *
 *   srs_check       whether the points of a handle ARE a reference string: the consecutive powers of one x over g and h, with the alpha
 *                   basis and the G2 half belonging to them.  (Loading checks every point on its own -- canonical, on the curve, in the
 *                   subgroup -- and nothing else: a file with one wrong element, or with bases of two trapdoors, loads.)  Run it on
 *                   every string that comes from outside, before the first prover or verifier is made over it.
 *                   The handle needs its G2 half (one that can still generate it does so first; none: SONIC_ERR_INVALID_ARG).
 *                   With randomizers rho_e the string passes iff
 *                     R0  G0[0] == g and H0[0] == h, as bytes
 *                     R1  e(P, H0[1]) = e(P+, h),          P = sum_{e=-d}^{d-1} rho_e G0[e],  P+ = sum_{e=-d}^{d-1} rho_e G0[e+1]
 *                     R2  e(A, h) = e(A0, H1[0]),          A = sum_{e!=0} rho_e G1[e],        A0 = sum_{e!=0} rho_e G0[e]
 *                     R3  e(g, B) = e(sum_e rho_e G0[e], h),          B = sum_e rho_e H0[e]
 *                     R4  e(g, C) = e(sum_e rho_e G0[e], H1[0]),      C = sum_e rho_e H1[e]   (every element, e = 0 included)
 *                   *failed is the bit mask of the relations that do not hold (SONIC_SRS_CHECK_R0 .. R4), 0 for a string that passes.
 *                   The return value is SONIC_OK either way: errors are bad arguments and HIP failures only.
 *                   rho_e = the first 16 bytes of SHA-256("sonic-hip/srs-check/v1" || seed || le64 (e + d)) as a little-endian integer,
 *                   1 in place of 0; a wrong string passes with probability <= 2^-128 per relation.  seed = NULL draws 32 bytes from the
 *                   operating system (none to be had: SONIC_ERR_HIP).  The string is fixed before the seed is drawn, so the seed need not bind the string.  A
 *                   caller-supplied seed is for reproducible tests only: whoever knows the seed before choosing the string can defeat the check.
 *   srs_update      a contribution: a NEW handle on the same GPU with G0'[e] = x1^e G0[e], G1'[e] = alpha1 x1^e G1[e], H0'[e] = x1^e H0[e],
 *                   H1'[e] = alpha1 x1^e H1[e] -- the string of trapdoor (x x1, alpha alpha1) -- with its own tables.  The source handle
 *                   is untouched (provers hold it).  The new handle holds no trapdoor.  proof: 448 bytes,
 *                     X = x1 g (96) || A = alpha1 g (96) || Rx = kx g (96) || Ra = ka g (96) || sx (32) || sa (32),
 *                   two Schnorr proofs under one challenge that binds d and the Fiat-Shamir id of the OLD string
 *                   (sonic_amd/csrc/srs_update.hpp has the normative text).  seed = NULL: nonces from the operating system; a seed
 *                   derives them from the seed, the shares and the old id, for tests.
 *                   A share that is zero: SONIC_ERR_INVALID_ARG; not below r: SONIC_ERR_BAD_ENCODING; a source without a G2 half:
 *                   SONIC_ERR_INVALID_ARG -- each before anything is launched.  The library's named host copies of the shares, their
 *                   inverse and the nonces are wiped before the call returns, on every path.  Not wiped: what the compiler and the HIP
 *                   runtime copy on their own (stack temporaries of the field arithmetic, the kernels' argument buffers), and x1 and
 *                   alpha1 themselves, which are the caller's.  An operating system that gives no random bytes: SONIC_ERR_HIP.
 *   srs_verify_update   *ok = 1 iff new is old updated by someone who knew the shares behind the proof: the same d; the proof's four
 *                   points canonical, on the curve, in the subgroup, not infinity, its two scalars canonical; sx g = Rx + c X and
 *                   sa g = Ra + c A; e(G0'[1], h) = e(X, H0[1]); e(g, H1'[0]) = e(A, H1[0]); and, with check_new != 0, the new string
 *                   passes sonic_srs_check.  Without that check the two pairing equations say nothing about the other 8d + 2 points: pass
 *                   check_new = 0 only for a string that is checked elsewhere.  A malformed proof gives *ok = 0, not an error.  Both
 *                   handles need their G2 halves. */
#define SONIC_SRS_CHECK_R0 1
#define SONIC_SRS_CHECK_R1 2
#define SONIC_SRS_CHECK_R2 4
#define SONIC_SRS_CHECK_R3 8
#define SONIC_SRS_CHECK_R4 16
#define SONIC_SRS_UPDATE_PROOF_SIZE 448
int sonic_srs_check(const sonic_srs_t* srs, const uint8_t seed[32], int* failed);
int sonic_srs_update(const sonic_srs_t* srs, const uint8_t x1[32], const uint8_t alpha1[32], const uint8_t seed[32], sonic_srs_t** out, uint8_t proof[448]);
int sonic_srs_verify_update(const sonic_srs_t* old_srs, const sonic_srs_t* new_srs, const uint8_t proof[448], int check_new, int* ok);

/* ---- R1CS front end (ABI 7, additions only) ----
 * A layer in front of the entry points above for callers who arrive with a rank-1 constraint system: three sparse matrices A, B, C and
 * witness vectors z with <A_i, z> <B_i, z> = <C_i, z> for every row i.  A handle compiles the matrices into a Sonic constraint system (the
 * CSR that sonic_prover_new_csr takes) and turns K witness vectors into K assignments and their constants on the GPU: a batched sparse
 * matrix-vector product over Fr whose result lies in device memory, where a witness source reads it.
 *
 * The mapping ("layout 1", normative).
 *   Input.  A, B, C: m >= 1 rows over N >= 1 columns, each canonical CSR as the gate-weight CSR is: row_ptr has m + 1 int64 entries,
 *   starts at 0 and does not decrease; col lies in [0, N) and strictly increases within a row; val is 32-byte canonical Fr; explicit zeros
 *   are allowed and stay entries.  Column 0 is the constant one (z[0] = 1), columns 1..n_pub are the public inputs (0 <= n_pub <= N - 1),
 *   the rest are private.
 *   Gates.  n = m + g with g = N / 2 (rounded down); columns are 0-based.  Constraint gate i < m: aL[i] = <A_i, z>, aR[i] = <B_i, z>,
 *   aO[i] = <C_i, z> -- the C side, not the product, so an unsatisfied row is a broken multiplication gate i.  Variable j >= 1 has the
 *   home(j) = (wL if j - 1 is even, else wR; gate m + (j - 1) / 2): aL and aR of a variable gate hold its two variables (a missing partner,
 *   N even, is 0) and aO their product.
 *   Linear constraints.  Q = 3m + n_pub:
 *     row i            aL[i] - sum_{j >= 1} A_ij home(j) = A_i0        cs = A_i0 (0 if absent)
 *     row m + i        the same for B over aR[i]                       cs = B_i0
 *     row 2m + i       the same for C over aO[i]                       cs = C_i0
 *     row 3m + k - 1   home(k) = z[k],  k = 1..n_pub                   cs = z[k]
 *   In the stacked CSR of 3Q rows (wL rows, wR rows, wO rows) the weight 1 sits at (wL, q, i) for A rows, (wR, q, i) for B rows, (wO, q, i)
 *   for C rows and at home(k) for the public rows; the weight r - A_ij (0 for an explicit zero) at (wL or wR by home(j), q, home gate).
 *   Within a row every column is distinct and increasing; no entries are merged:
 *     nnz = nnz(A) + nnz(B) + nnz(C) - (entries in column 0) + 3m + n_pub.
 *   Constants.  The first 3m entries of cs depend on the circuit alone, the last n_pub are the public inputs: the split that
 *   sonic_prover_set_constants and the batches' cs serve.
 *
 *   r1cs_new[_on]   validates (a structure violation, n_pub > N - 1, or n, N or an entry count beyond 32 bits: SONIC_ERR_INVALID_ARG with a
 *                   message that names matrix and row; a value >= r: SONIC_ERR_BAD_ENCODING) and uploads A, B, C to one GPU.
 *   r1cs_shape      out = {n, Q, nnz of the Sonic CSR, g}.
 *   r1cs_circuit    host only: row_ptr[3Q + 1], col[nnz], val[32 nnz] and cs_fixed[32 Q] (public slots zero).
 *   r1cs_assign     K witnesses z_k (N elements each; kind SONIC_WIT_FR32 or SONIC_WIT_I64, on_device, z_stride in bytes with 0 = packed,
 *                   hip_stream: all as a witness source's, with its alignment, ordering and device rules) -> the three planes d_aL, d_aR,
 *                   d_aO (device pointers on the handle's GPU, 32-byte aligned; witness k at k * out_stride bytes, out_stride a multiple
 *                   of 32 and at least 32 n, 0 = packed; n x 32 canonical bytes each), out_cs (host, K x Q x 32 bytes, or NULL) and
 *                   out_bad (host, K pairs {the number of constraint gates with aL aR != aO, the smallest such gate or -1}, or NULL).
 *                   A non-canonical element: SONIC_ERR_BAD_ENCODING; a witness with z[0] != 1: SONIC_ERR_INVALID_ARG naming the first
 *                   such k; an output pointer that is host memory or lies on another GPU, a misaligned pointer: SONIC_ERR_INVALID_ARG.
 *                   Every refusal leaves the outputs untouched.  Witnesses pass through staging in chunks, so K is not bounded by device
 *                   memory; SONIC_R1CS_STAGE=<k> (read per call) caps the witnesses per chunk, with the same results.  Blocking.
 *   r1cs_row_chunk  rows of at most this many entries are summed by one thread each, longer rows by one block each.
 *
 * Costs to know.  A circuit made here has Q = 3m + n_pub, of the order of n.  A FULL proof needs Q buffers of 3n + 1 field elements (the
 * handle makes them on the first one) and circuit digest v1 hashes 96 Q n bytes: prove such circuits with core proofs and helped
 * verification under circuit digest v2 ("Circuits with Q ~ n", below), on handles that are not prepared. */
typedef struct sonic_r1cs sonic_r1cs_t;
typedef struct sonic_r1cs_matrix { const int64_t* row_ptr; const int64_t* col; const uint8_t* val; } sonic_r1cs_matrix_t;
int sonic_r1cs_new(int64_t m, int64_t N, int64_t n_pub, const sonic_r1cs_matrix_t* A, const sonic_r1cs_matrix_t* B, const sonic_r1cs_matrix_t* C,
                   sonic_r1cs_t** out);
int sonic_r1cs_new_on(int device, int64_t m, int64_t N, int64_t n_pub, const sonic_r1cs_matrix_t* A, const sonic_r1cs_matrix_t* B,
                      const sonic_r1cs_matrix_t* C, sonic_r1cs_t** out);
void sonic_r1cs_free(sonic_r1cs_t* r);
int sonic_r1cs_device(const sonic_r1cs_t* r);
int sonic_r1cs_shape(const sonic_r1cs_t* r, int64_t out[4]);
int sonic_r1cs_circuit(const sonic_r1cs_t* r, int64_t* row_ptr, int64_t* col, uint8_t* val, uint8_t* cs_fixed);
int sonic_r1cs_assign(sonic_r1cs_t* r, int64_t K, const void* z, int kind, int on_device, int64_t z_stride, void* hip_stream, void* d_aL,
                      void* d_aR, void* d_aO, int64_t out_stride, uint8_t* out_cs, int64_t* out_bad);
int sonic_r1cs_row_chunk(void);

/* ---- Circuits with Q ~ n: weights digest v2, circuit digest v2, the prover's signature state on first use ----
 * Circuit digest v1 hashes the 96 Q n dense bytes the gate weights stand for, whichever form they come in.  With Q of the order of n that
 * is seconds of hashing per handle.  Digest v2 hashes the ENTRIES of the stacked CSR, O(nnz), as a SHA-256 tree that the GPU computes from
 * a handle's resident CSR.  The normative text (sonic_amd/csrc/fs.hpp), repeated:
 *
 *   input    the validated stacked CSR of 3Q rows ("gate weights as CSR"), AS GIVEN.  An explicit zero value is an entry: two CSRs of the
 *            same matrix that differ in explicit zeros have DIFFERENT digests (v1 does not tell them apart).  Prover and verifier must
 *            hold the same CSR, not merely the same matrix.
 *   items    entry k (0 <= k < nnz, CSR order) is two items of 32 bytes: item 2k = le64 r || le64 c || 16 zero bytes (r in [0, 3Q) the
 *            stacked row, c in [0, n) the column); item 2k + 1 = the 32 canonical little-endian bytes of val[k]
 *   leaves   L = max(1, ceil(nnz / 16));  leaf_i = SHA256(H_leaf(i) || items 32 i .. min(32 (i+1), 2 nnz) - 1); nnz = 0: one leaf over zero items
 *   nodes    as in witness digest v2: while a level has c > 1 digests the next has ceil(c / 32) nodes,
 *            node_j = SHA256(H_node(level, j) || the digests 32 j .. min(32 (j+1), c) - 1 of the level below)
 *   headers  64 bytes, those of witness digest v2 under the labels "sonic-hip/weights-leaf/v2" (zero-padded to 56 bytes, then le64 i) and
 *            "sonic-hip/weights-node/v2" (zero-padded to 48 bytes, then le64 level -- 1 for the first level of nodes -- and le64 j)
 *   root   = the single digest left (leaf_0 when L = 1)
 *   weights digest v2 = SHA256("sonic-hip/weights/v2" || le64 n || le64 Q || le64 nnz || root)
 *   circuit digest v2 = SHA256("sonic-hip/circuit/v2" || weights digest v2 || le64 Q || cs),   cs = Q x 32 canonical bytes
 *
 * A statement's digest costs 32 Q bytes of hashing from the weights digest (what midstate / resume gives v1).  The prover's Fiat-Shamir
 * and helper calls take `circuit_digest` and `weights_digest` as arguments, so they work under either kind: pass v2 bytes.  A proof or an
 * aggregate made under one kind is a REJECTED proof (not an error) on a verifier handle of the other.  The one-shot sonic_verify_core_fs[_csr]
 * and sonic_fs_core_challenges keep v1.
 *
 *   sonic_fs_weights_digest_v2_csr    host only, no device.  Validation and errors are those of sonic_fs_circuit_midstate_csr.
 *   sonic_fs_circuit_digest_v2        host only.  A cs[q] >= r: SONIC_ERR_BAD_ENCODING naming q.
 *   sonic_prover_weights_digest_v2    on the GPU, from the resident CSR of a handle made by sonic_prover_new_csr; a handle with dense weights:
 *                                     SONIC_ERR_INVALID_ARG (make the handle from CSR); a proof in flight: SONIC_ERR_INVALID_ARG.  Cached.
 *   sonic_verifier_weights_digest_v2  the same on a verifier handle, which always holds CSR (made from dense weights: their non-zero entries).
 *   sonic_verifier_new_digest         digest_kind 1: exactly sonic_verifier_new_csr.  digest_kind 2: no dense byte is hashed -- the GPU
 *                                     computes weights digest v2; the handle's circuit digest is circuit digest v2 of (it, cs), in the `_cs`
 *                                     batches proof k's is circuit digest v2 of (it, cs_k), and the helped calls bind it as the weights
 *                                     digest.  Batch digests, randomizers, transcripts and checks are unchanged: they take the 32 bytes
 *                                     they are given.  Any other kind: SONIC_ERR_INVALID_ARG.
 *   sonic_verifier_digest_kind        1 or 2 (-1 for NULL).
 *   sonic_prover_device_bytes         the device memory the handle owns now: all its buffers, lane workspaces included; not the SRS it borrows.
 *
 *   sonic_prover_host_bytes           the pinned host memory the handle owns now (the staging of transcript, pairs, MSM slots, evaluations,
 *                                     flags and digest root); same locking and errors as sonic_prover_device_bytes.
 *
 * Signature state on first use.  A prover handle is made with what a CORE proof reads: 8 MSM slots (of 12 304 bytes, on the device and in
 * pinned host memory), 8 transcript elements, 5 evaluation-point pairs and 3 evaluations, whatever Q is.  Everything else a proof with a
 * signature needs -- the other 5 Q slots on both sides, the transcript, pairs and evaluations beyond those prefixes, and the Q buffers of
 * 3n + 1 field elements for s(X, y_j) with their Q events -- is made by the first enqueue of such a proof: a full proof, a share, every pass
 * of sonic_prover_prove_fs / submit_fs, the batch calls over them.  Core proofs in every form (blocking, submit_core / collect_core,
 * Fiat-Shamir, the batch calls), sonic_prover_aggregate_core, eval_constraints, the witness calls, the digests, sonic_prover_prepare and
 * sonic_prover_hsc_prove (which work in buffers of the call) never make it.  It is made before anything of the proof is queued; when an
 * allocation fails the call returns SONIC_ERR_HIP with a message that names the sizes, whatever it had got is freed, and the handle remains
 * good for core proofs.  A core proof's enqueue and finish do no host work, allocation or copy that grows with Q beyond what its statement
 * needs (the Q constants of a call that brings its own, and the Q-long device arrays of k(y) and s(X, y)).  Proof bytes are unchanged, in
 * every order of calls.
 *
 * k(y) = sum_q cs[q] y^(n+1+q) runs in one block of 256 threads below a threshold of Q and over ceil(Q / span) blocks from it on (a second,
 * one-block launch adds their partial sums; the sums are exact, so the proof's bytes do not depend on the form).  SONIC_K_OF_Y_SPLIT=<Q>
 * sets the threshold (default 2^14, the smallest measured Q from which the split wins; 0: never split), SONIC_K_OF_Y_SPAN=<q per block> the
 * span (default 2048); both are read per call. */
int sonic_fs_weights_digest_v2_csr(int64_t n, int64_t Q, const int64_t* row_ptr, const int64_t* col, const uint8_t* val, uint8_t out[32]);
int sonic_fs_circuit_digest_v2(const uint8_t weights_digest[32], int64_t Q, const uint8_t* cs, uint8_t out[32]);
int sonic_prover_weights_digest_v2(sonic_prover_t* p, uint8_t out[32]);
int sonic_verifier_weights_digest_v2(sonic_verifier_t* v, uint8_t out[32]);
int sonic_verifier_new_digest(const sonic_srs_t* srs, int64_t n, int64_t Q, const int64_t* row_ptr, const int64_t* col, const uint8_t* val,
                              const uint8_t* cs, int digest_kind, sonic_verifier_t** out);
int sonic_verifier_digest_kind(const sonic_verifier_t* v);
int sonic_prover_device_bytes(sonic_prover_t* p, int64_t* out);
int sonic_prover_host_bytes(sonic_prover_t* p, int64_t* out);

/* ---- device memory for callers without a HIP binding ---- */
int sonic_dev_alloc(size_t bytes, void** out);                       /* on the default device */
int sonic_dev_alloc_on(int device, size_t bytes, void** out);         /* free / upload / download find the pointer's device themselves */
int sonic_dev_free(void* p);
int sonic_dev_upload(void* dst, const void* src, size_t bytes);
int sonic_dev_download(void* dst, const void* src, size_t bytes);

/* ---- per-kernel HIP-event timing (bench.py's roofline leg) ---- */
int sonic_profile_enable(int on);
int sonic_profile_reset(void);
int sonic_profile_get(const char* kernel, double* total_ms, int64_t* launches);
int sonic_profile_names(char* buf, size_t cap);     /* newline-separated kernel names seen so far */

#ifdef __cplusplus
}
#endif
#if defined(__GNUC__)
#pragma GCC visibility pop
#endif
#endif
