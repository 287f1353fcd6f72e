// Prover-specific polynomial builders (poly.hip); see internal.hpp for the generic ones.
#pragma once
#include "common.hpp"
#include "field.hpp"
#include "g1.hpp"
#include "k_of_y_plan.hpp"

namespace sonic {

void build_r1_enqueue(hipStream_t st, const Fr* aL, const Fr* aR, const Fr* aO, const Fr* cns, long n, Fr* r1);
void s_of_y_enqueue(hipStream_t st, const Fr* wL, const Fr* wR, const Fr* wO, const Fr* ypow, long n, long Q, Fr* s);
void weight_row_poly_enqueue(hipStream_t st, const Fr* wL, const Fr* wR, const Fr* wO, long n, long q, Fr* s);
void s_diag_part_enqueue(hipStream_t st, const Fr* ypow, long n, long Q, Fr* diag, Fr* yq);
void s_of_u_enqueue(hipStream_t st, const Fr* wL, const Fr* wR, const Fr* wO, const Fr* upow, long n, long Q, Fr* s, DevBuf& tmp);
// from sparse gate weights (csr.hpp): s(X,y) over the column-major copy, s(u,Y) over the rows cut into chunks (partial: one Fr per chunk),
// and the (point, scalar) terms of one constraint-row polynomial P_q; seg = {first entry, count} of rows q, Q + q, 2Q + q
void s_of_y_csc_enqueue(hipStream_t st, const int32_t* col_ptr, const int32_t* row, const Fr* val, const Fr* ypow, long n, long Q, Fr* s);
void s_of_u_csr_enqueue(hipStream_t st, const int32_t* row_ptr, const int32_t* col, const Fr* val, const int32_t* chunk_row, const int32_t* chunk_begin,
                        long nchunks, const int32_t* row_chunk, const Fr* upow, long n, long Q, Fr* s, Fr* partial);
void csr_row_terms_enqueue(hipStream_t st, const int32_t* col, const Fr* val, const int32_t seg[6], long n, PointArray A, G1Affine* pts, Fr* scal);
void add_into_enqueue(hipStream_t st, Fr* dst, const Fr* src, long n);
void t_operands_enqueue(hipStream_t st, const Fr* r1, long r_len, long r_lo, const Fr* sy, long s_off, long s_len, const Fr* ypair, Fr* fa, Fr* fb, long M);
// *slot -= k(y) = sum_q cs[q] ypow_nq[q], in one block (plan.blocks == 0) or over plan.blocks spans (k_of_y_plan.hpp; partial: one Fr per
// block, the handle's).  k_of_y_choose: the form for Q constraints under the threshold and the knobs SONIC_K_OF_Y_SPLIT / SONIC_K_OF_Y_SPAN.
// K_OF_Y_SPLIT_DEFAULT: the threshold when the knob is unset -- the smallest measured Q from which the split form wins by more than the
// spread (us per proof's k(y), HIP events, one block / split at span 2048: Q = 2^10 9.9 / 17.2, 2^12 22.3 / 21.7 (spreads 5.0 / 3.8),
// 2^14 69.1 / 23.3, 98 306 401 / 23.4, 786 434 3182 / 29.2; profiles/r23_core_scale.txt, part 3)
constexpr long K_OF_Y_SPLIT_DEFAULT = 1L << 14;
KOfYPlan k_of_y_choose(long Q);
void sub_k_of_y_enqueue(hipStream_t st, Fr* slot, const Fr* cs, const Fr* ypow_nq, long Q, int* flags, int flag_bit, const KOfYPlan& plan, Fr* partial);
void flag_nonzero_enqueue(hipStream_t st, const Fr* a, long n, int* flags, int bit);
// runs of equal coefficients (poly.hip): tiles of RUN_TILE coefficients that hold one non-zero value are zeroed in `masked` and recorded;
// run_terms turns the records into 2 * (len / RUN_TILE) (scalar, running-sum point) slots
constexpr int RUN_TILE = 256;
void run_tiles_enqueue(hipStream_t st, const Fr* poly, long len, Fr* masked, Fr* val, uint32_t* uniform);
void run_terms_enqueue(hipStream_t st, const Fr* val, const uint32_t* uniform, long ntiles, PointArray ps, long ps_first, Fr* scal, G1Affine* pts);
void fr_with_inverse_enqueue(hipStream_t st, const Fr* in, int k, Fr* out);
void fr_mul_scalar_enqueue(hipStream_t st, const Fr* a, const Fr* b, Fr* out);
void scale_terms_enqueue(hipStream_t st, const int64_t* e, const Fr* c, long nt, const Fr* pair, Fr* out);
void sparse_to_dense_enqueue(hipStream_t st, const int64_t* exps, const Fr* coeffs, long nt, long lo, Fr* dense);

// Several openings of polynomials over ONE exponent range [lo, lo + len), lo <= 0 <= lo + len - 1, as one launch per step: fz_k = f_k(z_k)
// and q_k = the quotient (f_k(X) - f_k(z_k)) / (X - z_k) over [lo, lo + len - 2], by two Horner sweeps per side of X^0 (poly.hip, "Horner
// sweeps") -- what poly_scale_powers / poly_prefix_sum / poly_quotient do for one opening in six launches and seven array passes, for up to
// OPEN_BATCH_MAX openings in three launches and three passes.  The openings of a group (r(X,1) at z and yz; s(X,y_j) at z_j and u;
// s(u,Y) at y_1 .. y_Q and v) share their polynomial.
constexpr int OPEN_BATCH_MAX = 16;
constexpr int SWEEP_BLOCK = 256;    // threads of a sweep workgroup: a tile is SWEEP_BLOCK chunks of open_sweep_chunk(len) coefficients
// Coefficients per thread (a chunk).  16 for arrays long enough to fill the chip with such threads; a short array keeps ~64 workgroups
// (see scale_per in poly.hip: n = 2^14 would otherwise run on 12 of them), never below 2
constexpr int SWEEP_CHUNK_MAX = 16;
inline int open_sweep_chunk(long len) {
  const long L = len / ((long)SWEEP_BLOCK * 64);
  return (int)(L > SWEEP_CHUNK_MAX ? SWEEP_CHUNK_MAX : (L < 2 ? 2 : L));
}
// Entries of OpenBatch::tiles: for at most len / tile + 2 tiles over the two sides of X^0 (tile = SWEEP_BLOCK * chunk coefficients), the
// carry into each of a tile's SWEEP_BLOCK chunks and one tile value; then, per side, the SWEEP_BLOCK powers (z^+-chunk)^t and z^+-tile
// (chunk: 0 = open_sweep_chunk(len), what prove() runs; 2 .. SWEEP_CHUNK_MAX: that chunk at any length, for tests of the tile edges)
inline long open_sweep_entries(long len, int chunk = 0) {
  const long tile = (long)SWEEP_BLOCK * (chunk ? chunk : open_sweep_chunk(len));
  return (len / tile + 2) * (SWEEP_BLOCK + 1) + 2 * (SWEEP_BLOCK + 1);
}
struct OpenBatch {
  int k;
  const Fr* poly[OPEN_BATCH_MAX];   // len entries each; equal pointers are fine
  Fr* q[OPEN_BATCH_MAX];            // len + 1 entries each (unused when quotient = false)
  Fr* tiles[OPEN_BATCH_MAX];        // open_sweep_entries(len, chunk) entries each: chunk carries, tile values, power tables
  const Fr* zpair[OPEN_BATCH_MAX];  // {z, z^-1}, z != 0
  Fr* fz[OPEN_BATCH_MAX];           // where f(z) goes (never null)
};
void open_batch_enqueue(hipStream_t st, const OpenBatch& b, long lo, long len, bool quotient = true, int chunk = 0);      // quotient = false: only the evaluations fz_k

}  // namespace sonic
