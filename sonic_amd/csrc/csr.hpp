// The circuit of one call, as the host sees it (CircuitView), and sparse gate weights (include/sonic_hip.h, "gate weights as CSR"): the
// three Q x n matrices stacked as ONE CSR of 3Q rows (wL rows 0..Q-1, wR rows Q..2Q-1, wO rows 2Q..3Q-1; column i = gate i + 1 of the
// reference).  The reference's circuits are lists of mostly-zero rows (Constraints.hs:34-53) that sPoly walks entry by entry; the CSR is
// that walk's input without the zeros.
//
// Host side, shared by prove.hip (the handle), prove_multi.hip (the one-shot call) and verify.hip: every entry point that takes a circuit,
// dense or `_csr`, wraps its arguments in a CircuitView and runs ONE implementation on it -- circuit_validate, circuit_runs_hint,
// circuit_digest here, s(u, v) in verify.hip, the upload in prove.hip.  Below them the layouts the device kernels read of a sparse circuit
// (poly.hip): the rows as given, the column-major transpose (counting sort, O(nnz + n)) and the chunks of at most CSR_CHUNK entries that
// s(u,Y)'s row sums are cut into.
#pragma once
#include <stdint.h>
#include <string.h>
#include <algorithm>
#include <vector>
#include "internal.hpp"
#include "fs.hpp"

namespace sonic {

// entries per chunk of a row in k_s_of_u_csr (one wave per chunk: 8 products per lane)
constexpr int CSR_CHUNK = 512;

// borrowed pointers, valid for the duration of the call
struct CircuitView {
  long n, Q;
  const uint8_t* cs;                                   // Q x 32 B (the callers check it: hscVerify has none)
  bool csr;
  const uint8_t *wL, *wR, *wO;                         // dense: Q x n x 32 B each
  const int64_t *row_ptr, *col; const uint8_t* val;    // csr: 3Q + 1, nnz, nnz x 32 B
};
inline CircuitView dense_view(long n, long Q, const uint8_t* wL, const uint8_t* wR, const uint8_t* wO, const uint8_t* cs) {
  return CircuitView{n, Q, cs, false, wL, wR, wO, nullptr, nullptr, nullptr};
}
inline CircuitView csr_view(long n, long Q, const int64_t* row_ptr, const int64_t* col, const uint8_t* val, const uint8_t* cs) {
  return CircuitView{n, Q, cs, true, nullptr, nullptr, nullptr, row_ptr, col, val};
}

inline bool circuit_args_ok(const CircuitView& c) { return c.n >= 1 && c.Q >= 1 && (c.csr ? c.row_ptr != nullptr : c.wL && c.wR && c.wO); }

// SONIC_OK, SONIC_ERR_INVALID_ARG (a missing argument, or the structure of the rows: the message names the row) or SONIC_ERR_BAD_ENCODING
// (a sparse value >= r).  Dense weights are not read here: the device flags a non-canonical one when it converts them.
inline int circuit_validate(const char* who, const CircuitView& c) {
  const long n = c.n, Q = c.Q;
  const int64_t *row_ptr = c.row_ptr, *col = c.col;
  const uint8_t* val = c.val;
  if (!circuit_args_ok(c)) {
    set_error("%s: bad argument (need n >= 1, Q >= 1, %s)", who, c.csr ? "row_ptr" : "wL, wR, wO");
    return SONIC_ERR_INVALID_ARG;
  }
  if (!c.csr) return SONIC_OK;
  if (n > INT32_MAX - 1) { set_error("%s: n = %ld does not fit the 32-bit column indices", who, n); return SONIC_ERR_INVALID_ARG; }
  const long R = 3 * Q;
  const char* mat[3] = {"wL", "wR", "wO"};
  if (row_ptr[0] != 0) { set_error("%s: row_ptr[0] = %lld, must be 0 (row 0 = %s row 0)", who, (long long)row_ptr[0], mat[0]); return SONIC_ERR_INVALID_ARG; }
  for (long r = 0; r < R; r++)
    if (row_ptr[r + 1] < row_ptr[r]) {
      set_error("%s: row_ptr decreases at row %ld (%s row %ld): %lld after %lld", who, r, mat[r / Q], r % Q, (long long)row_ptr[r + 1], (long long)row_ptr[r]);
      return SONIC_ERR_INVALID_ARG;
    }
  const int64_t nnz = row_ptr[R];
  if (nnz > INT32_MAX) { set_error("%s: %lld entries, at most 2^31 - 1", who, (long long)nnz); return SONIC_ERR_INVALID_ARG; }
  if (nnz > 0 && (!col || !val)) { set_error("%s: %lld entries and a NULL col or val", who, (long long)nnz); return SONIC_ERR_INVALID_ARG; }
  for (long r = 0; r < R; r++)
    for (int64_t k = row_ptr[r]; k < row_ptr[r + 1]; k++) {
      if (col[k] < 0 || col[k] >= n) {
        set_error("%s: row %ld (%s row %ld): column %lld outside [0, %ld)", who, r, mat[r / Q], r % Q, (long long)col[k], n);
        return SONIC_ERR_INVALID_ARG;
      }
      if (k > row_ptr[r] && col[k] <= col[k - 1]) {
        set_error("%s: row %ld (%s row %ld): columns not strictly increasing (%lld after %lld)", who, r, mat[r / Q], r % Q, (long long)col[k], (long long)col[k - 1]);
        return SONIC_ERR_INVALID_ARG;
      }
    }
  for (long r = 0; r < R; r++)
    for (int64_t k = row_ptr[r]; k < row_ptr[r + 1]; k++) {
      Fr v;
      memcpy(v.l, val + 32 * k, 32);
      if (!fp_is_canonical(v)) { set_error("%s: row %ld (%s row %ld): non-canonical field element at column %lld", who, r, mat[r / Q], r % Q, (long long)col[k]); return SONIC_ERR_BAD_ENCODING; }
    }
  return SONIC_OK;
}

// what the device reads of a validated CSR circuit, laid out on the host
struct CsrLayout {
  long n = 0, Q = 0, nnz = 0;
  std::vector<int32_t> row_ptr, col;            // 3Q + 1, nnz: the rows as given
  std::vector<int32_t> col_ptr, row;            // n + 1, nnz: column-major (the entries of gate i, rows ascending)
  std::vector<uint8_t> cval;                    // nnz x 32: the values in column-major order (canonical bytes)
  std::vector<int32_t> chunk_row, chunk_begin;  // per chunk of <= CSR_CHUNK entries of one row: its row and first entry
  std::vector<int32_t> row_chunk;               // 3Q + 1: the chunks of row r are [row_chunk[r], row_chunk[r + 1])
};

// (of a validated sparse view)
inline void csr_layout(const CircuitView& c, CsrLayout& L) {
  const int64_t *row_ptr = c.row_ptr, *col = c.col;
  const uint8_t* val = c.val;
  const long n = c.n, R = 3 * c.Q, nnz = (long)row_ptr[R];
  L.n = n; L.Q = c.Q; L.nnz = nnz;
  L.row_ptr.resize((size_t)R + 1);
  for (long r = 0; r <= R; r++) L.row_ptr[(size_t)r] = (int32_t)row_ptr[r];
  L.col.resize((size_t)nnz);
  for (long k = 0; k < nnz; k++) L.col[(size_t)k] = (int32_t)col[k];
  // counting sort by column; rows are visited in order, so every column lists its rows ascending
  L.col_ptr.assign((size_t)n + 1, 0);
  for (long k = 0; k < nnz; k++) L.col_ptr[(size_t)L.col[(size_t)k] + 1]++;
  for (long i = 0; i < n; i++) L.col_ptr[(size_t)i + 1] += L.col_ptr[(size_t)i];
  std::vector<int32_t> at(L.col_ptr.begin(), L.col_ptr.end() - 1);
  L.row.resize((size_t)nnz);
  L.cval.resize(32 * (size_t)nnz);
  for (long r = 0; r < R; r++)
    for (long k = L.row_ptr[(size_t)r]; k < L.row_ptr[(size_t)r + 1]; k++) {
      const int32_t dst = at[(size_t)L.col[(size_t)k]]++;
      L.row[(size_t)dst] = (int32_t)r;
      memcpy(&L.cval[32 * (size_t)dst], val + 32 * k, 32);
    }
  L.row_chunk.resize((size_t)R + 1);
  L.chunk_row.clear(); L.chunk_begin.clear();
  for (long r = 0; r < R; r++) {
    L.row_chunk[(size_t)r] = (int32_t)L.chunk_row.size();
    for (long k = L.row_ptr[(size_t)r]; k < L.row_ptr[(size_t)r + 1]; k += CSR_CHUNK) { L.chunk_row.push_back((int32_t)r); L.chunk_begin.push_back((int32_t)k); }
  }
  L.row_chunk[(size_t)R] = (int32_t)L.chunk_row.size();
}

// Does the circuit HAVE runs of equal coefficients (sonic_prover::circuit_has_runs)?  32 tiles of `tile` consecutive gate indices, spread
// over [0, n): a tile counts when every row of wL AND of wR repeats one value across it -- then s(X, y) has a run of equal coefficients
// there (u_i = sum_q wL[q][i] y^{n+q}, Constraints.hs:39-49) -- and the circuit "has runs" when at least a quarter of the sampled tiles
// do.  ~0.5 MB read at Q = 2, microseconds.  Sparse rows are sampled without densifying, by binary search: a row holds one value across a
// tile when its present entries agree and either cover the tile or are zero (an absent entry is a zero) -- the same tiles, the same decision.
inline bool circuit_runs_hint(const CircuitView& c, long tile) {
  const long n = c.n, Q = c.Q;
  const long ntiles = n / tile;
  if (ntiles < 1) return false;
  const long samples = ntiles < 32 ? ntiles : 32;
  static const uint8_t zero[32] = {0};
  long uniform = 0;
  for (long sidx = 0; sidx < samples; sidx++) {
    const long t = sidx * ntiles / samples, a = t * tile, b = a + tile;
    bool uni = true;
    for (long r = 0; r < 2 * Q && uni; r++) {                      // the rows of wL, then of wR
      if (!c.csr) {
        const uint8_t* row = (r < Q ? c.wL + 32 * (r * n) : c.wR + 32 * ((r - Q) * n)) + 32 * a;
        for (long i = 1; i < tile && uni; i++) uni = memcmp(row, row + 32 * i, 32) == 0;
        continue;
      }
      const int64_t* lo = std::lower_bound(c.col + c.row_ptr[r], c.col + c.row_ptr[r + 1], (int64_t)a);
      const int64_t* hi = std::lower_bound(lo, c.col + c.row_ptr[r + 1], (int64_t)b);
      const long cnt = (long)(hi - lo);
      if (cnt == 0) continue;
      const uint8_t* v0 = c.val + 32 * (size_t)(lo - c.col);
      for (long k = 1; k < cnt && uni; k++) uni = memcmp(v0, v0 + 32 * k, 32) == 0;
      if (uni && cnt < tile) uni = memcmp(v0, zero, 32) == 0;
    }
    uniform += uni ? 1 : 0;
  }
  return 4 * uniform >= samples;
}

// The statement part of the Fiat-Shamir transcript (fs.hpp): SHA-256 of (n, Q, wL, wR, wO, cs), in two halves.  circuit_midstate hashes
// the weights -- sparse rows streamed in order as the dense bytes they stand for (32 zero bytes per absent entry), so that a proof made on
// either form verifies under either; O(Q n) hashing, once per circuit -- and fs_circuit_digest_resume adds one statement's constants.
inline void circuit_midstate(const CircuitView& c, uint8_t out[FS_MIDSTATE_SIZE]) {
  Sha256 h;
  fs_circuit_begin(h, c.n, c.Q);
  if (!c.csr) fs_circuit_absorb_dense(h, c.n, c.Q, c.wL, c.wR, c.wO);
  else fs_circuit_absorb_csr(h, c.n, c.Q, c.row_ptr, c.col, c.val);
  fs_midstate_save(h, c.Q, out);
}
// (the digest hashes cs as the bytes they are: whether they are canonical is the caller's check, as it always was)
inline void circuit_digest(const CircuitView& c, uint8_t out[32]) {
  uint8_t mid[FS_MIDSTATE_SIZE];
  circuit_midstate(c, mid);
  fs_circuit_digest_resume(mid, c.cs, out, nullptr, /*check_cs=*/false);
}
// (the two exported digests: the argument checks first)
inline int circuit_digest_checked(const char* who, const CircuitView& c, uint8_t out[32]) {
  if (!c.cs || !out) { set_error("%s: bad argument", who); return SONIC_ERR_INVALID_ARG; }
  int rc = circuit_validate(who, c);
  if (!rc) circuit_digest(c, out);
  return rc;
}
inline int circuit_midstate_checked(const char* who, const CircuitView& c, uint8_t out[FS_MIDSTATE_SIZE]) {
  if (!out) { set_error("%s: bad argument", who); return SONIC_ERR_INVALID_ARG; }
  int rc = circuit_validate(who, c);
  if (!rc) circuit_midstate(c, out);
  return rc;
}

}  // namespace sonic
