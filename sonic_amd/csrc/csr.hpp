// Sparse gate weights (include/sonic_hip.h, "gate weights as CSR"): the three Q x n matrices stacked as ONE CSR of 3Q rows (wL rows
// 0..Q-1, wR rows Q..2Q-1, wO rows 2Q..3Q-1; column i = gate i + 1 of the reference).  The reference's circuits are lists of mostly-zero
// rows (Constraints.hs:34-53) that sPoly walks entry by entry; this is that walk's input without the zeros.
//
// Host side, shared by prove.hip (the handle), prove_multi.hip (the one-shot call) and verify.hip: the ONE validator every `_csr` entry
// point runs, and the layouts the device kernels read (poly.hip): the rows as given, the column-major transpose (counting sort, O(nnz + n))
// and the chunks of at most CSR_CHUNK entries that s(u,Y)'s row sums are cut into.
#pragma once
#include <stdint.h>
#include <string.h>
#include <algorithm>
#include <vector>
#include "internal.hpp"

namespace sonic {

// entries per chunk of a row in k_s_of_u_csr (one wave per chunk: 8 products per lane)
constexpr int CSR_CHUNK = 512;

// SONIC_OK, SONIC_ERR_INVALID_ARG (structure: the message names the row) or SONIC_ERR_BAD_ENCODING (a value >= r)
inline int csr_validate(const char* who, long n, long Q, const int64_t* row_ptr, const int64_t* col, const uint8_t* val) {
  if (n < 1 || Q < 1 || !row_ptr) { set_error("%s: bad argument (need n >= 1, Q >= 1, row_ptr)", who); return SONIC_ERR_INVALID_ARG; }
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
  const uint8_t* val = nullptr;                 // the caller's values in row order (canonical bytes; valid during the call)
  const uint8_t* cs = nullptr;
};

inline void csr_layout(long n, long Q, const int64_t* row_ptr, const int64_t* col, const uint8_t* val, const uint8_t* cs, CsrLayout& L) {
  const long R = 3 * Q, nnz = (long)row_ptr[R];
  L.n = n; L.Q = Q; L.nnz = nnz; L.val = val; L.cs = cs;
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

// circuit_runs_hint (prove.hip) on the sparse rows, without densifying: a sampled tile of RUN_TILE gates counts when every row of wL and
// of wR holds ONE value across it -- its present entries agree and either cover the tile or are zero (an absent entry is a zero).  The
// same tiles and the same decision as the dense hint.
inline bool circuit_runs_hint_csr(const CsrLayout& L, long tile) {
  const long n = L.n, Q = L.Q;
  const long ntiles = n / tile;
  if (ntiles < 1) return false;
  const long samples = ntiles < 32 ? ntiles : 32;
  static const uint8_t zero[32] = {0};
  long uniform = 0;
  for (long sidx = 0; sidx < samples; sidx++) {
    const long t = sidx * ntiles / samples, a = t * tile, b = a + tile;
    bool uni = true;
    for (long r = 0; r < 2 * Q && uni; r++) {
      const int32_t* c0 = L.col.data() + L.row_ptr[(size_t)r];
      const int32_t* c1 = L.col.data() + L.row_ptr[(size_t)r + 1];
      const int32_t* lo = std::lower_bound(c0, c1, (int32_t)a);
      const int32_t* hi = std::lower_bound(lo, c1, (int32_t)b);
      const long cnt = (long)(hi - lo);
      if (cnt == 0) continue;
      const uint8_t* v0 = L.val + 32 * (size_t)(lo - L.col.data());
      for (long k = 1; k < cnt && uni; k++) uni = memcmp(v0, v0 + 32 * k, 32) == 0;
      if (uni && cnt < tile) uni = memcmp(v0, zero, 32) == 0;
    }
    uniform += uni ? 1 : 0;
  }
  return 4 * uniform >= samples;
}

}  // namespace sonic
