// R1CS front end, host half (include/sonic_hip.h, "R1CS front end"): the checks of three CSR matrices A, B, C, the Sonic constraint system
// they compile to under layout 1, and the layout the kernels of r1cs.hip read.  Host only -- no device code, no HIP header -- so that the
// plain program of tests/host/r1cs_host.cpp compiles the same text as the library.
//
// Layout 1.  m rows over N columns; column 0 is the constant one, columns 1..n_pub the public inputs.  n = m + g gates, g = N / 2:
//   gate i < m               aL = <A_i, z>, aR = <B_i, z>, aO = <C_i, z>      (an unsatisfied row is a broken multiplication gate i)
//   gate m + t               aL = z[2t + 1], aR = z[2t + 2] (0 when 2t + 2 == N), aO = their product
// so variable j >= 1 has the home (wL if j - 1 is even, else wR; gate m + (j - 1) / 2).  Q = 3m + n_pub linear constraints:
//   q = i, m + i, 2m + i     aL[i] (aR[i], aO[i]) - sum_{j >= 1} M_ij home(j) = M_i0       weight 1 at (wL / wR / wO, q, i), -M_ij at home(j)
//   q = 3m + k - 1           home(k) = z[k]                                              weight 1 at home(k)
// Within a stacked row every column is distinct and increasing (i < m <= every home gate; the two variables of a gate live in different
// matrices), so no entries are merged: nnz = nnz(A) + nnz(B) + nnz(C) - (entries in column 0) + 3m + n_pub.
#pragma once
#include <stdint.h>
#include <stdio.h>
#include <string.h>
#include <vector>
#include "../../include/sonic_hip.h"
#include "field.hpp"

namespace sonic {

// rows of at most R1CS_ROW_CHUNK entries are summed by one thread each, longer ones by one block each (r1cs.hip)
constexpr int R1CS_ROW_CHUNK = 32;

// borrowed pointers, valid for the duration of the call
struct R1csView {
  int64_t m, N, n_pub;
  sonic_r1cs_matrix_t M[3];      // A, B, C
};
struct R1csShape { int64_t n, Q, nnz, g; };

inline const char* r1cs_matrix_name(int k) { return k == 0 ? "A" : k == 1 ? "B" : "C"; }

// SONIC_OK, SONIC_ERR_INVALID_ARG (a missing argument, a bound, or the structure of the rows: the message names the matrix and the row) or
// SONIC_ERR_BAD_ENCODING (a value >= r).  The reason goes to msg.
inline int r1cs_validate(const R1csView& v, char* msg, size_t cap) {
  const int64_t m = v.m, N = v.N, l = v.n_pub;
  if (m < 1 || N < 1) { snprintf(msg, cap, "bad argument (need m >= 1, N >= 1)"); return SONIC_ERR_INVALID_ARG; }
  if (l < 0 || l > N - 1) { snprintf(msg, cap, "n_pub = %lld outside [0, N - 1 = %lld] (column 0 is the constant one)", (long long)l, (long long)(N - 1)); return SONIC_ERR_INVALID_ARG; }
  if (N > INT32_MAX) { snprintf(msg, cap, "N = %lld does not fit the 32-bit column indices", (long long)N); return SONIC_ERR_INVALID_ARG; }
  if (m > INT32_MAX || m + N / 2 > (int64_t)INT32_MAX - 1) { snprintf(msg, cap, "n = m + N / 2 = %lld does not fit the 32-bit column indices", (long long)(m + N / 2)); return SONIC_ERR_INVALID_ARG; }
  int64_t total = 3 * m + l;
  for (int k = 0; k < 3; k++) {
    const sonic_r1cs_matrix_t& M = v.M[k];
    const char* name = r1cs_matrix_name(k);
    if (!M.row_ptr) { snprintf(msg, cap, "bad argument (%s has no row_ptr)", name); return SONIC_ERR_INVALID_ARG; }
    if (M.row_ptr[0] != 0) { snprintf(msg, cap, "%s: row_ptr[0] = %lld, must be 0", name, (long long)M.row_ptr[0]); return SONIC_ERR_INVALID_ARG; }
    for (int64_t r = 0; r < m; r++)
      if (M.row_ptr[r + 1] < M.row_ptr[r]) {
        snprintf(msg, cap, "%s: row_ptr decreases at row %lld: %lld after %lld", name, (long long)r, (long long)M.row_ptr[r + 1], (long long)M.row_ptr[r]);
        return SONIC_ERR_INVALID_ARG;
      }
    const int64_t nnz = M.row_ptr[m];
    if (nnz > INT32_MAX) { snprintf(msg, cap, "%s: %lld entries, at most 2^31 - 1", name, (long long)nnz); return SONIC_ERR_INVALID_ARG; }
    if (nnz > 0 && (!M.col || !M.val)) { snprintf(msg, cap, "%s: %lld entries and a NULL col or val", name, (long long)nnz); return SONIC_ERR_INVALID_ARG; }
    for (int64_t r = 0; r < m; r++)
      for (int64_t e = M.row_ptr[r]; e < M.row_ptr[r + 1]; e++) {
        if (M.col[e] < 0 || M.col[e] >= N) { snprintf(msg, cap, "%s: row %lld: column %lld outside [0, %lld)", name, (long long)r, (long long)M.col[e], (long long)N); return SONIC_ERR_INVALID_ARG; }
        if (e > M.row_ptr[r] && M.col[e] <= M.col[e - 1]) {
          snprintf(msg, cap, "%s: row %lld: columns not strictly increasing (%lld after %lld)", name, (long long)r, (long long)M.col[e], (long long)M.col[e - 1]);
          return SONIC_ERR_INVALID_ARG;
        }
      }
    total += nnz;      // (an upper bound of the compiled system's entries, and at most 3m above it)
  }
  if (total > INT32_MAX) { snprintf(msg, cap, "the compiled system has about %lld entries, at most 2^31 - 1", (long long)total); return SONIC_ERR_INVALID_ARG; }
  for (int k = 0; k < 3; k++) {
    const sonic_r1cs_matrix_t& M = v.M[k];
    for (int64_t r = 0; r < m; r++)
      for (int64_t e = M.row_ptr[r]; e < M.row_ptr[r + 1]; e++) {
        Fr x;
        memcpy(x.l, M.val + 32 * e, 32);
        if (!fp_is_canonical(x)) { snprintf(msg, cap, "%s: row %lld: non-canonical field element at column %lld", r1cs_matrix_name(k), (long long)r, (long long)M.col[e]); return SONIC_ERR_BAD_ENCODING; }
      }
  }
  return SONIC_OK;
}

// (of a validated view)
inline R1csShape r1cs_shape(const R1csView& v) {
  R1csShape s;
  s.g = v.N / 2;
  s.n = v.m + s.g;
  s.Q = 3 * v.m + v.n_pub;
  s.nnz = 3 * v.m + v.n_pub;
  for (int k = 0; k < 3; k++)
    for (int64_t r = 0; r < v.m; r++) {
      const int64_t a = v.M[k].row_ptr[r], b = v.M[k].row_ptr[r + 1];
      s.nnz += b - a - (b > a && v.M[k].col[a] == 0 ? 1 : 0);
    }
  return s;
}

inline bool r1cs_home_is_left(int64_t j) { return ((j - 1) & 1) == 0; }
inline int64_t r1cs_home_gate(int64_t m, int64_t j) { return m + (j - 1) / 2; }

// The Sonic CSR of a validated view: row_ptr[3Q + 1], col[nnz], val[32 nnz] as sonic_prover_new_csr takes them, and cs_fixed[32 Q] with
// the public slots zero.
inline void r1cs_compile(const R1csView& v, int64_t* row_ptr, int64_t* col, uint8_t* val, uint8_t* cs_fixed) {
  const int64_t m = v.m, l = v.n_pub, Q = 3 * m + l;
  uint8_t one[32] = {1};
  int64_t at = 0;
  memset(cs_fixed, 0, 32 * (size_t)Q);
  for (int w = 0; w < 3; w++)           // wL rows, wR rows, wO rows
    for (int64_t q = 0; q < Q; q++) {
      row_ptr[w * Q + q] = at;
      if (q >= 3 * m) {                 // home(k) = z[k]
        const int64_t k = q - 3 * m + 1;
        if (w == (r1cs_home_is_left(k) ? 0 : 1)) { col[at] = r1cs_home_gate(m, k); memcpy(val + 32 * at, one, 32); at++; }
        continue;
      }
      const int mat = (int)(q / m);
      const int64_t i = q % m;
      const sonic_r1cs_matrix_t& M = v.M[mat];
      if (w == mat) { col[at] = i; memcpy(val + 32 * at, one, 32); at++; }
      for (int64_t e = M.row_ptr[i]; e < M.row_ptr[i + 1]; e++) {
        const int64_t j = M.col[e];
        if (j == 0) { if (w == 0) memcpy(cs_fixed + 32 * q, M.val + 32 * e, 32); continue; }
        if (w != (r1cs_home_is_left(j) ? 0 : 1)) continue;
        Fr x;
        memcpy(x.l, M.val + 32 * e, 32);
        x = fp_neg(x);                  // an explicit zero stays an entry, of value 0
        col[at] = r1cs_home_gate(m, j);
        memcpy(val + 32 * at, x.l, 32);
        at++;
      }
    }
  row_ptr[3 * Q] = at;
}

// What the kernels read of A, B, C: the three matrices stacked as 3m rows (A rows, B rows, C rows) with 32-bit indices, and the rows split
// into two classes by length -- at most R1CS_ROW_CHUNK entries (one thread per row) and more (one block per row).
struct R1csDeviceLayout {
  std::vector<int32_t> row_ptr, col;          // 3m + 1, nnz(A) + nnz(B) + nnz(C)
  std::vector<uint8_t> val;                   // 32 bytes per entry, canonical
  std::vector<int32_t> short_rows, long_rows; // stacked row indices, ascending
};
inline void r1cs_device_layout(const R1csView& v, R1csDeviceLayout& L) {
  const int64_t m = v.m;
  int64_t total = 0;
  for (int k = 0; k < 3; k++) total += v.M[k].row_ptr[m];
  L.row_ptr.resize(3 * (size_t)m + 1);
  L.col.resize((size_t)total);
  L.val.resize(32 * (size_t)total);
  L.short_rows.clear(); L.long_rows.clear();
  int64_t at = 0;
  for (int k = 0; k < 3; k++) {
    const sonic_r1cs_matrix_t& M = v.M[k];
    for (int64_t r = 0; r < m; r++) {
      const int64_t a = M.row_ptr[r], b = M.row_ptr[r + 1];
      L.row_ptr[(size_t)(k * m + r)] = (int32_t)at;
      for (int64_t e = a; e < b; e++) L.col[(size_t)(at + e - a)] = (int32_t)M.col[e];
      if (b > a) memcpy(&L.val[32 * (size_t)at], M.val + 32 * a, 32 * (size_t)(b - a));
      (b - a <= R1CS_ROW_CHUNK ? L.short_rows : L.long_rows).push_back((int32_t)(k * m + r));
      at += b - a;
    }
  }
  L.row_ptr[3 * (size_t)m] = (int32_t)at;
}

}  // namespace sonic
