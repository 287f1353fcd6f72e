// Which exponents an SRS handle holds and where (host only, no HIP, like srs_policy.hpp; tests/host/srs_view_host.cpp).  A whole string
// holds the one window [-d, d]; a circuit-sized VIEW of it (sonic_srs_for_circuit) holds only the exponents a proof over (n, Q) touches:
//   low  [t_lo(n), max(3n, n + Q)]   T, the S_j, C with its Q-term tail, every opening (both bases)
//   high [d - 3n - 4, d]             R, committed with max = n and so shifted by d - n (alpha basis only)
// merged into one window where they touch.  Consecutive exponents of a window sit in consecutive slots, the high window right behind the
// low one, so every table of a handle is npts points long and every address is basis + slot(e).  For a whole string slot(e) = e + d, the
// stride is 2d + 1 and the symmetric sums have d + 1 slots: what the code computed before views existed.
// Also here: the window width of a view, the byte ranges of a view's points in both on-disk containers, and the reader of those ranges.
#pragma once
#include <stdint.h>
#include <stdio.h>
#include <string.h>
#include <string>
#include <vector>
#include "proof_layout.hpp"
#include "srs_policy.hpp"
#include "srs_file.hpp"

namespace sonic {

struct SrsGeometry {
  int64_t d = 0;
  int64_t lo0 = 0, hi0 = -1, lo1 = 1, hi1 = 0;      // one window: lo1 = 1, hi1 = 0
  bool two() const { return hi1 >= lo1; }
  bool full() const { return !two() && lo0 == -d && hi0 == d; }
  int64_t len0() const { return hi0 - lo0 + 1; }
  int64_t len1() const { return two() ? hi1 - lo1 + 1 : 0; }
  int64_t npts() const { return len0() + len1(); }                 // points per table = the stride between window tables
  int64_t centre() const { return -lo0; }                         // the slot of exponent 0 (every handle holds it: lo0 <= 0 <= hi0)
  // the symmetric sums A[e] + A[-e] need both: one table holds exponents 0 .. sym_n - 1
  int64_t sym_n() const { return (hi0 < -lo0 ? hi0 : -lo0) + 1; }
  bool holds(int64_t e) const { return (e >= lo0 && e <= hi0) || (e >= lo1 && e <= hi1); }
  // exponents [e0, e0 + count) inside ONE window (an MSM job never straddles two: the slots would be consecutive, the exponents not)
  bool contains(int64_t e0, int64_t count) const {
    if (count <= 0) return true;
    const int64_t e1 = e0 + count - 1;
    return (e0 >= lo0 && e1 <= hi0) || (two() && e0 >= lo1 && e1 <= hi1);
  }
  // the slot of a held exponent (anything else: slot 0, never an address outside the table)
  int64_t slot(int64_t e) const { return e >= lo0 && e <= hi0 ? e - lo0 : (two() && e >= lo1 && e <= hi1 ? len0() + (e - lo1) : 0); }
};

inline SrsGeometry srs_full_geometry(int64_t d) {
  SrsGeometry g;
  g.d = d; g.lo0 = -d; g.hi0 = d;
  return g;
}

// what a circuit of (n, Q) needs of d: the prover's own rule (Protocol.hs:54-55) and room for t's blinded low end.  0: fine, else the bound missed
inline int64_t srs_view_d_needed(int64_t d, int64_t n) {
  if (d < 7 * n) return 7 * n;
  if (d < -ProofLayout::t_lo(n)) return -ProofLayout::t_lo(n);
  return 0;
}

// (n >= 1, Q >= 1, srs_view_d_needed(d, n) == 0)
inline SrsGeometry srs_view_geometry(int64_t d, int64_t n, int64_t Q) {
  const ProofLayout L{Q};
  SrsGeometry g;
  g.d = d;
  g.lo0 = ProofLayout::t_lo(n);
  const int64_t t_hi = ProofLayout::t_lo(n) + ProofLayout::t_len(n) - 1, u_hi = ProofLayout::u_lo(n) + L.u_len(n) - 1;
  g.hi0 = t_hi > u_hi ? t_hi : u_hi;
  if (g.hi0 > d) g.hi0 = d;                       // (a C tail past d has no SRS element under any handle)
  const int64_t shift = d - n;                    // R: commitPoly with max = n
  g.lo1 = ProofLayout::r_lo(n) + shift;
  g.hi1 = ProofLayout::r_lo(n) + ProofLayout::r_len(n) - 1 + shift;
  if (g.lo1 <= g.hi0 + 1) { g.hi0 = g.hi1; g.lo1 = 1; g.hi1 = 0; }
  return g;
}

// the window width of a view for n: what the rule gives a string of d = 8n -- every width in the rule was measured at n = d / 8 -- with
// the memory questions asked with the view's own point count
inline SrsWindows srs_view_window_policy(int64_t n, int64_t npts, size_t free_bytes, const SrsKnobs& k) {
  return srs_window_policy(8 * n, (size_t)npts, free_bytes, k);
}

// the G2 elements a view holds -- exactly what the verifiers fetch (verify_host.hpp, fetch_g2; sonic_srs_pairing): basis 0 at n - d and 0,
// basis 1 at 0 and 1
struct SrsViewG2 { int64_t e[2][2]; };
inline SrsViewG2 srs_view_g2(int64_t d, int64_t n) { return SrsViewG2{{{n - d, 0}, {0, 1}}}; }

// ---- a view's points in a file ------------------------------------------------------------------------------------------------------
// Both containers are a 24-byte header and four vectors of 2d + 1 fixed-size points, exponent e at index e + d.
struct SrsFileHead { bool compressed = false; uint32_t version = 0, flags = 0; int64_t d = 0; bool has_g2() const { return (flags & 1u) != 0; } };
constexpr uint64_t SRS_FILE_HEADER_BYTES = 24;
inline uint64_t srs_file_g1_point_bytes(const SrsFileHead& h) { return h.compressed ? 48 : 96; }
inline uint64_t srs_file_g2_point_bytes(const SrsFileHead& h) { return h.compressed ? 96 : 192; }
inline uint64_t srs_file_bytes(const SrsFileHead& h) {
  const uint64_t n = 2ull * (uint64_t)h.d + 1ull;
  return SRS_FILE_HEADER_BYTES + 2ull * n * srs_file_g1_point_bytes(h) + (h.has_g2() ? 2ull * n * srs_file_g2_point_bytes(h) : 0ull);
}
// the offset of exponent e of vector v (0, 1: the G1 bases; 2, 3: the G2 bases)
inline uint64_t srs_file_offset(const SrsFileHead& h, int v, int64_t e) {
  const uint64_t n = 2ull * (uint64_t)h.d + 1ull, i = (uint64_t)(e + h.d);
  if (v < 2) return SRS_FILE_HEADER_BYTES + ((uint64_t)v * n + i) * srs_file_g1_point_bytes(h);
  return SRS_FILE_HEADER_BYTES + 2ull * n * srs_file_g1_point_bytes(h) + ((uint64_t)(v - 2) * n + i) * srs_file_g2_point_bytes(h);
}
struct SrsFileRange { uint64_t offset, bytes; int vector; int64_t e0, count; };
// every range a view reads, in file order: the windows of both G1 bases, then the four G2 points where the file has them
inline std::vector<SrsFileRange> srs_view_file_ranges(const SrsFileHead& h, const SrsGeometry& g, int64_t n) {
  std::vector<SrsFileRange> r;
  for (int b = 0; b < 2; b++) {
    r.push_back(SrsFileRange{srs_file_offset(h, b, g.lo0), (uint64_t)g.len0() * srs_file_g1_point_bytes(h), b, g.lo0, g.len0()});
    if (g.two()) r.push_back(SrsFileRange{srs_file_offset(h, b, g.lo1), (uint64_t)g.len1() * srs_file_g1_point_bytes(h), b, g.lo1, g.len1()});
  }
  if (h.has_g2()) {
    const SrsViewG2 q = srs_view_g2(h.d, n);
    for (int b = 0; b < 2; b++)
      for (int i = 0; i < 2; i++) r.push_back(SrsFileRange{srs_file_offset(h, 2 + b, q.e[b][i]), srs_file_g2_point_bytes(h), 2 + b, q.e[b][i], 1});
  }
  return r;
}

// Opens either container and checks its header against the file's real size, before any seek into the body or allocation (as
// srs_file_read does for a whole file).  0 on success with the stream left open in *fp; otherwise srs_file_read's codes and a message.
inline int srs_file_open_head(const char* path, FILE** fp, SrsFileHead& out, std::string& err) {
  FILE* f = fopen(path, "rb");
  if (!f) { err = std::string("cannot open ") + path; return 1; }
  char magic[8];
  SrsFileHead h;
  bool head = fread(magic, 1, 8, f) == 8 && fread(&h.version, 4, 1, f) == 1 && fread(&h.flags, 4, 1, f) == 1 && fread(&h.d, 8, 1, f) == 1;
  if (head && memcmp(magic, SRS_ZFILE_MAGIC, 8) == 0) { h.compressed = true; head = h.version == 1; }
  else if (head && memcmp(magic, SRS_FILE_MAGIC, 8) == 0) head = (h.version == 1 || h.version == 2) && !(h.version == 1 && h.flags);
  else head = false;
  head = head && h.d >= 1 && h.d < SRS_FILE_MAX_D && (h.flags & ~1u) == 0;
  if (!head) { fclose(f); err = std::string(path) + " is not an SRS file (SONICSRS version 1/2, SONICSRZ version 1)"; return 2; }
  if (fseek(f, 0, SEEK_END) != 0) { fclose(f); err = "cannot seek"; return 3; }
  const long long actual = ftell(f);
  if (actual < 0 || (unsigned long long)actual != srs_file_bytes(h)) { fclose(f); err = std::string(path) + " is truncated or has trailing bytes"; return 3; }
  out = h; *fp = f;
  return 0;
}

// what a view reads of a file: its geometry, npts points per G1 basis in slot order and the four G2 points (basis-major), in the file's encoding
struct SrsViewFile {
  SrsFileHead head;
  SrsGeometry geo;
  std::vector<uint8_t> g[2], g2;
};
// 0 on success; 1 cannot open, 2 not an SRS file, 3 sizes disagree or a read failed, 4 the string is too short for the circuit
inline int srs_view_file_read(const char* path, int64_t n, int64_t Q, SrsViewFile& out, std::string& err) {
  FILE* f = nullptr;
  SrsViewFile v;
  const int rc = srs_file_open_head(path, &f, v.head, err);
  if (rc) return rc;
  struct Closer { FILE* f; ~Closer() { fclose(f); } } closer{f};
  const int64_t need = srs_view_d_needed(v.head.d, n);
  if (need) { err = std::string(path) + ": d = " + std::to_string(v.head.d) + " is below the " + std::to_string(need) + " a circuit of n = " + std::to_string(n) + " needs"; return 4; }
  v.geo = srs_view_geometry(v.head.d, n, Q);
  const uint64_t total = srs_file_bytes(v.head);
  for (int b = 0; b < 2; b++) v.g[b].resize((size_t)((uint64_t)v.geo.npts() * srs_file_g1_point_bytes(v.head)));
  if (v.head.has_g2()) v.g2.resize((size_t)(4 * srs_file_g2_point_bytes(v.head)));
  size_t at[2] = {0, 0}, at2 = 0;
  for (const SrsFileRange& r : srs_view_file_ranges(v.head, v.geo, n)) {
    if (r.offset < SRS_FILE_HEADER_BYTES || r.offset + r.bytes > total) { err = "range outside the file"; return 3; }
    uint8_t* dst = r.vector < 2 ? v.g[r.vector].data() + at[r.vector] : v.g2.data() + at2;
    if (fseek(f, (long)r.offset, SEEK_SET) != 0 || fread(dst, 1, (size_t)r.bytes, f) != (size_t)r.bytes) { err = std::string(path) + ": read failed"; return 3; }
    if (r.vector < 2) at[r.vector] += (size_t)r.bytes; else at2 += (size_t)r.bytes;
  }
  out = std::move(v);
  return 0;
}

}  // namespace sonic
