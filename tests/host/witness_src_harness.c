/* witness_src_harness.c -- witness sources (include/sonic_hip.h, "Witness sources") from plain C99: nothing but the header, pointers and
 * sizes, as a `foreign import ccall` shim binds them.
 *
 * The circuit is abi_harness.c's (arithCircuitExample, examples/Main.hs:38-63 of the reference, with z = 2).  The assignment is handed
 * over twice -- as three host buffers of canonical bytes (sonic_prover_set_assignment) and as a host source of int64_t with aO derived
 * (sonic_prover_set_witness: aL = (2, 7), aR = (7, 2), aO = NULL) -- and sonic_prover_prove must give the same bytes; then once with
 * negative integers, whose proof must equal the proof of r - |v| written out as bytes; then the refusals that need no launch.
 *
 *   gcc -std=c99 -pedantic -Wall -Wextra -Werror -Iinclude tests/host/witness_src_harness.c -Lsonic_amd/csrc -lsonic_hip -o witness_src_harness
 *   LD_LIBRARY_PATH=sonic_amd/csrc ./witness_src_harness        -> "witness_src_harness: OK" (exit 0); exit 77 without a GPU
 */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "sonic_hip.h"

static void fr_small(uint8_t out[32], uint64_t v) {
  int i;
  memset(out, 0, 32);
  for (i = 0; i < 8; i++) out[i] = (uint8_t)(v >> (8 * i));
}
/* r - v for a small v >= 1, little-endian: r = 0x73eda753299d7d483339d80809a1d80553bda402fffe5bfeffffffff00000001 */
static void fr_minus(uint8_t out[32], unsigned v) {
  static const uint8_t r_be[32] = {0x73, 0xed, 0xa7, 0x53, 0x29, 0x9d, 0x7d, 0x48, 0x33, 0x39, 0xd8, 0x08, 0x09, 0xa1, 0xd8, 0x05,
                                   0x53, 0xbd, 0xa4, 0x02, 0xff, 0xfe, 0x5b, 0xfe, 0xff, 0xff, 0xff, 0xff, 0x00, 0x00, 0x00, 0x01};
  int i, borrow = (int)v;
  for (i = 0; i < 32; i++) {
    int d = (int)r_be[31 - i] - (borrow & 0xff);
    borrow >>= 8;
    if (d < 0) { d += 256; borrow += 1; }
    out[i] = (uint8_t)d;
  }
}

#define N 2
#define Q 5
#define D (25 * N)

static int fail(const char* what, int rc) {
  char msg[512];
  sonic_last_error(msg, sizeof msg);
  fprintf(stderr, "witness_src_harness: %s failed with status %d: %s\n", what, rc, msg);
  return 1;
}

int main(void) {
  uint8_t wL[Q * N * 32], wR[Q * N * 32], wO[Q * N * 32], cs[Q * 32], aL[N * 32], aR[N * 32], aO[N * 32];
  uint8_t x[32], alpha[32], tr[(8 + 2 * Q) * 32], cs2[Q * 32];
  int64_t iL[N] = {2, 7}, iR[N] = {7, 2}, gates[2];
  int64_t nL[N] = {-2, 7}, nR[N] = {7, -2};
  uint8_t *proof, *proof2;
  size_t psz = sonic_proof_size(Q);
  sonic_srs_t* srs = NULL;
  sonic_prover_t* p = NULL;
  sonic_witness_src_t src;
  int rc, i;
  char msg[512];

  rc = sonic_init(0);
  if (rc == SONIC_ERR_NO_DEVICE) {
    sonic_last_error(msg, sizeof msg);
    fprintf(stderr, "witness_src_harness: SONIC_ERR_NO_DEVICE: %s\n", msg);
    return 77;
  }
  if (rc) return fail("sonic_init", rc);

  memset(wL, 0, sizeof wL); memset(wR, 0, sizeof wR); memset(wO, 0, sizeof wO);
  fr_small(wL + 32 * (1 * N + 0), 1); fr_small(wL + 32 * (2 * N + 1), 1);
  fr_small(wR + 32 * (3 * N + 0), 1); fr_small(wR + 32 * (4 * N + 1), 1);
  fr_small(wO + 32 * (0 * N + 0), 1); fr_minus(wO + 32 * (0 * N + 1), 1);
  fr_small(cs + 0, 0); fr_small(cs + 32, 2); fr_small(cs + 64, 7); fr_small(cs + 96, 7); fr_small(cs + 128, 2);
  fr_small(aL, 2); fr_small(aL + 32, 7); fr_small(aR, 7); fr_small(aR + 32, 2); fr_small(aO, 14); fr_small(aO + 32, 14);
  fr_small(x, 0x1234567u); fr_small(alpha, 0x7654321u);
  for (i = 0; i < 8 + 2 * Q; i++) fr_small(tr + 32 * i, 1000003u * (uint64_t)(i + 1) + 17);

  proof = malloc(psz); proof2 = malloc(psz);
  if (!proof || !proof2) return 1;
  if ((rc = sonic_srs_new(D, x, alpha, &srs))) return fail("sonic_srs_new", rc);
  if ((rc = sonic_prover_new(srs, N, Q, wL, wR, wO, cs, &p))) return fail("sonic_prover_new", rc);
  if ((rc = sonic_prover_set_assignment(p, aL, aR, aO))) return fail("sonic_prover_set_assignment", rc);
  if ((rc = sonic_prover_prove(p, tr, proof))) return fail("sonic_prover_prove", rc);

  /* the same assignment as a host source of integers, aO derived on the GPU */
  memset(&src, 0, sizeof src);
  src.aL = iL; src.aR = iR; src.aO = NULL; src.kind = SONIC_WIT_I64; src.on_device = 0; src.stride = 0; src.hip_stream = NULL;
  if ((rc = sonic_prover_set_witness(p, &src))) return fail("sonic_prover_set_witness", rc);
  if ((rc = sonic_prover_prove(p, tr, proof2))) return fail("sonic_prover_prove (after set_witness)", rc);
  if (memcmp(proof, proof2, psz)) { fprintf(stderr, "witness_src_harness: set_witness(int64, aO derived) and set_assignment give other proofs\n"); return 1; }
  if ((rc = sonic_prover_eval_constraints_src(p, 1, &src, cs2, gates))) return fail("sonic_prover_eval_constraints_src", rc);
  if (memcmp(cs, cs2, sizeof cs) || gates[0] != 0 || gates[1] != -1) { fprintf(stderr, "witness_src_harness: eval_constraints_src gives other constants than the circuit's\n"); return 1; }

  /* negative integers stand for r - |v|: aL = (-2, 7), aR = (7, -2), so aO = (-14, -14) and the constants follow */
  src.aL = nL; src.aR = nR;
  if ((rc = sonic_prover_eval_constraints_src(p, 1, &src, cs2, gates))) return fail("sonic_prover_eval_constraints_src (negative)", rc);
  if ((rc = sonic_prover_set_constants(p, cs2))) return fail("sonic_prover_set_constants", rc);
  if ((rc = sonic_prover_set_witness(p, &src))) return fail("sonic_prover_set_witness (negative)", rc);
  if ((rc = sonic_prover_prove(p, tr, proof2))) return fail("sonic_prover_prove (negative)", rc);
  fr_minus(aL, 2); fr_minus(aR + 32, 2); fr_minus(aO, 14); fr_minus(aO + 32, 14);
  if ((rc = sonic_prover_set_assignment(p, aL, aR, aO))) return fail("sonic_prover_set_assignment (negative)", rc);
  if ((rc = sonic_prover_prove(p, tr, proof))) return fail("sonic_prover_prove (negative, bytes)", rc);
  if (memcmp(proof, proof2, psz)) { fprintf(stderr, "witness_src_harness: a negative int64 is not r - |v|\n"); return 1; }

  /* refusals made before any launch: an unknown kind, a host pointer passed as device memory */
  src.kind = 2;
  rc = sonic_prover_set_witness(p, &src);
  sonic_last_error(msg, sizeof msg);
  if (rc != SONIC_ERR_INVALID_ARG || !strstr(msg, "kind")) { fprintf(stderr, "witness_src_harness: an unknown kind gave %d (%s)\n", rc, msg); return 1; }
  src.kind = SONIC_WIT_I64; src.on_device = 1;
  rc = sonic_prover_set_witness(p, &src);
  sonic_last_error(msg, sizeof msg);
  if (rc != SONIC_ERR_INVALID_ARG || !strstr(msg, "host pointer")) { fprintf(stderr, "witness_src_harness: a host pointer with on_device = 1 gave %d (%s)\n", rc, msg); return 1; }
  /* and neither touched the resident assignment */
  if ((rc = sonic_prover_prove(p, tr, proof2))) return fail("sonic_prover_prove (after refusals)", rc);
  if (memcmp(proof, proof2, psz)) { fprintf(stderr, "witness_src_harness: a refused source changed the resident assignment\n"); return 1; }

  sonic_prover_free(p);
  sonic_srs_free(srs);
  free(proof); free(proof2);
  printf("witness_src_harness: OK (%lu proof bytes; int64 host source with aO derived == canonical bytes, negatives, refusals)\n", (unsigned long)psz);
  return 0;
}
