/* core_proof_harness.c -- core proofs (include/sonic_hip.h, "Core proofs") from plain C99: nothing but the header, pointers and sizes, as
 * a `foreign import ccall` shim binds them.
 *
 * The circuit is abi_harness.c's (arithCircuitExample, examples/Main.hs:38-63 of the reference, with z = 2).  sonic_prover_prove_core must
 * give the first SONIC_CORE_PROOF_SIZE bytes of sonic_prover_prove for a transcript that starts with the same six elements, before and
 * after a full proof on the handle and through submit_core / collect_core; sonic_verify_core must accept it, reject it with s + 1 and with
 * another y, and report y = 0 as SONIC_ERR_INEXACT_DIVISION; the compressed form must round-trip; the Fiat-Shamir form must verify and its
 * challenges be the ones sonic_fs_core_challenges recomputes; and the flights must refuse each other's collects and survive that.
 *
 *   gcc -std=c99 -pedantic -Wall -Wextra -Werror -Iinclude tests/host/core_proof_harness.c -Lsonic_amd/csrc -lsonic_hip -o core_proof_harness
 *   LD_LIBRARY_PATH=sonic_amd/csrc ./core_proof_harness        -> "core_proof_harness: OK" (exit 0); exit 77 without a GPU
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
#define CORE SONIC_CORE_PROOF_SIZE

static int fail(const char* what, int rc) {
  char msg[512];
  sonic_last_error(msg, sizeof msg);
  fprintf(stderr, "core_proof_harness: %s failed with status %d: %s\n", what, rc, msg);
  return 1;
}
static int wrong(const char* what) {
  fprintf(stderr, "core_proof_harness: %s\n", what);
  return 1;
}

int main(void) {
  uint8_t wL[Q * N * 32], wR[Q * N * 32], wO[Q * N * 32], cs[Q * 32], aL[N * 32], aR[N * 32], aO[N * 32];
  uint8_t x[32], alpha[32], tr[(8 + 2 * Q) * 32], tr2[(8 + 2 * Q) * 32], digest[32], srs_id[32], seed[32];
  uint8_t core[CORE], core2[CORE], bad[CORE], z[SONIC_CORE_PROOF_SIZE_COMPRESSED], yz[64], yz2[64];
  uint8_t* proof;
  size_t psz = sonic_proof_size(Q);
  sonic_srs_t* srs = NULL;
  sonic_prover_t* p = NULL;
  int rc, i, ok = 0;
  char msg[512];

  rc = sonic_init(0);
  if (rc == SONIC_ERR_NO_DEVICE) {
    sonic_last_error(msg, sizeof msg);
    fprintf(stderr, "core_proof_harness: SONIC_ERR_NO_DEVICE: %s\n", msg);
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
  /* the same six elements, every later one different */
  memcpy(tr2, tr, sizeof tr);
  for (i = 6; i < 8 + 2 * Q; i++) fr_small(tr2 + 32 * i, 999983u * (uint64_t)(i + 1) + 5);
  memset(seed, 0x5a, sizeof seed);

  proof = malloc(psz);
  if (!proof) return 1;
  if ((rc = sonic_srs_new(D, x, alpha, &srs))) return fail("sonic_srs_new", rc);
  if ((rc = sonic_prover_new(srs, N, Q, wL, wR, wO, cs, &p))) return fail("sonic_prover_new", rc);
  if ((rc = sonic_prover_set_assignment(p, aL, aR, aO))) return fail("sonic_prover_set_assignment", rc);

  /* prove_core first on the handle, then a full proof, then again: the head each time */
  if ((rc = sonic_prover_prove_core(p, tr, core))) return fail("sonic_prover_prove_core", rc);
  if ((rc = sonic_prover_prove(p, tr2, proof))) return fail("sonic_prover_prove", rc);
  if (memcmp(core, proof, CORE)) return wrong("prove_core is not the head of sonic_prover_prove");
  if ((rc = sonic_prover_prove_core(p, tr, core2))) return fail("sonic_prover_prove_core (after a full proof)", rc);
  if (memcmp(core, core2, CORE)) return wrong("prove_core differs after a full proof on the handle");
  if ((rc = sonic_prover_prepare(p))) return fail("sonic_prover_prepare", rc);
  if ((rc = sonic_prover_prove_core(p, tr, core2))) return fail("sonic_prover_prove_core (prepared)", rc);
  if (memcmp(core, core2, CORE)) return wrong("prove_core differs on a prepared handle");

  /* flights: each collect refuses the other's flight and leaves it */
  if ((rc = sonic_prover_collect_core(p, core2)) != SONIC_ERR_INVALID_ARG) return wrong("collect_core with nothing in flight is not INVALID_ARG");
  if ((rc = sonic_prover_submit_core(p, tr))) return fail("sonic_prover_submit_core", rc);
  if ((rc = sonic_prover_collect(p, proof)) != SONIC_ERR_INVALID_ARG) return wrong("sonic_prover_collect on a core flight is not INVALID_ARG");
  if ((rc = sonic_prover_prove_core(p, tr, core2)) != SONIC_ERR_INVALID_ARG) return wrong("prove_core with a proof in flight is not INVALID_ARG");
  memset(core2, 0, CORE);
  if ((rc = sonic_prover_collect_core(p, core2))) return fail("sonic_prover_collect_core", rc);
  if (memcmp(core, core2, CORE)) return wrong("submit_core / collect_core differ from prove_core");
  if ((rc = sonic_prover_submit(p, tr2))) return fail("sonic_prover_submit", rc);
  if ((rc = sonic_prover_collect_core(p, core2)) != SONIC_ERR_INVALID_ARG) return wrong("collect_core on a transcript flight is not INVALID_ARG");
  if ((rc = sonic_prover_collect(p, proof))) return fail("sonic_prover_collect (after the refused collect_core)", rc);
  if (memcmp(core, proof, CORE)) return wrong("the transcript flight did not survive the refused collect_core");

  /* the verifier: accepts; rejects s + 1 and another y; y = 0 is a status */
  if ((rc = sonic_verify_core(srs, N, Q, wL, wR, wO, cs, core, tr + 32 * 4, tr + 32 * 5, &ok))) return fail("sonic_verify_core", rc);
  if (!ok) return wrong("sonic_verify_core rejects an honest core proof");
  memcpy(bad, core, CORE);
  bad[CORE - 32] ^= 1;                                  /* s with its lowest bit flipped: still canonical */
  if ((rc = sonic_verify_core(srs, N, Q, wL, wR, wO, cs, bad, tr + 32 * 4, tr + 32 * 5, &ok))) return fail("sonic_verify_core (s changed)", rc);
  if (ok) return wrong("sonic_verify_core accepts a proof whose s is not s(z, y)");
  if ((rc = sonic_verify_core(srs, N, Q, wL, wR, wO, cs, core, tr + 32 * 5, tr + 32 * 5, &ok))) return fail("sonic_verify_core (another y)", rc);
  if (ok) return wrong("sonic_verify_core accepts a proof at another y");
  memset(yz, 0, 32);
  if ((rc = sonic_verify_core(srs, N, Q, wL, wR, wO, cs, core, yz, tr + 32 * 5, &ok)) != SONIC_ERR_INEXACT_DIVISION || ok) return wrong("y = 0 is not SONIC_ERR_INEXACT_DIVISION");
  if ((rc = sonic_verify_core(srs, N, Q, wL, wR, wO, cs, NULL, tr + 32 * 4, tr + 32 * 5, &ok)) != SONIC_ERR_INVALID_ARG) return wrong("a NULL proof is not INVALID_ARG");

  /* compressed: 336 bytes and back */
  if ((rc = sonic_core_proof_compress(core, z))) return fail("sonic_core_proof_compress", rc);
  if ((rc = sonic_core_proof_decompress(z, core2))) return fail("sonic_core_proof_decompress", rc);
  if (memcmp(core, core2, CORE)) return wrong("compress / decompress do not round-trip");

  /* Fiat-Shamir: its own challenges, recomputed on the host, and the verifier that recomputes them */
  if ((rc = sonic_fs_circuit_digest(N, Q, wL, wR, wO, cs, digest))) return fail("sonic_fs_circuit_digest", rc);
  if ((rc = sonic_fs_srs_id(srs, srs_id))) return fail("sonic_fs_srs_id", rc);
  if ((rc = sonic_prover_prove_core_fs(p, digest, seed, core2, yz))) return fail("sonic_prover_prove_core_fs", rc);
  if ((rc = sonic_fs_core_challenges(N, Q, D, digest, srs_id, core2, yz2))) return fail("sonic_fs_core_challenges", rc);
  if (memcmp(yz, yz2, 64)) return wrong("prove_core_fs reports other challenges than sonic_fs_core_challenges recomputes");
  if ((rc = sonic_verify_core_fs(srs, N, Q, wL, wR, wO, cs, core2, &ok))) return fail("sonic_verify_core_fs", rc);
  if (!ok) return wrong("sonic_verify_core_fs rejects an honest proof");
  if ((rc = sonic_verify_core_fs(srs, N, Q, wL, wR, wO, cs, core, &ok))) return fail("sonic_verify_core_fs (a proof made at other challenges)", rc);
  if (ok) return wrong("sonic_verify_core_fs accepts a proof made at challenges that are not its transcript's");

  sonic_prover_free(p);
  sonic_srs_free(srs);
  free(proof);
  printf("core_proof_harness: OK (%d core proof bytes, %d compressed; head of the %lu-byte proof, flights, verify_core, Fiat-Shamir)\n", CORE,
         SONIC_CORE_PROOF_SIZE_COMPRESSED, (unsigned long)psz);
  return 0;
}
