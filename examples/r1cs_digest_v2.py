#!/usr/bin/env python3
"""A Fiat-Shamir core proof of a compiled R1CS under circuit digest v2, verified by a verifier handle of digest kind 2.

    python examples/r1cs_digest_v2.py      ->  Success: True

The statement is the one of r1cs_cubic.py, "I know x with x^3 + x + 5 = 35".  A circuit made from R1CS has Q of the order of n, and
circuit digest v1 hashes the 96 Q n dense bytes its weights stand for; digest v2 hashes the entries of the CSR, and the GPU computes it
from the CSR a handle already holds.  Nothing here grows as Q n: the handle is not prepared, the proof is a core proof (the handle never
makes the Q buffers of a full proof's signature), and the verifier is made with digest=2.

    weights digest v2  = Prover.weights_digest_v2()          (= fs_weights_digest_v2(circuit) on the host, = Verifier.weights_digest_v2())
    circuit digest v2  = fs_circuit_digest_v2(wd2, cs)        one per statement, 32 Q bytes of hashing
    proof              = Prover.prove_core_fs(cd2, seed)
    verdict            = Verifier(srs, circuit, digest=2).verify_core_fs_batch([proof], constants=[cs])"""
import os
import secrets
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import sonic_amd as S  # noqa: E402
from r1cs_cubic import cubic  # noqa: E402

R = S.R_MODULUS


def run_example() -> bool:
    N, n_pub, A, B, C, z = cubic(3)
    r = S.R1CS.from_rows(N, n_pub, A, B, C)
    srs = S.SRS.new(64, secrets.randbelow(R - 1) + 1, secrets.randbelow(R - 1) + 1)
    circuit = r.circuit(public=[35])
    wb, cs, bad = r.assign([z])
    assert bad == [(0, -1)], f"the witness breaks {bad[0][0]} constraints, the first is row {bad[0][1]}"
    p = S.Prover(srs, circuit, prepare=False)
    fresh = p.device_bytes
    p.set_witness(wb.aL[0], wb.aR[0], wb.aO[0])
    p.set_constants(cs[0])
    wd2 = p.weights_digest_v2()
    assert wd2 == S.fs_weights_digest_v2(circuit)
    cd2 = S.fs_circuit_digest_v2(wd2, cs[0])
    core, _y, _z = p.prove_core_fs(cd2, secrets.token_bytes(32))
    v2 = S.Verifier(srs, circuit, digest=2)
    assert v2.digest_kind == 2 and v2.weights_digest_v2() == wd2
    ok = v2.verify_core_fs_batch([core], constants=[cs[0]])
    # the same proof against out = 36, and on a verifier of digest kind 1: rejected proofs, not errors
    moved = list(cs[0])
    moved[-1] = 36
    wrong = v2.verify_core_fs_batch([core], constants=[moved])
    v1 = S.Verifier(srs, circuit, digest=1)
    other = v1.verify_core_fs_batch([core], constants=[cs[0]])
    print(f"x^3 + x + 5 = 35 under circuit digest v2: n = {r.n}, Q = {r.Q}; accepted: {ok}; against out = 36: {wrong}; by a kind-1 verifier: {other}")
    print(f"the handle owns {p.device_bytes} bytes of device memory ({fresh} when it was made); a full proof would add {32 * r.Q * (3 * r.n + 1)}")
    print(f"Success: {ok and not wrong and not other}")
    for h in (v1, v2, p, srs, r):
        h.close()
    return ok and not wrong and not other


if __name__ == "__main__":
    sys.exit(0 if run_example() else 1)
