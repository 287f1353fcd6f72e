#!/usr/bin/env python3
"""The R1CS front end on the textbook statement "I know x with x^3 + x + 5 = 35" (x = 3), proved and verified on the GPU path.

    python examples/r1cs_cubic.py      ->  Success: True

The rank-1 constraint system has m = 3 rows over N = 5 columns z = (1, out, x, v1, v2) with one public input (out):

    x  * x = v1
    v1 * x = v2
    (v2 + x + 5) * 1 = out

sonic_amd.R1CS compiles it to a Sonic constraint system of n = 5 gates and Q = 10 linear constraints and turns the witness into an
assignment on the GPU.  A core proof is what a circuit made from R1CS should use (its Q is of the order of n); this circuit is small
enough for a full proof as well, so both are made and verified.  d = 64 is large enough."""
import os
import secrets
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import sonic_amd as S  # noqa: E402

R = S.R_MODULUS


def cubic(x: int = 3):
    """(N, n_pub, A rows, B rows, C rows, z) of x^3 + x + 5 = out"""
    v1 = x * x % R
    v2 = v1 * x % R
    out = (v2 + x + 5) % R
    A = [{2: 1}, {3: 1}, {0: 5, 2: 1, 4: 1}]
    B = [{2: 1}, {2: 1}, {0: 1}]
    C = [{3: 1}, {4: 1}, {1: 1}]
    return 5, 1, A, B, C, [1, out, x, v1, v2]


def run_example() -> bool:
    N, n_pub, A, B, C, z = cubic(3)
    r = S.R1CS.from_rows(N, n_pub, A, B, C)
    assert (r.n, r.Q) == (5, 10)
    srs = S.SRS.new(64, secrets.randbelow(R - 1) + 1, secrets.randbelow(R - 1) + 1)
    circuit = r.circuit(public=[35])
    wb, cs, bad = r.assign([z])
    assert bad == [(0, -1)], f"the witness breaks {bad[0][0]} constraints, the first is row {bad[0][1]}"
    p = S.Prover(srs, circuit, prepare=False)
    p.set_witness(wb.aL[0], wb.aR[0], wb.aO[0])
    p.set_constants(cs[0])
    # a core proof: the four blinders, y, z
    tr = S.protocol.draw_transcript(r.Q)
    core = p.prove_core_bytes(tr[:6])
    ok = S.verify_core(srs, circuit, core, tr[4] % R, tr[5] % R)
    wrong = S.verify_core(srs, r.circuit(public=[36]), core, tr[4] % R, tr[5] % R)
    # the full proof, 7 + 4Q multi-scalar multiplications
    proof = S.Proof.from_bytes(p.prove_bytes(tr), r.Q)
    t = [v % R for v in tr]
    full = S.verify(srs, circuit, proof, t[4], t[5], list(zip(t[6:6 + r.Q], t[6 + r.Q:6 + 2 * r.Q])))
    print(f"x^3 + x + 5 = 35: n = {r.n}, Q = {r.Q}; core proof accepted: {ok}; against out = 36: {wrong}; full proof accepted: {full}")
    print(f"Success: {ok and full and not wrong}")
    return ok and full and not wrong


if __name__ == "__main__":
    sys.exit(0 if run_example() else 1)
