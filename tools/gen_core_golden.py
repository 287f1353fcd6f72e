"""Writes tests/golden/core_head_big.json: the CPU oracle's head (R, T, a, W_a, b, W_b, W_t, s: the first 576 bytes of its proof) for the
one multi-tile shape of tests/test_gpu_core_proofs.py, n = 3 * 4096 + 5, Q = 2.  The oracle needs ~25 s of CPU for a proof of that size
(its signature part included), which no test may spend per run; the inputs are regenerated from the seeds recorded here.  CPU only:

    python tools/gen_core_golden.py
"""
import json
import os
import random
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from oracle import orc                                              # noqa: E402
from sonic_amd.workload import big_circuit, fr_bytes                # noqa: E402

R = 0x73EDA753299D7D483339D80809A1D80553BDA402FFFE5BFEFFFFFFFF00000001
CASE = dict(n=3 * 4096 + 5, Q=2, d=7 * (3 * 4096 + 5) + 3, x=0x1234567891, alpha=0x987654321, circuit_seed=77, transcript_seed=4242)


def transcript(case):
    pyr = random.Random(case["transcript_seed"])
    return [pyr.randrange(1, R) for _ in range(8 + 2 * case["Q"])]


def main():
    c = big_circuit(CASE["circuit_seed"], CASE["n"], CASE["Q"])
    srs = orc.SRS(CASE["d"], CASE["x"], CASE["alpha"], threads=os.cpu_count() or 1)
    proof = orc.prove(srs, CASE["n"], CASE["Q"], c["wL"], c["wR"], c["wO"], c["cs"], c["aL"], c["aR"], c["aO"], fr_bytes(transcript(CASE)))
    out = dict(CASE, head=bytes(proof[:576]).hex())
    path = os.path.join(ROOT, "tests", "golden", "core_head_big.json")
    with open(path, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print("wrote", path)


if __name__ == "__main__":
    main()
