#!/usr/bin/env python3
"""Writes profiles/r10_statements.txt on one MI355X: what one statement per proof costs beside the existing entry points, every pair
measured in this one process on the same GPU and the same handles.

  resources  VGPRs / SGPRs / scratch / occupancy of the kernels of statement.hip (the compiler's remarks)
  (a)        sonic_prove_batch_statements (K constant sets) against sonic_prove_batch (one) on the same two handles, n = 2^16, Q = 2, K = 64
  (b)        verify_batch with constants (sonic_verifier_verify_batch_cs) against verify_batch at n = 2^14, Q = 2, K in {1, 64, 1024}
  (c)        eval_constraints at n = 2^18: the dense Q = 2 rndCircuit and a CSR circuit at Q = 64 with <= 4 entries per row, B in {1, 16},
             beside the Python-integer computation sonic_amd.workload does for the same constants

Run from the repository root after the library is built:  python tools/statements.py [--quick]
Times are wall times of the call, the best of five after one warm-up, with the spread (max - min) beside them: the new forms add O(Q) work
per proof, so a difference beyond the spread is a finding to explain, not noise to average away."""
import os
import random
import re
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
CSRC = os.path.join(ROOT, "sonic_amd", "csrc")
R = 0x73EDA753299D7D483339D80809A1D80553BDA402FFFE5BFEFFFFFFFF00000001
QUICK = "--quick" in sys.argv
out_lines = []


def say(line=""):
    print(line, flush=True)
    out_lines.append(line)


def resources():
    say("## kernel resources (hipcc --offload-arch=gfx950 -O3 -Rpass-analysis=kernel-resource-usage)")
    say("%-16s %6s %6s %10s %10s %8s" % ("kernel", "VGPRs", "SGPRs", "scratch B", "occupancy", "LDS B"))
    err = subprocess.run(["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-Rpass-analysis=kernel-resource-usage", "-c",
                          os.path.join(CSRC, "statement.hip"), "-o", os.devnull], stderr=subprocess.PIPE, text=True).stderr
    for name in ("k_cs_csr", "k_cs_dense", "k_cs_finish", "k_gates"):
        m = re.search(r"Function Name: \S*%s\S*.*?TotalSGPRs: (\d+).*?VGPRs: (\d+).*?ScratchSize \[bytes/lane\]: (\d+).*?Occupancy \[waves/SIMD\]: (\d+).*?LDS Size \[bytes/block\]: (\d+)"
                      % name, err, re.S)
        say("%-16s %6s %6s %10s %10s %8s" % ((name, m.group(2), m.group(1), m.group(3), m.group(4), m.group(5)) if m else (name, "?", "?", "?", "?", "?")))
    say()


def timed(fn, reps=5):
    """(best, spread) in ms after one warm-up"""
    fn()
    ts = []
    for _ in range(reps):
        t = time.perf_counter()
        fn()
        ts.append((time.perf_counter() - t) * 1e3)
    return min(ts), max(ts) - min(ts)


def assignments(rng, K, n):
    """K satisfied assignments without Python integers: aL uniform, aR in {0, 1}, aO = aL aR"""
    from sonic_amd.workload import rand_fr_array
    out = []
    for _ in range(K):
        aL = rand_fr_array(rng, n)
        bits = rng.integers(0, 2, size=n, dtype=np.uint8)
        aR = np.zeros((n, 32), np.uint8)
        aR[:, 0] = bits
        out.append((aL, aR, aL * bits[:, None]))
    return out


def main():
    resources()
    if "--resources" in sys.argv:
        say("## (a), (b), (c): not collected yet (they need the GPU)")
        write()
        return
    import sonic_amd as sonic
    from sonic_amd import _lib
    from sonic_amd.workload import big_circuit, sparse_circuit
    L = _lib.lib()
    _lib.check(L.sonic_init(0))
    pyr = random.Random(10)
    rng = np.random.default_rng(10)
    draw = lambda Q: [pyr.randrange(1, R) for _ in range(8 + 2 * Q)]      # noqa: E731
    oracle = lambda t, Q: (t[4], t[5], list(zip(t[6:6 + Q], t[6 + Q:6 + 2 * Q])))      # noqa: E731

    # ---- (a) ----
    n, Q, K = 1 << (12 if QUICK else 16), 2, 16 if QUICK else 64
    say("## (a) prove_batch (one constant set) against prove_batch with K constant sets, two handles, n = 2^%d, Q = %d, K = %d (ms per batch)" % (n.bit_length() - 1, Q, K))
    b = big_circuit(n + Q, n, Q)
    circuit = sonic.ArithCircuit(sonic.GateWeights(b["wL"], b["wR"], b["wO"]), b["cs"])
    srs = sonic.SRS.new(8 * n, pyr.randrange(2, R), pyr.randrange(2, R))
    provers = [sonic.Prover(srs, circuit) for _ in range(2)]
    asgs = [sonic.Assignment(*a) for a in assignments(rng, K, n)]
    css, gates = provers[0].eval_constraints(asgs)
    assert gates == [(0, -1)] * K
    same = [sonic.Assignment(b["aL"], b["aR"], b["aO"])] * K
    trs = [draw(Q) for _ in range(K)]
    old = lambda: sonic.prove_batch(provers, trs, same)                                 # noqa: E731
    new = lambda: sonic.prove_batch(provers, trs, asgs, constants=css)                  # noqa: E731
    to, so = timed(old)
    tn, sn = timed(new)
    say("%-28s %10s %10s %12s" % ("call", "best", "spread", "proofs / s"))
    say("%-28s %10.2f %10.2f %12.1f" % ("sonic_prove_batch", to, so, K / to * 1e3))
    say("%-28s %10.2f %10.2f %12.1f" % ("sonic_prove_batch_statements", tn, sn, K / tn * 1e3))
    say("ratio new / old = %.3f" % (tn / to))
    for p in provers:
        p.close()
    srs.close()
    say()

    # ---- (b) ----
    n, Q = 1 << (10 if QUICK else 14), 2
    Ks = [1, 64] + ([] if QUICK else [1024])
    say("## (b) verify_batch against verify_batch with per-proof constants at n = 2^%d, Q = %d (ms per batch, fixed seed)" % (n.bit_length() - 1, Q))
    b = big_circuit(n + Q, n, Q)
    circuit = sonic.ArithCircuit(sonic.GateWeights(b["wL"], b["wR"], b["wO"]), b["cs"])
    srs = sonic.SRS.new(8 * n, pyr.randrange(2, R), pyr.randrange(2, R))
    provers = [sonic.Prover(srs, circuit) for _ in range(2)]
    provers[0].set_assignment(sonic.Assignment(b["aL"], b["aR"], b["aO"]))
    Kmax = max(Ks)
    trs = [draw(Q) for _ in range(Kmax)]
    own = [bytes(provers[0].prove_bytes(t)) for t in trs]                               # K proofs of the handle's statement
    asgs = [sonic.Assignment(*a) for a in assignments(rng, Kmax, n)]
    css = []
    for i in range(0, Kmax, 64):
        css += provers[0].eval_constraints(asgs[i:i + 64])[0]
    many = sonic.prove_batch(provers, trs, asgs, constants=css)                         # K proofs of K statements
    for p in provers:
        p.close()
    ch = [oracle(t, Q) for t in trs]
    ver = sonic.Verifier(srs, circuit)
    seed = bytes(range(32))
    say("%-6s %14s %10s %14s %10s %7s" % ("K", "verify_batch", "spread", "with constants", "spread", "ratio"))
    for K in Ks:
        plain = lambda: ver.verify_batch(own[:K], ch[:K], seed=seed)                            # noqa: E731
        withcs = lambda: ver.verify_batch(many[:K], ch[:K], seed=seed, constants=css[:K])       # noqa: E731
        assert plain() is True and withcs() is True
        tp, sp = timed(plain)
        tc, sc = timed(withcs)
        say("%-6d %14.3f %10.3f %14.3f %10.3f %7.3f" % (K, tp, sp, tc, sc, tc / tp))
    ver.close()
    srs.close()
    say()

    # ---- (c) ----
    n = 1 << (14 if QUICK else 18)
    say("## (c) eval_constraints at n = 2^%d (ms per call; Python = the integer computation of sonic_amd.workload for ONE assignment)" % (n.bit_length() - 1))
    srs = sonic.SRS.new(7 * n + 8, pyr.randrange(2, R), pyr.randrange(2, R))
    say("%-28s %8s %10s %10s %12s" % ("circuit", "B", "best", "spread", "Python"))
    ints = lambda a: [int.from_bytes(a[i].tobytes(), "little") for i in range(a.shape[0])]      # noqa: E731

    def python_dense(bc, asg):
        la, lb = ints(asg[0]), ints(asg[1])
        lo = [x * y % R for x, y in zip(la, lb)]
        sums = [sum(la) % R, sum(lb) % R, sum(lo) % R]
        cs = [0] * Q2
        for k, r_ in enumerate(bc["rows"]):
            cs[r_] = (cs[r_] + sums[k]) % R
        return cs

    def python_csr(sc, asg):
        la, lb = ints(asg[0]), ints(asg[1])
        lo = [x * y % R for x, y in zip(la, lb)]
        val = ints(sc["val"])
        cs = [0] * Q2
        for r in range(3 * Q2):
            m, q = divmod(r, Q2)
            a = (la, lb, lo)[m]
            for k in range(int(sc["row_ptr"][r]), int(sc["row_ptr"][r + 1])):
                cs[q] = (cs[q] + val[k] * a[int(sc["col"][k])]) % R
        return cs

    for name in ("dense Q = 2 rndCircuit", "CSR Q = 64, <= 4 per row"):
        if name.startswith("dense"):
            Q2 = 2
            bc = big_circuit(n + Q2, n, Q2)
            circuit = sonic.ArithCircuit(sonic.GateWeights(bc["wL"], bc["wR"], bc["wO"]), bc["cs"])
            py = python_dense
        else:
            Q2 = 64
            bc = sparse_circuit(n + Q2, n, Q2)
            circuit = sonic.SparseCircuit(n, Q2, bc["row_ptr"], bc["col"], bc["val"], bc["cs"])
            py = python_csr
        p = sonic.Prover(srs, circuit, prepare=False)
        raw = assignments(rng, 16, n)
        asgs = [sonic.Assignment(*a) for a in raw]
        t0 = time.perf_counter()
        want = py(bc, raw[0])
        tpy = (time.perf_counter() - t0) * 1e3
        got, gates = p.eval_constraints(asgs[:1])
        assert got == [want] and gates == [(0, -1)]
        stacked = [np.ascontiguousarray(np.stack([a[m] for a in raw])) for m in range(3)]      # the C call on its own: inputs laid out once
        out, gbuf = np.zeros((16, Q2, 32), np.uint8), np.zeros((16, 2), np.int64)
        for B in (1, 16):
            t, s = timed(lambda: _lib.check(L.sonic_prover_eval_constraints(p._h, B, stacked[0].ctypes.data, stacked[1].ctypes.data, stacked[2].ctypes.data,
                                                                            out.ctypes.data, gbuf.ctypes.data)))
            say("%-28s %8d %10.3f %10.3f %12s" % (name, B, t, s, "%.1f" % tpy if B == 1 else ""))
        p.close()
    srs.close()
    if not QUICK:
        write()


def write():
    with open(os.path.join(ROOT, "profiles", "r10_statements.txt"), "w") as f:
        f.write("\n".join(out_lines) + "\n")


if __name__ == "__main__":
    main()
