#!/usr/bin/env python3
"""Writes profiles/r11_fs_stream.txt on one MI355X: what Fiat-Shamir proofs cost in flight (sonic_prover_submit_fs / collect_fs,
sonic_prove_batch_fs, witness digest v2 on the GPU) beside the blocking sonic_prover_prove_fs, which is the yardstick of every line: it
is unchanged, and it is measured in this same process on the same GPU and handles.

  resources  VGPRs / SGPRs / scratch / occupancy / LDS of the kernels of witness.hip (the compiler's remarks)
  (1)        the witness digest at n = 2^14 and 2^18: v1 as the blocking call computes it (the first prove_fs after set_assignment minus
             the second) against sonic_prover_witness_digest_v2 after set_assignment, with the kernels' own times (HIP events)
  (2)        ms per proof with the assignment resident, n = 2^14 and 2^18, Q = 2, d = 8n: blocking prove_fs on one handle; submit_fs /
             collect_fs one at a time; the same over two handles driven by this one thread; explicit-transcript submit / collect over
             the same two handles
  (3)        64 proofs at n = 2^16 with an assignment and constants per proof: sonic_prove_batch_fs against
             sonic_prove_batch_statements on the same two handles, and against 64 x (set_assignment, set_constants, blocking prove_fs)

Run from the repository root after the library is built:  python tools/fs_stream.py [--quick] [--resources]
Times are wall times of the calls, the best of five after one warm-up, with the spread (max - min) beside them."""
import ctypes as C
import hashlib
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
    say("%-22s %6s %6s %10s %10s %8s" % ("kernel", "VGPRs", "SGPRs", "scratch B", "waves/SIMD", "LDS B"))
    err = subprocess.run(["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-Rpass-analysis=kernel-resource-usage", "-c",
                          os.path.join(CSRC, "witness.hip"), "-o", os.devnull], stderr=subprocess.PIPE, text=True).stderr
    for name in ("k_witness_leaves", "k_witness_nodes"):
        m = re.search(r"Function Name: \S*%sE\S*.*?TotalSGPRs: (\d+).*?VGPRs: (\d+).*?ScratchSize \[bytes/lane\]: (\d+).*?Occupancy \[waves/SIMD\]: (\d+).*?LDS Size \[bytes/block\]: (\d+)"
                      % name, err, re.S)
        say("%-22s %6s %6s %10s %10s %8s" % ((name, m.group(2), m.group(1), m.group(3), m.group(4), m.group(5)) if m else (name, "?", "?", "?", "?", "?")))
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


def clock(fn):
    t = time.perf_counter()
    fn()
    return (time.perf_counter() - t) * 1e3


def seed_of(tag) -> bytes:
    return hashlib.sha256(b"fs_stream %s" % str(tag).encode()).digest()


def main():
    resources()
    if "--resources" in sys.argv:
        say("## (1), (2), (3): not collected yet (they need the GPU)")
        write()
        return
    import sonic_amd as sonic
    from sonic_amd import _lib
    from sonic_amd.workload import big_circuit, rand_fr_array
    L = _lib.lib()
    _lib.check(L.sonic_init(0))
    pyr = random.Random(11)
    rng = np.random.default_rng(11)
    draw = lambda Q: [pyr.randrange(1, R) for _ in range(8 + 2 * Q)]      # noqa: E731
    verdicts = []

    def kernel_ms(names, fn):
        """the HIP-event time of the named kernels over one call of fn (ms, summed)"""
        L.sonic_profile_reset()
        L.sonic_profile_enable(1)
        fn()
        total = 0.0
        for name in names:
            ms, cnt = C.c_double(0), C.c_int64(0)
            L.sonic_profile_get(name.encode(), C.byref(ms), C.byref(cnt))
            total += ms.value
        L.sonic_profile_enable(0)
        return total

    sizes = [10, 12] if QUICK else [14, 18]
    Q = 2
    fs_two, blocking = {}, {}
    for lg in sizes:
        n = 1 << lg
        b = big_circuit(n + Q, n, Q)
        circuit = sonic.ArithCircuit(sonic.GateWeights(b["wL"], b["wR"], b["wO"]), b["cs"])
        digest = sonic.fs_circuit_digest(circuit)
        asg = sonic.Assignment(b["aL"], b["aR"], b["aO"])
        srs = sonic.SRS.new(8 * n, pyr.randrange(2, R), pyr.randrange(2, R))
        provers = [sonic.Prover(srs, circuit) for _ in range(2)]
        A, B = provers
        for p in provers:
            p.set_assignment(asg)
            p.prove_fs(digest, seed_of(0))                  # (the workspaces grow on the first proof)

        # ---- (1) ----
        say("## (1) witness digest at n = 2^%d (%d bytes): ms per digest" % (lg, 96 * n))
        v1 = []
        for r in range(6):
            A.set_assignment(asg)
            first = clock(lambda: A.prove_fs(digest, seed_of(r)))
            second = clock(lambda: A.prove_fs(digest, seed_of(r)))
            v1.append(first - second)
        v1 = v1[1:]

        def v2_once():
            A.set_assignment(asg)
            return clock(A.witness_digest)
        v2_once()
        v2 = [v2_once() for _ in range(5)]
        A.set_assignment(asg)
        kern = kernel_ms(("k_witness_leaves", "k_witness_nodes"), A.witness_digest)
        say("%-44s %10s %10s" % ("digest", "best", "spread"))
        say("%-44s %10.3f %10.3f" % ("v1: download + SHA-256 on one host core", min(v1), max(v1) - min(v1)))
        say("%-44s %10.3f %10.3f" % ("v2: sonic_prover_witness_digest_v2 (call)", min(v2), max(v2) - min(v2)))
        say("%-44s %10.3f" % ("v2: its kernels alone (HIP events)", kern))
        say()

        # ---- (2) ----
        N = 8 if lg <= 14 else 4
        say("## (2) ms per proof, assignment resident, n = 2^%d, Q = %d, d = 8n (%d proofs per timing)" % (lg, Q, 2 * N))
        seeds = [seed_of(("s", k)) for k in range(2 * N)]
        trs = [draw(Q) for _ in range(2 * N)]

        def leg_blocking():
            for s in seeds:
                A.prove_fs(digest, s)

        def leg_one():
            for s in seeds:
                A.submit_fs(digest, s)
                A.collect_fs()

        def leg_two():
            A.submit_fs(digest, seeds[0])
            B.submit_fs(digest, seeds[1])
            for k in range(2, 2 * N, 2):
                A.collect_fs()
                A.submit_fs(digest, seeds[k])
                B.collect_fs()
                B.submit_fs(digest, seeds[k + 1])
            A.collect_fs()
            B.collect_fs()

        def leg_explicit():
            A.submit(trs[0])
            B.submit(trs[1])
            for k in range(2, 2 * N, 2):
                A.collect()
                A.submit(trs[k])
                B.collect()
                B.submit(trs[k + 1])
            A.collect()
            B.collect()
        say("%-52s %10s %10s" % ("leg", "best", "spread"))
        res = {}
        for name, leg in (("blocking prove_fs, one handle", leg_blocking), ("submit_fs / collect_fs, one at a time", leg_one),
                          ("submit_fs / collect_fs over two handles", leg_two), ("explicit transcript submit / collect, two handles", leg_explicit)):
            t, s = timed(leg)
            res[name] = (t / (2 * N), s / (2 * N))
            say("%-52s %10.3f %10.3f" % (name, t / (2 * N), s / (2 * N)))
        blk, two, exp = res["blocking prove_fs, one handle"], res["submit_fs / collect_fs over two handles"], res["explicit transcript submit / collect, two handles"]
        fs_two[lg], blocking[lg] = two, blk
        say("Fiat-Shamir over two handles / explicit transcript over two handles = %.3f" % (two[0] / exp[0]))
        ok = blk[0] - two[0] > max(blk[1], two[1])
        verdicts.append(("n = 2^%d: Fiat-Shamir over two handles costs less per proof than blocking prove_fs by more than the larger spread "
                         "(%.3f < %.3f - %.3f)" % (lg, two[0], blk[0], max(blk[1], two[1])), ok))
        say()
        for p in provers:
            p.close()
        srs.close()

    # ---- (3) ----
    lg, K = (12, 8) if QUICK else (16, 64)
    n = 1 << lg
    say("## (3) %d proofs at n = 2^%d, Q = %d, an assignment and constants per proof (ms per batch)" % (K, lg, Q))
    b = big_circuit(n + Q, n, Q)
    circuit = sonic.ArithCircuit(sonic.GateWeights(b["wL"], b["wR"], b["wO"]), b["cs"])
    srs = sonic.SRS.new(8 * n, pyr.randrange(2, R), pyr.randrange(2, R))
    provers = [sonic.Prover(srs, circuit) for _ in range(2)]
    raw = []
    for _ in range(K):                  # K satisfied assignments without Python integers: aL uniform, aR in {0, 1}, aO = aL aR
        aL = rand_fr_array(rng, n)
        bits = rng.integers(0, 2, size=n, dtype=np.uint8)
        aR = np.zeros((n, 32), np.uint8)
        aR[:, 0] = bits
        raw.append((aL, aR, aL * bits[:, None]))
    asgs = [sonic.Assignment(*a) for a in raw]
    css, gates = provers[0].eval_constraints(asgs)
    assert gates == [(0, -1)] * K
    mid = sonic.fs_circuit_midstate(circuit)
    digests = [sonic.fs_circuit_digest_resume(mid, cs) for cs in css]
    seeds = [seed_of(("b", k)) for k in range(K)]
    trs = [draw(Q) for _ in range(K)]
    got = []

    def leg_batch_fs():
        got[:] = sonic.prove_batch_fs(provers, digests, seeds, assignments=asgs, constants=css)

    def leg_batch_explicit():
        sonic.prove_batch(provers, trs, asgs, constants=css)

    def leg_blocking_calls():
        p = provers[0]
        for k in range(K):
            p.set_assignment(asgs[k])
            p.set_constants(css[k])
            p.prove_fs(digests[k], seeds[k])
    say("%-58s %10s %10s %12s" % ("call", "best", "spread", "proofs / s"))
    res = {}
    for name, leg in (("sonic_prove_batch_fs, two handles", leg_batch_fs), ("sonic_prove_batch_statements, two handles", leg_batch_explicit),
                      ("%d x (set_assignment, set_constants, prove_fs), one handle" % K, leg_blocking_calls)):
        res[name] = timed(leg)
        say("%-58s %10.2f %10.2f %12.1f" % (name, res[name][0], res[name][1], K / res[name][0] * 1e3))
    ver = sonic.Verifier(srs, circuit)
    assert ver.verify_fs_batch([r for r, _ in got], seed=bytes(range(32)), constants=css) is True
    ver.close()
    fsb, exb, blb = res["sonic_prove_batch_fs, two handles"], res["sonic_prove_batch_statements, two handles"], list(res.values())[2]
    say("Fiat-Shamir batch / explicit-transcript batch = %.3f" % (fsb[0] / exb[0]))
    verdicts.append(("the Fiat-Shamir batch beats the %d blocking calls by more than the larger spread (%.2f < %.2f - %.2f)" % (K, fsb[0], blb[0], max(fsb[1], blb[1])),
                     blb[0] - fsb[0] > max(fsb[1], blb[1])))
    for p in provers:
        p.close()
    srs.close()
    say()
    say("## what has to hold, against the unchanged blocking call in this run")
    for text, ok in verdicts:
        say("%s  %s" % ("HOLDS" if ok else "FAILS", text))
    if not QUICK:
        write()


def write():
    with open(os.path.join(ROOT, "profiles", "r11_fs_stream.txt"), "w") as f:
        f.write("\n".join(out_lines) + "\n")


if __name__ == "__main__":
    main()
