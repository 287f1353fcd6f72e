#!/usr/bin/env python3
"""The pairing on the GPU against the pairing on host threads, in one process on one MI355X -> profiles/r20_pairing.txt.

  (a)  sonic_pairing_check, where = HOST against where = GPU, groups of 4 pairs, G = 1 .. 4096 groups: wall ms, best of five alternating
       rounds after a warm-up, spread (max - min of the five) in brackets.
  (b)  Verifier.verify_batch(each=True) at n = 2^14, Q = 2 with exactly one false proof, K = 1 .. 1024, SONIC_PAIRING_GPU=0 against =1, and
       the device form's split by kernel from one profiled call (HIP-event time, sonic_profile_get).
  (c)  the compiler's resource table of the new kernels (needs no GPU: --resources-only writes it alone).

The AUTO rules (pairing_device.hpp: PAIRING_GPU_MIN_GROUPS, EACH_GPU_MIN_PROOFS) are read off the last column of (a) and (b): the
smallest size from which the device form is faster by more than the larger of the two spreads, there and at every larger size.

    python tools/pairing.py [--resources-only | --keep-resources] [--quick]

--keep-resources takes section (c) from the file as it stands instead of compiling again (a machine with the GPU need not hold the compiler's
time): run --resources-only where the library is built, then --keep-resources on the MI355X.
"""
import ctypes as C
import os
import random
import re
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
CSRC = os.path.join(ROOT, "sonic_amd", "csrc")
OUT = os.path.join(ROOT, "profiles", "r20_pairing.txt")
KNOB = "SONIC_PAIRING_GPU"
QUICK = "--quick" in sys.argv
GROUPS = [1, 4, 16, 64] if QUICK else [1, 4, 16, 64, 256, 1024, 4096]
BATCHES = [1, 16] if QUICK else [1, 16, 64, 1024]
SEED = bytes(range(32))

out_lines = []


def say(s=""):
    print(s, flush=True)
    out_lines.append(s)


def write():
    with open(OUT, "w") as f:
        f.write("\n".join(out_lines) + "\n")


def resources():
    say("## (c) kernel resources (hipcc --offload-arch=gfx950 -O3 -Rpass-analysis=kernel-resource-usage)")
    say("%-22s %6s %6s %6s %10s %8s %10s" % ("kernel", "VGPRs", "AGPRs", "SGPRs", "scratch B", "LDS B", "waves/SIMD"))
    want = {"pairing.hip": ["k_miller_loops", "k_gt_plan", "k_gt_group_product", "k_final_exp", "k_pairing_points", "k_pairing_verdicts"],
            "verify_batch.hip": ["k_each_terms", "k_each_sums"]}
    procs = {f: subprocess.Popen(["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-Rpass-analysis=kernel-resource-usage", "-c",
                                  os.path.join(CSRC, f), "-o", os.devnull], stderr=subprocess.PIPE, text=True) for f in want}
    for f, names in want.items():
        err = procs[f].communicate()[1]
        for name in names:
            m = re.search(r"Function Name: \S*%s\S*.*?TotalSGPRs: (\d+).*?VGPRs: (\d+).*?AGPRs: (\d+).*?ScratchSize \[bytes/lane\]: (\d+).*?Occupancy \[waves/SIMD\]: (\d+)"
                          r".*?LDS Size \[bytes/block\]: (\d+)" % name, err, re.S)
            say("%-22s %6s %6s %6s %10s %8s %10s" % ((name, m.group(2), m.group(3), m.group(1), m.group(4), m.group(6), m.group(5)) if m else (name,) + ("?",) * 6))
    say()


def alternate(fns, rounds=5):
    """best and spread (max - min) of `rounds` timings per function, the functions taken in turn within every round, after one warm-up each"""
    for fn in fns:
        fn()
    ts = [[] for _ in fns]
    for _ in range(rounds):
        for i, fn in enumerate(fns):
            t = time.perf_counter()
            fn()
            ts[i].append((time.perf_counter() - t) * 1e3)
    return [(min(t), max(t) - min(t)) for t in ts]


def rule(sizes, held):
    """the smallest size from which `held` is true there and at every larger measured size; None when there is none"""
    first = None
    for s, h in zip(sizes, held):
        first = (s if first is None else first) if h else None
    return first


def main():
    if "--resources-only" in sys.argv:
        resources()
        say("(a) and (b) are not collected: no MI355X run of this tool is recorded.  The resource table above is all this file holds.")
        write()
        return
    kept = None
    if "--keep-resources" in sys.argv:
        old = open(OUT).read().split("\n")
        at = next(i for i, line in enumerate(old) if line.startswith("## (c)"))
        kept = old[at:at + old[at:].index("") + 1]
    import numpy as np
    import sonic_amd as sonic
    from sonic_amd import _lib, workload
    L = _lib.lib()
    _lib.check(L.sonic_init(0))
    os.environ.pop(KNOB, None)

    def split(fn):
        L.sonic_profile_enable(1)
        try:
            L.sonic_profile_reset()
            t = time.perf_counter()
            fn()
            wall = (time.perf_counter() - t) * 1e3
            buf = C.create_string_buffer(1 << 16)
            L.sonic_profile_names(buf, len(buf))
            got = {}
            for name in buf.value.decode().split("\n"):
                ms, cnt = C.c_double(0), C.c_int64(0)
                L.sonic_profile_get(name.encode(), C.byref(ms), C.byref(cnt))
                if cnt.value:
                    got[name] = ms.value
            return got, wall
        finally:
            L.sonic_profile_enable(0)

    # ---- (a) ----
    d = 64
    s = sonic.SRS.new(d, 0x5eed, 0xa1fa)
    p1 = np.concatenate([s.points(0, -d, 2 * d + 1), s.points(1, -d, 2 * d + 1)])
    p2 = np.concatenate([s.g2_points(0, -d, 2 * d + 1), s.g2_points(1, -d, 2 * d + 1)])
    s.close()
    say("## (a) sonic_pairing_check, groups of 4 pairs: wall ms, best of five alternating rounds after a warm-up (spread = max - min of the five)")
    say("%-6s %7s %20s %20s %9s   %s" % ("G", "pairs", "where = HOST", "where = GPU", "host/gpu", "GPU faster by more than the larger spread"))
    held_a, splits = [], {}
    for G in GROUPS:
        n = 4 * G
        g1 = np.ascontiguousarray(p1[(7 * np.arange(n) + 1) % len(p1)])
        g2 = np.ascontiguousarray(p2[(5 * np.arange(n) + 3) % len(p2)])
        ge = 4 * (1 + np.arange(G, dtype=np.int64))
        vh = sonic.pairing_check(g1, g2, ge, where="host")
        assert bytes(vh) == bytes(sonic.pairing_check(g1, g2, ge, where="gpu"))
        (th, sh), (tg, sg_) = alternate([lambda: sonic.pairing_check(g1, g2, ge, where="host"), lambda: sonic.pairing_check(g1, g2, ge, where="gpu")])
        held_a.append(th - tg > max(sh, sg_))
        say("%-6d %7d %12.2f (%5.2f) %12.2f (%5.2f) %8.2fx   %s" % (G, n, th, sh, tg, sg_, th / tg, "held" if held_a[-1] else "NOT held"))
        splits[G] = split(lambda: sonic.pairing_check(g1, g2, ge, where="gpu"))
    ra = rule(GROUPS, held_a)
    say("rule (a): " + ("the device form from G = %d groups upward" % ra if ra is not None else "the device form wins at no measured G: AUTO stays on the host"))
    say()
    say("## the GPU call of (a), one profiled call split by kernel (ms of HIP-event time; rest = wall of the profiled call - all kernels)")
    say("%-6s %10s %10s %10s %10s %10s %10s %10s" % ("G", "validate", "miller", "product", "final exp", "other k.", "rest", "wall"))
    for G, (k, wall) in splits.items():
        val = sum(v for nm, v in k.items() if nm.startswith(("k_g1_subgroup", "k_g2_subgroup", "k_pairing_points")))
        mil, fe = k.get("k_miller_loops", 0.0), k.get("k_final_exp", 0.0)
        prod = k.get("k_gt_plan", 0.0) + k.get("k_gt_group_product", 0.0)
        say("%-6d %10.2f %10.2f %10.2f %10.2f %10.2f %10.2f %10.2f" % (G, val, mil, prod, fe, sum(k.values()) - val - mil - prod - fe, wall - sum(k.values()), wall))
    say("(the profiled call runs with an event pair around every launch)")
    say()
    write()

    # ---- (b) ----
    log2n, Q = (10 if QUICK else 14), 2
    n = 1 << log2n
    b = workload.big_circuit(log2n, n, Q)
    circuit = sonic.ArithCircuit(sonic.GateWeights(b["wL"], b["wR"], b["wO"]), b["cs"])
    srs = sonic.SRS.new(7 * n + 9, 3, 5)
    pipe = sonic.ProverPipeline(srs, circuit)
    pipe.set_assignment(sonic.Assignment(b["aL"], b["aR"], b["aO"]))
    pyr = random.Random(log2n * 1000 + Q)
    nd = min(64, max(BATCHES))
    R = sonic.R_MODULUS
    trs = [[pyr.randrange(1, R) for _ in range(8 + 2 * Q)] for _ in range(nd)]
    proofs = pipe.prove_all(trs)
    pipe.close()
    vtr = [(t[4], t[5], list(zip(t[6:6 + Q], t[6 + Q:6 + 2 * Q]))) for t in trs]
    ver = sonic.Verifier(srs, circuit)
    say("## (b) verify_batch(each=True), n = 2^%d, Q = %d, exactly one false proof (the last): wall ms of the whole call, best of five alternating (spread)" % (log2n, Q))
    say("%-6s %20s %20s %9s   %s" % ("K", KNOB + "=0 (host)", KNOB + "=1 (device)", "host/gpu", "device faster by more than the larger spread"))
    held_b, bsplits = [], {}
    for K in BATCHES:
        bp, bt = [proofs[k % nd] for k in range(K)], [vtr[k % nd] for k in range(K)]
        y, z, yzs = bt[K - 1]
        bt[K - 1] = (y, (z + 1) % R, yzs)
        want = (False, [True] * (K - 1) + [False])

        def run(knob):
            os.environ[KNOB] = knob
            try:
                assert ver.verify_batch(bp, bt, seed=SEED, each=True) == want
            finally:
                del os.environ[KNOB]
        (th, sh), (tg, sg_) = alternate([lambda: run("0"), lambda: run("1")])
        held_b.append(th - tg > max(sh, sg_))
        say("%-6d %12.1f (%5.1f) %12.1f (%5.1f) %8.2fx   %s" % (K, th, sh, tg, sg_, th / tg, "held" if held_b[-1] else "NOT held"))
        bsplits[K] = (split(lambda: run("1")), split(lambda: run("0")))
    rb = rule(BATCHES, held_b)
    say("rule (b): " + ("the device form from K = %d proofs upward" % rb if rb is not None else "the device form wins at no measured K: `each` stays on the host"))
    say()
    say("## the per-proof fold of (b), one profiled call each (ms; device: HIP-event time by kernel, each_gpu = the host's wall around them; host: the phase)")
    say("%-6s %10s %10s %10s %10s %10s %12s %14s" % ("K", "terms", "sums", "miller", "product", "final exp", "each_gpu", "each (host)"))
    for K, ((k, _), (kh, _)) in bsplits.items():
        say("%-6d %10.2f %10.2f %10.2f %10.2f %10.2f %12.2f %14.2f" % (K, k.get("k_each_terms", 0.0), k.get("k_each_sums", 0.0), k.get("k_miller_loops", 0.0),
                                                                   k.get("k_gt_plan", 0.0) + k.get("k_gt_group_product", 0.0), k.get("k_final_exp", 0.0),
                                                                   k.get("verify_batch:each_gpu", 0.0), kh.get("verify_batch:each", 0.0)))
    say()
    ver.close()
    srs.close()
    write()
    if kept is not None:
        for line in kept:
            say(line)
    else:
        resources()
    write()


if __name__ == "__main__":
    main()
