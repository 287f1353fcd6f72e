#!/usr/bin/env python3
"""Writes profiles/r09_compressed.txt on one MI355X: what the compressed encodings cost beside the uncompressed paths, every pair measured
in this one process on the same GPU.

  resources  VGPRs / SGPRs / scratch / occupancy of the four kernels of compress.hip and of k_g1_validate (the compiler's remarks)
  (a)        sonic_g1_decompress (check_subgroup = 1) against sonic_g1_validate at 2^10, 2^16, 2^20 points; sonic_g2_decompress against the
             validation of sonic_srs_set_g2_points (k_g2_points_from_bytes, run through sonic_g2_compress) at 2^10, 2^16 points
  (b)        save / load wall time and file size of both SRS containers at d = 2^18 with the G2 half
  (c)        verify_batch against its `_z` form at n = 2^14, Q = 2, K in {1, 64, 1024}

Run from the repository root after the library is built:  python tools/compressed_points.py [--quick]
Times are the best of three calls after one warm-up; "kernel" is the HIP-event time of the named kernel (sonic_profile_get), "call" the wall
time of the C entry point with its copies."""
import ctypes as C
import os
import random
import re
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
CSRC = os.path.join(ROOT, "sonic_amd", "csrc")
R = 0x73EDA753299D7D483339D80809A1D80553BDA402FFFE5BFEFFFFFFFF00000001
QUICK = "--quick" in sys.argv
out_lines = []


def say(line=""):
    print(line, flush=True)
    out_lines.append(line)


def resources():
    say("## kernel resources (hipcc --offload-arch=gfx950 -O3 -Rpass-analysis=kernel-resource-usage)")
    say("%-28s %6s %6s %10s %10s" % ("kernel", "VGPRs", "SGPRs", "scratch B", "occupancy"))
    want = {"compress.hip": ["k_g1_decompress", "k_g1_compress", "k_g2_decompress", "k_g2_compress"], "verify_batch.hip": ["k_g1_validate"],
            "srs_g2.hip": ["k_g2_points_from_bytes"]}
    procs = {f: subprocess.Popen(["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-Rpass-analysis=kernel-resource-usage", "-c",
                                  os.path.join(CSRC, f), "-o", os.devnull], stderr=subprocess.PIPE, text=True) for f in want}
    for f, names in want.items():
        err = procs[f].communicate()[1]
        for name in names:
            m = re.search(r"Function Name: \S*%s\S*.*?TotalSGPRs: (\d+).*?VGPRs: (\d+).*?ScratchSize \[bytes/lane\]: (\d+).*?Occupancy \[waves/SIMD\]: (\d+)" % name, err, re.S)
            say("%-28s %6s %6s %10s %10s" % ((name, m.group(2), m.group(1), m.group(3), m.group(4)) if m else (name, "?", "?", "?", "?")))
    say()


def best(fn, reps=3):
    fn()
    ts = []
    for _ in range(reps):
        t = time.perf_counter()
        fn()
        ts.append((time.perf_counter() - t) * 1e3)
    return min(ts)


def main():
    resources()
    import sonic_amd as sonic
    from sonic_amd import _lib
    from util import big_circuit
    L = _lib.lib()
    _lib.check(L.sonic_init(0))

    def kernel_ms(name, fn):
        """best HIP-event time of one launch of `name` inside fn()"""
        L.sonic_profile_enable(1)
        try:
            vals = []
            for _ in range(3):
                L.sonic_profile_reset()
                fn()
                ms, cnt = C.c_double(0), C.c_int64(0)
                L.sonic_profile_get(name.encode(), C.byref(ms), C.byref(cnt))
                vals.append(ms.value / max(cnt.value, 1))
            return min(vals)
        finally:
            L.sonic_profile_enable(0)

    # ---- (a) ----
    say("## (a) decompress-and-validate against validate (ms; ratio = decompress / validate)")
    lg_max = 16 if QUICK else 20
    srs = sonic.SRS.new(1 << (lg_max - 1), 0x1234567, 0x7654321)
    pts = srs.points(0, -(1 << (lg_max - 1)), 1 << lg_max)
    srs.close()
    zs = sonic.g1_compress(pts)
    say("%-10s %14s %14s %7s %14s %14s %7s" % ("G1 points", "validate kern", "decompr kern", "ratio", "validate call", "decompr call", "ratio"))
    for lg in [10, 16] + ([] if QUICK else [20]):
        n = 1 << lg
        p, z, fl = pts[:n], zs[:n], np.zeros(n, np.uint8)
        val = lambda: _lib.check(L.sonic_g1_validate(p.ctypes.data, n, fl.ctypes.data))            # noqa: E731
        dec = lambda: sonic.g1_decompress(z, check_subgroup=True, flags=True)                      # noqa: E731
        assert bytes(sonic.g1_decompress(z)) == bytes(p)
        kv, kd, cv, cd = kernel_ms("k_g1_validate", val), kernel_ms("k_g1_decompress", dec), best(val), best(dec)
        say("2^%-8d %14.3f %14.3f %7.2f %14.3f %14.3f %7.2f" % (lg, kv, kd, kd / kv, cv, cd, cd / cv))
    del pts, zs
    srs = sonic.SRS.new(1 << 15, 0x1234567, 0x7654321)
    g2 = srs.g2_points(0, -(1 << 15), 1 << 16)
    srs.close()
    z2 = sonic.g2_compress(g2)
    say("%-10s %14s %14s %7s %14s" % ("G2 points", "from_bytes kern", "decompr kern", "ratio", "decompr call"))
    for lg in (10, 16):
        n = 1 << lg
        p, z = g2[:n], z2[:n]
        dec = lambda: sonic.g2_decompress(z, check_subgroup=True, flags=True)                      # noqa: E731
        assert bytes(sonic.g2_decompress(z)) == bytes(p)
        kv, kd = kernel_ms("k_g2_points_from_bytes", lambda: sonic.g2_compress(p)), kernel_ms("k_g2_decompress", dec)
        say("2^%-8d %14.3f %14.3f %7.2f %14.3f" % (lg, kv, kd, kd / kv, best(dec)))
    del g2, z2
    say()

    # ---- (b) ----
    d = 1 << (14 if QUICK else 18)
    say("## (b) SRS containers at d = 2^%d with the G2 half (one save and one load each; s)" % (d.bit_length() - 1))
    srs = sonic.SRS.new(d, 0xabcdef01, 0x10fedcba)
    srs.g2_points(0, 0, 1)                                     # the G2 half generated before the clock starts
    first = bytes(srs.points(0, -d, 8))
    say("%-12s %14s %10s %10s" % ("container", "bytes", "save", "load"))
    with tempfile.TemporaryDirectory() as tmp:
        for name, compressed in (("SONICSRS", False), ("SONICSRZ", True)):
            path = os.path.join(tmp, name)
            t0 = time.perf_counter()
            srs.save(path, g2=True, compressed=compressed)
            t1 = time.perf_counter()
            loaded = sonic.SRS.load(path)
            _lib.check(L.sonic_device_sync())
            t2 = time.perf_counter()
            assert bytes(loaded.points(0, -d, 8)) == first
            loaded.close()
            say("%-12s %14d %10.2f %10.2f" % (name, os.path.getsize(path), t1 - t0, t2 - t1))
            os.unlink(path)
    srs.close()
    say()

    # ---- (c) ----
    n, Q = 1 << (10 if QUICK else 14), 2
    Ks = [1, 64] + ([] if QUICK else [1024])
    say("## (c) verify_batch against verify_batch_z at n = 2^%d, Q = %d (ms per batch, fixed seed; ratio = _z / uncompressed)" % (n.bit_length() - 1, Q))
    pyr = random.Random(9)
    b = big_circuit(n + Q, n, Q)
    circuit = sonic.ArithCircuit(sonic.GateWeights(b["wL"], b["wR"], b["wO"]), b["cs"])
    srs = sonic.SRS.new(8 * n, pyr.randrange(2, R), pyr.randrange(2, R))
    prover = sonic.Prover(srs, circuit)
    prover.set_assignment(sonic.Assignment(b["aL"], b["aR"], b["aO"]))
    proofs, trs = [], []
    for _ in range(max(Ks)):
        tr = [pyr.randrange(1, R) for _ in range(8 + 2 * Q)]
        proofs.append(bytes(prover.prove_bytes(tr)))
        trs.append((tr[4], tr[5], list(zip(tr[6:6 + Q], tr[6 + Q:6 + 2 * Q]))))
    prover.close()
    comp = [sonic.proof_compress(p, Q) for p in proofs]
    ver = sonic.Verifier(srs, circuit)
    seed = bytes(range(32))
    say("%-6s %12s %12s %7s %16s %16s" % ("K", "verify_batch", "_z", "ratio", "k_g1_validate", "k_g1_decompress"))
    for K in Ks:
        plain = lambda: ver.verify_batch(proofs[:K], trs[:K], seed=seed)          # noqa: E731
        zform = lambda: ver.verify_batch(comp[:K], trs[:K], seed=seed)            # noqa: E731
        assert plain() is True and zform() is True
        tp, tz = best(plain), best(zform)
        say("%-6d %12.3f %12.3f %7.2f %16.3f %16.3f" % (K, tp, tz, tz / tp, kernel_ms("k_g1_validate", plain), kernel_ms("k_g1_decompress", zform)))
    ver.close()
    srs.close()
    if not QUICK:
        with open(os.path.join(ROOT, "profiles", "r09_compressed.txt"), "w") as f:
            f.write("\n".join(out_lines) + "\n")


if __name__ == "__main__":
    main()
