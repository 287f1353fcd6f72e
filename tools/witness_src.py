#!/usr/bin/env python3
"""Writes profiles/r12_witness_src.txt on one MI355X: what an assignment costs on its way into a prover handle, by where it comes from
(include/sonic_hip.h, "Witness sources").  Every line is measured in this one process on the same GPU and handles, beside the calls that
take three host buffers of canonical bytes, which are unchanged.

  (d)  VGPRs / SGPRs / scratch / occupancy / LDS of the four instantiations of k_witness_ingest (the compiler's remarks; needs no GPU)
  (a)  64 proofs at n = 2^16, Q = 2, two prepared handles, ms per batch: sonic_prove_batch with the assignment resident (the yardstick),
       sonic_prove_batch_statements from host buffers (the path before witness sources), and sonic_prove_batch_src from host / device
       memory, 32-byte elements / int64 with aO derived.  All rows prove the SAME 64 statements: aL, aR are non-negative 31-bit integers,
       so that one set of values has both encodings and aO = aL aR fits.
  (b)  setting one assignment at n = 2^14 and 2^18: sonic_prover_set_assignment against sonic_prover_set_witness from the four sources
  (c)  sonic_prover_eval_constraints over sixteen assignments at n = 2^18 against sonic_prover_eval_constraints_src from device memory

Run from the repository root after the library is built:  python tools/witness_src.py [--quick] [--resources]
Times are wall times of the C calls on prepared buffers, the best of five after one warm-up, with the spread (max - min) beside them."""
import ctypes as C
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
    say("## (d) k_witness_ingest<kind, aO given> (hipcc --offload-arch=gfx950 -O3 -Rpass-analysis=kernel-resource-usage)")
    say("%-34s %6s %6s %10s %10s %8s" % ("instantiation", "VGPRs", "SGPRs", "scratch B", "waves/SIMD", "LDS B"))
    err = subprocess.run(["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-Rpass-analysis=kernel-resource-usage", "-c",
                          os.path.join(CSRC, "witness_src.hip"), "-o", os.devnull], stderr=subprocess.PIPE, text=True).stderr
    for label, tag in (("FR32, aO given", "ILi0ELb1E"), ("FR32, aO derived", "ILi0ELb0E"), ("I64, aO given", "ILi1ELb1E"), ("I64, aO derived", "ILi1ELb0E")):
        m = re.search(r"Function Name: \S*k_witness_ingest%s\S*.*?TotalSGPRs: (\d+).*?VGPRs: (\d+).*?ScratchSize \[bytes/lane\]: (\d+).*?Occupancy \[waves/SIMD\]: (\d+).*?LDS Size \[bytes/block\]: (\d+)"
                      % tag, err, re.S)
        say("%-34s %6s %6s %10s %10s %8s" % ((label, m.group(2), m.group(1), m.group(3), m.group(4), m.group(5)) if m else (label, "?", "?", "?", "?", "?")))
    say("a block is 256 threads (four waves); per gate 96 bytes are read (24: int64 with aO derived) and 96 written, for three Montgomery products")
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


def small_assignments(rng, K, n):
    """K assignments in both encodings: int64 [K, n] (aL, aR in [0, 2^31), aO = aL aR) and canonical bytes uint8 [K, n, 32]"""
    i64 = [rng.integers(0, 1 << 31, size=(K, n), dtype=np.int64) for _ in range(2)]
    i64.append(i64[0] * i64[1])
    fr = []
    for a in i64:
        b = np.zeros((K, n, 32), np.uint8)
        b[:, :, :8] = a.astype("<i8").view(np.uint8).reshape(K, n, 8)
        fr.append(b)
    return i64, fr


def main():
    resources()
    if "--resources" in sys.argv:
        say("## (a), (b), (c): not collected yet (they need the GPU)")
        write()
        return
    import torch
    import sonic_amd as sonic
    from sonic_amd import _lib
    from sonic_amd.workload import big_circuit
    L = _lib.lib()
    _lib.check(L.sonic_init(0))
    pyr = random.Random(12)
    rng = np.random.default_rng(12)
    Q = 2
    FR32, I64 = _lib.WIT_FR32, _lib.WIT_I64
    ptr = lambda a: a.data_ptr() if hasattr(a, "data_ptr") else a.ctypes.data      # noqa: E731

    def source(vecs, kind, on_device, derived):
        return _lib.WitnessSrc(ptr(vecs[0]), ptr(vecs[1]), None if derived else ptr(vecs[2]), kind, on_device, 0, None), vecs

    def handles(lg, count, prepare):
        n = 1 << lg
        b = big_circuit(n + Q, n, Q)
        circuit = sonic.ArithCircuit(sonic.GateWeights(b["wL"], b["wR"], b["wO"]), b["cs"])
        srs = sonic.SRS.new(8 * n, pyr.randrange(2, R), pyr.randrange(2, R))
        return srs, [sonic.Prover(srs, circuit, prepare=prepare) for _ in range(count)]

    def four_sources(i64, fr):
        d64, dfr = [torch.from_numpy(a).cuda() for a in i64], [torch.from_numpy(a).cuda() for a in fr]
        torch.cuda.synchronize()
        return [("host, 32-byte elements, aO given", source(fr, FR32, 0, False)), ("host, int64, aO derived", source(i64, I64, 0, True)),
                ("device, 32-byte elements, aO given", source(dfr, FR32, 1, False)), ("device, int64, aO derived", source(d64, I64, 1, True))]

    verdicts = []

    # ---- (a) ----
    lg, K = (12, 8) if QUICK else (16, 64)
    n = 1 << lg
    say("## (a) %d proofs at n = 2^%d, Q = %d, two prepared handles (ms per batch)" % (K, lg, Q))
    srs, provers = handles(lg, 2, True)
    i64, fr = small_assignments(rng, K, n)
    srcs = four_sources(i64, fr)
    css = np.zeros((K, Q, 32), np.uint8)
    _lib.check(L.sonic_prover_eval_constraints_src(provers[0]._h, K, C.byref(srcs[3][1][0]), css.ctypes.data, None))
    trs = np.ascontiguousarray(np.stack([sonic.encoding.fr_array([pyr.randrange(1, R) for _ in range(8 + 2 * Q)]) for _ in range(K)]))
    psz = L.sonic_proof_size(Q)
    out = np.zeros((K, psz), np.uint8)
    status = (C.c_int * K)()
    arr = (C.c_void_p * 2)(*[p._h for p in provers])

    def resident():
        _lib.check(L.sonic_prove_batch(arr, 2, K, None, None, None, trs.ctypes.data, out.ctypes.data, status))

    def parent():
        _lib.check(L.sonic_prove_batch_statements(arr, 2, K, fr[0].ctypes.data, fr[1].ctypes.data, fr[2].ctypes.data, css.ctypes.data, trs.ctypes.data, out.ctypes.data, status))
    rows = []
    parent()
    ref = out.copy()
    for p in provers:                       # the resident yardstick proves statement 0 with every transcript
        one = _lib.WitnessSrc(i64[0].ctypes.data, i64[1].ctypes.data, None, I64, 0, 0, None)
        _lib.check(L.sonic_prover_set_witness(p._h, C.byref(one)))
        _lib.check(L.sonic_prover_set_constants(p._h, css[0].ctypes.data))
    rows.append(("sonic_prove_batch, assignment resident (yardstick)", timed(resident)))
    rows.append(("sonic_prove_batch_statements, host buffers (the path before)", timed(parent)))
    for name, (s, _keep) in srcs:
        def leg(s=s):
            _lib.check(L.sonic_prove_batch_src(arr, 2, K, C.byref(s), css.ctypes.data, trs.ctypes.data, out.ctypes.data, status))
        rows.append(("sonic_prove_batch_src, " + name, timed(leg)))
        assert (out == ref).all(), name                              # the same statements: the same proofs
    say("%-68s %10s %10s %10s %12s" % ("call", "best", "spread", "proofs/s", "/ yardstick"))
    yard = rows[0][1][0]
    for name, (t, s) in rows:
        say("%-68s %10.2f %10.2f %10.1f %12.3f" % (name, t, s, K / t * 1e3, t / yard))
    par = rows[1][1]
    for name, (t, s) in rows[4:]:
        verdicts.append(("(a) %s costs no more per batch than the host-buffer call beyond the larger spread (%.2f <= %.2f + %.2f)" % (name, t, par[0], max(s, par[1])),
                         t <= par[0] + max(s, par[1])))
    say("(the yardstick proves one resident statement %d times, once per transcript)" % K)
    say()
    for p in provers:
        p.close()
    srs.close()
    del srcs

    # ---- (b) ----
    for lg in ([10, 12] if QUICK else [14, 18]):
        n = 1 << lg
        say("## (b) setting one assignment, n = 2^%d (ms per call, the call returns when the assignment is resident and checked)" % lg)
        srs, (p,) = handles(lg, 1, False)
        i64, fr = small_assignments(rng, 1, n)
        i64, fr = [a[0] for a in i64], [a[0] for a in fr]
        say("%-58s %10s %10s" % ("call", "best", "spread"))
        t, s = timed(lambda: _lib.check(L.sonic_prover_set_assignment(p._h, fr[0].ctypes.data, fr[1].ctypes.data, fr[2].ctypes.data)))
        say("%-58s %10.3f %10.3f" % ("sonic_prover_set_assignment (host, 32-byte elements)", t, s))
        for name, (sv, _keep) in four_sources(i64, fr):
            t, s = timed(lambda sv=sv: _lib.check(L.sonic_prover_set_witness(p._h, C.byref(sv))))
            say("%-58s %10.3f %10.3f" % ("sonic_prover_set_witness, " + name, t, s))
        say()
        if lg != (12 if QUICK else 18):
            p.close()
            srs.close()

    # ---- (c) on the handle of the last size ----
    B = 16
    say("## (c) eval_constraints, %d assignments at n = 2^%d (ms per call; out_gates requested)" % (B, lg))
    i64, fr = small_assignments(rng, B, n)
    want, got = np.zeros((B, Q, 32), np.uint8), np.zeros((B, Q, 32), np.uint8)
    g0, g1 = np.zeros((B, 2), np.int64), np.zeros((B, 2), np.int64)
    say("%-58s %10s %10s" % ("call", "best", "spread"))
    t, s = timed(lambda: _lib.check(L.sonic_prover_eval_constraints(p._h, B, fr[0].ctypes.data, fr[1].ctypes.data, fr[2].ctypes.data, want.ctypes.data, g0.ctypes.data)))
    say("%-58s %10.3f %10.3f" % ("sonic_prover_eval_constraints (host, 32-byte elements)", t, s))
    for name, (sv, _keep) in four_sources(i64, fr):
        t, s = timed(lambda sv=sv: _lib.check(L.sonic_prover_eval_constraints_src(p._h, B, C.byref(sv), got.ctypes.data, g1.ctypes.data)))
        assert (got == want).all() and (g1 == g0).all(), name
        say("%-58s %10.3f %10.3f" % ("sonic_prover_eval_constraints_src, " + name, t, s))
    say()
    p.close()
    srs.close()
    say("## what has to hold, against the unchanged host-buffer call in this run")
    for text, ok in verdicts:
        say("%s  %s" % ("HOLDS" if ok else "FAILS", text))
    if not QUICK:
        write()


def write():
    with open(os.path.join(ROOT, "profiles", "r12_witness_src.txt"), "w") as f:
        f.write("\n".join(out_lines) + "\n")


if __name__ == "__main__":
    main()
