#!/usr/bin/env python3
"""Writes profiles/r21_r1cs.txt on one MI355X: what the R1CS front end costs, and what a circuit made by it costs the layers behind it
(include/sonic_hip.h, "R1CS front end").  One process, one GPU; no thresholds -- the figures are the record.

  (d)  VGPRs / SGPRs / scratch / occupancy / LDS of the new kernels (the compiler's remarks; needs no GPU)
  (a)  sonic_r1cs_assign alone at m = 2^12 and 2^16 (three entries per row on average plus one row over all columns), K = 1 and 16, z
       resident on the device: ms per call, the same call per kernel, and beside it on the same witnesses the Python-integer model and
       sonic_prover_eval_constraints_src of the compiled circuit, the nearest existing kernel (m = 2^12 only: see (b) for why)
  (b)  one circuit made from R1CS at m = 2^12: compile time, sonic_prover_new_csr time, the handle's device memory, ms per core proof one
       at a time and streamed; beside them workload.sparse_circuit at the same n and about the same nnz with Q = 64
  (c)  fs_circuit_midstate and Verifier(...) construction for the circuit of (b): the two costs that grow as Q n

Run from the repository root after the library is built:  python tools/r1cs.py [--quick] [--resources]
Times are wall times of the calls on prepared buffers, the best of five after one warm-up, with the spread (max - min) beside them."""
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
sys.path.insert(0, os.path.join(ROOT, "tests"))
CSRC = os.path.join(ROOT, "sonic_amd", "csrc")
R = 0x73EDA753299D7D483339D80809A1D80553BDA402FFFE5BFEFFFFFFFF00000001
QUICK = "--quick" in sys.argv
out_lines = []


def say(line=""):
    print(line, flush=True)
    out_lines.append(line)


def write():
    with open(os.path.join(ROOT, "profiles", "r21_r1cs.txt"), "w") as f:
        f.write("\n".join(out_lines) + "\n")


def resources():
    say("## (d) the kernels of r1cs.hip (hipcc --offload-arch=gfx950 -O3 -Rpass-analysis=kernel-resource-usage)")
    say("%-34s %6s %6s %10s %10s %8s" % ("kernel", "VGPRs", "SGPRs", "scratch B", "waves/SIMD", "LDS B"))
    err = subprocess.run(["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-Rpass-analysis=kernel-resource-usage", "-c",
                          os.path.join(CSRC, "r1cs.hip"), "-o", os.devnull], stderr=subprocess.PIPE, text=True).stderr
    for label, tag in (("k_r1cs_ingest<FR32>", r"k_r1cs_ingestILi0E"), ("k_r1cs_ingest<I64>", r"k_r1cs_ingestILi1E"), ("k_r1cs_short", "k_r1cs_short"),
                       ("k_r1cs_long", "k_r1cs_long"), ("k_r1cs_fill", "k_r1cs_fill")):
        m = re.search(r"Function Name: \S*%s\S*.*?TotalSGPRs: (\d+).*?VGPRs: (\d+).*?ScratchSize \[bytes/lane\]: (\d+).*?Occupancy \[waves/SIMD\]: (\d+).*?LDS Size \[bytes/block\]: (\d+)"
                      % tag, err, re.S)
        say("%-34s %6s %6s %10s %10s %8s" % ((label, m.group(2), m.group(1), m.group(3), m.group(4), m.group(5)) if m else (label, "?", "?", "?", "?", "?")))
    say("a block is 256 threads (four waves); no kernel uses scratch.  One thread carries one witness; carrying two or four (8 VGPRs per")
    say("accumulator, each val load reused) has not been measured")
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


def chain_system(rng, n_in, m):
    """a system every choice of inputs satisfies: z = (1, n_in inputs, m products), row i: <a, z> <b, z> = z[1 + n_in + i] over earlier
    columns, one or two entries in a and in b (three per row with c, on average) -- and the last row's a runs over all earlier columns"""
    N = 1 + n_in + m
    A, B, C = [], [], []
    for i in range(m):
        top = 1 + n_in + i
        ca = sorted(rng.sample(range(top), rng.choice([1, 1, 2]))) if i < m - 1 else list(range(top))
        cb = sorted(rng.sample(range(top), rng.choice([1, 1, 2])))
        A.append([(j, rng.choice([1, R - 1, rng.randrange(R)])) for j in ca])
        B.append([(j, rng.choice([1, R - 1, rng.randrange(R)])) for j in cb])
        C.append([(top, 1)])

    def solve(inputs):
        z = [1] + [v % R for v in inputs]
        for i in range(m):
            z.append(sum(v * z[j] for j, v in A[i]) * sum(v * z[j] for j, v in B[i]) % R)
        return z
    return N, A, B, C, solve


def csr(M):
    from sonic_amd.encoding import fr_array
    rp = np.zeros(len(M) + 1, np.int64)
    rp[1:] = np.cumsum([len(r) for r in M])
    return rp, np.array([j for r in M for j, _ in r], np.int64), fr_array([v for r in M for _, v in r])


def fr_rows(zs):
    return np.frombuffer(b"".join(v.to_bytes(32, "little") for z in zs for v in z), np.uint8).reshape(len(zs), len(zs[0]), 32).copy()


def main():
    resources()
    if "--resources" in sys.argv:
        say("## (a), (b), (c): not collected (they need the GPU)")
        write()
        return
    import torch
    import sonic_amd as sonic
    from sonic_amd import _lib, workload
    import r1cs_ref as ref
    L = _lib.lib()
    _lib.check(L.sonic_init(0))
    rng = random.Random(21)
    free = lambda: torch.cuda.mem_get_info()[0]      # noqa: E731
    kept = {}

    # ---- (a) ----
    for lg in ([8, 10] if QUICK else [12, 16]):
        m, n_in, n_pub = 1 << lg, 64, 2
        N, A, B, Cm, solve = chain_system(rng, n_in, m)
        t0 = time.perf_counter()
        r = sonic.R1CS(m, N, n_pub, csr(A), csr(B), csr(Cm))
        t_new = (time.perf_counter() - t0) * 1e3
        say("## (a) sonic_r1cs_assign, m = 2^%d, N = %d, n = %d, Q = %d, %d entries in A, B, C (the longest row: %d); handle made in %.1f ms" %
            (lg, N, r.n, r.Q, sum(len(x) for M in (A, B, Cm) for x in M), N - 1, t_new))
        zs = [solve([rng.randrange(R) for _ in range(n_in)]) for _ in range(16)]
        zd = torch.from_numpy(fr_rows(zs)).cuda()
        planes = [torch.empty((16, r.n, 32), dtype=torch.uint8, device="cuda") for _ in range(3)]
        cs, bad = np.zeros((16, r.Q, 32), np.uint8), np.zeros((16, 2), np.int64)
        torch.cuda.synchronize()

        def call(K):
            _lib.check(L.sonic_r1cs_assign(r._h, K, zd.data_ptr(), 0, 1, 0, None, planes[0].data_ptr(), planes[1].data_ptr(), planes[2].data_ptr(), 0, cs.ctypes.data, bad.ctypes.data))
        say("%-58s %10s %10s" % ("call", "best ms", "spread"))
        for K in (1, 16):
            t, s = timed(lambda K=K: call(K))
            say("%-58s %10.3f %10.3f" % ("sonic_r1cs_assign, K = %d, z on the device (FR32)" % K, t, s))
            assert (bad[:K] == np.array([0, -1])).all()
            L.sonic_profile_reset()
            L.sonic_profile_enable(1)
            call(K)
            L.sonic_profile_enable(0)
            names = C.create_string_buffer(1 << 16)
            L.sonic_profile_names(names, 1 << 16)
            for name in names.value.decode().split("\n"):
                if "r1cs" in name:
                    ms, launches = C.c_double(), C.c_int64()
                    L.sonic_profile_get(name.encode(), C.byref(ms), C.byref(launches))
                    say("%-58s %10.3f %10s" % ("    " + name + " (%d launches, HIP events)" % launches.value, ms.value, ""))
        rows = [[sorted(x) for x in M] for M in (A, B, Cm)]
        t0 = time.perf_counter()
        want = ref.assign(m, N, n_pub, rows[0], rows[1], rows[2], zs[0])
        say("%-58s %10.1f %10s" % ("the Python-integer model (tests/r1cs_ref.py), one witness", (time.perf_counter() - t0) * 1e3, ""))
        assert planes[0][0].cpu().numpy().tobytes() == b"".join(v.to_bytes(32, "little") for v in want[0]) and cs[0].tobytes() == b"".join(v.to_bytes(32, "little") for v in want[3])
        if lg == (10 if QUICK else 12):
            kept = dict(r=r, m=m, N=N, zs=zs, planes=planes, cs=cs.copy())
        else:
            say("(no sonic_prover_eval_constraints_src beside it at this size: a prover handle for Q = %d, n = %d would need Q (3n + 1) 32 B = %.0f GB)" %
                (r.Q, r.n, r.Q * (3 * r.n + 1) * 32 / 1e9))
            r.close()
        say()

    # ---- (b) ----
    r, m, N, zs, planes = kept["r"], kept["m"], kept["N"], kept["zs"], kept["planes"]
    n, Q = r.n, r.Q
    say("## (b) the circuit made from the R1CS of (a) at m = %d: n = %d, Q = %d, nnz = %d" % (m, n, Q, r.nnz))
    t0 = time.perf_counter()
    circuit = r.circuit(public=zs[0][1:3])
    say("%-66s %10.1f ms" % ("compile (sonic_r1cs_circuit, host)", (time.perf_counter() - t0) * 1e3))
    srs = sonic.SRS.new(7 * n + 64, rng.randrange(2, R), rng.randrange(2, R))
    torch.cuda.synchronize()
    f0 = free()
    t0 = time.perf_counter()
    p = sonic.Prover(srs, circuit, prepare=False)
    torch.cuda.synchronize()
    say("%-66s %10.1f ms" % ("sonic_prover_new_csr", (time.perf_counter() - t0) * 1e3))
    say("%-66s %10.2f GB   (Q (3n + 1) 32 B = %.2f GB)" % ("the handle's device memory (free memory before - after)", (f0 - free()) / 1e9, Q * (3 * n + 1) * 32 / 1e9))
    wb = sonic.WitnessBatch(planes[0], planes[1], planes[2])
    cs_ints = [[int.from_bytes(kept["cs"][k, q].tobytes(), "little") for q in range(Q)] for k in range(16)]
    trs = [[rng.randrange(1, R) for _ in range(6)] for _ in range(16)]
    t, s = timed(lambda: sonic.Prover.eval_constraints(p, sonic.WitnessBatch(planes[0][:1], planes[1][:1], planes[2][:1])))
    say("%-66s %10.3f ms  spread %.3f   (beside (a), K = 1)" % ("sonic_prover_eval_constraints_src of the compiled circuit, K = 1", t, s))
    t, s = timed(lambda: sonic.Prover.eval_constraints(p, wb))
    say("%-66s %10.3f ms  spread %.3f   (beside (a), K = 16)" % ("sonic_prover_eval_constraints_src of the compiled circuit, K = 16", t, s))
    p.set_witness(planes[0][0], planes[1][0], planes[2][0])
    p.set_constants(cs_ints[0])
    core = p.prove_core_bytes(trs[0])
    assert sonic.verify_core(srs, circuit, core, trs[0][4], trs[0][5])
    t, s = timed(lambda: p.prove_core_bytes(trs[0]))
    say("%-66s %10.2f ms  spread %.2f" % ("core proof, one at a time (sonic_prover_prove_core)", t, s))
    t, s = timed(lambda: sonic.prove_core_batch([p], trs, wb, constants=cs_ints))
    say("%-66s %10.2f ms  spread %.2f   (16 proofs per call, one handle)" % ("core proof, streamed (sonic_prove_batch_core_src), per proof", t / 16, s / 16))
    per = max(1, round(r.nnz / (3 * 64)))
    w = workload.sparse_circuit(21, n, 64, per)
    sp = sonic.SparseCircuit(n, 64, w["row_ptr"], w["col"], w["val"], w["cs"])
    f0 = free()
    p2 = sonic.Prover(srs, sp, prepare=False)
    torch.cuda.synchronize()
    mem2 = (f0 - free()) / 1e9
    p2.set_assignment(sonic.Assignment(w["aL"], w["aR"], w["aO"]))
    t, s = timed(lambda: p2.prove_core_bytes(trs[0]))
    say("%-66s %10.2f ms  spread %.2f   (n = %d, Q = 64, nnz = %d, handle %.2f GB)" % ("core proof of workload.sparse_circuit, one at a time", t, s, n, w["nnz"], mem2))
    p2.close()
    say()

    # ---- (c) ----
    say("## (c) the two costs that grow as Q n, for the circuit of (b) (96 Q n = %.2f GB hashed)" % (96 * Q * n / 1e9))
    t0 = time.perf_counter()
    sonic.fs_circuit_midstate(circuit)
    say("%-66s %10.1f ms" % ("fs_circuit_midstate (sonic_fs_circuit_midstate_csr, host)", (time.perf_counter() - t0) * 1e3))
    f0 = free()
    t0 = time.perf_counter()
    v = sonic.Verifier(srs, circuit)
    torch.cuda.synchronize()
    say("%-66s %10.1f ms   (device memory %.2f GB)" % ("Verifier(srs, circuit) (sonic_verifier_new_csr)", (time.perf_counter() - t0) * 1e3, (f0 - free()) / 1e9))
    v.close()
    p.close()
    srs.close()
    r.close()
    if not QUICK:
        write()


if __name__ == "__main__":
    main()
