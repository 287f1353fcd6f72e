#!/usr/bin/env python3
"""Writes profiles/r22_large_q.txt on one MI355X: what a circuit with Q ~ n (a compiled R1CS) costs the digests, the handles and a core
proof, this build against another build of the library (include/sonic_hip.h, "Circuits with Q ~ n").

  (a)  compiled R1CS at m = 2^12, N = 4161 (the shape of profiles/r21_r1cs.txt), in this process: sonic_fs_circuit_midstate_csr, the host
       sonic_fs_weights_digest_v2_csr, Verifier.weights_digest_v2(), and Verifier(...) construction with digest=1 and digest=2
  (b)  Prover(..., prepare=False) at the same shape: construction time and device memory, this build against the baseline
       (--baseline-lib); device_bytes where the build has it, the free-memory difference for both
  (c)  a core proof on that handle, one at a time and streamed (16 per call), both builds, and beside them workload.sparse_circuit at the
       same n with Q = 64.  The condition: this build is faster than the baseline by more than the larger spread on both legs.
  (d)  m = 2^15, N ~ m, this build only: handle, assign, prove_core_fs under circuit digest v2, Verifier(digest=2).verify_core_fs_batch;
       a step that cannot run is recorded with its message
  (e)  the compiler's account of the new kernels (-Rpass-analysis=kernel-resource-usage; needs no GPU)

(b), (c) and (d) run in fresh child processes, each under its own `timeout -k 10`; the baseline's children load it through SONIC_HIP_LIB.
A baseline from before this commit has to lie in a copy of its own package (PATH = .../sonic_amd/csrc/libsonic_hip.so): its children
import that copy's Python, since this tree's loader refuses a library without the new symbols.  Times in this process are the best of
--rounds after a warm-up; the children alternate baseline / this build for --rounds rounds (each child: a warm-up, then the best of
three), and the figure is the best round with spread = max - min over the rounds.  The first child that fails ends (b) and (c).

    python tools/large_q.py [--baseline-lib PATH] [--rounds 5] [--quick] [--resources-only] [--skip-d]
"""
import argparse
import json
import os
import random
import re
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "sonic_amd", "csrc")
R = 0x73EDA753299D7D483339D80809A1D80553BDA402FFFE5BFEFFFFFFFF00000001
out_lines = []


def say(line=""):
    print(line, flush=True)
    out_lines.append(line)


def write():
    with open(os.path.join(ROOT, "profiles", "r22_large_q.txt"), "w") as f:
        f.write("\n".join(out_lines) + "\n")


# ---- (e) ---------------------------------------------------------------------------------------------------------------------------------
def resources():
    say("## (e) the kernels of weights_digest.hip (hipcc --offload-arch=gfx950 -O3 -Rpass-analysis=kernel-resource-usage)")
    say("%-22s %6s %6s %10s %12s %8s %12s" % ("kernel", "VGPRs", "SGPRs", "scratch B", "waves/SIMD", "LDS B", "SGPR spills"))
    err = subprocess.run(["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-Rpass-analysis=kernel-resource-usage", "-c",
                          os.path.join(CSRC, "weights_digest.hip"), "-o", os.devnull], stderr=subprocess.PIPE, text=True).stderr
    for name in ("k_weights_leaves", "k_weights_nodes"):
        m = re.search(r"Function Name: \S*%s\S*.*?TotalSGPRs: (\d+).*?VGPRs: (\d+).*?ScratchSize \[bytes/lane\]: (\d+).*?Occupancy \[waves/SIMD\]: (\d+).*?SGPRs Spill: (\d+).*?LDS Size \[bytes/block\]: (\d+)"
                      % name, err, re.S)
        say("%-22s %6s %6s %10s %12s %8s %12s" % ((name, m.group(2), m.group(1), m.group(3), m.group(4), m.group(6), m.group(5)) if m else (name, "?", "?", "?", "?", "?", "?")))
    say("a block is one wave (64 threads), one digest per thread; no scratch memory.  What bounds the kernels has not been measured here:")
    say("(a) gives their wall time inside Verifier.weights_digest_v2() only")
    say()


# ---- the circuit ------------------------------------------------------------------------------------------------------------------------
def chain_system(rng, n_in, m):
    """tools/r1cs.py's system: z = (1, n_in inputs, m products), row i: <a, z> <b, z> = z[1 + n_in + i] over earlier columns, one or two
    entries in a and in b, and the last row's a runs over all earlier columns"""
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


def compiled(lg, K):
    """(R1CS handle, circuit for witness 0, K witnesses as a [K, N, 32] array, srs): the same system on every side (seeded)"""
    import sonic_amd as sonic
    rng = random.Random(22 + lg)
    m, n_in, n_pub = 1 << lg, 64, 2
    N, A, B, Cm, solve = chain_system(rng, n_in, m)
    r = sonic.R1CS(m, N, n_pub, csr(A), csr(B), csr(Cm))
    zs = [solve([rng.randrange(R) for _ in range(n_in)]) for _ in range(K)]
    za = np.frombuffer(b"".join(v.to_bytes(32, "little") for z in zs for v in z), np.uint8).reshape(K, N, 32).copy()
    circuit = r.circuit(public=zs[0][1:3])
    srs = sonic.SRS.new(7 * r.n + 64, 0x1234567, 0x7654321)
    return r, circuit, za, srs


def timed(fn, reps):
    fn()
    ts = []
    for _ in range(reps):
        t = time.perf_counter()
        fn()
        ts.append((time.perf_counter() - t) * 1e3)
    return min(ts), max(ts) - min(ts)


# ---- (a) ---------------------------------------------------------------------------------------------------------------------------------
def part_a(lg, rounds):
    import torch
    import sonic_amd as sonic
    from sonic_amd import _lib
    _lib.check(_lib.lib().sonic_init(0))
    r, circuit, _za, srs = compiled(lg, 1)
    n, Q = r.n, r.Q
    say("## (a) the digests of a compiled R1CS, m = 2^%d: n = %d, Q = %d, nnz = %d (96 Q n = %.2f GB of dense bytes; the entries are %.2f MB)" %
        (lg, n, Q, circuit.nnz, 96 * Q * n / 1e9, 72 * circuit.nnz / 1e6))
    say("%-72s %12s %10s" % ("call (ms: best of %d after a warm-up, spread = max - min)" % rounds, "best", "spread"))
    held = {}

    def row(label, fn):
        t, s = timed(fn, rounds)
        held[label] = t
        say("%-72s %12.3f %10.3f" % (label, t, s))
    row("sonic_fs_circuit_midstate_csr (host, v1: 96 Q n bytes)", lambda: sonic.fs_circuit_midstate(circuit))
    row("sonic_fs_weights_digest_v2_csr (host, v2: the entries)", lambda: sonic.fs_weights_digest_v2(circuit))
    v = sonic.Verifier(srs, circuit, digest=2)
    wd = sonic.fs_weights_digest_v2(circuit)
    assert v.weights_digest_v2() == wd
    L = _lib.lib()
    v1 = []

    def make(kind):
        h = sonic.Verifier(srs, circuit, digest=kind)
        torch.cuda.synchronize()
        v1.append(h)
        while len(v1) > 1:
            v1.pop(0).close()
    row("Verifier(srs, circuit, digest=1) (sonic_verifier_new_csr)", lambda: make(1))
    row("Verifier(srs, circuit, digest=2) (sonic_verifier_new_digest)", lambda: make(2))
    # Verifier.weights_digest_v2() on a kind-1 handle computes the tree on its first call: a fresh handle per repetition is 17 s each, so
    # the call is timed through the kernels' HIP events on one handle instead, plus the wall time of that one first call
    h = sonic.Verifier(srs, circuit, digest=1)
    torch.cuda.synchronize()
    L.sonic_profile_reset(); L.sonic_profile_enable(1)
    t0 = time.perf_counter()
    assert h.weights_digest_v2() == wd
    wall = (time.perf_counter() - t0) * 1e3
    L.sonic_profile_enable(0)
    import ctypes as C
    for name in ("k_weights_leaves", "k_weights_nodes"):
        ms, launches = C.c_double(), C.c_int64()
        L.sonic_profile_get(name.encode(), C.byref(ms), C.byref(launches))
        say("%-72s %12.3f %10s" % ("    %s (%d launches, HIP events, one call)" % (name, launches.value), ms.value, ""))
    say("%-72s %12.3f %10s" % ("Verifier.weights_digest_v2(), first call on a kind-1 handle (with event timing on)", wall, ""))
    h.close()
    for x in v1:
        x.close()
    v.close(); srs.close(); r.close()
    say()
    return held


# ---- (b), (c), (d): the children -------------------------------------------------------------------------------------------------------------
def child_handle(lg):
    """(b) and (c) for one build"""
    import torch
    import sonic_amd as sonic
    from sonic_amd import _lib, workload
    _lib.check(_lib.lib().sonic_init(0))
    K = 16
    r, circuit, za, srs = compiled(lg, K)
    n, Q = r.n, r.Q
    wb, cs, bad = r.assign(torch.from_numpy(za).cuda())
    assert bad == [(0, -1)] * K
    torch.cuda.synchronize()
    free = lambda: torch.cuda.mem_get_info()[0]      # noqa: E731
    res = {"n": n, "Q": Q}
    f0 = free()
    t0 = time.perf_counter()
    p = sonic.Prover(srs, circuit, prepare=False)
    torch.cuda.synchronize()
    res["construct_ms"] = (time.perf_counter() - t0) * 1e3
    res["free_diff_gb"] = (f0 - free()) / 1e9
    res["device_bytes_gb"] = p.device_bytes / 1e9 if hasattr(p, "device_bytes") else None
    rng = random.Random(5)
    trs = [[rng.randrange(1, R) for _ in range(6)] for _ in range(K)]
    p.set_witness(wb.aL[0], wb.aR[0], wb.aO[0])
    p.set_constants(cs[0])
    core = p.prove_core_bytes(trs[0])
    assert sonic.verify_core(srs, circuit, core, trs[0][4], trs[0][5])
    res["core_one_ms"] = timed(lambda: p.prove_core_bytes(trs[0]), 3)[0]
    res["core_streamed_ms"] = timed(lambda: sonic.prove_core_batch([p], trs, wb, constants=cs), 3)[0] / K
    res["device_bytes_after_gb"] = p.device_bytes / 1e9 if hasattr(p, "device_bytes") else None
    res["free_diff_after_gb"] = (f0 - free()) / 1e9
    # one more core proof with SONIC_DEBUG_TIMING=1 (read per proof): the library says on stderr how long the enqueue took on the host
    # and how long it then waited for the device; run_child reads the line behind the marker
    os.environ["SONIC_DEBUG_TIMING"] = "1"
    print("[large_q] compiled", file=sys.stderr, flush=True)
    p.prove_core_bytes(trs[0])
    os.environ.pop("SONIC_DEBUG_TIMING")
    p.close()
    w = workload.sparse_circuit(21, n, 64, max(1, round(r.nnz / (3 * 64))))
    sp = sonic.SparseCircuit(n, 64, w["row_ptr"], w["col"], w["val"], w["cs"])
    p2 = sonic.Prover(srs, sp, prepare=False)
    p2.set_assignment(sonic.Assignment(w["aL"], w["aR"], w["aO"]))
    res["q64_one_ms"] = timed(lambda: p2.prove_core_bytes(trs[0]), 3)[0]
    os.environ["SONIC_DEBUG_TIMING"] = "1"
    print("[large_q] q64", file=sys.stderr, flush=True)
    p2.prove_core_bytes(trs[0])
    os.environ.pop("SONIC_DEBUG_TIMING")
    p2.close()
    return res


def child_big(lg):
    """(d): every step timed; the first step that fails is recorded with its message and ends the child"""
    import torch
    import sonic_amd as sonic
    from sonic_amd import _lib
    _lib.check(_lib.lib().sonic_init(0))
    steps = []
    state = {}

    def step(label, fn):
        t0 = time.perf_counter()
        try:
            fn()
            torch.cuda.synchronize()
        except Exception as e:      # noqa: BLE001  (the message is the record)
            steps.append((label, None, "%s: %s" % (type(e).__name__, str(e)[:300])))
            return False
        steps.append((label, (time.perf_counter() - t0) * 1e3, ""))
        return True

    def build():
        state["r"], state["circuit"], state["za"], state["srs"] = compiled(lg, 1)
    free = lambda: torch.cuda.mem_get_info()[0]      # noqa: E731

    def handle():
        f0 = free()
        state["p"] = sonic.Prover(state["srs"], state["circuit"], prepare=False)
        torch.cuda.synchronize()
        state["mem"] = (state["p"].device_bytes / 1e9, (f0 - free()) / 1e9)

    def assign():
        state["wb"], state["cs"], bad = state["r"].assign(torch.from_numpy(state["za"]).cuda())
        assert bad == [(0, -1)]
        state["p"].set_witness(state["wb"].aL[0], state["wb"].aR[0], state["wb"].aO[0])
        state["p"].set_constants(state["cs"][0])

    def digests():
        state["wd2"] = state["p"].weights_digest_v2()
        state["cd2"] = sonic.fs_circuit_digest_v2(state["wd2"], state["cs"][0])

    def prove():
        state["proof"] = state["p"].prove_core_fs(state["cd2"], b"\x11" * 32)

    def prove_again():
        state["p"].prove_core_fs(state["cd2"], b"\x12" * 32)

    def verifier():
        state["v"] = sonic.Verifier(state["srs"], state["circuit"], digest=2)

    def verify():
        ok, each = state["v"].verify_core_fs_batch([state["proof"][0]], seed=b"\x13" * 32, each=True, constants=[state["cs"][0]])
        assert ok and each == [True], (ok, each)
    for label, fn in (("the system, its R1CS handle, the compiled circuit and the SRS (host Python included)", build),
                      ("Prover(srs, circuit, prepare=False)", handle), ("R1CS.assign (1 witness), set_witness, set_constants", assign),
                      ("Prover.weights_digest_v2() and fs_circuit_digest_v2", digests), ("prove_core_fs under circuit digest v2 (first)", prove),
                      ("prove_core_fs under circuit digest v2 (second)", prove_again), ("Verifier(srs, circuit, digest=2)", verifier),
                      ("verify_core_fs_batch, K = 1, constants given: accepted", verify)):
        if not step(label, fn):
            break
    r = state.get("r")
    return {"steps": steps, "n": r.n if r else None, "Q": r.Q if r else None, "nnz": state["circuit"].nnz if "circuit" in state else None, "mem": state.get("mem")}


CHILDREN = {"handle": child_handle, "big": child_big}


def run_child(kind, lib, lg, limit):
    env = dict(os.environ)
    if lib:
        env["SONIC_HIP_LIB"] = lib
    else:
        env.pop("SONIC_HIP_LIB", None)
    cmd = ["timeout", "-k", "10", str(limit), sys.executable, os.path.abspath(__file__), "--child", kind, "--lg", str(lg)]
    pkg = os.path.dirname(os.path.dirname(os.path.dirname(lib))) if lib else None
    if pkg and os.path.exists(os.path.join(pkg, "sonic_amd", "__init__.py")):
        cmd += ["--pkg-root", pkg]
    t0 = time.perf_counter()
    out = subprocess.run(cmd, env=env, capture_output=True, text=True)
    print("  [%s, %s: %.0f s]" % (kind, "baseline" if lib else "this build", time.perf_counter() - t0), flush=True)
    if out.returncode != 0:
        return None, "status %d: %s" % (out.returncode, (out.stdout[-600:] + out.stderr[-1500:]).strip())
    res = json.loads(out.stdout.strip().splitlines()[-1])
    for tag in ("compiled", "q64"):      # (child_handle: the SONIC_DEBUG_TIMING line of one core proof on each handle)
        m = re.search(r"\[large_q\] %s\s.*?enqueue ([0-9.]+) ms, then waited ([0-9.]+) ms" % tag, out.stderr, re.S)
        if m and isinstance(res, dict):
            res["%s_enqueue_ms" % tag], res["%s_wait_ms" % tag] = float(m.group(1)), float(m.group(2))
    return res, ""


def part_bc(baseline, lg, rounds):
    say("## (b), (c) Prover(..., prepare=False) and core proofs at m = 2^%d: the baseline library against this build, fresh processes, alternating" % lg)
    say("(best of %d rounds, spread = max - min over the rounds; a child times each call as the best of three after a warm-up)" % rounds)
    rows = {"baseline": [], "this": []}
    for _ in range(rounds):
        for side, lib in (("baseline", baseline), ("this", None)):
            res, msg = run_child("handle", lib, lg, 600)
            if res is None:
                say("child (%s) failed, nothing more is started: %s" % (side, msg))
                say()
                return None
            rows[side].append(res)
    n, Q = rows["this"][0]["n"], rows["this"][0]["Q"]
    say("n = %d, Q = %d; Q (3n + 1) 32 B = %.2f GB" % (n, Q, Q * (3 * n + 1) * 32 / 1e9))
    say("%-58s %12s %10s %12s %10s %8s" % ("", "baseline", "spread", "this build", "spread", "ratio"))
    stats = {}
    for key, label in (("construct_ms", "(b) construction (ms)"), ("free_diff_gb", "(b) device memory, free before - after (GB)"),
                       ("device_bytes_gb", "(b) device_bytes of the fresh handle (GB)"), ("device_bytes_after_gb", "    device_bytes after the core proofs (GB)"),
                       ("free_diff_after_gb", "    free-memory difference after the core proofs (GB)"),
                       ("core_one_ms", "(c) core proof, one at a time (ms)"), ("core_streamed_ms", "(c) core proof, streamed, per proof (ms)"),
                       ("q64_one_ms", "(c) workload.sparse_circuit, same n, Q = 64, one at a time (ms)"),
                       ("compiled_enqueue_ms", "    SONIC_DEBUG_TIMING, one core proof: host enqueue (ms)"),
                       ("compiled_wait_ms", "    SONIC_DEBUG_TIMING, one core proof: then waited for the device (ms)"),
                       ("q64_enqueue_ms", "    the same at Q = 64: host enqueue (ms)"), ("q64_wait_ms", "    the same at Q = 64: waited for the device (ms)")):
        if any(key not in x for x in rows["baseline"] + rows["this"]):
            continue
        b, t = [x[key] for x in rows["baseline"]], [x[key] for x in rows["this"]]
        if any(v is None for v in b):
            say("%-58s %12s %10s %12.3f %10.3f %8s" % (label, "-", "-", min(t), max(t) - min(t), "-"))
            continue
        stats[key] = (min(b), max(b) - min(b), min(t), max(t) - min(t))
        say("%-58s %12.3f %10.3f %12.3f %10.3f %8.2f" % (label, min(b), max(b) - min(b), min(t), max(t) - min(t), min(b) / min(t) if min(t) > 0 else float("nan")))
    holds = all(stats[k][0] - stats[k][2] > max(stats[k][1], stats[k][3]) for k in ("core_one_ms", "core_streamed_ms"))
    say("condition (c): this build is %s the baseline by more than the larger spread on both legs (ratios %.2f and %.2f)" %
        ("faster than" if holds else "NOT faster than", stats["core_one_ms"][0] / stats["core_one_ms"][2], stats["core_streamed_ms"][0] / stats["core_streamed_ms"][2]))
    say()
    return holds


def part_d(lg):
    say("## (d) m = 2^%d, N ~ m, this build only (one fresh process; wall times of single calls, no repetition)" % lg)
    res, msg = run_child("big", None, lg, 1100)
    if res is None:
        say("the child did not finish: %s" % msg)
        say()
        return
    say("n = %s, Q = %s, nnz = %s; the fresh handle: device_bytes %s GB, free-memory difference %s GB" %
        (res["n"], res["Q"], res["nnz"], *(("%.2f" % v for v in res["mem"]) if res["mem"] else ("?", "?"))))
    for label, ms, err in res["steps"]:
        say("%-88s %s" % (label, "%12.1f ms" % ms if ms is not None else "COULD NOT RUN: " + err))
    say()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--baseline-lib")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--quick", action="store_true", help="m = 2^8 and 2^10 instead of 2^12 and 2^15; nothing is written")
    ap.add_argument("--resources-only", action="store_true")
    ap.add_argument("--skip-d", action="store_true")
    ap.add_argument("--child", choices=sorted(CHILDREN))
    ap.add_argument("--lg", type=int)
    ap.add_argument("--pkg-root")
    a = ap.parse_args()
    if a.child:
        sys.path.insert(0, a.pkg_root or ROOT)
        print(json.dumps(CHILDREN[a.child](a.lg)), flush=True)
        return
    sys.path.insert(0, ROOT)
    say("# circuits with Q ~ n: digest v2, per-pair state on first use (tools/large_q.py)")
    say()
    if a.resources_only:
        say("## (a), (b), (c), (d): not collected (they need the GPU)")
        say()
        resources()
        write()
        return
    if a.baseline_lib and not os.path.exists(a.baseline_lib):
        raise SystemExit("--baseline-lib %s: no such file" % a.baseline_lib)
    lg, lg_big = (8, 10) if a.quick else (12, 15)
    part_a(lg, a.rounds)
    if a.baseline_lib:
        part_bc(os.path.abspath(a.baseline_lib), lg, a.rounds)
    else:
        say("## (b), (c) skipped: no --baseline-lib was given")
        say()
    if not a.skip_d:
        part_d(lg_big)
    resources()
    if not a.quick:
        write()


if __name__ == "__main__":
    main()
