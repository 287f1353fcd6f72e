#!/usr/bin/env python3
"""Writes profiles/r23_core_scale.txt on one MI355X: what a handle that only makes core proofs holds and what a core proof costs the host
when Q ~ n, this build against another build of the library (include/sonic_hip.h, "Circuits with Q ~ n": signature state on first use,
k(y) over many blocks).

  (1)  compiled R1CS at m = 2^12 and m = 2^15 (the shapes of profiles/r22_large_q.txt; tools/large_q.py builds them): a fresh
       Prover(prepare=False) -- construction time, device_bytes, host_bytes where the build has them, the free-memory difference for both
       -- then a core proof one at a time, streamed (16 per call) and prove_core_fs, and the SONIC_DEBUG_TIMING split of one proof.
       The condition: at m = 2^15 this build is faster than the baseline on all three legs by more than the larger spread.
  (2)  no regression where Q is small: workload.sparse_circuit n = 2^14, Q = 64 and rndCircuit n = 2^14, Q = 2; core and full proofs, one
       at a time and streamed.  The condition: this build is not slower than the baseline by more than the larger spread on any leg.
  (3)  the k(y) kernels by HIP events (sonic_profile_*), one process, alternating SONIC_K_OF_Y_SPLIT=0 / =1 proof by proof, at
       Q in {2^10, 2^12, 2^14, 98 306, 786 434}: the one-block kernel against the two launches of the split form
  (4)  m = 2^18, N ~ m, this build only, single calls: every step with its time; a step that cannot run with its message
  (5)  the compiler's account of the new kernels (needs no GPU)

(1), (2) and (4) run in fresh child processes, each under its own `timeout -k 10`; the baseline's children load it through SONIC_HIP_LIB
and import the Python of the package copy it lies in (PATH = .../sonic_amd/csrc/libsonic_hip.so), as in tools/large_q.py.  The children
alternate baseline / this build for --rounds rounds (each child: a warm-up, then the best of three); the figure is the best round and
spread = max - min over the rounds.  The first child that fails ends its part.

    python tools/core_scale.py [--baseline-lib PATH] [--rounds 5] [--parts 1,2,3,4,5] [--out FILE] [--big-limit S] [--quick] [--resources-only]
"""
import argparse
import ctypes as C
import json
import os
import random
import re
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "sonic_amd", "csrc")
sys.path.insert(0, os.path.join(ROOT, "tools"))
import large_q      # noqa: E402  (the compiled systems of profiles/r22_large_q.txt, `timed`)

R = large_q.R
out_lines = []


def say(line=""):
    print(line, flush=True)
    out_lines.append(line)


def write(path="profiles/r23_core_scale.txt"):
    with open(os.path.join(ROOT, path), "w") as f:
        f.write("\n".join(out_lines) + "\n")


# ---- (5) ---------------------------------------------------------------------------------------------------------------------------------
def resources():
    say("## (5) the k(y) kernels of poly.hip (hipcc --offload-arch=gfx950 -O3 -Rpass-analysis=kernel-resource-usage)")
    say("%-22s %6s %6s %10s %12s %8s %12s" % ("kernel", "VGPRs", "SGPRs", "scratch B", "waves/SIMD", "LDS B", "SGPR spills"))
    err = subprocess.run(["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-Rpass-analysis=kernel-resource-usage", "-c",
                          os.path.join(CSRC, "poly.hip"), "-o", os.devnull], stderr=subprocess.PIPE, text=True).stderr
    for name in ("k_sub_k_of_y", "k_k_of_y_partials", "k_k_of_y_finish"):
        m = re.search(r"Function Name: \S*%s\S*.*?TotalSGPRs: (\d+).*?VGPRs: (\d+).*?ScratchSize \[bytes/lane\]: (\d+).*?Occupancy \[waves/SIMD\]: (\d+).*?SGPRs Spill: (\d+).*?LDS Size \[bytes/block\]: (\d+)"
                      % name, err, re.S)
        say("%-22s %6s %6s %10s %12s %8s %12s" % ((name, m.group(2), m.group(1), m.group(3), m.group(4), m.group(6), m.group(5)) if m else (name, "?", "?", "?", "?", "?", "?")))
    say("blocks of 256 threads; the LDS is the 256 field elements of the block's tree; no scratch memory (k_sub_k_of_y: the one-block form, unchanged)")
    say()


# ---- the children ----------------------------------------------------------------------------------------------------------------------
def debug_timing(tag, fn):
    """one call with SONIC_DEBUG_TIMING=1 (read per proof): the library's line on stderr follows the marker, run_child reads it"""
    os.environ["SONIC_DEBUG_TIMING"] = "1"
    print("[core_scale] %s" % tag, file=sys.stderr, flush=True)
    fn()
    os.environ.pop("SONIC_DEBUG_TIMING")


def child_handle(lg):
    """(1) for one build"""
    import torch
    import sonic_amd as sonic
    from sonic_amd import _lib
    _lib.check(_lib.lib().sonic_init(0))
    K = 16
    r, circuit, za, srs = large_q.compiled(lg, K)
    wb, cs, bad = r.assign(torch.from_numpy(za).cuda())
    assert bad == [(0, -1)] * K
    torch.cuda.synchronize()
    free = lambda: torch.cuda.mem_get_info()[0]      # noqa: E731
    res = {"n": r.n, "Q": r.Q, "nnz": circuit.nnz}
    f0 = free()
    t0 = time.perf_counter()
    p = sonic.Prover(srs, circuit, prepare=False)
    torch.cuda.synchronize()
    res["construct_ms"] = (time.perf_counter() - t0) * 1e3
    res["free_diff_gb"] = (f0 - free()) / 1e9
    res["device_bytes_gb"] = p.device_bytes / 1e9 if hasattr(p, "device_bytes") else None
    res["host_bytes_gb"] = p.host_bytes / 1e9 if hasattr(p, "host_bytes") else None
    rng = random.Random(5)
    trs = [[rng.randrange(1, R) for _ in range(6)] for _ in range(K)]
    p.set_witness(wb.aL[0], wb.aR[0], wb.aO[0])
    p.set_constants(cs[0])
    core = p.prove_core_bytes(trs[0])
    assert sonic.verify_core(srs, circuit, core, trs[0][4], trs[0][5])
    cd2 = sonic.fs_circuit_digest_v2(p.weights_digest_v2(), cs[0])
    res["core_one_ms"] = large_q.timed(lambda: p.prove_core_bytes(trs[0]), 3)[0]
    res["core_streamed_ms"] = large_q.timed(lambda: sonic.prove_core_batch([p], trs, wb, constants=cs), 3)[0] / K
    res["core_fs_ms"] = large_q.timed(lambda: p.prove_core_fs(cd2, b"\x11" * 32), 3)[0]
    res["device_bytes_after_gb"] = p.device_bytes / 1e9 if hasattr(p, "device_bytes") else None
    res["host_bytes_after_gb"] = p.host_bytes / 1e9 if hasattr(p, "host_bytes") else None
    debug_timing("core", lambda: p.prove_core_bytes(trs[0]))
    p.close()
    return res


def child_small(_lg):
    """(2) for one build: Q = 64 (sparse) and Q = 2 (rndCircuit, dense) at n = 2^14; core and full, one at a time and streamed"""
    import sonic_amd as sonic
    from sonic_amd import _lib, workload
    _lib.check(_lib.lib().sonic_init(0))
    n, K = 1 << 14, 8
    srs = sonic.SRS.new(7 * n + 64, 0x1234567, 0x7654321)
    rng = random.Random(6)
    res = {}
    w = workload.sparse_circuit(21, n, 64, 4)
    shapes = [("q64", sonic.SparseCircuit(n, 64, w["row_ptr"], w["col"], w["val"], w["cs"]), sonic.Assignment(w["aL"], w["aR"], w["aO"]), 64)]
    rc = workload.big_circuit(22, n, 2)
    shapes.append(("q2", sonic.ArithCircuit(sonic.GateWeights(rc["wL"], rc["wR"], rc["wO"]), rc["cs"]), sonic.Assignment(rc["aL"], rc["aR"], rc["aO"]), 2))
    for tag, circuit, asg, Q in shapes:
        trs = [[rng.randrange(1, R) for _ in range(8 + 2 * Q)] for _ in range(K)]
        ps = [sonic.Prover(srs, circuit, prepare=False) for _ in range(2)]
        for p in ps:
            p.set_assignment(asg)
        res["%s_core_one_ms" % tag] = large_q.timed(lambda: ps[0].prove_core_bytes(trs[0][:6]), 3)[0]
        res["%s_core_streamed_ms" % tag] = large_q.timed(lambda: sonic.prove_core_batch(ps, [t[:6] for t in trs]), 3)[0] / K
        res["%s_full_one_ms" % tag] = large_q.timed(lambda: ps[0].prove_bytes(trs[0]), 3)[0]
        res["%s_full_streamed_ms" % tag] = large_q.timed(lambda: sonic.prove_batch(ps, trs), 3)[0] / K
        for p in ps:
            p.close()
    srs.close()
    return res


def child_big(lg):
    """(4): every step timed; the first step that fails is recorded with its message and ends the child"""
    import torch
    import sonic_amd as sonic
    from sonic_amd import _lib
    _lib.check(_lib.lib().sonic_init(0))
    steps, state = [], {}

    def step(label, fn):
        t0 = time.perf_counter()
        try:
            fn()
            torch.cuda.synchronize()
        except Exception as e:      # noqa: BLE001  (the message is the record)
            steps.append((label, None, "%s: %s" % (type(e).__name__, str(e)[:300])))
            return False
        steps.append((label, (time.perf_counter() - t0) * 1e3, ""))
        print("[core_scale] done: %s" % label, file=sys.stderr, flush=True)
        return True

    def build():
        state["r"], state["circuit"], state["za"], state["srs"] = large_q.compiled(lg, 1)
    free = lambda: torch.cuda.mem_get_info()[0]      # noqa: E731

    def handle():
        f0 = free()
        state["p"] = sonic.Prover(state["srs"], state["circuit"], prepare=False)
        torch.cuda.synchronize()
        state["mem"] = (state["p"].device_bytes / 1e9, state["p"].host_bytes / 1e9, (f0 - free()) / 1e9)

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
        state["mem_after"] = (state["p"].device_bytes / 1e9, state["p"].host_bytes / 1e9)

    def verifier():
        state["v"] = sonic.Verifier(state["srs"], state["circuit"], digest=2)

    def verify():
        ok, each = state["v"].verify_core_fs_batch([state["proof"][0]], seed=b"\x13" * 32, each=True, constants=[state["cs"][0]])
        assert ok and each == [True], (ok, each)
    for label, fn in (("the system, its R1CS handle, the compiled circuit and the SRS of d = 7n + 64 (host Python included)", build),
                      ("Prover(srs, circuit, prepare=False)", handle), ("R1CS.assign (1 witness), set_witness, set_constants", assign),
                      ("Prover.weights_digest_v2() and fs_circuit_digest_v2", digests), ("prove_core_fs under circuit digest v2 (first)", prove),
                      ("prove_core_fs under circuit digest v2 (second)", prove_again), ("Verifier(srs, circuit, digest=2)", verifier),
                      ("verify_core_fs_batch, K = 1, constants given: accepted", verify)):
        if not step(label, fn):
            break
    r = state.get("r")
    return {"steps": steps, "n": r.n if r else None, "Q": r.Q if r else None, "nnz": state["circuit"].nnz if "circuit" in state else None,
            "mem": state.get("mem"), "mem_after": state.get("mem_after")}


CHILDREN = {"handle": child_handle, "small": child_small, "big": child_big}


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
    m = re.search(r"\[core_scale\] core\s.*?enqueue ([0-9.]+) ms, then waited ([0-9.]+) ms", out.stderr, re.S)
    if m and isinstance(res, dict):
        res["enqueue_ms"], res["wait_ms"] = float(m.group(1)), float(m.group(2))
    return res, ""


def alternate(kind, baseline, lg, rounds, limit):
    rows = {"baseline": [], "this": []}
    for _ in range(rounds):
        for side, lib in (("baseline", baseline), ("this", None)):
            res, msg = run_child(kind, lib, lg, limit)
            if res is None:
                say("child (%s) failed, nothing more is started: %s" % (side, msg))
                say()
                return None
            rows[side].append(res)
    return rows


def table(rows, keys):
    say("%-64s %12s %10s %12s %10s %8s" % ("", "baseline", "spread", "this build", "spread", "ratio"))
    stats = {}
    for key, label in keys:
        if any(key not in x for x in rows["baseline"] + rows["this"]):
            continue
        b, t = [x[key] for x in rows["baseline"]], [x[key] for x in rows["this"]]
        if any(v is None for v in t):
            continue
        if any(v is None for v in b):
            say("%-64s %12s %10s %12.4f %10.4f %8s" % (label, "-", "-", min(t), max(t) - min(t), "-"))
            continue
        stats[key] = (min(b), max(b) - min(b), min(t), max(t) - min(t))
        say("%-64s %12.4f %10.4f %12.4f %10.4f %8.2f" % (label, min(b), max(b) - min(b), min(t), max(t) - min(t), min(b) / min(t) if min(t) > 0 else float("nan")))
    return stats


def part_1(baseline, lg, rounds, condition):
    say("## (1) compiled R1CS at m = 2^%d: the baseline library against this build, fresh processes, alternating" % lg)
    say("(best of %d rounds, spread = max - min over the rounds; a child times each call as the best of three after a warm-up)" % rounds)
    rows = alternate("handle", baseline, lg, rounds, 900)
    if rows is None:
        return
    say("n = %d, Q = %d, nnz = %d; 5 Q slots of 12 304 bytes = %.2f GB" % (rows["this"][0]["n"], rows["this"][0]["Q"], rows["this"][0]["nnz"], 5 * rows["this"][0]["Q"] * 12304 / 1e9))
    legs = ("core_one_ms", "core_streamed_ms", "core_fs_ms")
    stats = table(rows, (("construct_ms", "fresh Prover(prepare=False): construction (ms)"), ("free_diff_gb", "    device memory, free before - after (GB)"),
                         ("device_bytes_gb", "    device_bytes (GB)"), ("host_bytes_gb", "    host_bytes, pinned (GB)"),
                         ("device_bytes_after_gb", "    device_bytes after the core proofs (GB)"), ("host_bytes_after_gb", "    host_bytes after the core proofs (GB)"),
                         ("core_one_ms", "core proof, one at a time (ms)"), ("core_streamed_ms", "core proof, streamed, per proof (ms)"),
                         ("core_fs_ms", "prove_core_fs under circuit digest v2 (ms)"),
                         ("enqueue_ms", "    SONIC_DEBUG_TIMING, one core proof: host enqueue (ms)"), ("wait_ms", "    then waited for the device (ms)")))
    if condition and all(k in stats for k in legs):
        holds = all(stats[k][0] - stats[k][2] > max(stats[k][1], stats[k][3]) for k in legs)
        say("condition (1): this build is %s the baseline by more than the larger spread on all three legs (ratios %s)" %
            ("faster than" if holds else "NOT faster than", ", ".join("%.2f" % (stats[k][0] / stats[k][2]) for k in legs)))
    say()


def part_2(baseline, rounds):
    say("## (2) small Q at n = 2^14: workload.sparse_circuit Q = 64 and rndCircuit Q = 2, the baseline against this build, fresh processes, alternating")
    say("(best of %d rounds, spread = max - min; ms per proof; streamed = 8 proofs over two handles per call)" % rounds)
    rows = alternate("small", baseline, 14, rounds, 600)
    if rows is None:
        return
    keys = [("%s_%s_%s_ms" % (q, kind, how), "%s, %s proof, %s" % ("Q = 64" if q == "q64" else "Q = 2", kind, "one at a time" if how == "one" else "streamed"))
            for q in ("q64", "q2") for kind in ("core", "full") for how in ("one", "streamed")]
    stats = table(rows, keys)
    slower = [k for k, s in stats.items() if s[2] - s[0] > max(s[1], s[3])]
    say("condition (2): this build is %s" % ("not slower than the baseline by more than the larger spread on any leg" if not slower else
                                             "SLOWER than the baseline by more than the larger spread on: " + ", ".join(slower)))
    say()


def part_3(reps):
    import sonic_amd as sonic
    from sonic_amd import _lib
    _lib.check(_lib.lib().sonic_init(0))
    L = _lib.lib()
    say("## (3) k(y): the one-block kernel against the split form (span 2048), HIP events around each launch (sonic_profile_*), alternating proof by proof")
    say("(n = 16, one weight per row; us per proof's k(y): best of %d, spread = max - min; the split form is k_k_of_y_partials + k_k_of_y_finish)" % reps)
    say("%10s %8s %14s %10s %14s %10s %14s %14s" % ("Q", "blocks", "one block", "spread", "split", "spread", "= partials", "+ finish"))
    n = 16
    srs = sonic.SRS.new(7 * 256, 0x1234567, 0x7654321)
    rng = random.Random(7)
    aL, aR = [rng.randrange(1, R) for _ in range(n)], [rng.randrange(1, R) for _ in range(n)]
    asg = sonic.Assignment(aL, aR, [a * b % R for a, b in zip(aL, aR)])
    tr = [rng.randrange(1, R) for _ in range(6)]

    def events(names):
        out = []
        for name in names:
            ms, launches = C.c_double(), C.c_int64()
            L.sonic_profile_get(name.encode(), C.byref(ms), C.byref(launches))
            out.append(ms.value * 1e3)
        return out
    for Q in (1 << 10, 1 << 12, 1 << 14, 98306, 786434):
        w = [rng.randrange(1, R) for _ in range(Q)]
        sp = sonic.SparseCircuit(n, Q, list(range(Q + 1)) + [Q] * (2 * Q), [q % n for q in range(Q)], w, [w[q] * aL[q % n] % R for q in range(Q)])
        p = sonic.Prover(srs, sp, prepare=False)
        p.set_assignment(asg)
        one, split = [], []
        want = None
        for rep in range(reps + 1):
            for mode in ("0", "1"):
                os.environ["SONIC_K_OF_Y_SPLIT"] = mode
                L.sonic_profile_reset(); L.sonic_profile_enable(1)
                got = p.prove_core_bytes(tr)
                L.sonic_profile_enable(0)
                assert want is None or got == want
                want = got
                if rep:      # (the first pair is the warm-up)
                    (one if mode == "0" else split).append(events(["k_sub_k_of_y"] if mode == "0" else ["k_k_of_y_partials", "k_k_of_y_finish"]))
        os.environ.pop("SONIC_K_OF_Y_SPLIT")
        p.close()
        o = [x[0] for x in one]
        s = [x[0] + x[1] for x in split]
        best = min(split, key=lambda x: x[0] + x[1])
        say("%10d %8d %14.2f %10.2f %14.2f %10.2f %14.2f %14.2f" % (Q, -(-Q // 2048), min(o), max(o) - min(o), min(s), max(s) - min(s), best[0], best[1]))
    srs.close()
    say()


def part_4(lg, limit):
    say("## (4) m = 2^%d, N ~ m, this build only (one fresh process; wall times of single calls, no repetition)" % lg)
    res, msg = run_child("big", None, lg, limit)
    if res is None:
        say("the child did not finish: %s" % msg)
        say()
        return
    say("n = %s, Q = %s, nnz = %s; the fresh handle: device_bytes %s GB, host_bytes %s GB, free-memory difference %s GB; after two proofs: device_bytes %s GB, host_bytes %s GB" %
        (res["n"], res["Q"], res["nnz"], *(("%.4f" % v for v in res["mem"]) if res["mem"] else ("?", "?", "?")),
         *(("%.4f" % v for v in res["mem_after"]) if res.get("mem_after") else ("?", "?"))))
    for label, ms, err in res["steps"]:
        say("%-104s %s" % (label, "%12.1f ms" % ms if ms is not None else "COULD NOT RUN: " + err))
    say()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--baseline-lib")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--parts", default="1,2,3,4,5")
    ap.add_argument("--out", default="profiles/r23_core_scale.txt", help="where the report goes, relative to the repository")
    ap.add_argument("--big-limit", type=int, default=1100, help="time limit of part 4's child process, in seconds")
    ap.add_argument("--quick", action="store_true", help="m = 2^8 / 2^10 / 2^10 instead of 2^12 / 2^15 / 2^18; nothing is written")
    ap.add_argument("--resources-only", action="store_true")
    ap.add_argument("--child", choices=sorted(CHILDREN))
    ap.add_argument("--lg", type=int)
    ap.add_argument("--pkg-root")
    a = ap.parse_args()
    if a.child:
        sys.path.insert(0, a.pkg_root or ROOT)
        print(json.dumps(CHILDREN[a.child](a.lg)), flush=True)
        return
    sys.path.insert(0, ROOT)
    say("# core proofs free of Q: signature state on first use, k(y) over many blocks (tools/core_scale.py)")
    say()
    if a.resources_only:
        say("## (1), (2), (3), (4): not collected (they need the GPU)")
        say()
        resources()
        write(a.out)
        return
    if a.baseline_lib and not os.path.exists(a.baseline_lib):
        raise SystemExit("--baseline-lib %s: no such file" % a.baseline_lib)
    parts = set(a.parts.split(","))
    base = os.path.abspath(a.baseline_lib) if a.baseline_lib else None
    lgs = (8, 10, 10) if a.quick else (12, 15, 18)
    if "1" in parts and base:
        part_1(base, lgs[0], a.rounds, condition=False)
        part_1(base, lgs[1], a.rounds, condition=True)
    if "2" in parts and base:
        part_2(base, a.rounds)
    if ({"1", "2"} & parts) and not base:
        say("## (1), (2) skipped: no --baseline-lib was given")
        say()
    if "3" in parts:
        part_3(a.rounds)
    if "4" in parts:
        part_4(lgs[2], a.big_limit)
    if "5" in parts:
        resources()
    if not a.quick:
        write(a.out)


if __name__ == "__main__":
    main()
