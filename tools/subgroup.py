#!/usr/bin/env python3
"""Writes profiles/r19_subgroup.txt on one MI355X: what the endomorphism subgroup tests (g1.hpp, g2.hpp) cost beside the definition
they replace, r P = O by double-and-add.

  (a)  the two methods through sonic_g1_subgroup_check / sonic_g2_subgroup_check, in this one process: G1 at n = 15 (the points of one
       Q = 2 proof), 2^10, 2^16, 2^20; G2 at n = 4, 2^10, 2^16.  The condition per group: the endomorphism method is faster than the walk
       by more than the larger spread at every size.
  (b)  whole calls against another build of the library (--baseline-lib PATH, the parent commit's libsonic_hip.so): SRS.load with the G2
       half at d = 2^16, 2^19, 2^21; verify_batch at n = 2^14, Q = 2, K in {1, 64, 1024} with the split of a K = 1 call
       (tools/verify_batch.py); sonic_verify at the same shape; g1_decompress(check_subgroup = 1) at 2^16 points.  Each side runs in
       fresh child processes under SONIC_HIP_LIB, alternating; without the option (b) is skipped and the file says so.
  (c)  the compiler's account of the new and changed kernels (-Rpass-analysis=kernel-resource-usage; needs no GPU).

Every time is the best of --rounds alternating rounds after a warm-up, and the spread is max - min over the rounds.  Every child process
runs under its own `timeout -k 10`; the first one that fails ends the run.

    python tools/subgroup.py [--baseline-lib PATH] [--rounds 5] [--load-lg 16,19,21] [--resources-only]

A baseline library older than this commit has to lie in a copy of its own package (PATH = .../sonic_amd/csrc/libsonic_hip.so): the
children of that side then import that copy's Python, since this tree's loader refuses a library without the new symbols.
"""
import argparse
import json
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
sys.path.insert(0, os.path.join(ROOT, "tools"))
CSRC = os.path.join(ROOT, "sonic_amd", "csrc")
SEED = bytes(range(32))
X, ALPHA = 0x1234567, 0x7654321
LOG2N, Q, BATCHES = 14, 2, (1, 64, 1024)
out_lines = []


def say(line=""):
    print(line, flush=True)
    out_lines.append(line)


# ---- (c) -------------------------------------------------------------------------------------------------------------------------------------
def resources():
    say("## (c) kernel resources (hipcc --offload-arch=gfx950 -O3 -Rpass-analysis=kernel-resource-usage)")
    say("%-34s %6s %6s %6s %10s %12s" % ("kernel", "VGPRs", "AGPRs", "SGPRs", "scratch B", "waves/SIMD"))
    want = {"verify_batch.hip": ["k_g1_subgroupILi0E", "k_g1_subgroupILi1E", "k_g1_validate"], "srs_g2.hip": ["k_g2_subgroupILi0E", "k_g2_subgroupILi1E", "k_g2_points_from_bytes"],
            "encoding.hip": ["k_points_subgroup_check"], "compress.hip": ["k_g1_decompress", "k_g2_decompress"]}
    procs = {f: subprocess.Popen(["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-Rpass-analysis=kernel-resource-usage", "-c",
                                  os.path.join(CSRC, f), "-o", os.devnull], stderr=subprocess.PIPE, text=True) for f in want}
    scratch = 0
    for f, names in want.items():
        err = procs[f].communicate()[1]
        for name in names:
            m = re.search(r"Function Name: \S*%s\S*.*?TotalSGPRs: (\d+).*?VGPRs: (\d+).*?AGPRs: (\d+).*?ScratchSize \[bytes/lane\]: (\d+).*?Occupancy \[waves/SIMD\]: (\d+)" % name, err, re.S)
            label = name.replace("ILi0E", "<endo>").replace("ILi1E", "<walk>")
            say("%-34s %6s %6s %6s %10s %12s" % ((label, m.group(2), m.group(3), m.group(1), m.group(4), m.group(5)) if m else (label, "?", "?", "?", "?", "?")))
            scratch += int(m.group(4)) if m else 1
    say("scratch is 0 for all of them" if scratch == 0 else "NOT all of them are free of scratch")
    say()


# ---- (a) -------------------------------------------------------------------------------------------------------------------------------------
def alternate(fns, rounds):
    """fns: {label: callable}.  One warm-up each, then `rounds` rounds that run every callable once, in turn -> {label: (best ms, spread ms)}"""
    for f in fns.values():
        f()
    ts = {k: [] for k in fns}
    for _ in range(rounds):
        for k, f in fns.items():
            t = time.perf_counter()
            f()
            ts[k].append((time.perf_counter() - t) * 1e3)
    return {k: (min(v), max(v) - min(v)) for k, v in ts.items()}


def part_a(rounds):
    import sonic_amd as sonic
    from sonic_amd import _lib
    L = _lib.lib()
    _lib.check(L.sonic_init(0))
    say("## (a) the two methods through the public calls (ms per call with its copies: best of %d alternating rounds, spread = max - min)" % rounds)
    srs = sonic.SRS.new(1 << 19, X, ALPHA)
    g1 = srs.points(0, -(1 << 19), 1 << 20)
    srs.close()
    srs = sonic.SRS.new(1 << 15, X, ALPHA)
    g2 = srs.g2_points(0, -(1 << 15), 1 << 16)
    srs.close()
    held = {}
    for group, pts, check, sizes in (("G1", g1, sonic.g1_subgroup_check, (15, 1 << 10, 1 << 16, 1 << 20)), ("G2", g2, sonic.g2_subgroup_check, (4, 1 << 10, 1 << 16))):
        say("%-4s %9s %12s %10s %12s %10s %8s %10s" % (group, "n", "endo", "spread", "walk", "spread", "ratio", "condition"))
        held[group] = True
        for n in sizes:
            p = np.ascontiguousarray(pts[:n])
            assert not check(p, method="endo").any() and not check(p, method="walk").any()
            r = alternate({"endo": lambda: check(p, method="endo"), "walk": lambda: check(p, method="walk")}, rounds)
            (te, se), (tw, sw) = r["endo"], r["walk"]
            ok = tw - te > max(se, sw)
            held[group] = held[group] and ok
            say("%-4s %9d %12.3f %10.3f %12.3f %10.3f %8.2f %10s" % ("", n, te, se, tw, sw, tw / te, "holds" if ok else "FAILS"))
        say("%s: the endomorphism method is %s the walk by more than the larger spread at every size" % (group, "faster than" if held[group] else "NOT faster than"))
    say()
    return held


# ---- (b): the children ---------------------------------------------------------------------------------------------------------------------------
def child_prepare(tmp, load_lg):
    """the strings the load children read, written by this build"""
    import sonic_amd as sonic
    from sonic_amd import _lib
    _lib.check(_lib.lib().sonic_init(0))
    for lg in load_lg:
        srs = sonic.SRS.new(1 << lg, X, ALPHA)
        srs.save(os.path.join(tmp, "srs%d" % lg), g2=True)
        srs.close()
    return {}


def child_load(tmp, load_lg):
    import sonic_amd as sonic
    from sonic_amd import _lib
    L = _lib.lib()
    _lib.check(L.sonic_init(0))
    sonic.SRS.load(os.path.join(tmp, "srs%d" % load_lg[0])).close()          # warm-up: code objects, the file cache of the smallest string
    res = {}
    for lg in load_lg:
        path = os.path.join(tmp, "srs%d" % lg)
        with open(path, "rb") as f:                                            # the page cache, not the disk, is what both sides read
            while f.read(1 << 26):
                pass
        t = time.perf_counter()
        s = sonic.SRS.load(path)
        _lib.check(L.sonic_device_sync())
        res["SRS.load d=2^%d (s)" % lg] = time.perf_counter() - t
        assert s.has_g2()
        s.close()
    return res


def child_calls(_tmp, _load_lg):
    import sonic_amd as sonic
    from sonic_amd import _lib
    from verify_batch import PARTS, make, prof
    L = _lib.lib()
    _lib.check(L.sonic_init(0))
    res = {}
    n, sp, asg = make(LOG2N, Q, "rnd")
    circuit = sp.to_dense()
    g = sonic.SRS.new(7 * n + 9, 3, 5)
    pipe = sonic.ProverPipeline(g, circuit)
    pipe.set_assignment(asg)
    pyr = random.Random(LOG2N * 1000 + Q)
    trs = [[pyr.randrange(1, sonic.R_MODULUS) for _ in range(8 + 2 * Q)] for _ in range(64)]
    proofs = pipe.prove_all(trs)
    pipe.close()
    vtr = [(t[4], t[5], list(zip(t[6:6 + Q], t[6 + Q:6 + 2 * Q]))) for t in trs]
    ver = sonic.Verifier(g, circuit)
    assert ver.verify_batch(proofs[:2], vtr[:2], seed=SEED)

    def best(f, reps=3):
        f()
        ts = []
        for _ in range(reps):
            t = time.perf_counter()
            f()
            ts.append((time.perf_counter() - t) * 1e3)
        return min(ts)
    for K in BATCHES:
        bp, bt = [proofs[k % 64] for k in range(K)], [vtr[k % 64] for k in range(K)]
        res["verify_batch K=%d (ms)" % K] = best(lambda: ver.verify_batch(bp, bt, seed=SEED))
    L.sonic_profile_enable(1)
    L.sonic_profile_reset()
    t = time.perf_counter()
    assert ver.verify_batch(proofs[:1], vtr[:1], seed=SEED)
    wall = (time.perf_counter() - t) * 1e3
    L.sonic_profile_enable(0)
    known = 0.0
    for label, names in PARTS:
        v = sum(prof(L, nm) for nm in names)
        known += v
        res["  K=1 split: %s (ms)" % label] = v
    res["  K=1 split: everything else (ms)"] = max(wall - known, 0.0)
    p0 = sonic.Proof.from_bytes(proofs[0], Q)
    res["sonic_verify (ms)"] = best(lambda: sonic.verify(g, circuit, p0, *vtr[0]))
    ver.close()
    pts = g.points(0, -(1 << 15), 1 << 16)
    g.close()
    z = sonic.g1_compress(pts)
    res["g1_decompress(check_subgroup=1) 2^16 (ms)"] = best(lambda: sonic.g1_decompress(z, check_subgroup=True, flags=True))
    return res


CHILDREN = {"prepare": child_prepare, "load": child_load, "calls": child_calls}


def run_child(kind, lib, tmp, load_lg, limit):
    env = dict(os.environ)
    if lib:
        env["SONIC_HIP_LIB"] = lib
    else:
        env.pop("SONIC_HIP_LIB", None)
    cmd = ["timeout", "-k", "10", str(limit), sys.executable, os.path.abspath(__file__), "--child", kind, "--tmp", tmp, "--load-lg", ",".join(map(str, load_lg))]
    # a library from before this commit lacks symbols that this tree's _lib.py insists on: when it lies in a copy of the package
    # (.../sonic_amd/csrc/libsonic_hip.so), the child imports that copy's Python with it
    pkg = os.path.dirname(os.path.dirname(os.path.dirname(lib))) if lib else None
    if pkg and os.path.exists(os.path.join(pkg, "sonic_amd", "__init__.py")):
        cmd += ["--pkg-root", pkg]
    t0 = time.perf_counter()
    out = subprocess.run(cmd, env=env, capture_output=True, text=True)
    print("  [%s, %s: %.0f s]" % (kind, "baseline" if lib else "this build", time.perf_counter() - t0), flush=True)
    if out.returncode != 0:
        say("child '%s' (%s) ended with status %d; nothing more is started" % (kind, lib or "this build", out.returncode))
        say(out.stdout[-1500:] + out.stderr[-3000:])
        raise SystemExit(1)
    return json.loads(out.stdout.strip().splitlines()[-1])


def part_b(baseline, rounds, load_lg):
    say("## (b) whole calls: the baseline library (--baseline-lib) against this build, fresh processes, alternating (best of %d rounds; spread = max - min)" % rounds)
    with tempfile.TemporaryDirectory() as tmp:
        run_child("prepare", None, tmp, load_lg, 900)
        rows = {}
        for kind in ("load", "calls"):
            for _ in range(rounds):
                for side, lib in (("baseline", baseline), ("this", None)):
                    for k, v in run_child(kind, lib, tmp, load_lg, 600).items():
                        rows.setdefault(k, {"baseline": [], "this": []})[side].append(v)
    say("%-46s %12s %10s %12s %10s %8s" % ("call", "baseline", "spread", "this build", "spread", "ratio"))
    for k, v in rows.items():
        b, t = v["baseline"], v["this"]
        say("%-46s %12.3f %10.3f %12.3f %10.3f %8.2f" % (k, min(b), max(b) - min(b), min(t), max(t) - min(t), min(b) / min(t) if min(t) > 0 else float("nan")))
    say()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--baseline-lib")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--load-lg", default="16,19,21")
    ap.add_argument("--resources-only", action="store_true")
    ap.add_argument("--child", choices=sorted(CHILDREN))
    ap.add_argument("--tmp")
    ap.add_argument("--pkg-root")
    a = ap.parse_args()
    load_lg = [int(x) for x in a.load_lg.split(",")]
    if a.child:
        if a.pkg_root:
            sys.path.insert(0, a.pkg_root)
        print(json.dumps(CHILDREN[a.child](a.tmp, load_lg)), flush=True)
        return
    say("# subgroup membership: the endomorphism tests against r P = O by double-and-add (tools/subgroup.py)")
    say()
    if a.resources_only:
        resources()
        return
    if a.baseline_lib and not os.path.exists(a.baseline_lib):
        raise SystemExit("--baseline-lib %s: no such file" % a.baseline_lib)
    part_a(a.rounds)
    if a.baseline_lib:
        part_b(os.path.abspath(a.baseline_lib), a.rounds, load_lg)
    else:
        say("## (b) skipped: no --baseline-lib was given")
        say()
    resources()
    with open(os.path.join(ROOT, "profiles", "r19_subgroup.txt"), "w") as f:
        f.write("\n".join(out_lines) + "\n")


if __name__ == "__main__":
    main()
