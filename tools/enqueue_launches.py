#!/usr/bin/env python3
"""Per-kernel launch counts of ONE proof's enqueue (the library's own event timer, sonic_profile_*), over the smallest shapes that reach
every branch of prove_enqueue: for comparing two builds of the library after a change that must not move a launch.  The counts are those
of the second proof of a handle (the first one grows the workspaces).  One child process per environment (the knobs are read once).
    python tools/enqueue_launches.py > a.txt;  SONIC_HIP_LIB=other/libsonic_hip.so python tools/enqueue_launches.py > b.txt
    python tools/enqueue_launches.py --diff a.txt b.txt      # side by side; exit status 1 if any count differs"""
import ctypes as C
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
ENVS = ["", "SONIC_PROVE_FUSED=0", "SONIC_FUSED_LANES=2", "SONIC_PROVE_SYM=1", "SONIC_PROVE_RUNS=1"]
SHAPES = [(40, 2), (300, 3), (5000, 2)]         # (300, 3): 19 MSMs, two chunks of the proof's chain


def counted(L, label, proof):
    """runs proof() twice and prints the launches of the second run, one line per kernel"""
    proof()
    L.sonic_profile_reset(); L.sonic_profile_enable(1)
    proof()
    L.sonic_profile_enable(0)
    names = C.create_string_buffer(16384)
    L.sonic_profile_names(names, 16384)
    for nm in sorted(names.value.decode().split()):
        ms, cnt = C.c_double(), C.c_int64()
        L.sonic_profile_get(nm.encode(), C.byref(ms), C.byref(cnt))
        if cnt.value:
            print(f"{label} {nm} {cnt.value}", flush=True)


def child(env):
    import numpy as np
    import sonic_amd
    from sonic_amd import _lib
    from sonic_amd.workload import big_circuit, rand_fr_array
    L = _lib.lib()
    _lib.check(L.sonic_init(0))
    rng = np.random.default_rng(0)
    tag = env or "default"
    for n, Q in ([(700, 2)] if "RUNS" in env else SHAPES):       # (700: the smallest n of tests/test_gpu_runs.py that has 8 tiles)
        srs = sonic_amd.SRS.new(8 * n, 0x1234567, 0x7654321)
        c = big_circuit(1, n, Q)
        circuit = sonic_amd.ArithCircuit(sonic_amd.GateWeights(c["wL"], c["wR"], c["wO"]), c["cs"])
        tr = rand_fr_array(rng, 8 + 2 * Q)
        tr[:, 0] |= 1
        for prepare in ([False] if "RUNS" in env else [False, True]):
            p = sonic_amd.Prover(srs, circuit, prepare=prepare)
            p.set_assignment(sonic_amd.Assignment(c["aL"], c["aR"], c["aO"]))
            counted(L, f"[{tag}] n={n} Q={Q} prepared={int(prepare)}", lambda: p.prove_bytes(tr))
            if not env and prepare and (n, Q) == (300, 3):
                dg = sonic_amd.fs_circuit_digest(circuit)
                counted(L, f"[{tag}] n={n} Q={Q} prove_fs", lambda: p.prove_fs(dg, bytes(32)))
            if not env and prepare and (n, Q) == (5000, 2):
                for r in range(3):
                    p.set_share(r, 3)
                    counted(L, f"[{tag}] n={n} Q={Q} share={r}/3", lambda: p.prove_share(tr))
            p.close()
        srs.close()


def diff(a, b):
    rows = [{ln.rsplit(" ", 1)[0]: ln.rsplit(" ", 1)[1] for ln in open(f).read().splitlines() if ln.startswith("[")} for f in (a, b)]
    bad = 0
    for k in sorted(set(rows[0]) | set(rows[1])):
        x, y = rows[0].get(k, "-"), rows[1].get(k, "-")
        bad += x != y
        print(f"{k:<100} {x:>6} {y:>6}{'' if x == y else '   <-- differs'}")
    print(f"{len(rows[0])} / {len(rows[1])} rows, {bad} differ")
    return 1 if bad or not rows[0] else 0


if __name__ == "__main__":
    if sys.argv[1:2] == ["--diff"]:
        sys.exit(diff(sys.argv[2], sys.argv[3]))
    if sys.argv[1:2] == ["--child"]:
        sys.exit(child(sys.argv[2]))
    for e in ENVS:
        rc = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", e], env=dict(os.environ, **dict([e.split("=")] if e else [])), timeout=240).returncode
        if rc:
            sys.exit(f"environment {e!r}: exit status {rc}; stopped")
