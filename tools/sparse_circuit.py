"""Dense against CSR gate weights (include/sonic_hip.h, "gate weights as CSR"), shape by shape, on one GPU.

Per shape: host bytes handed over, HBM the circuit holds in the handle (from the buffers' sizes), sonic_prover_new* and prepare wall time,
streamed ms per prepared proof (two handles, submit / collect alternating: sonic_amd.ProverPipeline), and host verify time.  The dense and
CSR legs run in the same process, alternating, after a warm-up proof of every shape.  --kernels instead times, with the library's
per-launch event timer (sonic_profile_*), the kernels that read the circuit: k_s_of_y + k_s_of_u_rows (dense) against k_s_of_y_csc +
k_s_of_u_csr + k_s_of_u_csr_finish (CSR), per proof -- a run of its own, because the timer adds events around every launch.

    python tools/sparse_circuit.py [--proofs 8] [--rounds 2] [--kernels] [--shapes 14:2:rnd,16:64:4,...]
"""
import argparse
import ctypes as C
import os
import random
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import sonic_amd  # noqa: E402
from sonic_amd import _lib, workload  # noqa: E402

R = sonic_amd.R_MODULUS
DEFAULT_SHAPES = "14:2:rnd,14:16:4,14:64:4,16:2:rnd,16:16:4,16:64:4,18:2:rnd,18:16:4,18:64:4"


def make(log2n, Q, kind):
    n = 1 << log2n
    if kind == "rnd":
        b = workload.big_circuit(log2n, n, Q)
        rp, col, val = workload.csr_from_dense(b["wL"], b["wR"], b["wO"], n, Q)
        sp = sonic_amd.SparseCircuit(n, Q, rp, col, val, b["cs"])
        asg = sonic_amd.Assignment(b["aL"], b["aR"], b["aO"])
    else:
        c = workload.sparse_circuit(log2n * 100 + Q, n, Q, int(kind))
        sp = sonic_amd.SparseCircuit(n, Q, c["row_ptr"], c["col"], c["val"], c["cs"])
        asg = sonic_amd.Assignment(c["aL"], c["aR"], c["aO"])
    return n, sp, sp.to_dense(), asg


def csr_hbm(sp):
    nch = sum(-(-int(c) // 512) for c in np.diff(sp.row_ptr))
    return 2 * sp.nnz * 32 + 4 * (2 * sp.nnz + 2 * sp.nnz + sp.n + 1 + 2 * (3 * sp.Q + 1) + 2 * nch) + 32 * nch + 32 * sp.Q


def trs(Q, k, seed):
    pyr = random.Random(seed)
    return [[pyr.randrange(1, R) for _ in range(8 + 2 * Q)] for _ in range(k)]


def timed(f):
    t = time.perf_counter()
    r = f()
    return r, (time.perf_counter() - t) * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--proofs", type=int, default=8)
    ap.add_argument("--rounds", type=int, default=2, help="alternating dense / CSR rounds per shape")
    ap.add_argument("--kernels", action="store_true")
    ap.add_argument("--shapes", default=DEFAULT_SHAPES, help="log2n:Q:(rnd | max entries per row), comma-separated")
    ap.add_argument("--no-verify", action="store_true")
    a = ap.parse_args()
    _lib.check(_lib.lib().sonic_init(0))
    L = _lib.lib()
    shapes = [s.split(":") for s in a.shapes.split(",")]
    srs_by_n = {}
    for log2n, Q, kind in shapes:
        log2n, Q = int(log2n), int(Q)
        n, sp, dc, asg = make(log2n, Q, kind)
        if n not in srs_by_n:
            srs_by_n[n] = sonic_amd.SRS.new(7 * n + 9, 3, 5)
        g = srs_by_n[n]
        name = f"n=2^{log2n} Q={Q} {'rndCircuit' if kind == 'rnd' else '<=' + kind + ' nnz/row'} (nnz={sp.nnz})"
        host_dense, host_csr = 3 * Q * n * 32 + 32 * Q, sp.row_ptr.nbytes + sp.col.nbytes + sp.val.nbytes + sp.cs.nbytes
        hbm_dense, hbm_csr = 3 * Q * n * 32 + 32 * Q, csr_hbm(sp)
        forms = [("dense", dc), ("csr", sp)]
        pipes, t_new, t_prep = {}, {}, {}
        for f, circ in forms:
            handles = []
            tn = tp = 0.0
            for _ in range(2):
                p, dt = timed(lambda: sonic_amd.Prover(g, circ, prepare=False))
                tn += dt
                _, dt = timed(lambda: _lib.check(L.sonic_prover_prepare(p._h)))
                tp += dt
                p.set_assignment(asg)
                handles.append(p)
            pipe = sonic_amd.ProverPipeline.__new__(sonic_amd.ProverPipeline)
            pipe.provers = handles
            pipes[f], t_new[f], t_prep[f] = pipe, tn / 2, tp / 2
            pipe.prove_all(trs(Q, 2, 1))                               # warm-up (grows the workspaces)
        t = trs(Q, a.proofs, 2)
        if a.kernels:
            print(name)
            for f, _ in forms:
                L.sonic_profile_enable(1)
                L.sonic_profile_reset()
                for tr in t:
                    pipes[f].provers[0].prove_bytes(tr)
                L.sonic_profile_enable(0)
                parts = []
                tot = 0.0
                for k in (("k_s_of_y", "k_s_of_u_rows") if f == "dense" else ("k_s_of_y_csc", "k_s_of_u_csr", "k_s_of_u_csr_finish")):
                    ms, cnt = C.c_double(0), C.c_int64(0)
                    L.sonic_profile_get(k.encode(), C.byref(ms), C.byref(cnt))
                    parts.append(f"{k} {ms.value / len(t):.4f}")
                    tot += ms.value / len(t)
                print(f"  {f:5s} circuit kernels per proof: {tot:.4f} ms  ({', '.join(parts)} ms)")
        else:
            ms = {"dense": [], "csr": []}
            for _ in range(a.rounds):
                for f, _c in forms:
                    out, dt = timed(lambda: pipes[f].prove_all(t))
                    ms[f].append(dt / len(t))
                    if f == "dense":
                        want = out
                    else:
                        assert out == want, "CSR and dense proofs differ"
            tv = {}
            if not a.no_verify:
                pr = sonic_amd.Proof.from_bytes(want[0], Q)
                tt = [v % R for v in t[0]]
                for f, circ in forms:
                    ok, tv[f] = timed(lambda: sonic_amd.verify(g, circ, pr, tt[4], tt[5], list(zip(tt[6:6 + Q], tt[6 + Q:6 + 2 * Q]))))
                    assert ok
            print(name)
            print(f"  host bytes handed over   dense {host_dense / 1e6:10.3f} MB   csr {host_csr / 1e6:10.3f} MB")
            print(f"  circuit HBM per handle   dense {hbm_dense / 1e6:10.3f} MB   csr {hbm_csr / 1e6:10.3f} MB")
            print(f"  sonic_prover_new*        dense {t_new['dense']:10.2f} ms   csr {t_new['csr']:10.2f} ms")
            print(f"  prepare                  dense {t_prep['dense']:10.2f} ms   csr {t_prep['csr']:10.2f} ms")
            print(f"  streamed ms / proof      dense {' '.join(f'{v:.3f}' for v in ms['dense'])}   csr {' '.join(f'{v:.3f}' for v in ms['csr'])}")
            if tv:
                print(f"  host verify              dense {tv['dense']:10.1f} ms   csr {tv['csr']:10.1f} ms")
        sys.stdout.flush()
        for pipe in pipes.values():
            pipe.close()
    for g in srs_by_n.values():
        g.close()


if __name__ == "__main__":
    main()
