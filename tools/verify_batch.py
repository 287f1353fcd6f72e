"""The batched verifier (sonic_amd.Verifier) against consecutive sonic_verify[_csr] calls, shape by shape, on one GPU.

Per shape and batch size K: ms per proof of Verifier.verify_batch (median of --reps calls, fixed seed) and of sequential sonic_verify
calls on proofs of the same batch in the same process (at most --seq-cap calls are timed: the cost per proof does not depend on K);
the split of one batched call into validation kernel, s-kernel, the MSMs, the pairing tail and the rest, from the library's per-launch
event timer and its host phases (sonic_profile_*; a call of its own, the timer adds events around every launch); and the streamed
prove time per proof of the same shape from the same run (two handles, sonic_amd.ProverPipeline).  A batch cycles through --distinct
proofs of the shape (distinct transcripts); the verifier has no notion of a repeated proof, so its cost is that of K different ones.

    python tools/verify_batch.py [--shapes 14:2:rnd:dense,16:64:4:csr,18:2:rnd:csr] [--batches 1,16,64,1024] [--reps 3]
"""
import argparse
import ctypes as C
import os
import random
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import sonic_amd  # noqa: E402
from sonic_amd import _lib, workload  # noqa: E402

R = sonic_amd.R_MODULUS
SEED = bytes(range(32))
PARTS = [("validation kernel", ["k_g1_validate"]), ("s-kernel", ["k_s_of_uv_batch", "k_s_of_uv_finish"]), ("MSMs", ["verify_batch:msm"]),
         ("pairing tail", ["verify_batch:host_pairing"]), ("decode", ["verify_batch:host_decode"]), ("scalars + digest", ["verify_batch:host_scalars"])]


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
    return n, sp, asg


def timed(f):
    t = time.perf_counter()
    r = f()
    return r, (time.perf_counter() - t) * 1e3


def prof(L, name):
    ms, cnt = C.c_double(0), C.c_int64(0)
    L.sonic_profile_get(name.encode(), C.byref(ms), C.byref(cnt))
    return ms.value


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="14:2:rnd:dense,16:64:4:csr,18:2:rnd:csr", help="log2n:Q:(rnd | max entries per row):(dense | csr), comma-separated")
    ap.add_argument("--batches", default="1,16,64,1024")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--distinct", type=int, default=64)
    ap.add_argument("--seq-cap", type=int, default=8)
    a = ap.parse_args()
    _lib.check(_lib.lib().sonic_init(0))
    L = _lib.lib()
    batches = [int(k) for k in a.batches.split(",")]
    for log2n, Q, kind, form in (s.split(":") for s in a.shapes.split(",")):
        log2n, Q = int(log2n), int(Q)
        n, sp, asg = make(log2n, Q, kind)
        circuit = sp if form == "csr" else sp.to_dense()
        g = sonic_amd.SRS.new(7 * n + 9, 3, 5)
        pipe = sonic_amd.ProverPipeline(g, circuit)
        pipe.set_assignment(asg)
        pyr = random.Random(log2n * 1000 + Q)
        nd = min(a.distinct, max(batches))
        trs = [[pyr.randrange(1, R) for _ in range(8 + 2 * Q)] for _ in range(nd)]
        pipe.prove_all(trs[:2])                                        # warm-up (grows the workspaces)
        proofs, t_prove = timed(lambda: pipe.prove_all(trs))
        pipe.close()
        vtr = [(t[4], t[5], list(zip(t[6:6 + Q], t[6 + Q:6 + 2 * Q]))) for t in trs]
        print(f"n=2^{log2n} Q={Q} {'rndCircuit' if kind == 'rnd' else '<=' + kind + ' nnz/row'} ({form}, nnz={sp.nnz}): "
              f"streamed prove {t_prove / nd:.3f} ms / proof ({nd} proofs)")
        ver, t_new = timed(lambda: sonic_amd.Verifier(g, circuit))
        print(f"  sonic_verifier_new{'_csr' if form == 'csr' else ''}: {t_new:.1f} ms")
        assert ver.verify_batch(proofs[:2], vtr[:2], seed=SEED)         # warm-up
        for K in batches:
            bp, bt = [proofs[k % nd] for k in range(K)], [vtr[k % nd] for k in range(K)]
            ms = []
            for _ in range(a.reps):
                ok, dt = timed(lambda: ver.verify_batch(bp, bt, seed=SEED))
                assert ok
                ms.append(dt)
            nseq = min(K, a.seq_cap)
            _, t_seq = timed(lambda: [sonic_amd.verify(g, circuit, sonic_amd.Proof.from_bytes(bp[k], Q), *bt[k]) for k in range(nseq)])
            L.sonic_profile_enable(1)
            L.sonic_profile_reset()
            ok, wall = timed(lambda: ver.verify_batch(bp, bt, seed=SEED))
            L.sonic_profile_enable(0)
            parts, known = [], 0.0
            for label, names in PARTS:
                v = sum(prof(L, nm) for nm in names)
                known += v
                parts.append(f"{label} {v / K:.3f}")
            parts.append(f"everything else {max(wall - known, 0.0) / K:.3f}")
            med = statistics.median(ms)
            print(f"  K={K:5d}  batched {med / K:9.3f} ms / proof (call {med:9.1f} ms; runs {' '.join(f'{v:.1f}' for v in ms)})   "
                  f"sequential sonic_verify {t_seq / nseq:8.2f} ms / proof ({nseq} calls)   ratio {t_seq / nseq / (med / K):7.1f}x   "
                  f"verify / prove {med / K / (t_prove / nd):.2f}")
            print(f"           split, ms / proof (timed call {wall:.1f} ms): {', '.join(parts)}")
            sys.stdout.flush()
        # one rejected proof in a batch of 64: the cost of naming it (every proof folded on its own)
        K = min(64, max(batches))
        bp, bt = [proofs[k % nd] for k in range(K)], [vtr[k % nd] for k in range(K)]
        y, z, yzs = bt[K - 1]
        bt[K - 1] = (y, (z + 1) % R, yzs)
        (ok, each), dt = timed(lambda: ver.verify_batch(bp, bt, seed=SEED, each=True))
        assert not ok and each == [True] * (K - 1) + [False]
        print(f"  K={K:5d}  one rejected proof, each=True: {dt / K:.3f} ms / proof (call {dt:.1f} ms)")
        sys.stdout.flush()
        ver.close()
        g.close()


if __name__ == "__main__":
    main()
