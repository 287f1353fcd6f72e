#!/usr/bin/env python3
"""Writes profiles/r16_helped.txt on one MI355X, in one process: what helped verification (include/sonic_hip.h, "Helped verification") costs
the helper and saves the verifier.  Every figure sits beside the call it is compared with, on the same handles in the same run.

  (a)  the helper, ms per pair at K = 64: sonic_prover_aggregate_core, next to sonic_prover_hsc_prove(m = K) on the same handle with the
       same u, v, and next to the streamed core-proof time (two handles, submit / collect) -- rndCircuit n = 2^14 and 2^18, Q = 2, d = 8n;
       the sparse circuit n = 2^16, Q = 64, at most 4 non-zeros per row; each shape on a prepared and on an unprepared handle
  (b)  the verifier: Verifier.verify_core_batch_helped next to verify_core_batch on the same proofs -- n = 2^14 and 2^18, Q = 2, at
       K in {1, 64, 1024}; n = 2^16, Q = 64 at K = 64 (the batches cycle over four distinct proofs; the aggregate is over all K pairs)
  (c)  the compiler's report of the new kernels (hipcc -Rpass-analysis=kernel-resource-usage over sonic_amd/csrc/aggregate.hip)

Method: one warm-up, then five rounds; in every round the legs that are compared run one after the other, so that a drift of the machine
meets both alike.  Best of the five, and the spread (max - min) beside it.

Run from the repository root after the library is built:  python tools/helped.py [--quick]"""
import os
import random
import re
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
R = 0x73EDA753299D7D483339D80809A1D80553BDA402FFFE5BFEFFFFFFFF00000001
QUICK = "--quick" in sys.argv
ROUNDS = 5
out_lines = []


def say(line=""):
    print(line, flush=True)
    out_lines.append(line)


def write():
    with open(os.path.join(ROOT, "profiles", "r16_helped.txt"), "w") as f:
        f.write("\n".join(out_lines) + "\n")


def alternating(legs, rounds=ROUNDS):
    """legs: [(name, fn)]; one warm-up of each, then `rounds` rounds of all legs in turn: {name: (best ms, spread ms)}"""
    for _, fn in legs:
        fn()
    ts = {name: [] for name, _ in legs}
    for _ in range(rounds):
        for name, fn in legs:
            t = time.perf_counter()
            fn()
            ts[name].append((time.perf_counter() - t) * 1e3)
    return {name: (min(v), max(v) - min(v)) for name, v in ts.items()}


def kernel_report():
    """(kernel, VGPRs, SGPRs, scratch bytes per lane, LDS bytes per block, waves per SIMD) of the k_agg_* kernels"""
    src = os.path.join(ROOT, "sonic_amd", "csrc", "aggregate.hip")
    cmd = [os.environ.get("HIPCC", "/opt/rocm/bin/hipcc"), "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-I", os.path.join(ROOT, "include"),
           "-Rpass-analysis=kernel-resource-usage", "-c", src, "-o", os.devnull]
    err = subprocess.run(cmd, capture_output=True, text=True, timeout=600).stderr
    rows, cur = [], None
    for ln in err.splitlines():
        m = re.search(r"remark: Function Name: (\S+)", ln)
        if m:
            cur = {"name": m.group(1)}
            rows.append(cur)
            continue
        m = re.search(r"remark:\s+(TotalSGPRs|VGPRs|ScratchSize \[bytes/lane\]|Occupancy \[waves/SIMD\]|LDS Size \[bytes/block\]): (\d+)", ln)
        if m and cur is not None:
            cur[m.group(1)] = int(m.group(2))
    out = []
    for r in rows:
        m = re.search(r"(k_agg_\w+?)E", r["name"])
        if m:
            out.append((m.group(1), r.get("VGPRs"), r.get("TotalSGPRs"), r.get("ScratchSize [bytes/lane]"), r.get("LDS Size [bytes/block]"), r.get("Occupancy [waves/SIMD]")))
    return out


def main():
    import sonic_amd as sonic
    from sonic_amd import _lib
    from sonic_amd.protocol import _hsc_to_bytes
    from sonic_amd.workload import big_circuit, sparse_circuit
    _lib.check(_lib.lib().sonic_init(0))
    pyr = random.Random(16)
    verdicts, sides = [], []

    def rnd_shape(lg, Q):
        n = 1 << lg
        b = big_circuit(n + Q, n, Q)
        return n, Q, sonic.ArithCircuit(sonic.GateWeights(b["wL"], b["wR"], b["wO"]), b["cs"]), sonic.Assignment(b["aL"], b["aR"], b["aO"])

    def sparse_shape(lg, Q):
        n = 1 << lg
        s = sparse_circuit(n + Q, n, Q, 4)
        return n, Q, sonic.SparseCircuit(n, Q, s["row_ptr"], s["col"], s["val"], s["cs"]), sonic.Assignment(s["aL"], s["aR"], s["aO"])

    shapes = [("rndCircuit n = 2^%d, Q = 2" % lg, lambda lg=lg: rnd_shape(lg, 2), [1, 8] if QUICK else [1, 64, 1024]) for lg in ([10, 12] if QUICK else [14, 18])]
    shapes.append(("sparse (<= 4 per row) n = 2^%d, Q = %d" % ((10, 8) if QUICK else (16, 64)), lambda: sparse_shape(*((10, 8) if QUICK else (16, 64))), [8] if QUICK else [64]))
    KA = 8 if QUICK else 64
    for label, make, Ks in shapes:
        n, Q, circuit, asg = make()
        srs = sonic.SRS.new(8 * n, pyr.randrange(2, R), pyr.randrange(2, R))
        yzs = [(pyr.randrange(1, R), pyr.randrange(1, R)) for _ in range(KA)]
        wd = sonic.fs_weights_digest(circuit)
        four = None
        for prepare in (True, False):
            A, B = sonic.Prover(srs, circuit, prepare=prepare), sonic.Prover(srs, circuit, prepare=prepare)
            for p in (A, B):
                p.set_assignment(asg)
            agg = A.aggregate_core(yzs, wd)
            u, v = (int.from_bytes(agg[-64:-32], "little"), int.from_bytes(agg[-32:], "little"))
            assert _hsc_to_bytes(A.hsc_prove(yzs, u, v)) == agg
            N = 2 if n >= 1 << 18 else 8 if Q > 8 else 16
            trs = [[pyr.randrange(1, R) for _ in range(6)] for _ in range(N)]

            def streamed():
                A.submit_core(trs[0]); B.submit_core(trs[1])
                for k in range(2, N, 2):
                    A.collect_core(); A.submit_core(trs[k])
                    B.collect_core(); B.submit_core(trs[k + 1])
                A.collect_core(); B.collect_core()

            legs = [("aggregate_core (K = %d)" % KA, lambda: A.aggregate_core(yzs, wd)), ("hsc_prove (m = %d), same u, v" % KA, lambda: A.hsc_prove(yzs, u, v)),
                    ("prove_core, streamed over two handles", streamed)]
            per = {legs[0][0]: KA, legs[1][0]: KA, legs[2][0]: N}
            say("## (a) %s, d = 8n, %s handle: ms per pair (per proof for prove_core)" % (label, "prepared" if prepare else "unprepared"))
            say("%-46s %10s %10s" % ("leg", "best", "spread"))
            res = {k: (t / per[k], s / per[k]) for k, (t, s) in alternating(legs).items()}
            for name, _ in legs:
                say("%-46s %10.3f %10.3f" % (name, *res[name]))
            ag, hs = res[legs[0][0]], res[legs[1][0]]
            say("aggregate_core / hsc_prove = %.3f;  aggregate_core / streamed core proof = %.3f" % (ag[0] / hs[0], ag[0] / res[legs[2][0]][0]))
            verdicts.append(("(a) %s, %s: the aggregator is not slower per pair than hsc_prove by more than the larger spread (%.3f <= %.3f + %.3f)"
                             % (label, "prepared" if prepare else "unprepared", ag[0], hs[0], max(ag[1], hs[1])), ag[0] <= hs[0] + max(ag[1], hs[1])))
            say()
            if prepare:
                t4 = [[pyr.randrange(1, R) for _ in range(6)] for _ in range(4)]
                four = [(A.prove_core_bytes(t), (t[4], t[5])) for t in t4]
                helper = A
                B.close()
            else:
                A.close(); B.close()

        # ---- (b) ----
        ver = sonic.Verifier(srs, circuit)
        say("## (b) %s: ms per batch of K core proofs" % label)
        say("%-34s %8s %10s %10s %12s" % ("call", "K", "best", "spread", "ms / proof"))
        seed = bytes(range(32))
        for K in Ks:
            cores = [four[k % 4][0] for k in range(K)]
            pairs = [four[k % 4][1] for k in range(K)]
            aggK = helper.aggregate_core(pairs, wd)
            assert ver.verify_core_batch(cores, pairs, seed=seed) is True and ver.verify_core_batch_helped(cores, pairs, aggK, seed=seed) is True
            legs = [("verify_core_batch", lambda: ver.verify_core_batch(cores, pairs, seed=seed)),
                    ("verify_core_batch_helped", lambda: ver.verify_core_batch_helped(cores, pairs, aggK, seed=seed))]
            res = alternating(legs)
            for name, _ in legs:
                say("%-34s %8d %10.3f %10.3f %12.4f" % (name, K, res[name][0], res[name][1], res[name][0] / K))
            h, u_ = res["verify_core_batch_helped"], res["verify_core_batch"]
            side = "helped is faster" if u_[0] - h[0] > max(h[1], u_[1]) else "unhelped is faster" if h[0] - u_[0] > max(h[1], u_[1]) else "within the spread"
            say("helped / unhelped at K = %d: %.3f  (%s)" % (K, h[0] / u_[0], side))
            sides.append("(b) %s, K = %d: helped / unhelped = %.3f: %s" % (label, K, h[0] / u_[0], side))
        ver.close()
        helper.close()
        srs.close()
        say()

    say("## (c) the new kernels, as the compiler reports them for gfx950")
    say("%-22s %8s %8s %16s %16s %12s" % ("kernel", "VGPRs", "SGPRs", "scratch B/lane", "LDS B/block", "waves/SIMD"))
    for row in kernel_report():
        say("%-22s %8s %8s %16s %16s %12s" % row)
    say("(k_agg_s_of_y_csc stages the tile's J x Q powers in dynamic LDS when they fit 48 KiB: J Q 32 bytes per block, not in the static figure)")
    say()
    say("## the condition of (a): at every shape the aggregator is not slower per pair than hsc_prove(m = K) by more than the larger spread")
    for text, ok in verdicts:
        say("%s  %s" % ("HOLDS" if ok else "FAILS", text))
    say()
    say("## (b), which side of break-even each shape fell")
    for s in sides:
        say(s)
    if not QUICK:
        write()


if __name__ == "__main__":
    main()
