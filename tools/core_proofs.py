#!/usr/bin/env python3
"""Writes profiles/r15_core_proofs.txt on one MI355X, in one process: what a core proof (include/sonic_hip.h, "Core proofs": R, T, a, W_a,
b, W_b, W_t, s and no signature) costs to make and to check beside the reference-shaped proof.  Every core figure sits beside the
unchanged full-proof call on the same handles in the same run.

  (a)  ms per proof, assignment resident: sonic_prover_prove against sonic_prover_prove_core, streamed over two handles from one thread
       (submit / collect) and one at a time -- rndCircuit n = 2^14 and 2^18, Q = 2, d = 8n; the sparse circuit n = 2^16, Q = 64, at most 4
       non-zeros per row
  (b)  blocking sonic_prover_prove_fs against sonic_prover_prove_core_fs at n = 2^14 and 2^18
  (c)  Verifier.verify_batch against verify_core_batch at n = 2^14, Q = 2, K in {1, 64, 1024}, and at the Q = 64 shape, K in {1, 64}
       (the batches cycle over four distinct proofs: the verifier's work does not depend on their being distinct)
  (d)  proof bytes per form

Method: one warm-up, then five rounds; in every round the legs that are compared run one after the other (full, core, full, core, ...),
so that a drift of the machine meets both alike.  Best of the five, and the spread (max - min) beside it.

Run from the repository root after the library is built:  python tools/core_proofs.py [--quick]"""
import os
import random
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
    with open(os.path.join(ROOT, "profiles", "r15_core_proofs.txt"), "w") as f:
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


def main():
    import sonic_amd as sonic
    from sonic_amd import _lib
    from sonic_amd.workload import big_circuit, sparse_circuit
    _lib.check(_lib.lib().sonic_init(0))
    pyr = random.Random(15)
    draw = lambda Q: [pyr.randrange(1, R) for _ in range(8 + 2 * Q)]      # noqa: E731
    verdicts = []

    def rnd_shape(lg, Q):
        n = 1 << lg
        b = big_circuit(n + Q, n, Q)
        return n, Q, sonic.ArithCircuit(sonic.GateWeights(b["wL"], b["wR"], b["wO"]), b["cs"]), sonic.Assignment(b["aL"], b["aR"], b["aO"])

    def sparse_shape(lg, Q):
        n = 1 << lg
        s = sparse_circuit(n + Q, n, Q, 4)
        return n, Q, sonic.SparseCircuit(n, Q, s["row_ptr"], s["col"], s["val"], s["cs"]), sonic.Assignment(s["aL"], s["aR"], s["aO"])

    shapes = [("rndCircuit n = 2^%d, Q = 2" % lg, lambda lg=lg: rnd_shape(lg, 2), lg) for lg in ([10, 12] if QUICK else [14, 18])]
    shapes.append(("sparse (<= 4 per row) n = 2^%d, Q = %d" % ((10, 8) if QUICK else (16, 64)), lambda: sparse_shape(*((10, 8) if QUICK else (16, 64))), None))
    kept = {}          # what leg (c) reuses: (srs, circuit, Q, full proofs with their transcripts)
    for label, make, lg in shapes:
        n, Q, circuit, asg = make()
        srs = sonic.SRS.new(8 * n, pyr.randrange(2, R), pyr.randrange(2, R))
        A, B = sonic.Prover(srs, circuit), sonic.Prover(srs, circuit)
        for p in (A, B):
            p.set_assignment(asg)
        N = 2 if n >= 1 << 18 else 8 if Q > 8 else 16                   # proofs per timing (even: two handles)
        trs = [draw(Q) for _ in range(N)]
        check = A.prove_bytes(trs[0])                                   # (the workspaces grow on the first proof)
        assert A.prove_core_bytes(trs[0][:6]) == check[:576] == B.prove_core_bytes(trs[0][:6])
        B.prove_bytes(trs[0])

        def streamed(submit, collect):
            submit(A, trs[0]); submit(B, trs[1])
            for k in range(2, N, 2):
                collect(A); submit(A, trs[k])
                collect(B); submit(B, trs[k + 1])
            collect(A); collect(B)

        legs = [
            ("prove, streamed over two handles", lambda: streamed(lambda p, t: p.submit(t), lambda p: p.collect())),
            ("prove_core, streamed over two handles", lambda: streamed(lambda p, t: p.submit_core(t[:6]), lambda p: p.collect_core())),
            ("prove, one at a time", lambda: [A.prove_bytes(t) for t in trs]),
            ("prove_core, one at a time", lambda: [A.prove_core_bytes(t[:6]) for t in trs]),
        ]
        say("## (a) %s, d = 8n: ms per proof (%d proofs per timing, %d MSMs in a full proof, 5 in a core proof)" % (label, N, 7 + 4 * Q))
        say("%-46s %10s %10s" % ("leg", "best", "spread"))
        res = {k: (t / N, s / N) for k, (t, s) in alternating(legs).items()}
        for name, _ in legs:
            say("%-46s %10.3f %10.3f" % (name, *res[name]))
        for mode in ("streamed over two handles", "one at a time"):
            full, core = res["prove, " + mode], res["prove_core, " + mode]
            say("core / full, %s = %.3f" % (mode, core[0] / full[0]))
            verdicts.append(("(a) %s, %s: core costs less than full by more than the larger spread (%.3f < %.3f - %.3f)"
                             % (label, mode, core[0], full[0], max(core[1], full[1])), full[0] - core[0] > max(core[1], full[1])))
        say()

        if lg is not None:
            # ---- (b) ----
            digest = sonic.fs_circuit_digest(circuit)
            M = 2 if n >= 1 << 18 else 8
            seeds = [bytes([k + 1]) * 32 for k in range(M)]
            A.prove_fs(digest, seeds[0])
            raw, y, z = A.prove_core_fs(digest, seeds[0])
            assert sonic.fs_core_challenges(srs, circuit, raw) == (y, z)
            legs = [("blocking prove_fs (six passes)", lambda: [A.prove_fs(digest, s) for s in seeds]),
                    ("blocking prove_core_fs (three passes)", lambda: [A.prove_core_fs(digest, s) for s in seeds])]
            say("## (b) %s: ms per Fiat-Shamir proof, one handle (%d proofs per timing)" % (label, M))
            say("%-46s %10s %10s" % ("leg", "best", "spread"))
            res = {k: (t / M, s / M) for k, (t, s) in alternating(legs).items()}
            for name, _ in legs:
                say("%-46s %10.3f %10.3f" % (name, *res[name]))
            full, core = res[legs[0][0]], res[legs[1][0]]
            say("core / full = %.3f" % (core[0] / full[0]))
            verdicts.append(("(b) %s: prove_core_fs costs less than prove_fs by more than the larger spread (%.3f < %.3f - %.3f)"
                             % (label, core[0], full[0], max(core[1], full[1])), full[0] - core[0] > max(core[1], full[1])))
            say()
        if lg is None or n == 1 << (10 if QUICK else 14):
            four = trs[:4]
            kept[label] = (srs, circuit, Q, [(A.prove_bytes(t), t) for t in four])
            for p in (A, B):
                p.close()
        else:
            for p in (A, B):
                p.close()
            srs.close()

    # ---- (c) ----
    for label, (srs, circuit, Q, proofs) in kept.items():
        v = sonic.Verifier(srs, circuit)
        Ks = [1, 8] if QUICK else [1, 64, 1024] if Q == 2 else [1, 64]
        say("## (c) %s: ms per batch, %d checks per full proof against 3 and s(z, y)" % (label, 4 + 3 * Q))
        say("%-34s %8s %10s %10s %12s" % ("call", "K", "best", "spread", "ms / proof"))
        seed = bytes(range(32))
        for K in Ks:
            batch = [proofs[k % len(proofs)] for k in range(K)]
            fulls = [p for p, _ in batch]
            cores = [p[:576] for p in fulls]
            ftr = [(t[4], t[5], list(zip(t[6:6 + Q], t[6 + Q:6 + 2 * Q]))) for _, t in batch]
            yzs = [(t[4], t[5]) for _, t in batch]
            assert v.verify_batch(fulls, ftr, seed=seed) is True and v.verify_core_batch(cores, yzs, seed=seed) is True
            legs = [("verify_batch", lambda: v.verify_batch(fulls, ftr, seed=seed)), ("verify_core_batch", lambda: v.verify_core_batch(cores, yzs, seed=seed))]
            res = alternating(legs)
            for name, _ in legs:
                say("%-34s %8d %10.3f %10.3f %12.4f" % (name, K, res[name][0], res[name][1], res[name][0] / K))
            say("core / full at K = %d: %.3f" % (K, res["verify_core_batch"][0] / res["verify_batch"][0]))
        v.close()
        srs.close()
        say()

    # ---- (d) ----
    say("## (d) proof bytes per form")
    say("%-8s %14s %14s %14s %14s" % ("Q", "full", "full, compr.", "core", "core, compr."))
    for Q in (1, 2, 64):
        say("%-8d %14d %14d %14d %14d" % (Q, _lib.lib().sonic_proof_size(Q), _lib.lib().sonic_proof_size_compressed(Q), _lib.CORE_PROOF_SIZE, _lib.CORE_PROOF_SIZE_COMPRESSED))
    say()
    say("## the condition: at every shape in (a) and (b) the core form costs less than the full form by more than the larger spread")
    for text, ok in verdicts:
        say("%s  %s" % ("HOLDS" if ok else "FAILS", text))
    if not QUICK:
        write()


if __name__ == "__main__":
    main()
