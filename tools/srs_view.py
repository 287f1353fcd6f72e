#!/usr/bin/env python3
"""Writes profiles/r14_srs_view.txt on one MI355X: what a circuit-sized view of a universal string (sonic_srs_for_circuit) costs and saves
beside the whole string's handle.  One process, one SRS generated at d = 2^21; for n in 2^10, 2^12, 2^14, 2^16, 2^18 (Q = 2, rndCircuit):

  (i)    the whole string's handle            (ii)  its view for (n, Q)            (iii)  a native SRS of d = 8n  (n = 2^18: (i) itself)

  memory   sonic_srs_device_bytes of (i) and (ii), and each handle's plan for an MSM of n terms (sonic_msm_plan)
  making   the time to make the view from the handle, and from both file containers (written here from (i), G1 only)
  proofs   ms per proof, streamed over two prepared handles (submit / collect) and one at a time (prove) on one of them: the best of five
           rounds after a warm-up round, spread = max - min; a round runs (i), (ii), (iii) one after the other, so the three alternate

Run from the repository root after the library is built:  python tools/srs_view.py [--quick] [--no-files]
No figure is written that was not collected: a part that is skipped or fails says so in the file."""
import ctypes as C
import os
import random
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
R = 0x73EDA753299D7D483339D80809A1D80553BDA402FFFE5BFEFFFFFFFF00000001
QUICK = "--quick" in sys.argv
NO_FILES = "--no-files" in sys.argv
OUT = os.path.join(ROOT, "profiles", "r14_srs_view_quick.txt" if QUICK else "r14_srs_view.txt")
out_lines = []


def say(line=""):
    print(line, flush=True)
    out_lines.append(line)
    with open(OUT, "w") as f:
        f.write("\n".join(out_lines) + "\n")


def clock(fn):
    t = time.perf_counter()
    r = fn()
    return (time.perf_counter() - t) * 1e3, r


def main():
    import sonic_amd as sonic
    from sonic_amd import _lib
    from sonic_amd.workload import big_circuit
    L = _lib.lib()
    _lib.check(L.sonic_init(0))
    pyr = random.Random(14)
    D_LG = 15 if QUICK else 21
    sizes = [8, 10, 12] if QUICK else [10, 12, 14, 16, 18]
    Q, d = 2, 1 << D_LG
    x, alpha = pyr.randrange(2, R), pyr.randrange(2, R)

    def plan(srs, n):
        c, w, sets = C.c_int(), C.c_int(), C.c_int()
        _lib.check(L.sonic_msm_plan(srs._h, n, C.byref(c), C.byref(w), C.byref(sets)))
        return "c = %d, %d windows, %d bucket set%s of 2^%d" % (c.value, w.value, sets.value, "" if sets.value == 1 else "s", c.value - 1)

    say("# circuit-sized SRS views under one string of d = 2^%d (Q = %d, rndCircuit)%s" % (D_LG, Q, "  [--quick: not the committed sizes]" if QUICK else ""))
    ms, full = clock(lambda: sonic.SRS.new(d, x, alpha))
    say("(i) generated on the GPU with its tables in %.0f ms; device bytes %d (%.2f GB); windows %s" % (ms, full.device_bytes, full.device_bytes / 2**30, full.windows))
    try:
        ms, _ = clock(lambda: full.g2_points(1, 0, 1))
        say("its G2 half, generated on first use (a view asks its source for four G2 elements): %.0f ms" % ms)
    except sonic.SonicError as e:
        say("its G2 half could not be generated (%s): the views below have none" % e.message)
    say()

    # ---- files: both containers, G1 only (the G2 half of a view is four points of either container) ----
    paths = {}
    tmp = None
    if NO_FILES:
        say("## making a view from a file: not collected (--no-files)")
    else:
        tmp = tempfile.TemporaryDirectory()
        for name, z in (("SONICSRS", False), ("SONICSRZ", True)):
            p = os.path.join(tmp.name, name)
            ms, _ = clock(lambda: full.save(p, g2=False, compressed=z))
            paths[name] = p
            say("wrote the string as %s without its G2 half: %d bytes in %.0f ms" % (name, os.path.getsize(p), ms))
    say()

    verdicts = []
    rows = []
    for lg in sizes:
        n = 1 << lg
        say("## n = 2^%d" % lg)
        b = big_circuit(n + Q, n, Q)
        circuit = sonic.ArithCircuit(sonic.GateWeights(b["wL"], b["wR"], b["wO"]), b["cs"])
        asg = sonic.Assignment(b["aL"], b["aR"], b["aO"])
        ms_view, view = clock(lambda: full.for_circuit(n, Q))
        say("view from the handle: %.1f ms; windows %s; device bytes %d (%.4f of (i))" % (ms_view, view.windows, view.device_bytes, view.device_bytes / full.device_bytes))
        for name, p in paths.items():
            ms, v2 = clock(lambda: sonic.SRS.load(p, circuit=(n, Q)))
            same = v2.windows == view.windows and sonic.fs_srs_id(v2) == sonic.fs_srs_id(view)
            say("view from the %s file: %.1f ms%s" % (name, ms, "" if same else "  (!! differs from the handle's view)"))
            v2.close()
        native = full if 8 * n == d else sonic.SRS.new(8 * n, x, alpha)
        cfg = [("(i) whole string", full), ("(ii) view", view), ("(iii) native d = 8n" + (" = (i)" if native is full else ""), native)]
        for name, srs in cfg:
            say("%-24s plan of an n-term MSM: %s" % (name, plan(srs, n)))
        trs = [[pyr.randrange(1, R) for _ in range(8 + 2 * Q)] for _ in range(4)]
        handles = {}
        for name, srs in cfg:
            if srs is full and name.startswith("(iii)"):
                handles[name] = handles["(i) whole string"]
                continue
            hs = [sonic.Prover(srs, circuit, prepare=True) for _ in range(2)]
            for h in hs:
                h.set_assignment(asg)
            handles[name] = hs
        ref_bytes = handles["(i) whole string"][0].prove_bytes(trs[0])
        for name, _ in cfg[1:]:
            if name.startswith("(ii)") and handles[name][0].prove_bytes(trs[0]) != ref_bytes:
                say("!! the view's proof differs from the whole string's")
                verdicts.append(False)
        N = {8: 100, 10: 100, 12: 60, 14: 30, 16: 10, 18: 3}[lg]

        def streamed(hs):
            A, B = hs
            A.submit(trs[0]); B.submit(trs[1])
            for k in range(1, N):
                A.collect(); A.submit(trs[2 * k % 4])
                B.collect(); B.submit(trs[(2 * k + 1) % 4])
            A.collect(); B.collect()

        def one_at_a_time(hs):
            for k in range(N):
                hs[0].prove_bytes(trs[k % 4])
        times = {(name, leg): [] for name, _ in cfg for leg in ("streamed", "one")}
        for rnd in range(6):                                  # round 0 warms up
            for name, _ in cfg:
                if handles[name] is handles["(i) whole string"] and name.startswith("(iii)"):
                    continue
                t, _ = clock(lambda: streamed(handles[name]))
                u, _ = clock(lambda: one_at_a_time(handles[name]))
                if rnd:
                    times[(name, "streamed")].append(t / (2 * N))
                    times[(name, "one")].append(u / N)
        say("%-24s %12s %10s %14s %10s   (ms per proof; %d + %d proofs per round)" % ("", "streamed", "spread", "one at a time", "spread", 2 * N, N))
        res = {}
        for name, _ in cfg:
            ts, to = times[(name, "streamed")], times[(name, "one")]
            if not ts:
                say("%-24s %12s" % (name, "see (i)"))
                res[name] = res["(i) whole string"]
                continue
            res[name] = (min(ts), max(ts) - min(ts), min(to), max(to) - min(to))
            say("%-24s %12.3f %10.3f %14.3f %10.3f" % ((name,) + res[name]))
        i_, ii_, iii_ = (res[name] for name, _ in cfg)
        say("(ii) / (i): streamed %.3f, one at a time %.3f;  (ii) / (iii): streamed %.3f, one at a time %.3f" % (ii_[0] / i_[0], ii_[2] / i_[2], ii_[0] / iii_[0], ii_[2] / iii_[2]))
        if lg <= 14:
            ok = i_[0] - ii_[0] > max(i_[1], ii_[1]) and i_[2] - ii_[2] > max(i_[3], ii_[3])
            verdicts.append(ok)
            say("condition (n <= 2^14: (ii) below (i) by more than the larger spread, both legs): %s" % ("met" if ok else "NOT met"))
        elif ii_[0] > i_[0] + max(i_[1], ii_[1]) or ii_[2] > i_[2] + max(i_[3], ii_[3]):
            say("(ii) is SLOWER than (i) here by more than the spread")
        rows.append((lg, view.device_bytes, i_, ii_, iii_))
        say()
        for name, hs in handles.items():
            if not (name.startswith("(iii)") and hs is handles["(i) whole string"]):
                for h in hs:
                    h.close()
        view.close()
        if native is not full:
            native.close()

    say("## summary (ms per proof streamed over two prepared handles / one at a time)")
    say("%-6s %14s %22s %22s %22s" % ("n", "view bytes", "(i) whole string", "(ii) view", "(iii) native d = 8n"))
    for lg, vb, i_, ii_, iii_ in rows:
        say("2^%-4d %14d %22s %22s %22s" % (lg, vb, "%.3f / %.3f" % (i_[0], i_[2]), "%.3f / %.3f" % (ii_[0], ii_[2]), "%.3f / %.3f" % (iii_[0], iii_[2])))
    say("whole string: %d device bytes" % full.device_bytes)
    say("condition at every n <= 2^14: %s" % ("met" if verdicts and all(verdicts) else "NOT met"))
    full.close()
    if tmp:
        tmp.cleanup()


if __name__ == "__main__":
    main()
