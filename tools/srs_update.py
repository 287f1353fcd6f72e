#!/usr/bin/env python3
"""Writes profiles/r17_srs_update.txt on one MI355X: what the updatable SRS costs, everything measured in this one process on one GPU.

  resources  VGPRs / SGPRs / scratch / LDS / occupancy of the new kernels and of their neighbours (the compiler's remarks)
  (a)        SRS.check and SRS.update at d = 2^16, 2^19, 2^21, and beside them SRS.new and SRS.load (uncompressed container, with the G2
             half) of the same string: wall ms, best of five after one warm-up, with the spread (max - min of the five).  At every size
             the source string and one updated string must pass the check, or the run stops
  (b)        the split of one check and one update by kernel (HIP-event time, sonic_profile_get): scaling kernels, normalisation, table
             build, MSM kernels, G2 sum, and "host" = wall time of the profiled call minus every kernel in it (for the check: the eight
             Miller loops and four final exponentiations, the MSMs' host tails, the point fetches)

Run from the repository root after the library is built:  python tools/srs_update.py [--quick] [--sizes 16,19,21] [--resources-only]
--resources-only needs no GPU."""
import ctypes as C
import os
import re
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
CSRC = os.path.join(ROOT, "sonic_amd", "csrc")
R = 0x73EDA753299D7D483339D80809A1D80553BDA402FFFE5BFEFFFFFFFF00000001
QUICK = "--quick" in sys.argv
SIZES = [int(s) for s in sys.argv[sys.argv.index("--sizes") + 1].split(",")] if "--sizes" in sys.argv else ([12, 14] if QUICK else [16, 19, 21])
OUT = os.path.join(ROOT, "profiles", "r17_srs_update.txt")
out_lines = []

SCALE = {"k_g1_scale_each", "k_g2_scale_each"}
NORMALISE = {"k_batch_affine", "k_g2_batch_affine"}
TABLES = {"k_table_step", "k_ps_chunk", "k_ps_step", "k_ps_apply", "k_sym_sum"}
G2SUM = {"k_g2_scale_each", "k_g2_sum", "k_srs_check_rho"}
FETCH = {"k_points_to_bytes", "k_g2_points_to_bytes"}


def say(line=""):
    print(line, flush=True)
    out_lines.append(line)


def resources():
    say("## kernel resources (hipcc --offload-arch=gfx950 -O3 -Rpass-analysis=kernel-resource-usage)")
    say("%-24s %6s %6s %6s %10s %8s %10s" % ("kernel", "VGPRs", "AGPRs", "SGPRs", "scratch B", "LDS B", "waves/SIMD"))
    want = {"srs.hip": ["k_g1_scale_each", "k_srs_check_rho", "k_srs_points"], "srs_g2.hip": ["k_g2_scale_each", "k_g2_sum", "k_g2_srs_points", "k_g2_points_from_bytes"]}
    procs = {f: subprocess.Popen(["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-Rpass-analysis=kernel-resource-usage", "-c",
                                  os.path.join(CSRC, f), "-o", os.devnull], stderr=subprocess.PIPE, text=True) for f in want}
    for f, names in want.items():
        err = procs[f].communicate()[1]
        for name in names:
            m = re.search(r"Function Name: \S*%s\S*.*?TotalSGPRs: (\d+).*?VGPRs: (\d+).*?AGPRs: (\d+).*?ScratchSize \[bytes/lane\]: (\d+).*?Occupancy \[waves/SIMD\]: (\d+)"
                          r".*?LDS Size \[bytes/block\]: (\d+)" % name, err, re.S)
            say("%-24s %6s %6s %6s %10s %8s %10s" % ((name, m.group(2), m.group(3), m.group(1), m.group(4), m.group(6), m.group(5)) if m else (name,) + ("?",) * 6))
    say("(k_srs_points, k_g2_srs_points, k_g2_points_from_bytes: the neighbours, for comparison)")
    say()


def five(fn):
    fn()
    ts = []
    for _ in range(5):
        t = time.perf_counter()
        fn()
        ts.append((time.perf_counter() - t) * 1e3)
    return min(ts), max(ts) - min(ts)


def main():
    resources()
    if "--resources-only" in sys.argv:
        say("No GPU run was made: the resource table above is all this file holds.")
        with open(OUT, "w") as f:
            f.write("\n".join(out_lines) + "\n")
        return
    import sonic_amd as sonic
    from sonic_amd import _lib
    L = _lib.lib()
    _lib.check(L.sonic_init(0))
    seed = bytes(range(32))

    def split(fn):
        """{kernel name: ms} of one profiled fn() and its wall time"""
        L.sonic_profile_enable(1)
        try:
            L.sonic_profile_reset()
            t = time.perf_counter()
            fn()
            wall = (time.perf_counter() - t) * 1e3
            buf = C.create_string_buffer(1 << 16)
            L.sonic_profile_names(buf, len(buf))
            out = {}
            for name in buf.value.decode().split("\n"):
                ms, cnt = C.c_double(0), C.c_int64(0)
                L.sonic_profile_get(name.encode(), C.byref(ms), C.byref(cnt))
                if cnt.value:
                    out[name] = ms.value
            return out, wall
        finally:
            L.sonic_profile_enable(0)

    say("## (a) wall ms per call, best of five after one warm-up (spread = max - min of the five)")
    say("%-6s %20s %20s %20s %20s" % ("d", "check", "update", "SRS.new (+ G2 half)", "SRS.load (with G2)"))
    splits = {}
    with tempfile.TemporaryDirectory() as tmp:
        for lg in SIZES:
            d = 1 << lg
            x, alpha, x1, a1 = 0x1234567 + lg, 0x7654321 + lg, 0xabcdef01, 0x10fedcba

            def new():
                s = sonic.SRS.new(d, x, alpha)
                s.g2_points(0, 0, 1)                       # the G2 half: an update writes both halves, so the comparison makes both
                return s
            srs = new()
            path = os.path.join(tmp, "srs")
            srs.save(path, g2=True)

            def update():
                srs.update(x1, a1, seed=seed)[0].close()
            t_check, t_update = five(lambda: srs.check(seed)), five(update)
            t_new, t_load = five(lambda: new().close()), five(lambda: sonic.SRS.load(path).close())
            assert srs.check(seed) == (True, 0)
            updated = srs.update(x1, a1, seed=seed)[0]     # what was timed is also right at this size: the updated string passes the check
            assert updated.check(seed) == (True, 0)
            updated.close()
            say("2^%-4d %12.1f (%5.1f) %12.1f (%5.1f) %12.1f (%5.1f) %12.1f (%5.1f)" % ((lg,) + t_check + t_update + t_new + t_load))
            splits[lg] = (split(lambda: srs.check(seed)), split(update))
            srs.close()
            os.unlink(path)
    say()
    say("## (b) one profiled call split by kernel (ms of HIP-event time; host = wall of the profiled call - all kernels)")
    say("%-6s %-7s %9s %9s %9s %9s %9s %9s %9s %9s" % ("d", "call", "scaling", "normalise", "tables", "MSMs", "G2 sum", "fetches", "host", "wall"))
    for lg, (chk, upd) in splits.items():
        for label, (k, wall) in (("check", chk), ("update", upd)):
            g2sum = sum(v for n, v in k.items() if n in G2SUM) if label == "check" else 0.0
            scale = sum(v for n, v in k.items() if n in SCALE) if label == "update" else 0.0
            norm = sum(v for n, v in k.items() if n in NORMALISE)
            tabs = sum(v for n, v in k.items() if n in TABLES)
            fetch = sum(v for n, v in k.items() if n in FETCH)
            rest = sum(k.values()) - g2sum - scale - norm - tabs - fetch               # what is left are the MSM chains' kernels
            say("2^%-4d %-7s %9.1f %9.1f %9.1f %9.1f %9.1f %9.1f %9.1f %9.1f" % (lg, label, scale, norm, tabs, rest, g2sum, fetch, wall - sum(k.values()), wall))
    say("(normalise: every k_batch_affine / k_g2_batch_affine launch of the call -- in an update the bases' and the window tables'.")
    say(" G2 sum of a check: k_srs_check_rho, k_g2_scale_each over 128-bit scalars and k_g2_sum, two bases.  The profiled call runs with")
    say(" an event pair around every launch and is slower than the calls of (a).)")
    if not QUICK:
        with open(OUT, "w") as f:
            f.write("\n".join(out_lines) + "\n")


if __name__ == "__main__":
    main()
