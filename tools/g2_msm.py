#!/usr/bin/env python3
"""Writes profiles/r18_g2_msm.txt on one MI355X: what the G2 MSM costs and what it does to the structure check, everything measured in
this one process on one GPU.

  (c)  VGPRs / AGPRs / SGPRs / scratch / LDS / occupancy of the G2 MSM's kernels (the compiler's remarks); printed first, needs no GPU
  (a)  srs.check(seed) at d = 2^16, 2^19, 2^21 with SONIC_G2_MSM=0 (the walk over all 128 bits of every randomizer) against unset (the
       MSM): wall ms, best of five alternating rounds after a warm-up of both, with the spread (max - min of the five).  Both must accept
       the string, or the run stops.  CONDITION, size by size: the default check is faster than the walk by more than the larger of the
       two spreads.  Then the split of one profiled default check by kernel (HIP-event time, sonic_profile_get)
  (b)  sonic_msm_g2_srs at n = 2^12, 2^16, 2^20 with uniformly random full-width scalars on the host, beside sonic_msm_g1_srs of the same
       n over the same string: wall ms (best of five, alternating), and the G2 call as mixed additions per second, n W / t with
       W = ceil(255 / c) windows

Run from the repository root after the library is built:  python tools/g2_msm.py [--quick] [--sizes 16,19,21] [--resources-only]
--resources-only needs no GPU and says in the file that (a) and (b) are not collected."""
import ctypes as C
import os
import re
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
CSRC = os.path.join(ROOT, "sonic_amd", "csrc")
QUICK = "--quick" in sys.argv
SIZES = [int(s) for s in sys.argv[sys.argv.index("--sizes") + 1].split(",")] if "--sizes" in sys.argv else ([10, 12] if QUICK else [16, 19, 21])
MSM_SIZES = [8, 10] if QUICK else [12, 16, 20]
OUT = os.path.join(ROOT, "profiles", "r18_g2_msm.txt")
KNOB = "SONIC_G2_MSM"
out_lines = []

SORT = {"k_part_hist", "k_part_scatter", "k_part_scatter_staged", "k_part_sort", "k_scan_tile_sums", "k_scan_top", "k_scan_apply", "k_g2_chunk_count"}
REDUCE = {"k_g2_bucket_combine", "k_g2_bucket_segments", "k_g2_sum"}


def say(line=""):
    print(line, flush=True)
    out_lines.append(line)


def write():
    with open(OUT, "w") as f:
        f.write("\n".join(out_lines) + "\n")


def resources():
    say("## (c) kernel resources (hipcc --offload-arch=gfx950 -O3 -Rpass-analysis=kernel-resource-usage)")
    say("%-28s %6s %6s %6s %10s %8s %10s" % ("kernel", "VGPRs", "AGPRs", "SGPRs", "scratch B", "LDS B", "waves/SIMD"))
    want = {"msm_g2.hip": ["k_g2_chunk_count", "k_g2_bucket_accum", "k_g2_bucket_combine", "k_g2_bucket_segments", "k_g2_msm_points_from_bytes"],
            "srs_g2.hip": ["k_g2_sum", "k_g2_scale_each"]}
    procs = {f: subprocess.Popen(["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-Rpass-analysis=kernel-resource-usage", "-c",
                                  os.path.join(CSRC, f), "-o", os.devnull], stderr=subprocess.PIPE, text=True) for f in want}
    for f, names in want.items():
        err = procs[f].communicate()[1]
        for name in names:
            m = re.search(r"Function Name: \S*%s\S*.*?TotalSGPRs: (\d+).*?VGPRs: (\d+).*?AGPRs: (\d+).*?ScratchSize \[bytes/lane\]: (\d+).*?Occupancy \[waves/SIMD\]: (\d+)"
                          r".*?LDS Size \[bytes/block\]: (\d+)" % name, err, re.S)
            say("%-28s %6s %6s %6s %10s %8s %10s" % ((name, m.group(2), m.group(3), m.group(1), m.group(4), m.group(6), m.group(5)) if m else (name,) + ("?",) * 6))
    say("(k_g2_sum: generalised to several ranges, the tree of the window sums; k_g2_scale_each: the walk the MSM replaces in the check, for comparison)")
    say()


def alternate(fns, rounds=5):
    """best and spread (max - min) of `rounds` timings per function, the functions taken in turn within every round, after one warm-up each"""
    for fn in fns:
        fn()
    ts = [[] for _ in fns]
    for _ in range(rounds):
        for i, fn in enumerate(fns):
            t = time.perf_counter()
            fn()
            ts[i].append((time.perf_counter() - t) * 1e3)
    return [(min(t), max(t) - min(t)) for t in ts]


def main():
    resources()
    if "--resources-only" in sys.argv:
        say("(a) and (b) are not collected: no MI355X run of this tool is recorded.  The resource table above is all this file holds.")
        write()
        return
    import numpy as np
    import sonic_amd as sonic
    from sonic_amd import _lib
    from sonic_amd.commitment import msm_g1_srs
    L = _lib.lib()
    _lib.check(L.sonic_init(0))
    seed = bytes(range(32))
    os.environ.pop(KNOB, None)

    def split(fn):
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

    say("## (a) srs.check(seed): wall ms, best of five alternating rounds after a warm-up (spread = max - min of the five)")
    say("%-6s %20s %20s %8s   %s" % ("d", KNOB + "=0 (walk)", "unset (MSM)", "ratio", "condition: faster by more than the larger spread"))
    splits, srs = {}, None
    for lg in SIZES:
        d = 1 << lg
        if srs is not None:
            srs.close()
        srs = sonic.SRS.new(d, 0x1234567 + lg, 0x7654321 + lg)
        srs.g2_points(0, 0, 1)                             # the G2 half, outside the timings

        def walk():
            os.environ[KNOB] = "0"
            try:
                assert srs.check(seed) == (True, 0)
            finally:
                del os.environ[KNOB]

        def msm():
            assert srs.check(seed) == (True, 0)
        (tw, sw), (tm, sm) = alternate([walk, msm])
        held = tw - tm > max(sw, sm)
        say("2^%-4d %12.1f (%5.1f) %12.1f (%5.1f) %7.2fx   %s" % (lg, tw, sw, tm, sm, tw / tm, "held" if held else "NOT held"))
        splits[lg] = split(msm)
    say()
    say("## the default check of (a), one profiled call split by kernel (ms of HIP-event time; host = wall of the profiled call - all kernels)")
    say("%-6s %9s %9s %9s %9s %9s %9s %9s" % ("d", "rho", "sort", "accum", "reduce", "G1 MSMs", "host", "wall"))
    for lg, (k, wall) in splits.items():
        rho = k.get("k_srs_check_rho", 0.0)
        accum = k.get("k_g2_bucket_accum", 0.0)
        reduce_ = sum(v for n, v in k.items() if n in REDUCE)
        # the sort kernels run for the G1 MSMs of the check as well: their share is counted with the sort
        sort = sum(v for n, v in k.items() if n in SORT)
        rest = sum(k.values()) - rho - accum - reduce_ - sort
        say("2^%-4d %9.1f %9.1f %9.1f %9.1f %9.1f %9.1f %9.1f" % (lg, rho, sort, accum, reduce_, rest, wall - sum(k.values()), wall))
    say("(sort: digits, both sort passes, scans and k_g2_chunk_count of the G2 chains AND of the check's seven G1 MSMs, which run the same kernels;")
    say(" reduce: k_g2_bucket_combine, k_g2_bucket_segments, k_g2_sum; G1 MSMs: every other kernel of the call; host: eight Miller loops, four final")
    say(" exponentiations, the Horner folds.  The profiled call runs with an event pair around every launch and is slower than the calls of (a).)")
    say()

    say("## (b) one MSM over the string of d = 2^%d, uniformly random full-width scalars on the host: wall ms, best of five alternating (spread)" % SIZES[-1])
    say("%-6s %4s %4s %20s %20s %8s %16s" % ("n", "c", "W", "sonic_msm_g2_srs", "sonic_msm_g1_srs", "G2 / G1", "G2 madd / s"))
    rs = np.random.default_rng(18)
    for lg in MSM_SIZES:
        n = 1 << lg
        if n > 2 * srs.srsD + 1:
            continue
        sc = rs.integers(0, 256, size=(n, 32), dtype=np.uint8)
        sc[:, 31] &= 0x3F                                  # below 2^254 < r: canonical, on both sides of (r - 1) / 2
        e0 = -(n // 2)
        (t2, s2), (t1, s1) = alternate([lambda: sonic.msm_g2_srs(srs, 0, e0, sc), lambda: msm_g1_srs(srs, 0, e0, sc)])
        adds = 0
        for base in range(0, n, 1 << 19):                  # one chain per slab of 2^19 terms, each with the window rule of its own size
            m = min(n - base, 1 << 19)
            c = min(16, max(4, m.bit_length() - 1 - 4))
            adds += m * -(-255 // c)
        c0 = min(16, max(4, min(n, 1 << 19).bit_length() - 1 - 4))
        say("2^%-4d %4d %4d %12.2f (%5.2f) %12.2f (%5.2f) %7.1fx %16.3e" % (lg, c0, -(-255 // c0), t2, s2, t1, s1, t2 / t1, adds / (t2 * 1e-3)))
    say("(G2 madd / s: n W mixed additions of the accumulation over the wall time of the whole call -- upload, scalar check, sort, reduction and")
    say(" host fold included.  The G1 call runs over the string's window tables; the G2 half has none.)")
    srs.close()
    if not QUICK:
        write()


if __name__ == "__main__":
    main()
