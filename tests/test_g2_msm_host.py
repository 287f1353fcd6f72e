"""The host-only parts of the G2 MSM without a GPU (sonic_amd/csrc/msm_g2_host.hpp through tests/host/g2_msm_host.cpp, plain and under
ASan / UBSan with the flags of tests/host/Makefile): the window rule and the shifts, the cut of a bucket into chunks, and the Horner fold
of window sums, against Python integers and oracle/pairing.py.  Every comparison is of integers or bytes."""
import os
import random
import re
import subprocess

import pytest

from oracle import pairing as pr
from sonic_amd import _lib, encoding as enc

HERE = os.path.dirname(os.path.abspath(__file__))
HOST = os.path.join(HERE, "host")
ENV = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
R = enc.R_MODULUS
NEW_SYMBOLS = ["sonic_msm_g2", "sonic_msm_g2_srs", "sonic_msm_g2_srs_dev", "sonic_msm_g2_walk_max"]
BUILDS = ("plain", "san")


@pytest.fixture(scope="module")
def drivers():
    subprocess.check_call(["make", "-C", HOST, "-s", "-f", "g2_msm.mk", "g2_msm_host", "g2_msm_host_san"])
    return {"plain": os.path.join(HOST, "g2_msm_host"), "san": os.path.join(HOST, "g2_msm_host_san")}


def run_driver(path, lines):
    out = subprocess.run([path], input="\n".join(lines) + "\n", capture_output=True, text=True, timeout=600, env=ENV)
    assert out.returncode == 0 and out.stdout.endswith("g2_msm_host ok\n"), out.stdout[-2000:] + out.stderr[-3000:]
    return out.stdout.splitlines()[:-1]


@pytest.fixture(scope="module")
def walk_max(drivers):
    wm, slab = map(int, run_driver(drivers["plain"], ["walkmax"])[0].split())
    assert slab == 1 << 19              # the slab of g2_weighted_sum: the existing check test at d = 2^19 + 3 keeps crossing it
    assert 1 <= wm <= 5000              # a basis of d = 8200 can hold 3 G2_WALK_MAX + 5 equal scalars
    return wm


@pytest.mark.parametrize("build", BUILDS)
def test_window_rule_is_log2_minus_four_clamped(drivers, build):
    ns = [1, 2, 15, 16, 255, 256, 257, 511, 512, 601, 16401, (1 << 19) - 1, 1 << 19, (1 << 19) + 17, 1 << 20, (1 << 20) - 1, 1 << 21, 1 << 30]
    got = [int(x) for x in run_driver(drivers[build], ["rule %d" % n for n in ns])]
    assert got == [min(16, max(4, n.bit_length() - 1 - 4)) for n in ns]
    # the sizes the GPU tests name
    assert dict(zip(ns, got))[601] == 5 and dict(zip(ns, got))[16401] == 10 and dict(zip(ns, got))[1 << 19] == 15


@pytest.mark.parametrize("build", BUILDS)
def test_windows_cover_the_bits_and_the_recoding_carry(drivers, build):
    cases = [(bits, c) for bits in (129, 255, 256) for c in range(4, 17)]
    got = run_driver(drivers[build], ["win %d %d" % bc for bc in cases])
    for (bits, c), line in zip(cases, got):
        W, *shifts = map(int, line.split())
        assert W == -(-bits // c) and shifts == [c * w for w in range(W)]
        # scalars of this width are below 2^(bits - 1): the top window's digit plus a carry stays within 2^(c-1), so no carry leaves it
        top = ((1 << (bits - 1)) - 1) >> shifts[-1]
        assert W * c >= bits and top + 1 <= 1 << (c - 1), (bits, c)
        assert (W - 1) * c < bits                       # and no window is wasted
    assert int(got[cases.index((129, 15))].split()[0]) == 9 and int(got[cases.index((255, 15))].split()[0]) == 17


@pytest.mark.parametrize("build", BUILDS)
def test_chunk_cut_covers_every_entry_once(drivers, build, walk_max):
    wm = walk_max
    lens = [0, 1, wm - 1, wm, wm + 1, 2 * wm, 3 * wm, 3 * wm + 5, 7 * wm - 1, 1 << 19, (1 << 21) + 3]
    firsts = [0, 5, (1 << 31) + 11]
    cases = [(f, n) for f in firsts for n in lens]
    got = run_driver(drivers[build], ["cut %d %d" % fn for fn in cases])
    for (first, n), line in zip(cases, got):
        k, *ranges = line.split()
        ranges = [tuple(map(int, r.split(":"))) for r in ranges]
        assert int(k) == len(ranges) == -(-n // wm), (first, n)
        at = first
        for beg, end in ranges:                          # consecutive, none empty, none longer than G2_WALK_MAX
            assert beg == at and 0 < end - beg <= wm, (first, n, beg, end)
            at = end
        assert at == first + n
        assert all(e - b == wm for b, e in ranges[:-1])


@pytest.fixture(scope="module")
def fold_cases():
    rng = random.Random(1812)
    cases = [(4, 1, [7]), (4, 2, [0, 1]), (5, 3, [1, 0, 0]), (15, 9, [rng.randrange(1 << 40) for _ in range(9)]), (16, 16, [rng.randrange(1 << 64) for _ in range(16)]),
             (4, 64, [rng.randrange(3) for _ in range(64)]), (10, 26, [0] * 26), (13, 10, [0] * 9 + [5]), (7, 5, [3, 0, 0, 0, 0])]
    cases.append((9, 4, [5, (1 << 64) - 1, 2, 1]))
    want = []
    for c, W, ks in cases:
        total = sum(k << (c * w) for w, k in enumerate(ks)) % R
        want.append(enc.g2_to_bytes(pr.g2_mul(pr.G2_GEN, total) if total else None).hex())
    return cases, want


@pytest.mark.parametrize("build", BUILDS)
def test_horner_fold_of_window_sums_is_the_direct_sum(drivers, build, fold_cases):
    cases, want = fold_cases
    got = run_driver(drivers[build], ["fold %d %d %s" % (c, W, " ".join(map(str, ks))) for c, W, ks in cases])
    assert got == want
    assert want[6] == bytes(192).hex()                   # every window at infinity


def test_new_symbols_declared_exported_and_bound():
    hdr = open(os.path.join(os.path.dirname(HERE), "include", "sonic_hip.h")).read()
    L = _lib.lib()
    for name in NEW_SYMBOLS:
        assert re.search(r"\b%s\s*\(" % name, hdr), name
        assert name in _lib.EXPORTED and getattr(L, name).argtypes is not None, name
    assert L.sonic_abi_version() == 7 and _lib.ABI_VERSION == 7
    import sonic_amd
    assert callable(sonic_amd.msm_g2) and callable(sonic_amd.msm_g2_srs)
