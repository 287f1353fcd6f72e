"""The pairing as the device also compiles it, without a GPU: pairing.hpp and the segmented product of pairing_groups.hpp as the host
compiles them (tests/host/pairing_host.cpp, plain and under ASan / UBSan with the flags of tests/host/Makefile), against oracle/pairing.py
and plain integers.  Every comparison is of bytes or integers."""
import os
import re
import subprocess

import pytest

import pairing_ref as pref
from oracle import pairing as pr
from oracle import sonic_ref as ref
from sonic_amd import _lib
from sonic_amd import encoding as enc

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
HOST = os.path.join(HERE, "host")
ENV = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
Q, R = pref.Q, pref.R
BUILDS = ("plain", "san")


@pytest.fixture(scope="module")
def drivers():
    subprocess.check_call(["make", "-C", HOST, "-s", "-f", "pairing.mk", "pairing_host", "pairing_host_san"])
    return {"plain": os.path.join(HOST, "pairing_host"), "san": os.path.join(HOST, "pairing_host_san")}


def run_driver(path, lines):
    out = subprocess.run([path], input="\n".join(lines) + "\n", capture_output=True, text=True, timeout=600, env=ENV)
    assert out.returncode == 0 and out.stdout.endswith("pairing_host ok\n"), out.stdout[-2000:] + out.stderr[-3000:]
    return out.stdout.splitlines()[:-1]


def f2_pow(a, e):
    acc = pr.F2_ONE
    for bit in bin(e)[2:]:
        acc = pr.f2_mul(acc, acc)
        if bit == "1":
            acc = pr.f2_mul(acc, a)
    return acc


@pytest.mark.parametrize("build", BUILDS)
def test_generated_frobenius_constants_are_their_definition(drivers, build):
    """the driver itself compares constants.hpp with the run-time exponentiation (status 3 otherwise); here against Python integers"""
    vals = [int(v, 16) for v in run_driver(drivers[build], ["consts"])[0].split()]
    assert len(vals) == 10
    g = f2_pow((1, 1), (Q - 1) // 6)
    acc = pr.F2_ONE
    for i in range(1, 6):
        acc = pr.f2_mul(acc, g)
        assert (vals[2 * i - 2], vals[2 * i - 1]) == acc, i
    hdr = open(os.path.join(ROOT, "sonic_amd", "csrc", "pairing.hpp")).read()
    assert "FrobeniusConstants" not in hdr and "static const" not in hdr          # no run-time table, no function-local static


def cycled(G, sizes=(0, 1, 2, 17, 16, 3)):
    return " ".join(str(sizes[g % len(sizes)]) for g in range(G))


# the layouts of tests/test_gpu_pairing_shapes.py and their pass counts: four passes (n >= 4097, also as 4096 + 1: the passes come from
# n), every chunk edge, a launch bound beyond the buffers (G > 15 n / 16 over three passes), more groups than k_gt_plan has threads with
# per = 2 and 3 groups a thread and uneven slices, and one long group behind 255 empty ones
SHAPES = [("4097", 4), ("4096 1", 4), ("16 17 32 33 255 256 257 0 15", 3), ("257" + " 0" * 999, 3),
          ("257 " + " ".join("1" if g in (1, 255, 256, 257, 999) or g % 29 == 27 else "0" for g in range(1, 1000)), 3),
          (cycled(255), 3), (cycled(256), 3), (cycled(257), 3), (cycled(513), 3), (" ".join(str(g % 4) for g in range(600)), 3),
          ("0 " * 255 + "4097" + " 1" * 10, 4)]


@pytest.mark.parametrize("build", BUILDS)
def test_segmented_product_equals_the_straight_loop(drivers, build):
    cases = ["0 1 2 3 17 300", "0", "0 0 0", "1", "16", "17", "16 16 0 17", "300", "257 0 1"]
    got = run_driver(drivers[build], ["segments " + c for c in cases + [c for c, _ in SHAPES]])
    got, shaped = got[:len(cases)], got[len(cases):]
    assert len(got) == len(cases) and all(g.startswith("ok passes=") for g in got), got
    passes = [int(re.match(r"ok passes=(\d+)", g).group(1)) for g in got]
    # chunks of 16: 323 -> (<= 21 + 6) -> ... ; one pass while no group exceeds a chunk, three at 300
    assert passes[0] == 3 and passes[1] == 1 and passes[3] == 1 and passes[4] == 1 and passes[5] == 2 and passes[7] == 3
    assert len(shaped) == len(SHAPES)
    for (case, want), line in zip(SHAPES, shaped):
        m = re.match(r"ok passes=(\d+) values=(\d+)$", line)
        assert m and int(m.group(1)) == want and int(m.group(2)) == sum(int(x) for x in case.split()), (case[:60], line)


@pytest.mark.parametrize("build", BUILDS)
def test_gt_byte_layout_round_trips(drivers, build):
    import random
    rng = random.Random(20)
    vals = [b"".join(rng.randrange(Q).to_bytes(48, "little") for _ in range(12)) for _ in range(3)]
    vals += [pref.GT_ONE, bytes(576), b"".join((Q - 1).to_bytes(48, "little") for _ in range(12))]
    got = run_driver(drivers[build], ["gt " + v.hex() for v in vals] + ["gt " + (vals[0][:48 * 5] + Q.to_bytes(48, "little") + vals[0][48 * 6:]).hex()])
    assert got[:-1] == [v.hex() for v in vals] and got[-1] == "bad"
    for v in vals[:3]:
        assert pref.gt_bytes(pref.gt_from_bytes(v)) == v          # the test's own mapping to the oracle's basis is a bijection too


@pytest.fixture(scope="module")
def two_pairs():
    a, b = 0x1234567, 0xabcdef0123
    P1, Q1 = ref.g1_mul(ref.G1_GEN, a), pr.g2_mul(pr.G2_GEN, 5)
    P2, Q2 = ref.g1_mul(ref.G1_GEN, 3), pr.g2_mul(pr.G2_GEN, b)
    return ((P1, Q1), (P2, Q2))


@pytest.mark.parametrize("build", BUILDS)
def test_two_pairs_equal_the_oracles_pairing_cubed(drivers, build, two_pairs):
    line = "pairs " + " ".join(enc.g1_to_bytes(p).hex() + " " + enc.g2_to_bytes(q).hex() for p, q in two_pairs)
    one = "pairs " + enc.g1_to_bytes(two_pairs[0][0]).hex() + " " + enc.g2_to_bytes(two_pairs[0][1]).hex()
    got = run_driver(drivers[build], [line, one])
    assert bytes.fromhex(got[0]) == pref.oracle_value(two_pairs)
    assert bytes.fromhex(got[1]) == pref.oracle_value(two_pairs[:1])
    assert got[0] != got[1] and bytes.fromhex(got[1]) != pref.GT_ONE


@pytest.mark.parametrize("build", BUILDS)
def test_bilinearity_and_infinity(drivers, build):
    P, H = ref.G1_GEN, pr.G2_GEN
    g1, g2 = lambda p: enc.g1_to_bytes(p).hex(), lambda q: enc.g2_to_bytes(q).hex()
    lines = []
    for a in (2, 0xd201000000010001, R - 1):
        lines.append("pairs %s %s %s %s" % (g1(ref.g1_mul(P, a)), g2(H), g1(ref.g1_neg(P)), g2(pr.g2_mul(H, a))))
    lines.append("pairs %s %s %s %s" % (g1(ref.g1_mul(P, 2)), g2(H), g1(ref.g1_neg(P)), g2(pr.g2_mul(H, 3))))       # not one
    lines += ["pairs %s %s" % (bytes(96).hex(), g2(H)), "pairs %s %s" % (g1(P), bytes(192).hex()), "pairs %s %s" % (bytes(96).hex(), bytes(192).hex())]
    got = [bytes.fromhex(x) for x in run_driver(drivers[build], lines)]
    assert got[0] == got[1] == got[2] == pref.GT_ONE
    assert got[3] != pref.GT_ONE
    assert got[4] == got[5] == got[6] == pref.GT_ONE


def test_new_symbol_declared_exported_and_bound():
    hdr = open(os.path.join(ROOT, "include", "sonic_hip.h")).read()
    L = _lib.lib()
    assert re.search(r"\bsonic_pairing_check\s*\(", hdr)
    assert "sonic_pairing_check" in _lib.EXPORTED and L.sonic_pairing_check.argtypes is not None
    for name, val in (("AUTO", 0), ("HOST", 1), ("GPU", 2)):
        assert re.search(r"#define SONIC_PAIRING_%s\s+%d\b" % (name, val), hdr)
    assert (_lib.PAIRING_AUTO, _lib.PAIRING_HOST, _lib.PAIRING_GPU) == (0, 1, 2)
    assert L.sonic_abi_version() == 7 and _lib.ABI_VERSION == 7
    import sonic_amd
    assert callable(sonic_amd.pairing_check) and callable(sonic_amd.pairing)
    hs = open(os.path.join(ROOT, "haskell", "Sonic", "HIP.hs")).read()
    assert '"sonic_pairing_check"' in hs and re.search(r"^pairingCheck\b.*::", hs, flags=re.M)


def test_host_path_of_the_public_call_needs_no_device(two_pairs):
    """where = HOST is pairing.hpp on host threads: the value, the verdicts, the flags and the argument errors, all without a GPU"""
    import numpy as np
    import sonic_amd
    (P1, Q1), (P2, Q2) = two_pairs
    P, H = ref.G1_GEN, pr.G2_GEN
    g1 = [enc.g1_to_bytes(p) for p in (P1, P2, ref.g1_mul(P, 7), ref.g1_neg(P))]
    g2 = [enc.g2_to_bytes(q) for q in (Q1, Q2, H, pr.g2_mul(H, 7))]
    a1 = np.frombuffer(b"".join(g1), np.uint8).reshape(-1, 96)
    a2 = np.frombuffer(b"".join(g2), np.uint8).reshape(-1, 192)
    verdict, gt = sonic_amd.pairing_check(a1, a2, [0, 2, 4, 4], where="host", gt=True)
    assert verdict.tolist() == [0, 1, 0, 0]
    assert gt[0].tobytes() == pref.GT_ONE and gt[1].tobytes() == pref.oracle_value(two_pairs) and gt[2].tobytes() == gt[3].tobytes() == pref.GT_ONE
    assert sonic_amd.pairing(g1[0], g2[0], where="host") == pref.oracle_value(two_pairs[:1])
    # flags: a coordinate of q (non-canonical), y + 1 (off the curve); a bad point leaves the other groups alone
    bad1 = bytearray(g1[0]); bad1[:48] = Q.to_bytes(48, "little")
    bad2 = bytearray(g1[1]); bad2[48:96] = ((int.from_bytes(g1[1][48:96], "little") + 1) % Q).to_bytes(48, "little")
    b1 = np.frombuffer(bytes(bad1) + bytes(bad2) + g1[2] + g1[3], np.uint8).reshape(-1, 96)
    verdict, gt2 = sonic_amd.pairing_check(b1, a2, [1, 2, 4], where="host", gt=True)
    assert verdict.tolist() == [2, 4, 0] and gt2[0].tobytes() == bytes(576) and gt2[2].tobytes() == pref.GT_ONE
    assert sonic_amd.pairing_check(np.zeros((0, 96), np.uint8), np.zeros((0, 192), np.uint8), [0, 0], where="host").tolist() == [0, 0]
    for ge in ([2, 1, 4], [1, 2, 3], [-1, 4]):
        with pytest.raises(sonic_amd.SonicError) as e:
            sonic_amd.pairing_check(a1, a2, ge, where="host")
        assert e.value.code == 7 and "sonic_pairing_check" in e.value.message
    L = _lib.lib()
    v = np.zeros(1, np.uint8)
    ge = np.array([4], np.int64)
    assert L.sonic_pairing_check(a1.ctypes.data, a2.ctypes.data, 4, ge.ctypes.data, 1, 3, v.ctypes.data, None) == 7
    assert L.sonic_pairing_check(None, a2.ctypes.data, 4, ge.ctypes.data, 1, 1, v.ctypes.data, None) == 7
    assert L.sonic_pairing_check(a1.ctypes.data, a2.ctypes.data, 4, ge.ctypes.data, 1, 1, None, None) == 7
