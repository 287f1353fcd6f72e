"""Subgroup membership without a GPU: the endomorphism tests of g1.hpp / g2.hpp and the definition they replace, as the host compiles
them (tests/host/subgroup_host.cpp, plain and under ASan / UBSan with the flags of tests/host/Makefile), against the Python-integer mirror
(tests/subgroup_ref.py) over the adversarial sets -- points of small prime order, the generator plus such a point, [r](random point),
random points without cofactor clearing -- where an endomorphism test could be unsound.  Every comparison is of integers or bits."""
import math
import os
import re
import subprocess

import pytest

import subgroup_ref as sg
from oracle import pairing as pr
from sonic_amd import _lib

HERE = os.path.dirname(os.path.abspath(__file__))
HOST = os.path.join(HERE, "host")
ENV = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
Q, R, Z = sg.Q, sg.R, sg.Z
NEW_SYMBOLS = ["sonic_g1_subgroup_check", "sonic_g2_subgroup_check"]
BUILDS = ("plain", "san")


@pytest.fixture(scope="module")
def drivers():
    subprocess.check_call(["make", "-C", HOST, "-s", "-f", "subgroup.mk", "subgroup_host", "subgroup_host_san"])
    return {"plain": os.path.join(HOST, "subgroup_host"), "san": os.path.join(HOST, "subgroup_host_san")}


def run_driver(path, lines):
    out = subprocess.run([path], input="\n".join(lines) + "\n", capture_output=True, text=True, timeout=600, env=ENV)
    assert out.returncode == 0 and out.stdout.endswith("subgroup_host ok\n"), out.stdout[-2000:] + out.stderr[-3000:]
    return out.stdout.splitlines()[:-1]


def test_the_integer_identities_behind_both_criteria():
    lam = sg.LAMBDA
    assert lam * lam + lam + 1 == R                       # phi^2 + phi + 1 = 0 and phi = lambda  =>  r P = O
    assert 3 * sg.H1 == (Z - 1) ** 2 and Q - Z == sg.H1 * R     # psi^2 - t psi + q = 0, t = z + 1, and psi = z  =>  (q - z) P = O
    assert math.gcd(sg.H1, sg.H2) == 1                    # ... and the order of P divides h2 r, so it divides r
    assert (Z * Z).bit_length() == 128 and bin(Z * Z).count("1") == 17
    assert (-Z).bit_length() == 64 and bin(-Z).count("1") == 6
    assert sg.H1 * R == Q + 1 - (Z + 1)                   # #E(Fq) = q + 1 - t
    assert 9 * sg.H2 == Z ** 8 - 4 * Z ** 7 + 5 * Z ** 6 - 4 * Z ** 4 + 6 * Z ** 3 - 4 * Z ** 2 - 4 * Z + 13
    for ell in sg.G1_ORDERS:
        assert sg.H1 % ell == 0 and R % ell
    for ell in sg.G2_ORDERS:
        assert sg.H2 % ell == 0 and R % ell


def test_the_endomorphisms_satisfy_their_equations_on_random_points():
    import random
    rng = random.Random(7)
    for _ in range(3):
        p = sg.g1_random_point(rng)
        p1 = sg.g1_phi(p)
        assert sg.g1_on_curve(p1) and sg.g1_add(sg.g1_add(sg.g1_phi(p1), p1), p) is None        # phi^2 + phi + 1 = 0 on all of E(Fq)
    t = Z + 1
    for _ in range(2):
        p = sg.g2_random_point(rng)
        p1 = sg.g2_psi(p)
        assert pr.g2_on_curve(p1)
        # psi^2 (P) + q P = t psi(P), t < 0
        lhs = pr.g2_add(sg.g2_psi(p1), sg.g2_mul(p, Q))
        assert lhs == sg.g2_neg(sg.g2_mul(p1, -t))
        assert sg.g2_mul(p, sg.H2 * R) is None             # #E'(Fq2) = h2 r


@pytest.mark.parametrize("build", BUILDS)
def test_constants_are_their_definitions(drivers, build):
    b, cx0, cx1, cy0, cy1 = (int(v, 16) for v in run_driver(drivers[build], ["consts"])[0].split())
    assert pow(b, 3, Q) == 1 and b != 1 and b == sg.beta()
    cx, cy = (cx0, cx1), (cy0, cy1)
    assert pr.f2_mul(cx, sg.f2_pow((1, 1), (Q - 1) // 3)) == pr.F2_ONE
    assert pr.f2_mul(cy, sg.f2_pow((1, 1), (Q - 1) // 2)) == pr.F2_ONE
    assert (cx, cy) == sg.psi_consts()


@pytest.fixture(scope="module")
def mirror():
    """(definition, endomorphism test) of the mirror for every on-curve case of both sets"""
    g1 = [(n, b) for n, b, _ in sg.g1_cases() if b != bytes(96) and sg.g1_flag(b) in (0, sg.FLAG_OUTSIDE)]
    g2 = [(n, b) for n, b, _ in sg.g2_cases() if b != bytes(192) and sg.g2_flag(b) in (0, sg.FLAG_OUTSIDE)]
    from sonic_amd import encoding as enc
    v1 = [(sg.g1_walk(enc.g1_from_bytes(b)), sg.g1_endo(enc.g1_from_bytes(b))) for _, b in g1]
    v2 = [(sg.g2_walk(enc.g2_from_bytes(b)), sg.g2_endo(enc.g2_from_bytes(b))) for _, b in g2]
    return g1, v1, g2, v2


def test_the_mirror_agrees_with_the_definition_and_the_construction(mirror):
    g1, v1, g2, v2 = mirror
    for cases, names, verdicts in ((sg.g1_cases(), g1, v1), (sg.g2_cases(), g2, v2)):
        known = {n: f for n, _, f in cases}
        for (name, _), (walk, endo) in zip(names, verdicts):
            assert walk == endo, name
            if known[name] is not None:
                assert endo == (known[name] == 0), name
    # the classes an endomorphism test could get wrong are all there, and all refused
    for names, verdicts, orders, g in ((g1, v1, sg.G1_ORDERS, "G"), (g2, v2, sg.G2_ORDERS, "H")):
        d = {n: e for (n, _), (_, e) in zip(names, verdicts)}
        for ell in orders:
            assert d["T_%d" % ell] is False and d["%s+T_%d" % (g, ell)] is False
        assert not any(d["random%d" % i] for i in range(3)) and d["r*random"] is False
    assert {n: e for (n, _), (_, e) in zip(g2, v2)}["H+r*random"] is False
    # the flags the public calls give to the cases that never reach a walk
    for cases, flag in ((sg.g1_cases(), sg.g1_flag), (sg.g2_cases(), sg.g2_flag)):
        for name, b, f in cases:
            if f is not None:
                assert flag(b) == f, name


@pytest.mark.parametrize("build", BUILDS)
def test_host_functions_agree_with_the_mirror_on_the_adversarial_sets(drivers, build, mirror):
    g1, v1, g2, v2 = mirror
    got = run_driver(drivers[build], ["g1 " + b.hex() for _, b in g1] + ["g2 " + b.hex() for _, b in g2])
    assert len(got) == len(g1) + len(g2)
    for (name, _), (walk, endo), line in zip(g1 + g2, v1 + v2, got):
        e, w = (int(x) for x in line.split())
        assert (e, w) == (int(endo), int(walk)), name


def test_new_symbols_declared_exported_and_bound():
    hdr = open(os.path.join(os.path.dirname(HERE), "include", "sonic_hip.h")).read()
    L = _lib.lib()
    for name in NEW_SYMBOLS:
        assert re.search(r"\b%s\s*\(" % name, hdr), name
        assert name in _lib.EXPORTED and getattr(L, name).argtypes is not None, name
    assert re.search(r"#define SONIC_SUBGROUP_DEFAULT 0\b", hdr) and re.search(r"#define SONIC_SUBGROUP_WALK\s+1\b", hdr)
    assert L.sonic_abi_version() == 7 and _lib.ABI_VERSION == 7
    import sonic_amd
    assert callable(sonic_amd.g1_subgroup_check) and callable(sonic_amd.g2_subgroup_check)
    hs = open(os.path.join(os.path.dirname(HERE), "haskell", "Sonic", "HIP.hs")).read()
    for name in NEW_SYMBOLS:
        assert '"%s"' % name in hs, name
    assert re.search(r"^g1SubgroupCheck\b.*::", hs, flags=re.M) and re.search(r"^g2SubgroupCheck\b.*::", hs, flags=re.M)
