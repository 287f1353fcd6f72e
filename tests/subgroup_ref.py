"""Subgroup membership restated with Python integers (test infrastructure; the normative text: sonic_amd/csrc/g1.hpp, g2.hpp and
include/sonic_hip.h, "Subgroup membership"): the two endomorphism tests, the definition r P = O, the flags of the public calls, and the
adversarial point sets of tests/test_subgroup_host.py and tests/test_gpu_subgroup.py, built from a fixed seed.

Points are (x, y) or None on G1 and ((x0, x1), (y0, y1)) or None on G2, as everywhere under oracle/.  oracle's g1_mul / g2_mul reduce the
scalar mod r, which is wrong outside the subgroup; mul() here does not."""
import functools
import random

from oracle import pairing as pr
from oracle.sonic_ref import G1_GEN, g1_add, g1_neg
from sonic_amd import encoding as enc

Q, R = pr.Q, pr.R
Z = -0xD201000000010000                                   # the BLS parameter
LAMBDA = Z * Z - 1                                        # phi's eigenvalue on G1
H1 = (Z - 1) ** 2 // 3                                    # #E(Fq) = H1 r
H2 = (Z ** 8 - 4 * Z ** 7 + 5 * Z ** 6 - 4 * Z ** 4 + 6 * Z ** 3 - 4 * Z ** 2 - 4 * Z + 13) // 9       # #E'(Fq2) = H2 r
G1_ORDERS = (3, 11, 10177, 859267, 52437899)              # prime divisors of H1
G2_ORDERS = (13, 23, 2713, 11953, 262069)                 # prime divisors of H2
SEED = 1905
FLAG_NONCANONICAL, FLAG_OFF_CURVE, FLAG_OUTSIDE = 1, 2, 4


def mul(add, p, k: int):
    """k P by double-and-add over the integer k >= 0 (no reduction mod r)"""
    acc = None
    for bit in bin(k)[2:] if k else "":
        acc = add(acc, acc)
        if bit == "1":
            acc = add(acc, p)
    return acc


def g1_mul(p, k): return mul(g1_add, p, k)
def g2_mul(p, k): return mul(pr.g2_add, p, k)
def g2_neg(p): return None if p is None else (p[0], pr.f2_neg(p[1]))


def f2_pow(a, e: int):
    acc = pr.F2_ONE
    for bit in bin(e)[2:]:
        acc = pr.f2_sqr(acc)
        if bit == "1":
            acc = pr.f2_mul(acc, a)
    return acc


@functools.lru_cache(None)
def beta() -> int:
    """the cube root of unity with (beta x, y) = lambda (x, y) on the generator"""
    lg = g1_mul(G1_GEN, LAMBDA)
    assert lg[1] == G1_GEN[1]
    return lg[0] * pow(G1_GEN[0], -1, Q) % Q


@functools.lru_cache(None)
def psi_consts():
    """c_x = (1 + u)^(-(q-1)/3), c_y = (1 + u)^(-(q-1)/2)"""
    return pr.f2_inv(f2_pow((1, 1), (Q - 1) // 3)), pr.f2_inv(f2_pow((1, 1), (Q - 1) // 2))


def g1_phi(p): return (beta() * p[0] % Q, p[1])


def g2_psi(p):
    cx, cy = psi_consts()
    (x0, x1), (y0, y1) = p
    return (pr.f2_mul((x0, -x1 % Q), cx), pr.f2_mul((y0, -y1 % Q), cy))


# ---- the tests, for a finite point of the curve / twist -----------------------------------------------------------------------------------
def g1_endo(p) -> bool:
    """phi(P) == lambda P, with lambda P = z^2 P - P as g1.hpp walks it"""
    lp = g1_add(g1_mul(p, Z * Z), g1_neg(p))
    return lp is not None and lp == g1_phi(p)


def g1_walk(p) -> bool: return g1_mul(p, R) is None


def g2_endo(p) -> bool:
    """psi(P) == z P = -(|z| P)"""
    zp = g2_mul(p, -Z)
    return zp is not None and g2_psi(p) == g2_neg(zp)


def g2_walk(p) -> bool: return g2_mul(p, R) is None


def g1_on_curve(p) -> bool: return (p[1] * p[1] - p[0] ** 3 - 4) % Q == 0


# ---- flags of sonic_g1_subgroup_check / sonic_g2_subgroup_check over encodings --------------------------------------------------------------
@functools.lru_cache(None)
def g1_flag(b: bytes) -> int:
    if b == bytes(96):
        return 0
    x, y = int.from_bytes(b[:48], "little"), int.from_bytes(b[48:], "little")
    if x >= Q or y >= Q:
        return FLAG_NONCANONICAL
    if not g1_on_curve((x, y)):
        return FLAG_OFF_CURVE
    return 0 if g1_endo((x, y)) else FLAG_OUTSIDE


@functools.lru_cache(None)
def g2_flag(b: bytes) -> int:
    if b == bytes(192):
        return 0
    v = [int.from_bytes(b[48 * i:48 * i + 48], "little") for i in range(4)]
    if any(c >= Q for c in v):
        return FLAG_NONCANONICAL
    p = ((v[0], v[1]), (v[2], v[3]))
    if not pr.g2_on_curve(p):
        return FLAG_OFF_CURVE
    return 0 if g2_endo(p) else FLAG_OUTSIDE


# ---- the adversarial sets --------------------------------------------------------------------------------------------------------------------
def g1_random_point(rng):
    """a random point of E(Fq), no cofactor clearing"""
    while True:
        x = rng.randrange(Q)
        y = enc.fq_sqrt((x ** 3 + 4) % Q)
        if y is not None:
            return (x, y if rng.random() < 0.5 else Q - y)


def g2_random_point(rng):
    while True:
        x = (rng.randrange(Q), rng.randrange(Q))
        y = enc.fq2_sqrt(pr.f2_add(pr.f2_mul(pr.f2_sqr(x), x), pr.B2))
        if y is not None:
            return (x, y if rng.random() < 0.5 else pr.f2_neg(y))


def point_of_order(mulf, random_point, rng, order: int, ell: int):
    """a point of exact order ell: every power of ell stripped from the group order, a random point multiplied by the rest, then by ell while
    the result stays finite (the ell-parts are not cyclic, so [order / ell] P is always O)"""
    rest = order
    while rest % ell == 0:
        rest //= ell
    while True:
        t = mulf(random_point(rng), rest)
        if t is None:
            continue
        while True:
            nxt = mulf(t, ell)
            if nxt is None:
                return t
            t = nxt


@functools.lru_cache(None)
def g1_cases():
    """[(name, 96 bytes, the flag known by construction)]"""
    rng = random.Random(SEED)
    out = []
    def add(name, p, flag): out.append((name, enc.g1_to_bytes(p), flag))
    ks = [1, 2, 3, R - 1, rng.randrange(1, R), rng.randrange(1, R)]
    for k in ks:
        p = g1_mul(G1_GEN, k)
        add("gen*%d" % k, p, 0)
        add("-gen*%d" % k, g1_neg(p), 0)
    add("infinity", None, 0)
    add("(0,2)", (0, 2), FLAG_OUTSIDE)
    add("(0,-2)", (0, Q - 2), FLAG_OUTSIDE)
    for ell in G1_ORDERS:
        t = point_of_order(g1_mul, g1_random_point, rng, H1 * R, ell)
        assert g1_mul(t, ell) is None and t is not None
        add("T_%d" % ell, t, FLAG_OUTSIDE)
        add("G+T_%d" % ell, g1_add(G1_GEN, t), FLAG_OUTSIDE)
    add("r*random", g1_mul(g1_random_point(rng), R), None)            # in the cofactor part: out unless it came out as O
    for i in range(4):
        add("random%d" % i, g1_random_point(rng), None)
    add("off-curve", (G1_GEN[0], (G1_GEN[1] + 1) % Q), FLAG_OFF_CURVE)
    lifted = bytearray(enc.g1_to_bytes(G1_GEN))
    lifted[:48] = (G1_GEN[0] + Q).to_bytes(48, "little")
    out.append(("x+q", bytes(lifted), FLAG_NONCANONICAL))
    lifted = bytearray(enc.g1_to_bytes(G1_GEN))
    lifted[48:] = (G1_GEN[1] + Q).to_bytes(48, "little")
    out.append(("y+q", bytes(lifted), FLAG_NONCANONICAL))
    return out


@functools.lru_cache(None)
def g2_cases():
    """[(name, 192 bytes, the flag known by construction)]"""
    rng = random.Random(SEED + 1)
    out = []
    def add(name, p, flag): out.append((name, enc.g2_to_bytes(p), flag))
    for k in [1, 2, R - 1, rng.randrange(1, R)]:
        p = g2_mul(pr.G2_GEN, k)
        add("gen*%d" % k, p, 0)
        add("-gen*%d" % k, g2_neg(p), 0)
    add("infinity", None, 0)
    y = enc.fq2_sqrt(pr.B2)                                            # x = 0: the points of order 3, where the twist has them
    if y is not None:
        add("(0,y)", ((0, 0), y), FLAG_OUTSIDE)
        add("(0,-y)", ((0, 0), pr.f2_neg(y)), FLAG_OUTSIDE)
    for ell in G2_ORDERS:
        t = point_of_order(g2_mul, g2_random_point, rng, H2 * R, ell)
        assert g2_mul(t, ell) is None and t is not None
        add("T_%d" % ell, t, FLAG_OUTSIDE)
        add("H+T_%d" % ell, pr.g2_add(pr.G2_GEN, t), FLAG_OUTSIDE)
    rp = g2_mul(g2_random_point(rng), R)
    add("r*random", rp, None)
    add("H+r*random", pr.g2_add(pr.G2_GEN, rp), None)
    for i in range(3):
        add("random%d" % i, g2_random_point(rng), None)
    add("off-twist", (pr.G2_GEN[0], pr.f2_add(pr.G2_GEN[1], (1, 0))), FLAG_OFF_CURVE)
    for c in range(4):
        lifted = bytearray(enc.g2_to_bytes(pr.G2_GEN))
        v = int.from_bytes(lifted[48 * c:48 * c + 48], "little")
        lifted[48 * c:48 * c + 48] = (v + Q).to_bytes(48, "little")
        out.append(("coordinate %d + q" % c, bytes(lifted), FLAG_NONCANONICAL))
    return out


def case(cases, name: str) -> bytes:
    return next(b for n, b, _ in cases if n == name)
