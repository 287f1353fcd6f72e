"""What the pairing tests share: values of oracle/pairing.py in the 576-byte layout of sonic_srs_pairing / sonic_pairing_check, and points.

The oracle keeps Fq12 as twelve coefficients over Fq[w]/(w^12 - 2 w^6 + 2); the library's tower is Fq2[w]/(w^6 - (1 + u)) with u = w^6 - 1,
so the coefficient of w^i is (c_i + c_{i+6}) + c_{i+6} u, and w^i sits at [i % 2][i // 2] of Fq12 = Fq6[w]/(w^2 - v).  The library's exponent
is 3 (q^12 - 1) / r: its value is the oracle's `pairing` cubed."""
import functools

import numpy as np

from oracle import pairing as pr
from oracle.sonic_ref import G1_GEN, Q, R, g1_mul
from sonic_amd.encoding import g1_to_bytes, g2_to_bytes

GT_ONE = (1).to_bytes(48, "little") + bytes(528)


def gt_bytes(e) -> bytes:
    out = b""
    for i in range(2):
        for j in range(3):
            k = 2 * j + i
            out += ((e[k] + e[k + 6]) % Q).to_bytes(48, "little") + (e[k + 6] % Q).to_bytes(48, "little")
    return out


def gt_from_bytes(b: bytes):
    e = [0] * 12
    for i in range(2):
        for j in range(3):
            k, at = 2 * j + i, 96 * (3 * i + j)
            c0, c1 = int.from_bytes(b[at:at + 48], "little"), int.from_bytes(b[at + 48:at + 96], "little")
            e[k], e[k + 6] = (c0 - c1) % Q, c1
    return e


def cube(e):
    return pr.f12_mul(pr.f12_mul(e, e), e)


@functools.lru_cache(maxsize=None)
def oracle_value(pairs) -> bytes:
    """pairs: a tuple of (G1 point, G2 point) as integer tuples (None: infinity).  prod pairing(P, Q), cubed, as 576 bytes"""
    f = pr.F12_ONE
    for p, q in pairs:
        f = pr.f12_mul(f, pr.miller_loop(p, q))
    return gt_bytes(cube(pr.f12_pow(f, pr.FINAL_EXP)))


# ---- pairs with a known value ---------------------------------------------------------------------------------------------------------
# Pair i is (a_i G1_GEN, b_i G2_GEN) for integers a_i, b_i, so by bilinearity a group's value is E^(sum a_i b_i mod r) with E the value of
# (G1_GEN, G2_GEN): one pairing of the oracle and one f12_pow per distinct exponent, whatever the group's size.  The pools hold the
# scalars at which a Miller loop or a scalar walk changes behaviour (z is the curve's parameter, |z| the loop count).
Z_ABS = 0xd201000000010000
G1_POOL = (1, 2, R - 1, Z_ABS, Z_ABS + 1, R - Z_ABS, pow(2, 254, R), 3, 5, 7, 11, 13, 0x1234567)
G2_POOL = (1, R - 1, Z_ABS, (R - 1) // 2, 5, 0xabcdef0123)          # 13 and 6 entries: index j walks all 78 combinations


@functools.lru_cache(maxsize=None)
def g1_row(a: int) -> bytes:
    """the 96 bytes of a G1_GEN, a in [0, r) (zeros, the point at infinity, for 0)"""
    return g1_to_bytes(g1_mul(G1_GEN, a)) if a else bytes(96)


@functools.lru_cache(maxsize=None)
def g2_row(b: int) -> bytes:
    """the 192 bytes of b G2_GEN, b in [0, r)"""
    return g2_to_bytes(pr.g2_mul(pr.G2_GEN, b)) if b else bytes(192)


def pool_pairs(m: int, shift: int = 0):
    """m scalar pairs (a, b) cycling through the pools from index `shift`"""
    return [(G1_POOL[(shift + j) % len(G1_POOL)], G2_POOL[(shift + j) % len(G2_POOL)]) for j in range(m)]


def exponent(pairs) -> int:
    return sum(a * b for a, b in pairs) % R


def closed(pairs, off: int = 0):
    """the pairs and one more, (-(sum a_i b_i) G1_GEN, G2_GEN), that closes the group to one; with `off` that pair's scalar is off by it
    and the group's exponent is `off`"""
    return list(pairs) + [((off - exponent(pairs)) % R, 1)]


def build(groups):
    """groups: a list of lists of scalar pairs -> (g1 uint8 [n, 96], g2 uint8 [n, 192], group_end int64 [G], the groups' exponents)"""
    flat = [(a % R, b % R) for grp in groups for a, b in grp]
    g1 = np.frombuffer(b"".join(g1_row(a) for a, _ in flat), np.uint8).reshape(-1, 96).copy()
    g2 = np.frombuffer(b"".join(g2_row(b) for _, b in flat), np.uint8).reshape(-1, 192).copy()
    ends = np.cumsum(np.array([len(grp) for grp in groups], np.int64)).astype(np.int64)
    return g1, g2, ends, [exponent(grp) for grp in groups]


@functools.lru_cache(maxsize=None)
def expected(e: int) -> bytes:
    """the 576 bytes of a group whose exponent is e: E^e from the oracle's one pairing, GT_ONE for 0"""
    e %= R
    if e == 0:
        return GT_ONE
    return gt_bytes(pr.f12_pow(gt_from_bytes(oracle_value(((G1_GEN, pr.G2_GEN),))), e))


__all__ = ["GT_ONE", "gt_bytes", "gt_from_bytes", "cube", "oracle_value", "G1_GEN", "Q", "R", "Z_ABS", "G1_POOL", "G2_POOL", "g1_row", "g2_row",
           "pool_pairs", "exponent", "closed", "build", "expected"]
