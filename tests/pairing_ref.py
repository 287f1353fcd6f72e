"""What the pairing tests share: values of oracle/pairing.py in the 576-byte layout of sonic_srs_pairing / sonic_pairing_check, and points.

The oracle keeps Fq12 as twelve coefficients over Fq[w]/(w^12 - 2 w^6 + 2); the library's tower is Fq2[w]/(w^6 - (1 + u)) with u = w^6 - 1,
so the coefficient of w^i is (c_i + c_{i+6}) + c_{i+6} u, and w^i sits at [i % 2][i // 2] of Fq12 = Fq6[w]/(w^2 - v).  The library's exponent
is 3 (q^12 - 1) / r: its value is the oracle's `pairing` cubed."""
import functools

from oracle import pairing as pr
from oracle.sonic_ref import G1_GEN, Q, R

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


__all__ = ["GT_ONE", "gt_bytes", "gt_from_bytes", "cube", "oracle_value", "G1_GEN", "Q", "R"]
