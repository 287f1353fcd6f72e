"""Products of pairings checked in groups, on the host or on the GPU (sonic_pairing_check, include/sonic_hip.h "Pairing")."""
from __future__ import annotations

import numpy as np

from . import _lib

_WHERE = {"auto": _lib.PAIRING_AUTO, "host": _lib.PAIRING_HOST, "gpu": _lib.PAIRING_GPU}


def pairing_check(g1, g2, group_end=None, where: str = "auto", gt: bool = False):
    """g1: uint8 [n, 96], g2: uint8 [n, 192] (the encodings of msm_g1 / msm_g2; zeros are the point at infinity), group_end: the end of
    each group of pairs (non-decreasing, the last one n), None for one group.  Returns uint8 [groups]: 0 the product of the group's pairings
    is one, 1 it is not, else the OR over the group's points of 2 non-canonical, 4 off the curve / twist, 8 outside the subgroup.  With
    gt=True returns (verdicts, uint8 [groups, 576]): each group's value in the layout of SRS.pairing -- the cube of the textbook ate
    pairing, since the exponent is 3 (q^12 - 1) / r -- zeros for a group with a bad point.  where: 'host', 'gpu', or 'auto' (the
    library's measured rule; SONIC_PAIRING_GPU=0 / 1 in the environment overrides it)."""
    if where not in _WHERE:
        raise ValueError(f"where {where!r}: 'auto', 'host' or 'gpu'")
    a = np.ascontiguousarray(g1, np.uint8).reshape(-1, 96)
    b = np.ascontiguousarray(g2, np.uint8).reshape(-1, 192)
    if a.shape[0] != b.shape[0]:
        raise ValueError(f"{a.shape[0]} G1 points for {b.shape[0]} G2 points")
    ge = np.ascontiguousarray([a.shape[0]] if group_end is None else group_end, np.int64).reshape(-1)
    verdict = np.zeros(ge.shape[0], np.uint8)
    out = np.zeros((ge.shape[0], 576), np.uint8) if gt else None
    _lib.check(_lib.lib().sonic_pairing_check(a.ctypes.data, b.ctypes.data, a.shape[0], ge.ctypes.data, ge.shape[0], _WHERE[where], verdict.ctypes.data,
                                              out.ctypes.data if gt else None))
    return (verdict, out) if gt else verdict


def pairing(P, Q, where: str = "auto") -> bytes:
    """the 576 bytes of one pair's value (96 bytes of G1, 192 of G2): SRS.pairing's layout, the cube of the textbook ate pairing.  A point
    that is not a canonical encoding of an element of the subgroup raises ValueError with the verdict's bits"""
    verdict, out = pairing_check(np.frombuffer(bytes(P), np.uint8), np.frombuffer(bytes(Q), np.uint8), None, where, True)
    if verdict[0] > 1:
        raise ValueError(f"pairing: bad point (verdict {int(verdict[0])}: 2 non-canonical, 4 off the curve / twist, 8 outside the subgroup)")
    return out[0].tobytes()
