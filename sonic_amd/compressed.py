"""Bulk conversion between the 96- / 192-byte encodings of the C ABI and the compressed 48- / 96-byte ones, on the GPU (sonic_g1_compress
and its kin, include/sonic_hip.h "Compressed encodings"), one proof's re-encoding on the host, and the subgroup test of the loaders on its
own (g1_subgroup_check, g2_subgroup_check).  Single points as Python integers: encoding.py."""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib


def _convert(name: str, points, in_bytes: int, out_bytes: int) -> np.ndarray:
    a = np.ascontiguousarray(points, np.uint8).reshape(-1, in_bytes)
    out = np.zeros((a.shape[0], out_bytes), np.uint8)
    _lib.check(getattr(_lib.lib(), name)(a.ctypes.data, a.shape[0], out.ctypes.data))
    return out


def _expand(name: str, points, in_bytes: int, out_bytes: int, check_subgroup: bool, flags: bool):
    a = np.ascontiguousarray(points, np.uint8).reshape(-1, in_bytes)
    out = np.zeros((a.shape[0], out_bytes), np.uint8)
    fl = np.zeros(a.shape[0], np.uint8) if flags else None
    _lib.check(getattr(_lib.lib(), name)(a.ctypes.data, a.shape[0], 1 if check_subgroup else 0, out.ctypes.data, fl.ctypes.data if flags else None))
    return (out, fl) if flags else out


def g1_compress(points) -> np.ndarray:
    """uint8 [n, 96] -> uint8 [n, 48]; the input is validated (canonical, on the curve, in the subgroup): SonicError BAD_ENCODING otherwise"""
    return _convert("sonic_g1_compress", points, 96, 48)


def g1_decompress(points, check_subgroup: bool = True, flags: bool = False):
    """uint8 [n, 48] -> uint8 [n, 96].  flags=True: also one verdict per point (0 accepted; bits 1 malformed, 2 off the curve, 4 outside the
    subgroup), a refused point decodes to zeros; flags=False: any refused point raises SonicError BAD_ENCODING"""
    return _expand("sonic_g1_decompress", points, 48, 96, check_subgroup, flags)


def g2_compress(points) -> np.ndarray:
    """uint8 [n, 192] -> uint8 [n, 96]"""
    return _convert("sonic_g2_compress", points, 192, 96)


def g2_decompress(points, check_subgroup: bool = True, flags: bool = False):
    """uint8 [n, 96] -> uint8 [n, 192]; flags as for g1_decompress"""
    return _expand("sonic_g2_decompress", points, 96, 192, check_subgroup, flags)


_SUBGROUP_METHODS = {"endo": _lib.SUBGROUP_DEFAULT, "walk": _lib.SUBGROUP_WALK}


def _subgroup_check(name: str, points, in_bytes: int, method: str) -> np.ndarray:
    if method not in _SUBGROUP_METHODS:
        raise ValueError(f"method {method!r}: 'endo' (the endomorphism test) or 'walk' (r P = O by double-and-add)")
    a = np.ascontiguousarray(points, np.uint8).reshape(-1, in_bytes)
    fl = np.zeros(a.shape[0], np.uint8)
    _lib.check(getattr(_lib.lib(), name)(a.ctypes.data, a.shape[0], _SUBGROUP_METHODS[method], fl.ctypes.data))
    return fl


def g1_subgroup_check(points, method: str = "endo") -> np.ndarray:
    """uint8 [n, 96] -> uint8 [n]: 0 for a point of the order-r subgroup (infinity included), else bits 1 non-canonical, 2 off the curve,
    4 outside the subgroup (sonic_g1_subgroup_check, include/sonic_hip.h "Subgroup membership").  'endo' is the test every loader runs,
    'walk' the definition; both give the same flags"""
    return _subgroup_check("sonic_g1_subgroup_check", points, 96, method)


def g2_subgroup_check(points, method: str = "endo") -> np.ndarray:
    """uint8 [n, 192] -> uint8 [n]; flags and methods as for g1_subgroup_check"""
    return _subgroup_check("sonic_g2_subgroup_check", points, 192, method)


def proof_compress(proof: bytes, Q: int) -> bytes:
    """sonic_proof_size(Q) proof bytes -> the compressed proof (host only)"""
    L = _lib.lib()
    proof = bytes(proof)
    if len(proof) != L.sonic_proof_size(Q):
        raise ValueError(f"proof for Q = {Q} is {L.sonic_proof_size(Q)} bytes, got {len(proof)}")
    out = C.create_string_buffer(L.sonic_proof_size_compressed(Q))
    _lib.check(L.sonic_proof_compress(Q, proof, out))
    return out.raw


def proof_decompress(proof_z: bytes, Q: int) -> bytes:
    L = _lib.lib()
    proof_z = bytes(proof_z)
    if len(proof_z) != L.sonic_proof_size_compressed(Q):
        raise ValueError(f"compressed proof for Q = {Q} is {L.sonic_proof_size_compressed(Q)} bytes, got {len(proof_z)}")
    out = C.create_string_buffer(L.sonic_proof_size(Q))
    _lib.check(L.sonic_proof_decompress(Q, proof_z, out))
    return out.raw
