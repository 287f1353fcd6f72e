"""Bulk conversion between the 96- / 192-byte encodings of the C ABI and the compressed 48- / 96-byte ones, on the GPU (sonic_g1_compress
and its kin, include/sonic_hip.h "Compressed encodings"), and one proof's re-encoding on the host.  Single points as Python integers:
encoding.py."""
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
