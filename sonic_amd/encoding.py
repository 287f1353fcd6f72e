"""Canonical encodings at the C ABI (include/sonic_hip.h): Fr = 32 B LE, G1 = 96 B x||y LE,
infinity = 96 zero bytes.  Python-side values: Fr = int, G1 = (x, y) ints or None (`mempty`).

The compressed encodings (the Zcash / IETF serialization; normative text in include/sonic_hip.h) have a pure-Python integer implementation
here -- g1_compress / g1_decompress / g2_compress / g2_decompress over single points, the host mirror the kernels are tested against; the
bulk functions over uint8 arrays, on the GPU, are sonic_amd.g1_compress etc. (compressed.py)."""
from __future__ import annotations

import numpy as np

R_MODULUS = 0x73EDA753299D7D483339D80809A1D80553BDA402FFFE5BFEFFFFFFFF00000001
Q_MODULUS = 0x1A0111EA397FE69A4B1BA7B6434BACD764774B84F38512BF6730D2A0F6B0F6241EABFFFEB153FFFFB9FEFFFFFFFFAAAB


def fr_to_bytes(x: int) -> bytes:
    return (int(x) % R_MODULUS).to_bytes(32, "little")


def fr_from_bytes(b: bytes) -> int:
    return int.from_bytes(b, "little")


def g1_to_bytes(p) -> bytes:
    if p is None:
        return bytes(96)
    return int(p[0]).to_bytes(48, "little") + int(p[1]).to_bytes(48, "little")


def g1_from_bytes(b: bytes):
    b = bytes(b)
    if b == bytes(96):
        return None
    return (int.from_bytes(b[:48], "little"), int.from_bytes(b[48:], "little"))


def fr_array(vals) -> np.ndarray:
    """ints, or an already-encoded uint8 array [k, 32] -> contiguous uint8 [k, 32]."""
    if isinstance(vals, np.ndarray):
        a = np.ascontiguousarray(vals, dtype=np.uint8)
        return a.reshape(-1, 32)
    vals = list(vals)
    if not vals:
        return np.zeros((0, 32), np.uint8)
    return np.frombuffer(b"".join(fr_to_bytes(v) for v in vals), dtype=np.uint8).reshape(-1, 32).copy()


def fr_matrix(rows) -> np.ndarray:
    """list of Q rows of n ints (Bulletproofs GateWeights, `[[f]]`) or uint8 [Q, n, 32] -> uint8 [Q*n, 32]."""
    if isinstance(rows, np.ndarray):
        return np.ascontiguousarray(rows, dtype=np.uint8).reshape(-1, 32)
    return fr_array([v for row in rows for v in row])


# ---- witness sources (include/sonic_hip.h, "Witness sources") ----
WIT_FR32, WIT_I64 = 0, 1


def _is_torch(x) -> bool:
    return type(x).__module__.split(".")[0] == "torch"


def witness_vector(x, n: int, batch, who: str):
    """One vector of a witness source -> (kind, pointer, stride in bytes, device index or None for host memory, what to keep alive).
    x: a torch tensor or a numpy array, uint8 [n, 32] (canonical Fr) or int64 [n] -- with batch = K: [K, n, 32] or [K, n], inner
    dimensions contiguous, any leading stride that is a whole number of elements -- or, unbatched, a list of ints (fr_array).
    Everything that does not fit raises ValueError; nothing is copied except a list."""
    if not _is_torch(x) and not isinstance(x, np.ndarray):
        if batch is not None:
            raise ValueError(f"{who}: a batch is a torch tensor or a numpy array [K, n, 32] uint8 or [K, n] int64")
        x = fr_array(x)
    torch_like = _is_torch(x)
    dtype = str(x.dtype).replace("torch.", "")
    if dtype == "uint8":
        kind, elem, inner = WIT_FR32, 32, (n, 32)
    elif dtype == "int64":
        kind, elem, inner = WIT_I64, 8, (n,)
    else:
        raise ValueError(f"{who}: dtype {dtype} is neither uint8 ([n, 32] canonical Fr) nor int64 ([n])")
    want = inner if batch is None else (batch,) + inner
    if tuple(x.shape) != want:
        raise ValueError(f"{who}: shape {tuple(x.shape)}, need {want}")
    # strides in elements of the dtype (torch) or bytes (numpy) -> bytes
    item = 1 if kind == WIT_FR32 else 8
    strides = [s * item for s in x.stride()] if torch_like else list(x.strides)
    dense = [8] if kind == WIT_I64 else [32, 1]
    lead = strides[:len(strides) - len(dense)]
    if any(size > 1 and got != need for size, got, need in zip(inner, strides[len(lead):], dense)):
        raise ValueError(f"{who}: the inner dimensions must be contiguous")
    stride = n * elem
    if batch is not None:
        stride = lead[0] if batch > 1 else n * elem
        if stride < n * elem:
            raise ValueError(f"{who}: the leading stride ({stride} bytes) is below one assignment ({n * elem} bytes)")
    if torch_like:
        if x.device.type not in ("cuda", "cpu"):
            raise ValueError(f"{who}: a tensor on {x.device} is neither on a GPU nor on the CPU")
        device = x.device.index if x.device.type == "cuda" else None
        return kind, x.data_ptr(), stride, device, x
    return kind, x.ctypes.data, stride, None, x


# ---- compressed encodings: the host mirror (Python integers) ----
Z_MALFORMED, Z_OFF_CURVE, Z_OUTSIDE_SUBGROUP = 1, 2, 4          # verdicts: the error bits of the SRS loaders


class PointRefused(ValueError):
    """a compressed encoding that does not decode; .verdict holds Z_MALFORMED or Z_OFF_CURVE"""

    def __init__(self, verdict: int):
        super().__init__({Z_MALFORMED: "malformed compressed point", Z_OFF_CURVE: "compressed point not on the curve"}[verdict])
        self.verdict = verdict


def fq_sqrt(a: int):
    """a square root of a in Fq (q = 3 mod 4), or None when a is no square"""
    r = pow(a, (Q_MODULUS + 1) // 4, Q_MODULUS)
    return r if r * r % Q_MODULUS == a % Q_MODULUS else None


def fq2_sqrt(a):
    """a square root of a = (a0, a1) in Fq2 = Fq[u]/(u^2 + 1), or None"""
    q = Q_MODULUS
    a0, a1 = a[0] % q, a[1] % q
    if a1 == 0:
        r = fq_sqrt(a0)
        if r is not None:
            return (r, 0)
        return (0, fq_sqrt(-a0 % q))
    s = fq_sqrt((a0 * a0 + a1 * a1) % q)
    if s is None:
        return None
    inv2 = pow(2, -1, q)
    x0 = fq_sqrt((a0 + s) * inv2 % q)
    if x0 is None:
        x0 = fq_sqrt((a0 - s) * inv2 % q)
    x1 = a1 * pow(2 * x0, -1, q) % q
    return (x0, x1) if ((x0 * x0 - x1 * x1) % q, 2 * x0 * x1 % q) == (a0, a1) else None


def fq_is_high(y: int) -> bool:
    return y > (Q_MODULUS - 1) // 2


def fq2_is_high(y) -> bool:
    return fq_is_high(y[1]) if y[1] != 0 else fq_is_high(y[0])


def _x_and_flags(b: bytes):
    v = int.from_bytes(b, "big")
    return v & ((1 << 381) - 1), b[0] & 0xE0


def g1_compress(p) -> bytes:
    """(x, y) or None -> 48 bytes"""
    if p is None:
        return b"\xc0" + bytes(47)
    return (int(p[0]) | (1 << 383) | (int(fq_is_high(int(p[1]))) << 381)).to_bytes(48, "big")


def g1_decompress(b: bytes):
    """48 bytes -> (x, y) or None (infinity); PointRefused for a malformed or off-curve encoding.  No subgroup test."""
    b = bytes(b)
    if len(b) != 48:
        raise ValueError("a compressed G1 point is 48 bytes")
    x, fl = _x_and_flags(b)
    if not fl & 0x80:
        raise PointRefused(Z_MALFORMED)
    if fl & 0x40:
        if fl & 0x20 or x:
            raise PointRefused(Z_MALFORMED)
        return None
    if x >= Q_MODULUS:
        raise PointRefused(Z_MALFORMED)
    y = fq_sqrt((x * x * x + 4) % Q_MODULUS)
    if y is None:
        raise PointRefused(Z_OFF_CURVE)
    if fq_is_high(y) != bool(fl & 0x20):
        y = Q_MODULUS - y
    return (x, y)


def g2_compress(p) -> bytes:
    """((x0, x1), (y0, y1)) or None -> 96 bytes: x.c1 with the flags, then x.c0"""
    if p is None:
        return b"\xc0" + bytes(95)
    (x0, x1), y = p
    return (int(x1) | (1 << 383) | (int(fq2_is_high(y)) << 381)).to_bytes(48, "big") + int(x0).to_bytes(48, "big")


def g2_decompress(b: bytes):
    b = bytes(b)
    if len(b) != 96:
        raise ValueError("a compressed G2 point is 96 bytes")
    x1, fl = _x_and_flags(b[:48])
    x0, fl0 = _x_and_flags(b[48:])
    if not fl & 0x80 or fl0:
        raise PointRefused(Z_MALFORMED)
    if fl & 0x40:
        if fl & 0x20 or x0 or x1:
            raise PointRefused(Z_MALFORMED)
        return None
    if x0 >= Q_MODULUS or x1 >= Q_MODULUS:
        raise PointRefused(Z_MALFORMED)
    q = Q_MODULUS
    xx = ((x0 * x0 - x1 * x1) % q, 2 * x0 * x1 % q)
    rhs = ((xx[0] * x0 - xx[1] * x1 + 4) % q, (xx[0] * x1 + xx[1] * x0 + 4) % q)
    y = fq2_sqrt(rhs)
    if y is None:
        raise PointRefused(Z_OFF_CURVE)
    if fq2_is_high(y) != bool(fl & 0x20):
        y = (-y[0] % q, -y[1] % q)
    return ((x0, x1), y)


def g2_to_bytes(p) -> bytes:
    """the 192-byte G2 layout of the C ABI: x.c0 || x.c1 || y.c0 || y.c1, little-endian; infinity = zeros"""
    if p is None:
        return bytes(192)
    return b"".join(int(v).to_bytes(48, "little") for v in (p[0][0], p[0][1], p[1][0], p[1][1]))


def g2_from_bytes(b: bytes):
    b = bytes(b)
    if b == bytes(192):
        return None
    v = [int.from_bytes(b[48 * i:48 * i + 48], "little") for i in range(4)]
    return ((v[0], v[1]), (v[2], v[3]))
