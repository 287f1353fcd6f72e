"""Readers and writers for the two iden3 containers of a rank-1 constraint system and its witness, host Python only.

`.r1cs`   magic "r1cs", u32 version 1, u32 section count; each section u32 type, u64 size, body.
          header (type 1): u32 field size, the prime (little-endian), u32 nWires, nPubOut, nPubIn, nPrvIn, u64 nLabels, u32 mConstraints
          constraints (type 2): per constraint three linear combinations A, B, C, each u32 nTerms then (u32 wire, value little-endian)
          wire-to-label map (type 3): u64 per wire
`.wtns`   magic "wtns", u32 version 2, u32 section count; section 1: u32 field size, the prime, u32 count; section 2: the values

Wire 0 is the constant one and n_pub = nPubOut + nPubIn, which is the column order of sonic_amd.R1CS.  Terms are sorted by wire, and
duplicate wires summed, when read.  Only the scalar field of BLS12-381 is accepted.  All integers little-endian.

Interoperability with files written by circom / snarkjs is UNVERIFIED: the layouts above are implemented as stated, and the tests only
write files with this module and read them back.
"""
from __future__ import annotations

import struct
from dataclasses import dataclass, field
from typing import List

from .encoding import R_MODULUS


@dataclass
class R1csFile:
    n_wires: int
    n_pub_out: int
    n_pub_in: int
    n_prv_in: int
    A: List[dict]                   # per constraint {wire: value}
    B: List[dict]
    C: List[dict]
    n_labels: int = 0
    labels: List[int] = field(default_factory=list)
    prime: int = R_MODULUS

    @property
    def n_pub(self) -> int:
        return self.n_pub_out + self.n_pub_in

    @property
    def m(self) -> int:
        return len(self.A)

    def to_r1cs(self, device=None):
        """the sonic_amd.R1CS of this file (N = nWires, n_pub = nPubOut + nPubIn)"""
        from .r1cs import R1CS
        return R1CS.from_rows(self.n_wires, self.n_pub, self.A, self.B, self.C, device=device)


def _check_prime(prime: int, what: str) -> None:
    if prime != R_MODULUS:
        raise ValueError(f"{what}: the file's prime {prime:#x} is not the scalar field of BLS12-381, r = {R_MODULUS:#x}")


def _sections(raw: bytes, magic: bytes, version: int, what: str):
    if len(raw) < 12 or raw[:4] != magic:
        raise ValueError(f"{what}: not a {magic.decode()} file (magic {raw[:4]!r})")
    ver, count = struct.unpack_from("<II", raw, 4)
    if ver != version:
        raise ValueError(f"{what}: version {ver}, this reader knows version {version}")
    at, out = 12, {}
    for _ in range(count):
        if at + 12 > len(raw):
            raise ValueError(f"{what}: truncated section header")
        typ, size = struct.unpack_from("<IQ", raw, at)
        at += 12
        if at + size > len(raw):
            raise ValueError(f"{what}: section {typ} of {size} bytes runs past the end of the file")
        out.setdefault(typ, raw[at:at + size])
        at += size
    return out


def _container(magic: bytes, version: int, sections) -> bytes:
    out = magic + struct.pack("<II", version, len(sections))
    for typ, body in sections:
        out += struct.pack("<IQ", typ, len(body)) + body
    return out


def write_r1cs(path, f: R1csFile) -> None:
    fs = 32
    if not (len(f.A) == len(f.B) == len(f.C)):
        raise ValueError("write_r1cs: A, B, C need the same number of constraints")
    header = struct.pack("<I", fs) + f.prime.to_bytes(fs, "little") + struct.pack("<IIIIQI", f.n_wires, f.n_pub_out, f.n_pub_in, f.n_prv_in, f.n_labels, len(f.A))
    body = bytearray()
    for a, b, c in zip(f.A, f.B, f.C):
        for lc in (a, b, c):
            items = list(lc.items()) if isinstance(lc, dict) else list(lc)      # (a list of (wire, value) pairs is written as it is)
            body += struct.pack("<I", len(items))
            for wire, v in items:
                body += struct.pack("<I", int(wire)) + (int(v) % f.prime).to_bytes(fs, "little")
    sections = [(1, header), (2, bytes(body))]
    if f.labels:
        sections.append((3, b"".join(struct.pack("<Q", int(x)) for x in f.labels)))
    with open(path, "wb") as fh:
        fh.write(_container(b"r1cs", 1, sections))


def read_r1cs(path) -> R1csFile:
    with open(path, "rb") as fh:
        raw = fh.read()
    what = f"read_r1cs({path})"
    sec = _sections(raw, b"r1cs", 1, what)
    if 1 not in sec or 2 not in sec:
        raise ValueError(f"{what}: the header (type 1) or the constraints (type 2) are missing")
    h = sec[1]
    (fs,) = struct.unpack_from("<I", h, 0)
    if len(h) != 4 + fs + 28:
        raise ValueError(f"{what}: header of {len(h)} bytes, need {4 + fs + 28} for a field of {fs} bytes")
    prime = int.from_bytes(h[4:4 + fs], "little")
    _check_prime(prime, what)
    n_wires, n_pub_out, n_pub_in, n_prv_in, n_labels, m = struct.unpack_from("<IIIIQI", h, 4 + fs)
    body, at = sec[2], 0
    mats = ([], [], [])
    for i in range(m):
        for k in range(3):
            if at + 4 > len(body):
                raise ValueError(f"{what}: the constraints end inside constraint {i}")
            (nterms,) = struct.unpack_from("<I", body, at)
            at += 4
            if at + nterms * (4 + fs) > len(body):
                raise ValueError(f"{what}: the constraints end inside constraint {i}")
            lc = {}
            for _ in range(nterms):
                (wire,) = struct.unpack_from("<I", body, at)
                v = int.from_bytes(body[at + 4:at + 4 + fs], "little")
                at += 4 + fs
                if wire >= n_wires:
                    raise ValueError(f"{what}: constraint {i} names wire {wire}, the file has {n_wires}")
                if v >= prime:
                    raise ValueError(f"{what}: constraint {i}: a coefficient is not below the prime")
                lc[wire] = (lc.get(wire, 0) + v) % prime
            mats[k].append(dict(sorted(lc.items())))
    if at != len(body):
        raise ValueError(f"{what}: {len(body) - at} bytes follow the last constraint")
    labels = [x for (x,) in struct.iter_unpack("<Q", sec[3])] if 3 in sec and len(sec[3]) % 8 == 0 else []
    return R1csFile(n_wires, n_pub_out, n_pub_in, n_prv_in, mats[0], mats[1], mats[2], n_labels, labels, prime)


def write_wtns(path, values, prime: int = R_MODULUS) -> None:
    fs = 32
    values = [int(v) % prime for v in values]
    header = struct.pack("<I", fs) + prime.to_bytes(fs, "little") + struct.pack("<I", len(values))
    with open(path, "wb") as fh:
        fh.write(_container(b"wtns", 2, [(1, header), (2, b"".join(v.to_bytes(fs, "little") for v in values))]))


def read_wtns(path) -> List[int]:
    with open(path, "rb") as fh:
        raw = fh.read()
    what = f"read_wtns({path})"
    sec = _sections(raw, b"wtns", 2, what)
    if 1 not in sec or 2 not in sec:
        raise ValueError(f"{what}: section 1 (the header) or 2 (the values) is missing")
    h = sec[1]
    (fs,) = struct.unpack_from("<I", h, 0)
    if len(h) != 4 + fs + 4:
        raise ValueError(f"{what}: header of {len(h)} bytes, need {8 + fs} for a field of {fs} bytes")
    prime = int.from_bytes(h[4:4 + fs], "little")
    _check_prime(prime, what)
    (count,) = struct.unpack_from("<I", h, 4 + fs)
    if len(sec[2]) != count * fs:
        raise ValueError(f"{what}: {len(sec[2])} bytes of values, need {count} x {fs}")
    vals = [int.from_bytes(sec[2][fs * i:fs * i + fs], "little") for i in range(count)]
    if any(v >= prime for v in vals):
        raise ValueError(f"{what}: a value is not below the prime")
    return vals
