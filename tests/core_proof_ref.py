"""Independent restatement of the core-proof definitions (include/sonic_hip.h, "Core proofs"; sonic_amd/csrc/fs.hpp) with hashlib and plain
integers: the record, the transcript, the batch digest.  Test infrastructure: the tests hold the library against these, byte for byte."""
import hashlib

R = 0x73EDA753299D7D483339D80809A1D80553BDA402FFFE5BFEFFFFFFFF00000001
CORE_SIZE, CORE_SIZE_Z = 576, 336
# record order: (kind, index) -- G: MSM slot R T Wa Wb Wt = 0..4; F: evaluation a b s = 0..2
RECORD = [("G", 0), ("G", 1), ("F", 0), ("G", 2), ("F", 1), ("G", 3), ("G", 4), ("F", 2)]
OFFSETS = {"R": 0, "T": 96, "a": 192, "Wa": 224, "b": 320, "Wb": 352, "Wt": 448, "s": 544}
POINTS = ["R", "T", "Wa", "Wb", "Wt"]


def le64(v: int) -> bytes:
    return int(v).to_bytes(8, "little")


def fr(v: int) -> bytes:
    return int(v).to_bytes(32, "little")


def field_offsets(point_bytes: int = 96):
    """[(offset, kind, index)] of the record with points of point_bytes"""
    out, at = [], 0
    for kind, i in RECORD:
        out.append((at, kind, i))
        at += point_bytes if kind == "G" else 32
    return out


class Transcript:
    """the state machine of fs.hpp: st <- SHA256(st || label || data); challenge = (SHA256(st || label || le32 i || 0) || SHA256(.. || 1))
    as a little-endian integer mod r, 1 in place of 0"""

    def __init__(self, label: bytes, n, Q, d, circuit_digest: bytes, srs_id: bytes):
        self.st = hashlib.sha256(label + le64(n) + le64(Q) + le64(d) + circuit_digest + srs_id).digest()

    def absorb(self, label: bytes, data: bytes):
        self.st = hashlib.sha256(self.st + label + data).digest()

    def challenge(self, label: bytes, i: int = 0) -> int:
        wide = b"".join(hashlib.sha256(self.st + label + i.to_bytes(4, "little") + bytes([half])).digest() for half in (0, 1))
        return int.from_bytes(wide, "little") % R or 1


def core_challenges(n, Q, d, circuit_digest: bytes, srs_id: bytes, proof: bytes):
    """(y, z) of a core proof: absorb R -> y, absorb T -> z, under the core label"""
    t = Transcript(b"sonic-hip/fs-core/v1", n, Q, d, circuit_digest, srs_id)
    t.absorb(b"R", proof[0:96])
    y = t.challenge(b"y")
    t.absorb(b"T", proof[96:192])
    return y, t.challenge(b"z")


def full_challenges_yz(n, Q, d, circuit_digest: bytes, srs_id: bytes, proof: bytes):
    """(y, z) of a FULL Fiat-Shamir proof (label sonic-hip/fs/v2): what a core proof's must differ from"""
    t = Transcript(b"sonic-hip/fs/v2", n, Q, d, circuit_digest, srs_id)
    t.absorb(b"R", proof[0:96])
    y = t.challenge(b"y")
    t.absorb(b"T", proof[96:192])
    return y, t.challenge(b"z")


def core_batch_digest(n, Q, d, circuit_digest: bytes, srs_id: bytes, proofs, yzs, constants) -> bytes:
    """D of a batch of core proofs; proofs: 576 bytes each; yzs: (y, z) ints; constants: Q x 32 bytes per proof"""
    h = hashlib.sha256(b"sonic-hip/batch-digest/core/v1" + le64(n) + le64(Q) + le64(d) + circuit_digest + srs_id + le64(len(proofs)))
    for p, (y, z), cs in zip(proofs, yzs, constants):
        assert len(p) == CORE_SIZE and len(cs) == 32 * Q
        h.update(p + fr(y) + fr(z) + cs)
    return h.digest()
