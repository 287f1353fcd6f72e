"""Python restatement of the definitions of "One circuit, many statements" (include/sonic_hip.h; sonic_amd/csrc/fs.hpp), with hashlib and
integers only, independent of the library: the whole circuit digest, the batch digest v2 and its randomizers."""
import hashlib

R = 0x73EDA753299D7D483339D80809A1D80553BDA402FFFE5BFEFFFFFFFF00000001


def le64(v: int) -> bytes:
    return int(v).to_bytes(8, "little")


def fr(v: int) -> bytes:
    return (int(v) % R).to_bytes(32, "little")


def circuit_digest(n, Q, wL, wR, wO, cs) -> bytes:
    """SHA-256("sonic-hip/circuit/v1" || le64 n || le64 Q || wL || wR || wO || cs), weights as Q rows of n integers"""
    h = hashlib.sha256(b"sonic-hip/circuit/v1" + le64(n) + le64(Q))
    for w in (wL, wR, wO):
        for row in w:
            assert len(row) == n
            h.update(b"".join(fr(v) for v in row))
    h.update(b"".join(fr(c) for c in cs))
    return h.digest()


def weights_length(n, Q) -> int:
    """bytes hashed when the midstate is taken: the label, two le64 and 3 Q n field elements"""
    return 20 + 16 + 96 * Q * n


def batch_digest_v2(n, Q, d, circuit_digest_: bytes, srs_id: bytes, proofs, challenge_blocks, constants) -> bytes:
    """D = SHA-256("sonic-hip/batch-digest/v2" || le64 n || le64 Q || le64 d || circuit digest || srs id || le64 K ||
    K x (proof bytes || its challenges || cs_k)); constants: K byte strings of Q x 32"""
    h = hashlib.sha256(b"sonic-hip/batch-digest/v2" + le64(n) + le64(Q) + le64(d) + circuit_digest_ + srs_id + le64(len(proofs)))
    for p, c, k in zip(proofs, challenge_blocks, constants):
        h.update(p)
        h.update(c)
        h.update(k)
    return h.digest()


def randomizers(seed: bytes, D: bytes, count: int, i0: int = 0):
    """rho_i = the first 128 bits (little-endian) of SHA-256("sonic-hip/batch/v1" || seed || D || le64 i), 0 replaced by 1: derived from D
    exactly as for digest v1"""
    out = []
    for i in range(i0, i0 + count):
        rho = int.from_bytes(hashlib.sha256(b"sonic-hip/batch/v1" + seed + D + le64(i)).digest()[:16], "little")
        out.append(rho or 1)
    return out
