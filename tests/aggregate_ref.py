"""Independent restatement of the helped-verification definitions (include/sonic_hip.h, "Helped verification"; sonic_amd/csrc/fs.hpp) with
hashlib and plain integers: the weights digest, the transcript of an aggregate, the digest of a helped batch.  Test infrastructure: the tests
hold the library against these, byte for byte."""
import hashlib

R = 0x73EDA753299D7D483339D80809A1D80553BDA402FFFE5BFEFFFFFFFF00000001
MIDSTATE_SIZE, CORE_SIZE = 112, 576


def le64(v: int) -> bytes:
    return int(v).to_bytes(8, "little")


def fr(v: int) -> bytes:
    return int(v).to_bytes(32, "little")


def aggregate_size(K: int) -> int:
    """an HscProof with m = K: 4K + 2 points and 2K + 2 field elements"""
    return (4 * K + 2) * 96 + (2 * K + 2) * 32


def parts(K: int, agg: bytes) -> dict:
    """[S_j, s_j, W_j]_j, [s'_j, W'_j, Q_j]_j, Q_v, C, u, v"""
    assert len(agg) == aggregate_size(K)
    at = 448 * K
    return dict(hscS=agg[:224 * K], hscW=agg[224 * K:at], Qv=agg[at:at + 96], C=agg[at + 96:at + 192], u=agg[at + 192:at + 224], v=agg[at + 224:at + 256])


def s_of(K: int, agg: bytes, k: int) -> bytes:
    """s_k = s(z_k, y_k), as the aggregate states it"""
    return parts(K, agg)["hscS"][224 * k + 96:224 * k + 128]


def weights_digest(midstate: bytes) -> bytes:
    assert len(midstate) == MIDSTATE_SIZE
    return hashlib.sha256(b"sonic-hip/weights/v1" + midstate).digest()


def _challenge(st: bytes, label: bytes, i: int = 0) -> int:
    wide = b"".join(hashlib.sha256(st + label + i.to_bytes(4, "little") + bytes([half])).digest() for half in (0, 1))
    return int.from_bytes(wide, "little") % R or 1


def aggregate_challenges(n, Q, d, wdigest: bytes, srs_id: bytes, yzs, agg: bytes):
    """(u, v) from the bytes of an aggregate for the pairs yzs ((y, z) ints): its own u, v are not read"""
    K = len(yzs)
    p = parts(K, agg)
    st = hashlib.sha256(b"sonic-hip/fs-agg/v1" + le64(n) + le64(Q) + le64(d) + wdigest + srs_id).digest()
    st = hashlib.sha256(st + b"pairs" + le64(K) + b"".join(fr(y) + fr(z) for y, z in yzs)).digest()
    st = hashlib.sha256(st + b"hscS" + p["hscS"]).digest()
    u = _challenge(st, b"u")
    st = hashlib.sha256(st + b"hscW" + p["C"] + p["hscW"]).digest()
    return u, _challenge(st, b"v")


def helped_digest(n, Q, d, wdigest: bytes, srs_id: bytes, proofs, yzs, constants, agg: bytes) -> bytes:
    """D of a helped batch; proofs: 576 bytes each; yzs: (y, z) ints; constants: Q x 32 bytes per proof"""
    K = len(proofs)
    assert len(agg) == aggregate_size(K)
    h = hashlib.sha256(b"sonic-hip/batch-digest/helped/v1" + le64(n) + le64(Q) + le64(d) + wdigest + srs_id + le64(K))
    for p, (y, z), cs in zip(proofs, yzs, constants):
        assert len(p) == CORE_SIZE and len(cs) == 32 * Q
        h.update(p + fr(y) + fr(z) + cs)
    h.update(agg)
    return h.digest()
