"""The updatable SRS restated with hashlib and Python integers (test infrastructure; the normative text: sonic_amd/csrc/srs_update.hpp and
include/sonic_hip.h, "Updatable SRS"): the randomizers of the structure check, the proof of a contribution -- layout, challenge, seeded
nonces, maker, verifier -- and whole strings as lists of points over oracle/, small enough (d = 12) for the pure-Python pairing."""
import hashlib

from oracle import pairing as pr
from oracle.sonic_ref import G1_GEN, g1_add, g1_mul
from sonic_amd import encoding as enc

R = pr.R
PROOF_BYTES = 448
OFF = dict(X=0, A=96, Rx=192, Ra=288, sx=384, sa=416)


def le64(v: int) -> bytes:
    return v.to_bytes(8, "little")


def rho(seed: bytes, index: int) -> int:
    """randomizer of exponent e = index - d: the first 16 bytes of the digest as a little-endian integer, 1 in place of 0"""
    return int.from_bytes(hashlib.sha256(b"sonic-hip/srs-check/v1" + seed + le64(index)).digest()[:16], "little") or 1


def wide(d0: bytes, d1: bytes) -> int:
    return int.from_bytes(d0 + d1, "little") % R


def challenge(d: int, old_id: bytes, points384: bytes) -> int:
    st = hashlib.sha256(b"sonic-hip/srs-update/v1" + le64(d) + old_id).digest()
    st = hashlib.sha256(st + b"points" + points384).digest()
    h = [hashlib.sha256(st + b"c" + (0).to_bytes(4, "little") + bytes([half])).digest() for half in (0, 1)]
    return wide(h[0], h[1]) or 1


def seeded_nonce(seed: bytes, x1: int, a1: int, old_id: bytes, i: int) -> int:
    L = b"sonic-hip/srs-update-nonce/v1" + seed + enc.fr_to_bytes(x1) + enc.fr_to_bytes(a1) + old_id + i.to_bytes(4, "little")
    return wide(hashlib.sha256(L + b"\0").digest(), hashlib.sha256(L + b"\1").digest()) or 1


def make_proof(d: int, old_id: bytes, x1: int, a1: int, kx: int, ka: int) -> bytes:
    pts = b"".join(enc.g1_to_bytes(g1_mul(G1_GEN, k)) for k in (x1, a1, kx, ka))
    c = challenge(d, old_id, pts)
    return pts + enc.fr_to_bytes((kx + c * x1) % R) + enc.fr_to_bytes((ka + c * a1) % R)


def in_subgroup(p) -> bool:
    return p is not None and g1_add(g1_mul(p, R - 1), p) is None


def load_point(b: bytes):
    """a point a proof may hold, or False: canonical, on the curve, in the subgroup, not infinity"""
    x, y = int.from_bytes(b[:48], "little"), int.from_bytes(b[48:], "little")
    if (x, y) == (0, 0) or x >= pr.Q or y >= pr.Q or (y * y - x * x * x - 4) % pr.Q:
        return False
    return (x, y) if in_subgroup((x, y)) else False


def schnorr_ok(d: int, old_id: bytes, proof: bytes):
    """False, or (X, A): the encodings and sx g = Rx + c X, sa g = Ra + c A"""
    if len(proof) != PROOF_BYTES:
        return False
    X, A, Rx, Ra = (load_point(proof[o:o + 96]) for o in (0, 96, 192, 288))
    sx, sa = (int.from_bytes(proof[o:o + 32], "little") for o in (384, 416))
    if not (X and A and Rx and Ra) or sx >= R or sa >= R:
        return False
    c = challenge(d, old_id, proof[:384])
    if g1_mul(G1_GEN, sx) != g1_add(Rx, g1_mul(X, c)) or g1_mul(G1_GEN, sa) != g1_add(Ra, g1_mul(A, c)):
        return False
    return X, A


# ---- whole strings over Python integers: {"d", "G0", "G1", "H0", "H1"}, lists indexed by e + d; G1[d] (e = 0) is None --------------------
def make_string(d: int, x: int, alpha: int, g=G1_GEN, h=pr.G2_GEN):
    xs = [pow(x, e, R) for e in range(-d, d + 1)]
    return dict(d=d, G0=[g1_mul(g, p) for p in xs], G1=[None if e == d else g1_mul(g, alpha * p % R) for e, p in enumerate(xs)],
                H0=[pr.g2_mul(h, p) for p in xs], H1=[pr.g2_mul(h, alpha * p % R) for p in xs])


def update_string(s, x1: int, a1: int):
    d = s["d"]
    xs = [pow(x1, e, R) for e in range(-d, d + 1)]
    return dict(d=d, G0=[g1_mul(p, k) for p, k in zip(s["G0"], xs)], G1=[None if p is None else g1_mul(p, a1 * k % R) for p, k in zip(s["G1"], xs)],
                H0=[pr.g2_mul(p, k) for p, k in zip(s["H0"], xs)], H1=[pr.g2_mul(p, a1 * k % R) for p, k in zip(s["H1"], xs)])


def string_id(s) -> bytes:
    """fs.hpp's srs id: g^x, g^{alpha x}, g^{1/x}, g^{alpha/x}"""
    d = s["d"]
    pts = [s["G0"][d + 1], s["G1"][d + 1], s["G0"][d - 1], s["G1"][d - 1]]
    return hashlib.sha256(b"sonic-hip/srs/v1" + le64(d) + b"".join(enc.g1_to_bytes(p) for p in pts)).digest()


def g1_neg(p):
    return None if p is None else (p[0], (-p[1]) % pr.Q)


def pairs_equal(P1, Q1, P2, Q2) -> bool:
    return pr.pairing_product_is_one([(P1, Q1), (g1_neg(P2), Q2)])


def verify_update_links(old, new, proof: bytes) -> bool:
    """everything of the verifier but the structure check of the new string"""
    if old["d"] != new["d"]:
        return False
    got = schnorr_ok(old["d"], string_id(old), proof)
    if not got:
        return False
    X, A = got
    d = old["d"]
    return pairs_equal(new["G0"][d + 1], pr.G2_GEN, X, old["H0"][d + 1]) and pairs_equal(G1_GEN, new["H1"][d], A, old["H1"][d])


def g1_msm(points, scalars):
    acc = None
    for p, k in zip(points, scalars):
        if p is not None:
            acc = g1_add(acc, g1_mul(p, k))
    return acc


def g2_msm(points, scalars):
    acc = None
    for p, k in zip(points, scalars):
        acc = pr.g2_add(acc, pr.g2_mul(p, k))
    return acc


def check_string(s, seed: bytes) -> int:
    """the failed mask of sonic_srs_check, relation by relation as the header states them"""
    d = s["d"]
    n = 2 * d + 1
    r = [rho(seed, i) for i in range(n)]
    G0, G1, H0, H1 = s["G0"], s["G1"], s["H0"], s["H1"]
    failed = 0
    if G0[d] != G1_GEN or H0[d] != pr.G2_GEN:
        failed |= 1
    if not pairs_equal(g1_msm(G0[:-1], r[:-1]), H0[d + 1], g1_msm(G0[1:], r[:-1]), pr.G2_GEN):
        failed |= 2
    off0 = [k for i, k in enumerate(r) if i != d]
    if not pairs_equal(g1_msm([p for i, p in enumerate(G1) if i != d], off0), pr.G2_GEN, g1_msm([p for i, p in enumerate(G0) if i != d], off0), H1[d]):
        failed |= 4
    full = g1_msm(G0, r)
    if not pairs_equal(G1_GEN, g2_msm(H0, r), full, pr.G2_GEN):
        failed |= 8
    if not pairs_equal(G1_GEN, g2_msm(H1, r), full, H1[d]):
        failed |= 16
    return failed
