"""Python restatement of the batched verifier's definitions (include/sonic_hip.h, "the batched verifier"): the randomizers, the batch
digest, the list of a proof's pcV checks and the fold -- over oracle/sonic_ref.py and oracle/pairing.py, independent of the library."""
import hashlib

from oracle import pairing as pg
from oracle import sonic_ref as ref

R = ref.R


def le64(v: int) -> bytes:
    return int(v).to_bytes(8, "little")


def randomizers(seed: bytes, D: bytes, count: int, i0: int = 0):
    out = []
    for i in range(i0, i0 + count):
        rho = int.from_bytes(hashlib.sha256(b"sonic-hip/batch/v1" + seed + D + le64(i)).digest()[:16], "little")
        out.append(rho or 1)
    return out


def batch_digest(n, Q, d, circuit_digest: bytes, srs_id: bytes, proofs, challenge_blocks) -> bytes:
    h = hashlib.sha256(b"sonic-hip/batch-digest/v1" + le64(n) + le64(Q) + le64(d) + circuit_digest + srs_id + le64(len(proofs)))
    for p, c in zip(proofs, challenge_blocks):
        h.update(p)
        h.update(c)
    return h.digest()


def s_of_uv(n, Q, rows, u, v):
    """s(u, v) as s_of_uv of verify_host.hpp sums it; rows: 3Q lists of (gate index 0-based, value) -- wL, wR, wO"""
    ui, vi = pow(u, -1, R), pow(v, -1, R)
    acc = 0
    for q in range(Q):
        rs = 0
        for mat in range(3):
            for i0, w in rows[mat * Q + q]:
                i = i0 + 1
                rs += w * (pow(ui, i, R) if mat == 0 else pow(u, i if mat == 1 else i + n, R))
        acc += rs % R * pow(v, n + q + 1, R)
    up, vp, vm = pow(u, n, R), 1, 1
    for _ in range(1, n + 1):
        up, vp, vm = up * u % R, vp * v % R, vm * vi % R
        acc -= up * (vp + vm)
    return acc % R


def dense_rows(wL, wR, wO):
    return [[(i, w % R) for i, w in enumerate(row) if w % R] for m in (wL, wR, wO) for row in m]


def checks_of(circuit, d, proof, y, z, yzs):
    """the 4 + 3Q pcV checks (max, F, z, v, W) of verify (Protocol.hs:123-125, then Signature.hs:82-89), in sonic_verify's order"""
    wL, wR, wO, cs = circuit
    n, Q = len(wL[0]), len(cs)
    ky = sum(c * pow(y, n + q + 1, R) for q, c in enumerate(cs)) % R
    t = (proof["prA"] * (proof["prB"] + proof["prS"]) - ky) % R
    h = proof["prHscProof"]
    sv = s_of_uv(n, Q, dense_rows(wL, wR, wO), h["hscU"], h["hscV"])
    out = [(n, proof["prR"], z, proof["prA"], proof["prWa"]), (n, proof["prR"], y * z % R, proof["prB"], proof["prWb"]),
           (d, proof["prT"], z, t, proof["prWt"])]
    for (yj, zj), (cj, (sj, wj)), (sjp, wjp, qj) in zip(yzs, h["hscS"], h["hscW"]):
        out += [(d, cj, zj, sj, wj), (d, cj, h["hscU"], sjp, wjp), (d, h["hscC"], yj, sjp, qj)]
    out.append((d, h["hscC"], h["hscV"], sv, h["hscQv"]))
    return out


def fold_accepts(srs: "pg.SRS", checks, rhos) -> bool:
    """e(sum rho W, h^{alpha x}) e((sum rho v) g - sum rho z W, h^alpha) prod_m e(-sum_{max = m} rho F, h^{x^{m-d}}) == 1"""
    A = B = ref.INF
    gv = 0
    C = {}
    for (m, F, z, v, W), rho in zip(checks, rhos):
        A = ref.g1_add(A, ref.g1_mul(W, rho))
        B = ref.g1_add(B, ref.g1_mul(W, rho * z % R))
        gv = (gv + rho * v) % R
        C[m] = ref.g1_add(C.get(m, ref.INF), ref.g1_mul(F, rho))
    B = ref.g1_add(ref.g1_mul(ref.G1_GEN, gv), ref.g1_neg(B))
    pairs = [(A, srs.hPositiveAlphaX(1)), (B, srs.hPositiveAlphaX(0))]
    for m, Cm in C.items():
        diff = m - srs.d
        pairs.append((ref.g1_neg(Cm), srs.hPositiveX(diff) if diff >= 0 else srs.hNegativeX(-diff - 1)))
    return pg.pairing_product_is_one(pairs)
