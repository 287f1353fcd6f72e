"""Python-integer restatement of openPoly (src/Sonic/CommitmentScheme.hs:36-48), of s(X, y) / s(u, Y) of a circuit (sPoly,
src/Sonic/Constraints.hs:34-53, through evalY / evalX, src/Sonic/Utils.hs:17-21) and of the HscProof layout (src/Sonic/Signature.hs:22-72),
on DENSE coefficient lists, so that it stays affordable at a few hundred thousand coefficients where the dict-based restatement
(oracle/sonic_ref.py) is not.  Independent of the library: f(z) is Horner's rule and the quotient is synthetic division (the reference's
`divide`), NOT the prefix-sum identity of sonic_amd/csrc/poly.hip.  tests/test_open_ref.py holds it against both oracles at small sizes.

A dense Laurent polynomial is (lo, c): c[i] is the coefficient of X^(lo + i)."""
import numpy as np

R = 0x73EDA753299D7D483339D80809A1D80553BDA402FFFE5BFEFFFFFFFF00000001

# ---- the launch shapes of the stand-alone opening chain (sonic_amd/csrc/poly.hip), restated so that a test can say what a length exercises
SCALE_PER_MAX = 32          # SONIC_SCALE_PER
SCAN_TILE = 1024            # k_prefix_tiles / k_prefix_apply
TOP_CHUNK = 256             # tiles per iteration of k_prefix_top's carry loop


def scale_per(n: int) -> int:
    """scale_per (poly.hip): elements per thread of k_scale_powers over n elements"""
    return max(2, min(SCALE_PER_MAX, n // (256 * 64)))


def chain_shape(length: int) -> dict:
    """what one stand-alone opening of `length` coefficients launches: PER of the evaluation (n = length) and of the quotient
    (n = length - 1) pass, whether their last block is ragged, the scan tiles and the iterations of the carry loop"""
    pe, pq = scale_per(length), scale_per(max(length - 1, 1))
    tiles = -(-length // SCAN_TILE)
    return dict(per_eval=pe, per_quot=pq, ragged_eval=length % (256 * pe), ragged_quot=(length - 1) % (256 * pq), tiles=tiles,
                top_iters=-(-tiles // TOP_CHUNK) if tiles > 1 else 0)


def fr_pow(z: int, e: int) -> int:
    return pow(z, e, R) if e >= 0 else pow(pow(z, -1, R), -e, R)


def with_x0(lo: int, c):
    """the range extended to hold X^0 (openPoly subtracts f(z) there)"""
    c = [v % R for v in c]
    if not c:
        return 0, [0]
    if lo > 0:
        return 0, [0] * lo + c
    if lo + len(c) - 1 < 0:
        return lo, c + [0] * (-(lo + len(c) - 1))
    return lo, c


def evaluate(lo: int, c, z: int) -> int:
    """f(z) = z^lo * Horner(c, z); z = 0 needs lo >= 0 (0^-1 is undefined)"""
    acc = 0
    for v in reversed(c):
        acc = (acc * z + v) % R
    if z % R == 0:
        if lo < 0:
            raise ZeroDivisionError("evaluation at 0 of a negative power")
        return acc if lo == 0 else 0
    return acc * fr_pow(z, lo) % R


def open_dense(lo: int, c, z: int):
    """(f(z), (q_lo, q)) with q = (f(X) - f(z)) / (X - z): X^-lo (f - f(z)) is an ordinary polynomial that vanishes at z; synthetic
    division from the top, shifted back.  At z = 0 (lo >= 0 only) f(0) = c_0 and the quotient is the array shifted down by one."""
    lo, c = with_x0(lo, c)
    if z % R == 0:
        if lo < 0:
            raise ZeroDivisionError("openPoly at 0 of a polynomial with negative exponents")
        return c[0], (0, c[1:])
    fz = evaluate(lo, c, z)
    g = list(c)
    g[-lo] = (g[-lo] - fz) % R
    q = [0] * (len(g) - 1)
    carry = 0
    for k in range(len(g) - 1, 0, -1):
        carry = (g[k] + carry * z) % R
        q[k - 1] = carry
    if (g[0] + carry * z) % R:
        raise ValueError("inexact division")
    return fz, (lo, q)


def sparse(lo: int, c):
    """the normalised sparse form both oracles take: (int64 exponents, uint8 [k, 32] coefficients) of the non-zero terms"""
    idx = [i for i, v in enumerate(c) if v % R]
    exps = np.array([lo + i for i in idx], np.int64)
    raw = b"".join((c[i] % R).to_bytes(32, "little") for i in idx)
    return exps, np.frombuffer(raw, np.uint8).reshape(-1, 32).copy() if idx else np.zeros((0, 32), np.uint8)


def fr_rows(c) -> np.ndarray:
    """every coefficient, zeros included, as uint8 [len, 32]"""
    return np.frombuffer(b"".join((v % R).to_bytes(32, "little") for v in c), np.uint8).reshape(-1, 32).copy()


def as_dict(lo: int, c) -> dict:
    return {lo + i: v % R for i, v in enumerate(c) if v % R}


# ---- s(X, y) and s(u, Y) of a circuit -----------------------------------------------------------------------------------------------
# weights: three lists (wL, wR, wO) of Q rows, each a {gate index (0-based): value} mapping
def s_of_y(n: int, rows, y: int):
    """s(X, y) over [-n, 2n]: X^-i: sum_q wL[q][i] y^(n+q);  X^i: sum_q wR[q][i] y^(n+q);  X^(i+n): -y^i - y^-i + sum_q wO[q][i] y^(n+q)
    (q = 1..Q, i = 1..n)"""
    wL, wR, wO = rows
    c = [0] * (3 * n + 1)
    yi = pow(y, -1, R)
    p, m = 1, 1
    for i in range(1, n + 1):
        p, m = p * y % R, m * yi % R
        c[2 * n + i] = -(p + m) % R
    yq = pow(y, n, R)
    for q in range(len(wL)):
        yq = yq * y % R
        for i, v in wL[q].items():
            c[n - (i + 1)] = (c[n - (i + 1)] + v * yq) % R
        for i, v in wR[q].items():
            c[n + (i + 1)] = (c[n + (i + 1)] + v * yq) % R
        for i, v in wO[q].items():
            c[2 * n + (i + 1)] = (c[2 * n + (i + 1)] + v * yq) % R
    return -n, c


def s_of_u(n: int, rows, u: int):
    """s(u, Y) over [-n, n + Q]: Y^i and Y^-i: -u^(i+n);  Y^(n+q): sum_i wL[q][i] u^-i + wR[q][i] u^i + wO[q][i] u^(i+n)"""
    wL, wR, wO = rows
    Q = len(wL)
    c = [0] * (2 * n + Q + 1)
    up = [fr_pow(u, e) for e in range(-n, 2 * n + 1)]          # up[e + n] = u^e
    for i in range(1, n + 1):
        c[n + i] = c[n - i] = -up[2 * n + i] % R
    for q in range(Q):
        acc = 0
        for i, v in wL[q].items():
            acc += v * up[n - (i + 1)]
        for i, v in wR[q].items():
            acc += v * up[n + (i + 1)]
        for i, v in wO[q].items():
            acc += v * up[2 * n + (i + 1)]
        c[2 * n + 1 + q] = acc % R
    return -n, c


def dense_weights(n: int, rows):
    """the Q x n lists oracle/sonic_ref.py and ArithCircuit take"""
    return tuple([[row.get(i, 0) for i in range(n)] for row in w] for w in rows)


# ---- bivariate polynomials as term lists [(x exponent, y exponent, coefficient)] ---------------------------------------------------------
def biv_keep(terms, keep_x: bool, point: int):
    """evalY point (keep_x) / evalX point of a sparse bivariate Laurent polynomial, dense over the kept variable's range with X^0 in it"""
    kept = [(ex if keep_x else ey) for ex, ey, _ in terms]
    lo, hi = min(kept + [0]), max(kept + [0])
    c = [0] * (hi - lo + 1)
    for ex, ey, v in terms:
        k, o = (ex, ey) if keep_x else (ey, ex)
        c[k - lo] = (c[k - lo] + v * fr_pow(point, o)) % R
    return lo, c


# ---- hscProve (Signature.hs:38-72; oracle/sonic_ref.py hsc_prove names the order) ------------------------------------------------------
def hsc_expected(commit, open_, d: int, sxy, su, yzs, u: int, v: int) -> bytes:
    """The bytes of an HscProof -- [S_j, s_j, W_j]_j, [s'_j, W'_j, Q_j]_j, Q_v, C, u, v -- from a commitPoly and an openPoly:
    commit(max, lo, c) -> 96 bytes, open_(z, lo, c) -> (f(z), 96 bytes).  sxy: the dense s(X, y_j) per pair, su: the dense s(u, Y)."""
    fr = lambda a: (a % R).to_bytes(32, "little")      # noqa: E731
    out = []
    for (_y, z), (lo, c) in zip(yzs, sxy):             # :40-45
        s, w = open_(z, lo, c)
        out += [commit(d, lo, c), fr(s), w]
    for (y, _z), (lo, c) in zip(yzs, sxy):             # :53-57
        _, wp = open_(u, lo, c)
        sp, qj = open_(y, *su)
        out += [fr(sp), wp, qj]
    out += [open_(v, *su)[1], commit(d, *su), fr(u), fr(v)]      # :63, :52
    return b"".join(out)


def hsc_parts(raw: bytes, m: int):
    """the named elements of HscProof bytes, for comparing one by one"""
    assert len(raw) == (2 + 4 * m) * 96 + (2 + 2 * m) * 32
    names = [(f"{k}[{j}]", sz) for j in range(m) for k, sz in (("S", 96), ("s", 32), ("W", 96))]
    names += [(f"{k}[{j}]", sz) for j in range(m) for k, sz in (("s'", 32), ("W'", 96), ("Q", 96))]
    names += [("Qv", 96), ("C", 96), ("u", 32), ("v", 32)]
    parts, pos = [], 0
    for name, sz in names:
        parts.append((name, raw[pos:pos + sz]))
        pos += sz
    return parts
