"""The stand-alone commitment-scheme entry points -- sonic_commit_poly, sonic_open_poly, sonic_hsc_prove_poly, sonic_prover_hsc_prove
(commitPoly / openPoly, src/Sonic/CommitmentScheme.hs:20-48; hscProve, src/Sonic/Signature.hs:32-72) -- at the lengths where their kernel
chain changes shape.  prove() opens through the batched chain (open_batch_enqueue); these calls run open_job -> k_scale_powers<0|2> with a
PER chosen per length, k_prefix_tiles / k_prefix_top / k_prefix_apply, quotient_job / open_job_at_zero / commit_job with their clipping,
and the hscProve entry points add scratch reuse and a flush every MSM_MAX_JOBS = 16 jobs.

Everything is compared byte for byte (Fr and G1 are exact).  f(z) against Horner's rule in Python integers (tests/open_ref.py) AND the C
oracle; W against the oracle's openPoly, and -- where PYQ is set -- against the oracle's MSM over the quotient that Python's synthetic
division gave, so that a disagreement says which side moved.  Each case names what it is there for; its PER, scan tiles and carry-loop
iterations are computed by open_ref.chain_shape (restating scale_per and the tile size of sonic_amd/csrc/poly.hip) and asserted."""
import ctypes as C
import random

import numpy as np
import pytest

import open_ref
from open_ref import R, chain_shape
from util import NCPU, fr_bytes, fr_ints, rand_fr_array

pytestmark = pytest.mark.gpu

ERR_SRS_INDEX = 2           # SONIC_ERR_SRS_INDEX


class Pair:
    """one real SRS (random x, alpha) on both sides: generated on the GPU, handed to the oracle as points"""

    def __init__(self, sonic, orc, d, seed):
        pyr = random.Random(seed)
        self.d = d
        self.x, self.alpha = pyr.randrange(2, R), pyr.randrange(2, R)
        self.g = sonic.SRS.new(d, self.x, self.alpha)
        self.o = orc.SRS.from_points(d, self.g.points(0, -d, 2 * d + 1), self.g.points(1, -d, 2 * d + 1), threads=NCPU)
        orc.set_mode(1, NCPU)


def _pair_fixture(d, seed):
    @pytest.fixture(scope="module")
    def fx(sonic, orc):
        p = Pair(sonic, orc, d, seed)
        yield p
        p.g.close()
    return fx


D_TILE, D_MID, D_17, D_18 = 1024, 24704, 1 << 17, 1 << 18      # the smallest d that admits 2049 / 49408 / 262146 / 524290 coefficients
pair_tile = _pair_fixture(D_TILE, 101)
pair_mid = _pair_fixture(D_MID, 102)
pair_17 = _pair_fixture(D_17, 103)
pair_18 = _pair_fixture(D_18, 104)


def _lib(sonic):
    from sonic_amd import _lib as m
    return m.lib()


def gpu_open(sonic, g, z, exps, co):
    fz, W = C.create_string_buffer(32), C.create_string_buffer(96)
    rc = _lib(sonic).sonic_open_poly(g._h, (z % R).to_bytes(32, "little"), len(exps), exps.ctypes.data, co.ctypes.data, fz, W)
    return rc, int.from_bytes(fz.raw, "little"), W.raw


def gpu_commit(sonic, g, maxm, exps, co):
    out = C.create_string_buffer(96)
    rc = _lib(sonic).sonic_commit_poly(g._h, maxm, len(exps), exps.ctypes.data, co.ctypes.data, out)
    return rc, out.raw


def unity_root(orc, k):
    """a primitive 2^k-th root of unity, read off the oracle's own transform (omega = 7^((r-1)/2^k), oracle/sonic_oracle.c `ntt`): the
    transform of X is (omega^i)_i"""
    a = np.zeros((1 << k, 32), np.uint8)
    a[1, 0] = 1
    w = int.from_bytes(orc.ntt(a)[1].tobytes(), "little")
    assert pow(w, 1 << (k - 1), R) == R - 1
    return w


def coefficients(kind, length, seed, z):
    """`length` coefficients as Python integers"""
    pyr = random.Random(seed)
    if kind == "rand":
        c = fr_ints(rand_fr_array(np.random.default_rng(seed), length))
        c[0] = c[0] or 1
        c[-1] = c[-1] or 1
        return c
    if kind == "ones":
        return [1] * length
    if kind == "minus1":
        return [R - 1] * length
    if kind == "last":                                   # one non-zero coefficient, at the far end
        return [0] * (length - 1) + [pyr.randrange(1, R)]
    if kind == "first":                                  # ... and at the near end: every later tile lives on the carried sum alone
        return [pyr.randrange(1, R)] + [0] * (length - 1)
    if kind == "pairs":                                  # v, -v pairs: with z = 1 every full 1024-tile sums to zero; an odd last element stays
        assert z == 1
        c = []
        for _ in range(length // 2):
            v = pyr.randrange(1, R)
            c += [v, R - v]
        return c + [pyr.randrange(1, R)] * (length % 2)
    if kind == "root":                                   # f = (X - z) g: f(z) = 0, the quotient is g
        g = fr_ints(rand_fr_array(np.random.default_rng(seed), length - 1))
        g[0], g[-1] = g[0] or 1, g[-1] or 1
        return [(a - z * b) % R for a, b in zip([0] + g, g + [0])]
    raise ValueError(kind)


def check_open(sonic, orc, pair, lo, length, kind, z, seed, pyq, want=None):
    """one opening of `length` dense coefficients over [lo, lo + length) at z, against Horner, the oracle, and (pyq) the Python quotient"""
    assert lo <= 0 <= lo + length - 1 and -pair.d <= lo and lo + length - 1 <= pair.d + 1
    shape = chain_shape(length)
    if want:
        assert {k: shape[k] for k in want} == want, shape
    c = coefficients(kind, length, seed, z)
    exps = np.arange(lo, lo + length, dtype=np.int64)
    co = open_ref.fr_rows(c)                             # explicit zeros stay: they set the length of the dense array
    rc, fz, W = gpu_open(sonic, pair.g, z, exps, co)
    assert rc == 0, rc
    ofz, oW = orc.open_poly(pair.o, z, exps, co)
    if pyq:
        pfz, (qlo, q) = open_ref.open_dense(lo, c, z)
        if kind == "root":                               # the quotient of (X - z) g is g
            g = fr_ints(rand_fr_array(np.random.default_rng(seed), length - 1))
            g[0], g[-1] = g[0] or 1, g[-1] or 1
            assert pfz == 0 and (qlo, q) == (lo, g)
        pW = orc.msm_srs(pair.o, 0, qlo, open_ref.fr_rows(q), 1, NCPU)
        assert oW == pW, "the two references disagree on W"
    else:
        pfz = open_ref.evaluate(lo, c, z)
    print(f"len={length} lo={lo} {kind} shape={shape} f(z)={'ok' if fz == pfz else 'DIFF'} W={'ok' if W == oW else 'DIFF'}")
    assert ofz == pfz, "the two references disagree on f(z)"
    assert fz == pfz, "f(z) differs from Horner's rule"
    assert W == oW, "W differs from the oracle's openPoly"


# ---- tile edges of k_prefix_tiles / k_prefix_apply -------------------------------------------------------------------------------------
@pytest.mark.parametrize("length", [1, 2, 1023, 1024, 1025, 2048, 2049])
def test_open_tile_edges(sonic, orc, pair_tile, length):
    """1 tile up to 1024 coefficients (no k_prefix_top / k_prefix_apply), 2 up to 2048, then 3; X^0 in the middle, first and last"""
    pyr = random.Random(length)
    d = pair_tile.d
    for lo in sorted({-(length // 2), 0, -(length - 1)}):
        if lo < -d or lo + length - 1 > d + 1:           # (2048 and 2049 coefficients fit d = 1024 around X^0 only)
            continue
        check_open(sonic, orc, pair_tile, lo, length, "rand", pyr.randrange(2, R), length - 7 * lo, True,
                   dict(tiles=-(-length // 1024), per_eval=2, per_quot=2))


# ---- PER steps of scale_per, ragged last blocks, the position of X^0 -------------------------------------------------------------------
MID = [
    # (length, lo or None for -d, what the case is for, expected shape)
    (32767, None, "PER stays 2 below 2^15", dict(per_eval=2, per_quot=2)),
    (32768, None, "PER stays 2 at 2^15: 64 full blocks of 512", dict(per_eval=2, per_quot=2, ragged_eval=0)),
    (32769, None, "PER 2, evaluation one element into block 65", dict(per_eval=2, per_quot=2, ragged_eval=1, ragged_quot=0)),
    (33023, None, "PER 2, last block holds 255: only the first of a thread's 2 elements", dict(per_eval=2, ragged_eval=255)),
    (33024, None, "PER 2, the same for the quotient launch", dict(per_quot=2, ragged_quot=255)),
    (49151, None, "both launches still PER 2", dict(per_eval=2, per_quot=2)),
    (49152, None, "evaluation PER 3 (64 full blocks of 768), quotient PER 2", dict(per_eval=3, per_quot=2, ragged_eval=0)),
    (49153, None, "both PER 3; evaluation one element into block 65", dict(per_eval=3, per_quot=3, ragged_eval=1, ragged_quot=0)),
    (49154, None, "quotient PER 3, one element into block 65", dict(per_quot=3, ragged_quot=1)),
    (49407, None, "PER 3, last block holds 255: the i >= n break after one of 3 elements", dict(per_eval=3, ragged_eval=255)),
    (49408, None, "PER 3, the same for the quotient launch", dict(per_quot=3, ragged_quot=255)),
    (49153, -24576, "X^0 (the sign switch of the numerator) on a 768-element block edge: index 24576 = 32 * 768", dict(per_eval=3, per_quot=3)),
    (49153, -24577, "... and one past it", dict(per_eval=3, per_quot=3)),
    (5000, 0, "lo = 0: no negative exponents, X^0 the very first coefficient of 5 tiles", dict(tiles=5)),
    (5000, -4999, "hi = 0: negative exponents only, X^0 the very last coefficient", dict(tiles=5)),
    (5000, -1023, "X^0 at index 1023: last of tile 0", dict(tiles=5)),
    (5000, -1024, "X^0 at index 1024: first of tile 1, and a 512-element block edge", dict(tiles=5, per_quot=2)),
    (5000, -1025, "X^0 at index 1025", dict(tiles=5)),
    (5000, -2559, "X^0 one before the block edge 2560 = 5 * 512", dict(per_quot=2)),
    (5000, -2560, "X^0 on it", dict(per_quot=2)),
]


@pytest.mark.parametrize("length,lo,why,want", MID, ids=[f"{c[0]}@{c[1]}" for c in MID])
def test_open_per_steps_and_x0_position(sonic, orc, pair_mid, length, lo, why, want):
    lo = -pair_mid.d if lo is None else lo
    check_open(sonic, orc, pair_mid, lo, length, "rand", random.Random(length - lo).randrange(2, R), length ^ -lo, True, want)


# ---- the carry loop of k_prefix_top: 256 tiles per iteration ---------------------------------------------------------------------------
T256 = dict(tiles=256, top_iters=1)
T257 = dict(tiles=257, top_iters=2)
BIG = [
    # (length, coefficients, z, Python quotient too, what for, expected shape)
    (262143, "rand", "rand", False, "one short of 256 full tiles; PER 15", dict(per_eval=15, **T256)),
    (262144, "rand", "rand", False, "256 tiles exactly: one full iteration, no carry; evaluation PER 16, quotient 15", dict(per_eval=16, per_quot=15, **T256)),
    (262145, "root", "rand", True, "257 tiles: a second iteration of one tile; f(z) = 0, quotient known", dict(per_quot=16, **T257)),
    (262146, "rand", "rand", True, "257 tiles, two elements in the last", T257),
    (262145, "ones", "w256", False, "z^256 = 1: the thread step is 1, D repeats every 256, prefix sums are geometric sums that return to 0", T257),
    (262145, "minus1", "w1024", False, "z^256 of order 4; every tile sums to zero, so does every carry", T257),
    (262145, "last", "minus1", False, "one non-zero coefficient at the far end: tile 256 alone is non-zero, z = r - 1", T257),
    (262145, "first", "one", True, "one non-zero coefficient at the near end: tile 256 gets its value from the carry alone, z = 1", T257),
    (262145, "pairs", "one", False, "v, -v pairs at z = 1: all 256 full tile sums are zero, the carry is zero", T257),
]


@pytest.mark.parametrize("length,kind,zkind,pyq,why,want", BIG, ids=[f"{c[0]}-{c[1]}-{c[2]}" for c in BIG])
def test_open_carry_loop_257_tiles(sonic, orc, pair_17, length, kind, zkind, pyq, why, want):
    z = {"rand": random.Random(length).randrange(2, R), "one": 1, "minus1": R - 1}.get(zkind) or unity_root(orc, {"w256": 8, "w1024": 10}[zkind])
    lo = -pair_17.d + (1 if length == 262143 else 0)
    check_open(sonic, orc, pair_17, lo, length, kind, z, length + len(kind), pyq, want)


def test_open_three_carry_iterations_per_32(sonic, orc, pair_18):
    """d = 2^18, [-d, d + 1]: 524290 coefficients = 513 tiles, three iterations of the carry loop (the last with one tile), PER = 32 in
    both launches"""
    d = pair_18.d
    check_open(sonic, orc, pair_18, -d, 2 * d + 2, "rand", random.Random(18).randrange(2, R), 18, False,
               dict(tiles=513, top_iters=3, per_eval=32, per_quot=32))


# ---- z = 0: open_job_at_zero at size ---------------------------------------------------------------------------------------------------
def test_open_at_zero_at_size(sonic, orc, pair_17):
    """lo = 0, d + 2 coefficients: the quotient's last term is X^d, the last legal one.  One more non-zero coefficient needs X^(d+1)
    (SONIC_ERR_SRS_INDEX); an explicit zero there is no term at all"""
    d = pair_17.d
    co = rand_fr_array(np.random.default_rng(170), d + 3)
    co[d + 1, 0] |= 1                                    # top of the legal array, and the one past it: non-zero
    co[d + 2, 0] |= 1
    exps = np.arange(0, d + 3, dtype=np.int64)
    c = fr_ints(co[:d + 2])
    rc, fz, W = gpu_open(sonic, pair_17.g, 0, exps[:d + 2], co[:d + 2])
    assert rc == 0
    pfz, (qlo, q) = open_ref.open_dense(0, c, 0)
    assert (qlo, q) == (0, c[1:]) and fz == pfz == c[0]
    want = orc.msm_srs(pair_17.o, 0, 0, co[1:d + 2], 1, NCPU)
    assert orc.open_poly(pair_17.o, 0, exps[:d + 2], co[:d + 2]) == (pfz, want)
    assert W == want
    rc, _, _ = gpu_open(sonic, pair_17.g, 0, exps, co)
    assert rc == ERR_SRS_INDEX
    co[d + 2] = 0
    rc, fz, W = gpu_open(sonic, pair_17.g, 0, exps, co)
    assert (rc, fz, W) == (0, pfz, want)


# ---- commit_job's clipping on long arrays ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("back", [0, 5])
def test_commit_clipping_at_size(sonic, orc, pair_17, back):
    """max = d - back: the legal exponents are [-d - back, d - back] without -back (e' = 0, the omitted g^alpha).  A dense array that
    reaches 3 past both ends and covers the hole: explicit zeros at all three places are accepted and the result is the oracle's; a
    non-zero coefficient at any one of them is SONIC_ERR_SRS_INDEX"""
    d = pair_17.d
    maxm = d - back
    lo, hi = -d - back - 3, d - back + 3
    exps = np.arange(lo, hi + 1, dtype=np.int64)
    co = rand_fr_array(np.random.default_rng(back), len(exps))
    co[3, 0] |= 1                                        # the first and the last legal coefficient: non-zero
    co[-4, 0] |= 1
    outside = [0, 1, 2, len(exps) - 3, len(exps) - 2, len(exps) - 1]
    hole = -back - lo
    co[outside] = 0
    co[hole] = 0
    rc, got = gpu_commit(sonic, pair_17.g, maxm, exps, co)
    assert rc == 0
    assert got == orc.commit_poly(pair_17.o, maxm, exps, co)
    assert got == orc.msm_srs(pair_17.o, 1, -d, co[3:-3], 1, NCPU)       # (the hole's point is the zero slot of the oracle's alpha basis)
    for at in (2, len(exps) - 3, hole):                  # the nearest illegal exponent on either side, and the hole
        bad = co.copy()
        bad[at, 0] = 1
        rc, _ = gpu_commit(sonic, pair_17.g, maxm, exps, bad)
        assert rc == ERR_SRS_INDEX, at
        with pytest.raises(orc.OracleError) as e:
            orc.commit_poly(pair_17.o, maxm, exps, bad)
        assert e.value.code == 2


# ---- hscProve outside a proof ----------------------------------------------------------------------------------------------------------
def _circuit(sonic, n, Q, seed):
    """weights as {gate: value} rows (3 random gates per row, one full row per matrix), a satisfying assignment, both handle forms"""
    pyr = random.Random(seed)
    rows = []
    for _ in range(3):
        w = [{i: pyr.randrange(1, R) for i in pyr.sample(range(n), min(3, n))} for _ in range(Q)]
        w[pyr.randrange(Q)] = {i: pyr.randrange(1, R) for i in range(n)}
        rows.append(w)
    aL = [pyr.randrange(R) for _ in range(n)]
    aR = [pyr.randrange(R) for _ in range(n)]
    aO = [a * b % R for a, b in zip(aL, aR)]
    cs = [sum(sum(v * a[i] for i, v in w[q].items()) for w, a in zip(rows, (aL, aR, aO))) % R for q in range(Q)]
    wL, wR, wO = open_ref.dense_weights(n, rows)
    dense = sonic.ArithCircuit(sonic.GateWeights(wL, wR, wO), cs)
    sparse = sonic.SparseCircuit.from_rows(n, rows[0], rows[1], rows[2], cs)
    return rows, (aL, aR, aO), cs, dense, sparse


_ENV = {}


def _hsc_env(sonic, orc, n, Q):
    """SRS pair and circuit of a shape, shared by the cases of that shape"""
    if (n, Q) not in _ENV:
        _ENV[(n, Q)] = (Pair(sonic, orc, 7 * n + 3, 1000 * n + Q), _circuit(sonic, n, Q, n + Q))
    return _ENV[(n, Q)]


def _expected_hsc(orc, pair, sxy, su, yzs, u, v):
    return open_ref.hsc_expected(lambda mx, lo, c: orc.commit_poly(pair.o, mx, *open_ref.sparse(lo, c)),
                                 lambda z, lo, c: orc.open_poly(pair.o, z, *open_ref.sparse(lo, c)), pair.d, sxy, su, yzs, u, v)


def _assert_hsc(got: bytes, want: bytes, m, tag):
    assert len(got) == len(want)
    diff = [nm for (nm, a), (_, b) in zip(open_ref.hsc_parts(got, m), open_ref.hsc_parts(want, m)) if a != b]
    assert not diff, (tag, diff)


HSC = [(300, 3, m) for m in (0, 1, 14, 15, 16, 17, 33)] + [(1000, 1, 0), (1000, 1, 1), (4097, 2, 1), (700, 65, 1)]


@pytest.mark.parametrize("n,Q,m", HSC)
def test_handle_hsc_prove_matches_reference(sonic, orc, n, Q, m):
    """sonic_prover_hsc_prove on a dense and on a CSR handle, each against the reference assembly.  The s(u, Y) group holds m + 2 jobs:
    m = 14 fills the 16 slots without a flush, at m = 15 the flush before Q_v fires alone, at m = 16 the one inside the loop, m = 17 and
    33 wrap the scratch slots once and twice"""
    from sonic_amd.protocol import _hsc_to_bytes
    pair, (rows, _asg, _cs, dense, sparse) = _hsc_env(sonic, orc, n, Q)
    pyr = random.Random(n * 100 + m)
    yzs = [(pyr.randrange(2, R), pyr.randrange(2, R)) for _ in range(m)]
    u, v = pyr.randrange(2, R), pyr.randrange(2, R)
    want = _expected_hsc(orc, pair, [open_ref.s_of_y(n, rows, y) for y, _ in yzs], open_ref.s_of_u(n, rows, u), yzs, u, v)
    for tag, circuit in (("dense", dense), ("csr", sparse)):
        p = sonic.Prover(pair.g, circuit, prepare=False)
        got = p.hsc_prove(yzs, u, v)
        p.close()
        _assert_hsc(_hsc_to_bytes(got), want, m, tag)
        if tag == "dense":
            assert sonic.hsc_verify(pair.g, dense, yzs, got)


@pytest.mark.parametrize("form", ["dense", "csr"])
def test_handle_proves_after_hsc_prove(sonic, orc, form):
    """hsc_prove at m = 33 grows and reuses the scratch of the handle's first lane; the same handle then proves, and the proof is the
    oracle's"""
    from sonic_amd.protocol import _hsc_to_bytes
    n, Q, m = 300, 3, 33
    pair, (rows, asg, cs, dense, sparse) = _hsc_env(sonic, orc, n, Q)
    pyr = random.Random(33)
    yzs = [(pyr.randrange(2, R), pyr.randrange(2, R)) for _ in range(m)]
    u, v = pyr.randrange(2, R), pyr.randrange(2, R)
    tr = [pyr.randrange(2, R) for _ in range(8 + 2 * Q)]
    wL, wR, wO = open_ref.dense_weights(n, rows)
    flat = lambda w: fr_bytes([x for row in w for x in row])      # noqa: E731
    want = orc.prove(pair.o, n, Q, flat(wL), flat(wR), flat(wO), fr_bytes(cs), fr_bytes(asg[0]), fr_bytes(asg[1]), fr_bytes(asg[2]), fr_bytes(tr))
    p = sonic.Prover(pair.g, dense if form == "dense" else sparse)
    p.set_assignment(sonic.Assignment(*asg))
    first = _hsc_to_bytes(p.hsc_prove(yzs, u, v))
    assert p.prove_bytes(tr) == want
    assert _hsc_to_bytes(p.hsc_prove(yzs, u, v)) == first            # and the proof left the next hscProve unharmed
    assert p.prove_bytes(tr) == want
    p.close()
    _assert_hsc(first, _expected_hsc(orc, pair, [open_ref.s_of_y(n, rows, y) for y, _ in yzs], open_ref.s_of_u(n, rows, u), yzs, u, v), m, form)


D_POLY = 3000


@pytest.fixture(scope="module")
def pair_poly(sonic, orc):
    p = Pair(sonic, orc, D_POLY, 105)
    yield p
    p.g.close()


def _gpu_hsc_poly(sonic, g, terms, yzs, u, v):
    xe = np.array([t[0] for t in terms], np.int64)
    ye = np.array([t[1] for t in terms], np.int64)
    cf = fr_bytes([t[2] for t in terms])
    flat = fr_bytes([a for pair in yzs for a in pair]) if yzs else np.zeros((0, 32), np.uint8)
    L = _lib(sonic)
    out = C.create_string_buffer(L.sonic_hsc_proof_size(len(yzs)))
    rc = L.sonic_hsc_prove_poly(g._h, len(terms), xe.ctypes.data, ye.ctypes.data, cf.ctypes.data, len(yzs),
                                flat.ctypes.data if yzs else None, (u % R).to_bytes(32, "little"), (v % R).to_bytes(32, "little"), out)
    return rc, out.raw


def _biv_terms(seed, lo, hi, count):
    """`count` distinct terms with both exponents in [lo, hi] without 0 (X^0 / Y^0 would need the omitted g^alpha), the corners present"""
    pyr = random.Random(seed)
    pick = lambda: pyr.randrange(lo, hi + 1) or hi      # noqa: E731
    keys = {(lo or 1, hi), (hi, lo or 1)}
    while len(keys) < count:
        keys.add((pick(), pick()))
    return [(ex, ey, pyr.randrange(1, R)) for ex, ey in sorted(keys)]


@pytest.mark.parametrize("m", [0, 15, 16, 17])
def test_hsc_prove_poly_matches_reference(sonic, orc, pair_poly, m):
    """sonic_hsc_prove_poly: 3000 terms over [-2800, 2800]^2 -- s(X, y_j) and s(u, Y) are 5601 coefficients each, 6 scan tiles -- with
    the flush before Q_v alone (m = 15), the one in the loop (16), and a wrapped scratch slot (17)"""
    terms = _biv_terms(7, -2800, 2800, 3000)
    assert chain_shape(5601)["tiles"] == 6
    pyr = random.Random(m)
    yzs = [(pyr.randrange(2, R), pyr.randrange(2, R)) for _ in range(m)]
    u, v = pyr.randrange(2, R), pyr.randrange(2, R)
    rc, got = _gpu_hsc_poly(sonic, pair_poly.g, terms, yzs, u, v)
    assert rc == 0
    want = _expected_hsc(orc, pair_poly, [open_ref.biv_keep(terms, True, y) for y, _ in yzs], open_ref.biv_keep(terms, False, u), yzs, u, v)
    _assert_hsc(got, want, m, "poly")


def test_hsc_prove_poly_positive_exponents_and_zero_point(sonic, orc, pair_poly):
    """positive exponents only, z_1 = 0: open_any takes open_job_at_zero for W_1 (2900 coefficients, 3 tiles) between ordinary openings"""
    from sonic_amd.protocol import _hsc_from_bytes
    terms = _biv_terms(8, 1, 2900, 2500)
    pyr = random.Random(80)
    yzs = [(pyr.randrange(2, R), pyr.randrange(2, R)), (pyr.randrange(2, R), 0), (pyr.randrange(2, R), pyr.randrange(2, R))]
    u, v = pyr.randrange(2, R), pyr.randrange(2, R)
    rc, got = _gpu_hsc_poly(sonic, pair_poly.g, terms, yzs, u, v)
    assert rc == 0
    want = _expected_hsc(orc, pair_poly, [open_ref.biv_keep(terms, True, y) for y, _ in yzs], open_ref.biv_keep(terms, False, u), yzs, u, v)
    _assert_hsc(got, want, 3, "poly at 0")
    assert sonic.hsc_verify_poly(pair_poly.g, terms, yzs, _hsc_from_bytes(got, 3))
