"""Every kernel path of the G1 MSM (sonic_amd/csrc/msm.hip) over degenerate bases and digit-edge scalars, at the sizes where the
production kernels run.  Which path a launch takes depends on the plan and its size (util.msm_path); every case first asserts the path
it claims, then compares against a reference that shares no algorithm with the kernels:

  * over an SRS with trapdoor (x, alpha) the MSM is g * sum_i s_i a_b x^(e0 + i) (util.srs_exponent) -- one fixed-base multiplication;
    over caller points that are all k_j g it is g * sum_j s_j k_j;
  * otherwise the CPU oracle's Pippenger (orc.msm / orc.msm_srs) and, on a few hundred terms, its per-term fold (mode 0).

Degenerate trapdoors: x = 1 (the reference's benchmark SRS, bench/Main.hs:18-27: every basis element is g), x = r - 1 (g and -g in
turn: runs cancel), and primitive 4th / 256th roots of unity (the bases cycle through 4 or 256 points, negations among them).  There
every bucket walk, heavy stretch, tree level and running sum meets P + P, P + (-P) and the point at infinity."""
import ctypes as C
import os
import random
from collections import Counter

import numpy as np
import pytest

from util import (ENDO_BITS, HALF_R, NCPU, R, big_circuit, digit_families, digit_stream, fr_bytes, fr_ints, heavy_threshold,
                  msm_path, msm_plan_points, rand_fr_array, root_of_unity, srs_exponent, table_widths, valued_scalars)

pytestmark = pytest.mark.gpu
T = min(NCPU, 16)
TRAPDOORS = {"x1": 1, "xneg1": R - 1, "root4": root_of_unity(2), "root256": root_of_unity(8)}
ALPHA = 0x5EED5EED5EED5EED


def _plan(srs, n):
    from sonic_amd import _lib
    c, w, sets = C.c_int(), C.c_int(), C.c_int()
    _lib.check(_lib.lib().sonic_msm_plan(srs._h, n, C.byref(c), C.byref(w), C.byref(sets)))
    return c.value, w.value, sets.value


def _gen(orc, k):
    return orc.g1_mul(orc.g1_gen(), k % R)


def _bucket_sizes(vals, idx, widths, fold, shared):
    """entries per bucket of an MSM whose scalar j is vals[idx[j]] (the digit mirror of tests/test_msm_digits.py)"""
    mult = np.bincount(idx, minlength=len(vals))
    cnt = Counter()
    for v, m in zip(vals, mult):
        if m:
            for w, (dg, _) in enumerate(digit_stream(v, widths, fold)[0]):
                if dg:
                    cnt[(0 if shared else w, dg - 1)] += int(m)
    return cnt


def _heavy_partials(sizes, thr):
    """stretches k_heavy_accum cuts the largest heavy bucket into (msm.hip, HEAVY_GRID = 256 workgroups, stretches >= 2048 entries):
    the partial sums k_heavy_finish adds for it"""
    heavy = [s for s in sizes.values() if s > thr]
    total = sum(heavy)
    stretch = max(-(-total // 256), 2048)
    return max(-(-s // stretch) for s in heavy) if heavy else 0


def _table_case(srs, n, jobs=1):
    c, W, sets = _plan(srs, n)
    NB = 1 << (c - 1)
    assert sets == 1
    return c, W, NB, msm_path(jobs * sets, NB, shared=True)


def _check_srs(sonic, orc, srs, x, basis, e0, sc, osrs=None, ints=None):
    from sonic_amd.commitment import msm_g1_srs
    got = msm_g1_srs(srs, basis, e0, sc)
    want = _gen(orc, srs_exponent(x, ALPHA, basis, e0, fr_ints(sc) if ints is None else ints))
    assert got == want, (basis, e0, sc.shape[0])
    if osrs is not None:
        assert orc.msm_srs(osrs, basis, e0, sc, 1, T) == want


# ---- a. degenerate SRS, stand-alone MSMs over the window tables ------------------------------------------------------------------------
@pytest.mark.parametrize("x", list(TRAPDOORS))
@pytest.mark.parametrize("log2d,claim", [(13, (4, "tree_latency")), (20, (1, "tree_level"))],
                         ids=["d2p13-lanes4-tree_latency", "d2p20-lanes1-tree_level"])
def test_degenerate_srs_tables(sonic, orc, x, log2d, claim):
    xv, d = TRAPDOORS[x], 1 << log2d
    N = 2 * d + 1 if log2d <= 13 else 1 << 20
    srs = sonic.SRS.new(d, xv, ALPHA)
    osrs = orc.SRS(d, xv, ALPHA, threads=T) if log2d <= 13 else None
    try:
        c, W, NB, path = _table_case(srs, N)
        assert (c, W) == {13: (13, 20), 20: (20, 13)}[log2d]
        assert (path["lanes"], path["reduction"]) == claim
        widths = table_widths(W)
        rng, pyr = np.random.default_rng(log2d), random.Random(x)
        e0 = -d if N == 2 * d + 1 else -(N // 2)                     # crosses e = 0 (the empty slot of basis 1)
        uni = rand_fr_array(rng, N)
        few, vals, idx = valued_scalars(rng, pyr, N)
        sizes = _bucket_sizes(vals, idx, widths, True, True)
        assert max(sizes.values()) > heavy_threshold(N, W, 1, NB)         # k_heavy_accum + k_heavy_finish
        for sc in (uni, few):
            for basis in (0, 1):
                _check_srs(sonic, orc, srs, xv, basis, e0, sc, osrs)
        _check_srs(sonic, orc, srs, xv, 1, -7, few[:5000], osrs)
    finally:
        srs.close()


# ---- b. degenerate SRS, endomorphism tables -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("x", ["x1", "xneg1"])
def test_degenerate_srs_endo_tables(sonic, orc, monkeypatch, x):
    monkeypatch.setenv("SONIC_MSM_ENDO", "1")
    xv, d, N = TRAPDOORS[x], 1 << 20, 1 << 20
    srs = sonic.SRS.new(d, xv, ALPHA)
    try:
        c, W, NB, path = _table_case(srs, N, jobs=2)               # two device jobs: the halves s1, s2
        assert (c, W) == (19, 7)
        assert (path["M"], path["lanes"], path["reduction"]) == (1 << 19, 1, "tree_level")
        rng, pyr = np.random.default_rng(5), random.Random(5)
        for sc in (rand_fr_array(rng, N), valued_scalars(rng, pyr, N)[0]):
            for basis in (0, 1):
                _check_srs(sonic, orc, srs, xv, basis, -(N // 2), sc)
    finally:
        srs.close()


# ---- c. caller points: the unfolded per-window path of sonic_msm_g1 -----------------------------------------------------------------
POINT_SIZES = [((1 << 9) + 3, "seg_mul_small", 4), (1 << 13, "seg_mul_small", 4), (1 << 14, "seg_wave", 4),
               ((1 << 17) + 5, "seg_wave", 2), (1 << 18, "seg_wave", 1)]


@pytest.fixture(scope="module")
def random_points(sonic):
    pyr = random.Random(17)
    d = 1 << 17
    srs = sonic.SRS.new(d, pyr.randrange(2, R), pyr.randrange(2, R))
    pts = srs.points(0, -d, 2 * d + 1)
    # sonic_msm_g1 plans like an SRS without tables (msm_plan): the c the mirror predicts
    os.environ["SONIC_MSM_TABLES"] = "0"
    try:
        plain = sonic.SRS.new(16, 3, 5)
    finally:
        del os.environ["SONIC_MSM_TABLES"]
    for n, _, _ in POINT_SIZES:
        c, W = msm_plan_points(n)
        assert _plan(plain, n) == (c, (255 + c - 1) // c, (255 + c - 1) // c)
    plain.close()
    srs.close()
    return pts


@pytest.mark.parametrize("pointset", ["random", "equal", "plus_minus_inf"])
@pytest.mark.parametrize("n,red,lanes", POINT_SIZES, ids=[f"n{n}-{r}-lanes{l}" for n, r, l in POINT_SIZES])
def test_caller_points(sonic, orc, random_points, pointset, n, red, lanes):
    c, W = msm_plan_points(n)
    NB = 1 << (c - 1)
    path = msm_path(W, NB, shared=False)
    assert (path["reduction"], path["lanes"]) == (red, lanes)
    rng, pyr = np.random.default_rng(n), random.Random(n)
    k0 = pyr.randrange(2, R)
    if pointset == "random":
        pts, ks = random_points[:n], None
    else:
        P, mP = np.frombuffer(_gen(orc, k0), np.uint8), np.frombuffer(_gen(orc, R - k0), np.uint8)
        if pointset == "equal":
            ks = [k0] * n
        else:
            ks = [k0 if j % 2 == 0 else R - k0 for j in range(n)]
            for j in rng.choice(n, size=max(n // 50, 3), replace=False):
                ks[j] = 0
        table = np.stack([np.zeros(96, np.uint8), P, mP])
        pts = table[[0 if k == 0 else (1 if k == k0 else 2) for k in ks]]
    few, vals, idx = valued_scalars(rng, pyr, n)
    if n >= 1 << 13:                                  # heavy buckets inside the per-window sets
        assert max(_bucket_sizes(vals, idx, [c] * W, False, False).values()) > heavy_threshold(n, W, W, NB)
    for sc in (rand_fr_array(rng, n), few):
        got = sonic.msm_g1(pts, sc)
        if ks is None:
            assert got == orc.msm(pts, sc, 1, T)
        else:
            assert got == _gen(orc, sum(s * k for s, k in zip(fr_ints(sc), ks)))


# ---- d. digit-boundary scalars --------------------------------------------------------------------------------------------------------
def _family_scalars(widths, limit, fold):
    """the families of util.digit_families, each below (r-1)/2 and mirrored above it (r - s: the fold negates it)"""
    fam = digit_families(widths, limit)
    out = []
    for name, (s, _) in fam.items():
        out += [s, R - s] if fold or limit == R - 1 else [s]
    out += [HALF_R, HALF_R + 1, HALF_R - 1, HALF_R + 2]
    return out, fam["repeat"][0]


def _mixed(rng, n, edge):
    sc = rand_fr_array(rng, n)
    sc[::3][: n // 3] = fr_bytes(edge * (n // (3 * len(edge)) + 1))[: len(sc[::3][: n // 3])]
    return sc


@pytest.mark.parametrize("log2d,N", [(13, (1 << 14) + 1), (16, 1 << 17), (20, 1 << 20)], ids=["c13", "c16", "c20"])
def test_digit_edges_tables(sonic, orc, log2d, N):
    pyr = random.Random(log2d)
    d, x = 1 << log2d, pyr.randrange(2, R)
    srs = sonic.SRS.new(d, x, ALPHA)
    osrs = orc.SRS(d, x, ALPHA, threads=T) if log2d <= 13 else None
    try:
        c, W, NB, path = _table_case(srs, N)
        assert c == {13: 13, 16: 16, 20: 20}[log2d]
        widths = table_widths(W)
        edge, rep = _family_scalars(widths, HALF_R, True)
        rng = np.random.default_rng(log2d)
        sc = _mixed(rng, N, edge)
        e0 = -(N // 2)
        for basis in (0, 1):
            _check_srs(sonic, orc, srs, x, basis, e0, sc, osrs)
        # one digit value in every window: n W entries in ONE bucket, cut into far more than 16 partials for k_heavy_finish
        allrep = fr_bytes([rep])[np.zeros(N, np.int64)]
        sizes = _bucket_sizes([rep], np.zeros(N, np.int64), widths, True, True)
        assert max(sizes.values()) >= N * (W - 1) and _heavy_partials(sizes, heavy_threshold(N, W, 1, NB)) > 16
        _check_srs(sonic, orc, srs, x, 0, e0, allrep, osrs, ints=[rep] * N)
        mixed_rep = allrep.copy()
        mixed_rep[1::2] = fr_bytes([R - rep])                 # the same bucket with the opposite sign: the partials cancel in pairs
        _check_srs(sonic, orc, srs, x, 1, e0, mixed_rep, osrs)
        if osrs is not None:
            sub = fr_bytes(edge * 10)
            from sonic_amd.commitment import msm_g1_srs
            assert msm_g1_srs(srs, 1, -100, sub) == orc.msm_srs(osrs, 1, -100, sub, 0, T)          # the reference-shaped fold
    finally:
        srs.close()


def test_digit_edges_endo_halves(sonic, orc, monkeypatch):
    """scalars s = s1 + lambda s2 whose halves sit on the digit edges of the 130-bit windows"""
    from util import LAM
    monkeypatch.setenv("SONIC_MSM_ENDO", "1")
    pyr = random.Random(130)
    d, x = 1 << 13, pyr.randrange(2, R)
    srs = sonic.SRS.new(d, x, ALPHA)
    osrs = orc.SRS(d, x, ALPHA, threads=T)
    try:
        c, W, NB, path = _table_case(srs, 2 * d + 1, jobs=2)
        assert (c, W) == (13, 10) and path["reduction"] == "tree_latency"
        widths = table_widths(W, ENDO_BITS)
        edge = []
        for s1, _ in digit_families(widths, LAM - 1).values():
            for s2, _ in digit_families(widths, (R - 1 - s1) // LAM).values():
                edge.append(s1 + LAM * s2)
        sc = _mixed(np.random.default_rng(1), 2 * d + 1, edge)
        for basis in (0, 1):
            _check_srs(sonic, orc, srs, x, basis, -d, sc, osrs)
        rep = edge[-1]
        allrep = fr_bytes([rep] * (2 * d + 1))
        _check_srs(sonic, orc, srs, x, 0, -d, allrep, osrs)
        from sonic_amd.commitment import msm_g1_srs
        sub = fr_bytes(edge * 4)
        assert msm_g1_srs(srs, 0, -50, sub) == orc.msm_srs(osrs, 0, -50, sub, 0, T)
    finally:
        srs.close()


@pytest.mark.parametrize("n", [1 << 13, 1 << 18], ids=["c9-seg_mul_small", "c14-seg_wave"])
def test_digit_edges_caller_points(sonic, orc, random_points, n):
    c, W = msm_plan_points(n)
    edge, rep = _family_scalars([c] * W, R - 1, False)
    pts = random_points[:n]
    sc = _mixed(np.random.default_rng(n), n, edge)
    assert sonic.msm_g1(pts, sc) == orc.msm(pts, sc, 1, T)
    allrep = fr_bytes([rep] * n)
    assert sonic.msm_g1(pts, allrep) == orc.msm(pts, allrep, 1, T)
    sub = fr_bytes(edge * 10)
    assert sonic.msm_g1(pts[:sub.shape[0]], sub) == orc.msm(pts[:sub.shape[0]], sub, 0, T)


# ---- e. prove() over degenerate SRSs at production-shaped chains -------------------------------------------------------------------
def _degenerate_osrs(orc, d, x):
    """the oracle's SRS for x = +-1 from its four distinct points (generating 2 (2d + 1) points on the host is what would take time)"""
    g, ga = _gen(orc, 1), _gen(orc, ALPHA)
    pts = {(0, 1): g, (0, -1): _gen(orc, R - 1), (1, 1): ga, (1, -1): _gen(orc, R - ALPHA)}
    e = np.arange(-d, d + 1)
    neg = (e % 2 == 1) if x == R - 1 else np.zeros(2 * d + 1, bool)
    bases = []
    for b in (0, 1):
        arr = np.where(neg[:, None], np.frombuffer(pts[(b, -1)], np.uint8)[None, :], np.frombuffer(pts[(b, 1)], np.uint8)[None, :])
        if b == 1:
            arr[d] = 0                                               # the empty slot e = 0 of the alpha basis
        bases.append(np.ascontiguousarray(arr))
    return orc.SRS.from_points(d, bases[0], bases[1], threads=T), bases


@pytest.mark.parametrize("x", ["x1", "xneg1"])
@pytest.mark.parametrize("log2n,claim", [(14, (16, 15, "tree_level")), (17, (20, None, "seg_wave"))],
                         ids=["n2p14-fused15-lanes1-tree_level", "n2p17-segments-seg_wave"])
def test_prove_degenerate_srs(sonic, orc, x, log2n, claim):
    n, Q = 1 << log2n, 2
    d = 8 * n
    xv = TRAPDOORS[x]
    srs = sonic.SRS.new(d, xv, ALPHA)
    osrs, bases = _degenerate_osrs(orc, d, xv)
    try:
        for b in (0, 1):
            assert np.array_equal(srs.points(b, -d, 64), bases[b][:64]) and np.array_equal(srs.points(b, -3, 7), bases[b][d - 3:d + 4])
        c, W, sets = _plan(srs, n)
        NB = 1 << (c - 1)
        want_c, jobs, red = claim
        assert c == want_c and sets == 1
        if red == "tree_level":
            # the 7 + 4Q MSMs of a proof over c <= 18 tables run as ONE chain (prove.hip run_jobs, fused): 15 bucket sets of 2^15
            path = msm_path(jobs, NB, shared=True)
            assert 7 + 4 * Q == jobs and path["lanes"] == 1 and path["reduction"] == red
        else:
            # NB = 2^19 > 2^17: the groups that are not last reduce by running sums over K = 64-bucket segments (prove.hip:18-22, 58)
            assert NB > 1 << 17
            assert msm_path(1, NB, shared=False, K=64)["reduction"] == red == msm_path(1, NB, shared=False, K=8)["reduction"]
        circ = big_circuit(log2n + 100, n, Q)
        pyr = random.Random(log2n)
        tr = fr_bytes([pyr.randrange(2, R) for _ in range(8 + 2 * Q)])
        orc.set_mode(1, T)
        want = orc.prove(osrs, n, Q, circ["wL"], circ["wR"], circ["wO"], circ["cs"], circ["aL"], circ["aR"], circ["aO"], tr, True)
        p = sonic.Prover(srs, sonic.ArithCircuit(sonic.GateWeights(circ["wL"], circ["wR"], circ["wO"]), circ["cs"]))
        p.set_assignment(sonic.Assignment(circ["aL"], circ["aR"], circ["aO"]))
        assert p.prove_bytes(tr) == want
        p.close()
    finally:
        srs.close()
