"""tests/open_ref.py (the Python-integer reference that tests/test_gpu_open_sizes.py uses at size) held against the two CPU oracles where
the pure-Python one is affordable: openPoly at lengths 1, 2 and across a 1024 tile edge with X^0 first, last and in the middle; s(X, y),
s(u, Y) and the HscProof assembly for m in {0, 1, 3}.  No GPU."""
import random

import numpy as np
import pytest

import open_ref
from open_ref import R
from util import NCPU

D = 1100


@pytest.fixture(scope="module")
def srs_pair(orc, ref):
    pyr = random.Random(0x0BE)
    x, alpha = pyr.randrange(2, R), pyr.randrange(2, R)
    orc.set_mode(1, NCPU)
    return orc.SRS(D, x, alpha, threads=NCPU), ref.SRS(D, x, alpha)


def _case(pyr, length, where):
    """(lo, c): `length` coefficients with X^0 first / last / in the middle; a few zeros among them"""
    lo = {"first": 0, "last": -(length - 1), "middle": -(length // 2)}[where]
    c = [pyr.randrange(1, R) for _ in range(length)]
    for i in range(3, length, 97):
        c[i] = 0
    return lo, c


@pytest.mark.parametrize("where", ["first", "last", "middle"])
@pytest.mark.parametrize("length", [1, 2, 1023, 1024, 1025])
def test_open_dense_matches_both_oracles(orc, ref, srs_pair, length, where):
    o, s = srs_pair
    pyr = random.Random(length * 7 + len(where))
    lo, c = _case(pyr, length, where)
    f = open_ref.as_dict(lo, c)
    exps, co = open_ref.sparse(lo, c)
    for z in (pyr.randrange(2, R), 1, R - 1) + ((0,) if lo == 0 else ()):
        fz, (qlo, q) = open_ref.open_dense(lo, c, z)
        assert fz == ref.lp_eval(f, z) == open_ref.evaluate(lo, c, z)
        assert open_ref.as_dict(qlo, q) == ref.lp_divide_linear(ref.lp_add(f, {0: (-fz) % R}), z)
        ofz, oW = orc.open_poly(o, z, exps, co)
        assert ofz == fz
        assert oW == orc.msm_srs(o, 0, qlo, open_ref.fr_rows(q), 1, NCPU)
    if length <= 2:                                      # the literal fold over the SRS, group law included
        z = pyr.randrange(2, R)
        fz, W = ref.open_poly(s, z, f)
        assert (fz, ref.g1_to_bytes(W)) == orc.open_poly(o, z, exps, co)


def test_open_dense_root_and_zero_polynomial(ref):
    """f = (X - z) g: f(z) = 0 and the quotient is g; the zero polynomial; an exponent range without X^0"""
    pyr = random.Random(5)
    z = pyr.randrange(2, R)
    g = [pyr.randrange(R) for _ in range(40)]
    f = [(a - z * b) % R for a, b in zip([0] + g, g + [0])]
    fz, (qlo, q) = open_ref.open_dense(-17, f, z)
    assert fz == 0 and (qlo, q) == (-17, g)
    assert open_ref.open_dense(-3, [0] * 9, z) == (0, (-3, [0] * 8))
    assert open_ref.open_dense(0, [], z) == (0, (0, []))
    for lo in (3, -9):                                   # [3, 7] and [-9, -5]: the range grows to X^0
        c = [pyr.randrange(1, R) for _ in range(5)]
        fz, (qlo, q) = open_ref.open_dense(lo, c, z)
        f = open_ref.as_dict(lo, c)
        assert fz == ref.lp_eval(f, z)
        assert open_ref.as_dict(qlo, q) == ref.lp_divide_linear(ref.lp_add(f, {0: (-fz) % R}), z)
    with pytest.raises(ZeroDivisionError):
        open_ref.open_dense(-1, [1, 2], 0)


def _rows(pyr, n, Q, per_row):
    """weights as {gate: value} rows: `per_row` random gates each, and one full row per matrix (rndCircuit's shape)"""
    out = []
    for _ in range(3):
        w = [{i: pyr.randrange(1, R) for i in pyr.sample(range(n), min(per_row, n))} for _ in range(Q)]
        w[pyr.randrange(Q)] = {i: pyr.randrange(1, R) for i in range(n)}
        out.append(w)
    return tuple(out)


@pytest.mark.parametrize("n,Q", [(1, 1), (5, 3), (9, 7)])
def test_s_polynomials_match_spoly(ref, n, Q):
    pyr = random.Random(n * 10 + Q)
    rows = _rows(pyr, n, Q, 2)
    sXY = ref.s_poly(*open_ref.dense_weights(n, rows))
    for _ in range(2):
        a = pyr.randrange(2, R)
        assert open_ref.as_dict(*open_ref.s_of_y(n, rows, a)) == ref.eval_y(a, sXY)
        assert open_ref.as_dict(*open_ref.s_of_u(n, rows, a)) == ref.eval_x(a, sXY)
    terms = [(ex, ey, v) for ex, py in sXY.items() for ey, v in py.items()]
    a = pyr.randrange(2, R)
    assert open_ref.as_dict(*open_ref.biv_keep(terms, True, a)) == ref.eval_y(a, sXY)
    assert open_ref.as_dict(*open_ref.biv_keep(terms, False, a)) == ref.eval_x(a, sXY)


@pytest.mark.parametrize("m", [0, 1, 3])
def test_hsc_assembly_matches_hsc_prove(orc, ref, m):
    """the expected HscProof bytes, built from the C oracle's commitPoly / openPoly over open_ref's s(X, y_j) and s(u, Y), equal the literal
    hscProve of oracle/sonic_ref.py"""
    pyr = random.Random(60 + m)
    n, Q = 3, 2
    d = 7 * n + 3
    x, alpha = pyr.randrange(2, R), pyr.randrange(2, R)
    o, s = orc.SRS(d, x, alpha, threads=NCPU), ref.SRS(d, x, alpha)
    rows = _rows(pyr, n, Q, 2)
    yzs = [(pyr.randrange(2, R), pyr.randrange(2, R)) for _ in range(m)]
    u, v = pyr.randrange(2, R), pyr.randrange(2, R)
    got = open_ref.hsc_expected(lambda mx, lo, c: orc.commit_poly(o, mx, *open_ref.sparse(lo, c)),
                                lambda z, lo, c: orc.open_poly(o, z, *open_ref.sparse(lo, c)),
                                d, [open_ref.s_of_y(n, rows, y) for y, _ in yzs], open_ref.s_of_u(n, rows, u), yzs, u, v)
    w = ref.hsc_prove(s, ref.s_poly(*open_ref.dense_weights(n, rows)), yzs, u, v)
    g, f = ref.g1_to_bytes, ref.fr_to_bytes
    want = b"".join([g(cm) + f(sj) + g(wj) for cm, (sj, wj) in w["hscS"]] + [f(sp) + g(wp) + g(qj) for sp, wp, qj in w["hscW"]] +
                    [g(w["hscQv"]), g(w["hscC"]), f(u), f(v)])
    assert [nm for nm, _ in open_ref.hsc_parts(got, m)] == [nm for nm, _ in open_ref.hsc_parts(want, m)]
    assert open_ref.hsc_parts(got, m) == open_ref.hsc_parts(want, m)


def test_chain_shape_of_the_lengths_the_gpu_file_uses():
    """the launch shapes the GPU cases are chosen for, from scale_per and the tile size"""
    cs = open_ref.chain_shape
    assert [open_ref.scale_per(n) for n in (1, 32768, 49151, 49152, 65535, 65536, 262144, 524287, 524288, 1 << 22)] == [2, 2, 2, 3, 3, 4, 16, 31, 32, 32]
    assert cs(1)["tiles"] == 1 and cs(1)["top_iters"] == 0 and cs(1024)["tiles"] == 1 and cs(1025)["tiles"] == 2
    assert (cs(49152)["per_eval"], cs(49152)["per_quot"]) == (3, 2) and (cs(49153)["per_eval"], cs(49153)["per_quot"]) == (3, 3)
    assert cs(49153)["ragged_eval"] == 1 and cs(49154)["ragged_quot"] == 1 and cs(49407)["ragged_eval"] == 255
    assert cs(33023)["ragged_eval"] == 255 and cs(32769)["ragged_eval"] == 1
    assert (cs(262144)["tiles"], cs(262144)["top_iters"]) == (256, 1) and (cs(262145)["tiles"], cs(262145)["top_iters"]) == (257, 2)
    assert (cs(524290)["tiles"], cs(524290)["top_iters"], cs(524290)["per_eval"], cs(524290)["per_quot"]) == (513, 3, 32, 32)
    assert (cs(393218)["tiles"], cs(393218)["top_iters"]) == (385, 2)
