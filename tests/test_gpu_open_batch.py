"""The batched opening chain of prove() (open_batch_enqueue, sonic_amd/csrc/poly.hip: two chunked Horner sweeps per side of X^0) through
sonic_open_batch_dense, which uploads, runs the chain and downloads.  Quotients coefficient for coefficient against synthetic division
(open_ref.open_dense), f(z) against z^lo times Horner's rule (open_ref.evaluate: another association), and for three cases the MSM of
the quotient over the plain basis (sonic_msm_g1_srs) against the W of sonic_open_poly, which runs the unchanged prefix-sum chain.
(commitPoly cannot serve for that MSM: it commits over the alpha basis, openPoly's W is over the plain one.)

L = coefficients per thread, T = 256 L per workgroup tile.  prove() takes L by length (2 below 49152 coefficients, 16 from 262144 on);
the entry's `chunk` forces one, so that the edges of L = 16 tiles are met at a few thousand coefficients.  A side's chunks and tiles are
counted from its far end with the padding in front (open_sweeps_ref.py), so the edges move with the position of X^0 as well as with
the length: both are varied."""
import ctypes as C
import random

import numpy as np
import pytest

import open_ref
import open_sweeps_ref as sw
from open_ref import R
from util import root_of_unity

pytestmark = pytest.mark.gpu

INEXACT_DIVISION, INVALID_ARG = 4, 7


def _lib():
    from sonic_amd import _lib as m
    return m.lib()


def gpu_open_batch(polys, lo, zs, quotient=True, chunk=0):
    """polys: lists of Python integers (the SAME list object twice = one shared array).  Returns (rc, [f(z_k)], [quotient k])"""
    k, n = len(polys), len(polys[0])
    rows = {}
    for c in polys:
        if id(c) not in rows:
            rows[id(c)] = open_ref.fr_rows(c)
    ptrs = (C.c_void_p * k)(*[rows[id(c)].ctypes.data for c in polys])
    zb = open_ref.fr_rows(zs)
    fz = np.zeros((k, 32), np.uint8)
    qs = [np.zeros((max(n - 1, 1), 32), np.uint8) for _ in range(k)]
    qp = (C.c_void_p * k)(*[q.ctypes.data for q in qs])
    rc = _lib().sonic_open_batch_dense(k, ptrs, lo, n, zb.ctypes.data, 1 if quotient else 0, chunk, fz.ctypes.data, qp)
    ints = lambda a: [int.from_bytes(a[i].tobytes(), "little") for i in range(len(a))]      # noqa: E731
    return rc, ints(fz), [ints(q[:n - 1]) for q in qs]


def coefficients(kind, n, seed):
    pyr = random.Random(seed)
    if kind == "rand":
        return [pyr.randrange(R) for _ in range(n)]
    if kind == "ones":
        return [1] * n
    if kind == "ends":
        return [pyr.randrange(1, R)] + [0] * (n - 2) + ([pyr.randrange(1, R)] if n > 1 else [])
    if kind == "minus1":
        return [R - 1] * n
    raise ValueError(kind)


_REF = {}


def reference(lo, c, z):
    """(f(z), quotient) by synthetic division, once per (polynomial, point); f(z) held against Horner's rule"""
    key = (lo, id(c), z)
    if key not in _REF:
        fz, (qlo, q) = open_ref.open_dense(lo, c, z)
        assert qlo == lo and fz == open_ref.evaluate(lo, c, z)
        _REF[key] = (fz, q, c)                           # (c kept alive: its id is the key)
    return _REF[key][:2]


def check(polys, lo, zs, quotient=True, chunk=0):
    rc, fz, qs = gpu_open_batch(polys, lo, zs, quotient, chunk)
    assert rc == 0, rc
    for k, (c, z) in enumerate(zip(polys, zs)):
        want_fz, want_q = reference(lo, c, z)
        assert fz[k] == want_fz, f"f(z) of opening {k}: len={len(c)} lo={lo} chunk={chunk}"
        if quotient:
            bad = [i for i, (a, b) in enumerate(zip(qs[k], want_q)) if a != b]
            assert not bad, f"quotient of opening {k}: len={len(c)} lo={lo} chunk={chunk}: {len(bad)} differ, first at index {bad[0]}"


@pytest.mark.parametrize("L", [2, 16])
def test_lengths(sonic, L):
    """1, 2, L - 1, L, L + 1, T - 1, T, T + 1, 2T + 1 coefficients, X^0 first, in the middle and last"""
    T = sw.BLOCK * L
    pyr = random.Random(L)
    for n in sorted({1, 2, max(1, L - 1), L, L + 1, T - 1, T, T + 1, 2 * T + 1}):
        for i0 in sorted({0, n // 2, n - 1}):
            check([coefficients("rand", n, n + i0)], -i0, [pyr.randrange(2, R)], chunk=L)


@pytest.mark.parametrize("side", ["below", "above"])
def test_two_iterations_of_the_tile_scan(sonic, side):
    """257 tiles of L = 2 on one side of X^0: k_sweep_carries_b takes its tiles in two blocks and carries from the first into the second"""
    L, T = 2, 2 * sw.BLOCK
    n = 257 * T + 3
    assert -(-(n - 6) // T) == 257
    i0 = n - 6 if side == "below" else 5
    c = coefficients("rand", n, 257)
    check([c, c], -i0, [random.Random(i0).randrange(2, R), 1], chunk=L)


@pytest.mark.parametrize("L,n", [(16, 2 * 4096 + 1), (16, 3 * 4096 + 1000), (2, 1025), (2, 2000)])
def test_position_of_x0(sonic, L, n):
    """X^0 at index 0 (no negative part), 1, mid-chunk, on a chunk edge, on a tile edge and one past it, and last (no positive part)"""
    T = sw.BLOCK * L
    pyr = random.Random(n)
    c = coefficients("rand", n, n)
    for i0 in sorted({0, 1, L + L // 2, 2 * L, T, T + 1, n - 1 - T, n - 1 - 2 * L, n - 2, n - 1}):
        check([c], -i0, [pyr.randrange(2, R)], chunk=L)


@pytest.mark.parametrize("kind", ["rand", "ones", "ends", "minus1"])
def test_points_and_coefficients(sonic, kind):
    """z = 1, r - 1, a root of unity with z^L = 1 and one with z^T = 1 (every multiplier of the scans is 1), random: five openings of one
    shared array, three tiles below X^0 and two above"""
    L = 16
    T = sw.BLOCK * L
    n, i0 = 4 * T + 9, 2 * T + 7
    c = coefficients(kind, n, 7)
    zs = [1, R - 1, root_of_unity(4), root_of_unity(12), random.Random(len(kind)).randrange(2, R)]
    assert pow(zs[2], L, R) == 1 and pow(zs[3], T, R) == 1
    check([c] * 5, -i0, zs, chunk=L)


def test_batch_sizes(sonic):
    """k = 1; 2 sharing one array; 3 distinct arrays; 16 (four arrays, each opened at four points); at the chunk prove() takes"""
    pyr = random.Random(16)
    n, i0 = 5000, 1777
    a = [coefficients("rand", n, s) for s in range(4)]
    z = lambda: pyr.randrange(2, R)      # noqa: E731
    check([a[0]], -i0, [z()])
    check([a[0], a[0]], -i0, [z(), z()])
    check([a[0], a[1], a[2]], -i0, [z(), z(), z()])
    check([a[i % 4] for i in range(16)], -i0, [z() for _ in range(16)])


@pytest.mark.parametrize("n,i0,chunk", [(5000, 1777, 0), (3 * 4096 + 5, 4096 + 3, 16), (70001, 35000, 0)])
def test_evaluation_only(sonic, n, i0, chunk):
    """quotient = false, k = 3: the first sweep and the scans alone give f(z) (the s-polynomial evaluations of a proof); 70001
    coefficients take L = 4 on their own"""
    if not chunk:
        assert sw.sweep_chunk(n) == (2 if n == 5000 else 4)
    pyr = random.Random(n)
    a = [coefficients("rand", n, s) for s in range(2)]
    check([a[0], a[0], a[1]], -i0, [pyr.randrange(2, R) for _ in range(3)], quotient=False, chunk=chunk)
    check([a[0], a[0], a[1]], -i0, [pyr.randrange(2, R) for _ in range(3)], quotient=True, chunk=chunk)


def test_refusals(sonic):
    c = coefficients("rand", 10, 1)
    assert gpu_open_batch([c], -3, [0])[0] == INEXACT_DIVISION
    assert gpu_open_batch([c], 1, [5])[0] == INVALID_ARG              # X^0 outside the range
    assert gpu_open_batch([c], -10, [5])[0] == INVALID_ARG
    assert gpu_open_batch([c], -3, [5], chunk=1)[0] == INVALID_ARG
    assert gpu_open_batch([c] * 17, -3, [5] * 17)[0] == INVALID_ARG


@pytest.fixture(scope="module")
def srs(sonic):
    pyr = random.Random(8)
    s = sonic.SRS.new(12300, pyr.randrange(2, R), pyr.randrange(2, R))      # (3 * 4096 + 5 coefficients from X^-11 reach X^12281)
    yield s
    s.close()


@pytest.mark.parametrize("L,n,i0", [(16, 2 * 4096 + 1, 4096), (16, 3 * 4096 + 5, 11), (2, 2000, 1999)])
def test_w_of_the_quotient(sonic, srs, L, n, i0):
    """W: the MSM of this chain's quotient over g^(x^i) equals the W of sonic_open_poly (prefix-sum chain), and so does f(z)"""
    pyr = random.Random(n + i0)
    c, z = coefficients("rand", n, i0), pyr.randrange(2, R)
    rc, fz, (q,) = gpu_open_batch([c], -i0, [z], chunk=L)
    assert rc == 0
    exps = np.arange(-i0, -i0 + n, dtype=np.int64)
    co = open_ref.fr_rows(c)
    ofz, oW = C.create_string_buffer(32), C.create_string_buffer(96)
    assert _lib().sonic_open_poly(srs._h, z.to_bytes(32, "little"), n, exps.ctypes.data, co.ctypes.data, ofz, oW) == 0
    W = C.create_string_buffer(96)
    qr = open_ref.fr_rows(q)
    assert _lib().sonic_msm_g1_srs(srs._h, 0, -i0, qr.ctypes.data, n - 1, W) == 0
    assert fz[0] == int.from_bytes(ofz.raw, "little")
    assert W.raw == oW.raw
