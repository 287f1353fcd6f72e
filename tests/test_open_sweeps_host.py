"""The chunked Horner sweeps of the batched opening chain (sonic_amd/csrc/poly.hip), as a Python-integer model (tests/open_sweeps_ref.py),
against synthetic division and Horner's rule (tests/open_ref.py).  No GPU: this pins the algorithm -- the side split at X^0, the padding
in front, the shared multiplier of the scans, the carry folded into a block of tiles, the power table, the f(z) formula -- where the
kernels cannot run.  L = coefficients per thread, T = per workgroup tile; small workgroups (4 or 8 chunks) meet every edge at a few
hundred coefficients, and the library's own 256 runs over the same list once."""
import random

import pytest

import open_ref
import open_sweeps_ref as sw
from open_ref import R


def root_of_unity(order):
    """an element of exact order `order` (a power of two dividing r - 1 = 2^32 * odd)"""
    assert order & (order - 1) == 0 and (R - 1) % order == 0
    w = pow(7, (R - 1) // order, R)
    assert pow(w, order, R) == 1 and (order == 1 or pow(w, order // 2, R) == R - 1)
    return w


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


def lengths(L, T, block):
    """1, 2, L - 1, L, L + 1, T - 1, T, T + 1, 2T + 1, and one side of more than `block` tiles: two iterations of the tile scan"""
    return sorted({1, 2, max(1, L - 1), L, L + 1, T - 1, T, T + 1, 2 * T + 1})


def x0_positions(n, L, T):
    """index of X^0: first, second, mid-chunk, a chunk edge, a tile edge, last"""
    return sorted({p for p in (0, 1, L + L // 2, 2 * L, T, T + 1, n // 2, n - 2, n - 1) if 0 <= p < n})


def check(lo, c, z, L, block):
    fz, q = sw.open_chunked(lo, c, z, L, block)
    want_fz, (qlo, want_q) = open_ref.open_dense(lo, c, z)
    assert qlo == lo
    assert fz == want_fz == open_ref.evaluate(lo, c, z)
    assert q == want_q


@pytest.mark.parametrize("L,block", [(2, 4), (3, 4), (4, 8), (16, 4)])
def test_lengths_and_x0_positions(L, block):
    T = L * block
    pyr = random.Random(L * 100 + block)
    for n in lengths(L, T, block):
        for i0 in x0_positions(n, L, T):
            check(-i0, coefficients("rand", n, n + i0), pyr.randrange(2, R), L, block)


@pytest.mark.parametrize("L,block", [(2, 4), (4, 8)])
def test_two_iterations_of_the_tile_scan(L, block):
    """more than `block` tiles on one side, on the other, and on both: the carry between blocks of the tile scan"""
    T = L * block
    n = (block + 1) * T + 3
    pyr = random.Random(n)
    for i0 in (0, 1, n - 1, n - 2, T * block, T * block + 1, 5):
        check(-i0, coefficients("rand", n, i0), pyr.randrange(2, R), L, block)
    n2 = 2 * (block + 2) * T + 1
    check(-(n2 // 2), coefficients("rand", n2, 3), pyr.randrange(2, R), L, block)


@pytest.mark.parametrize("kind", ["rand", "ones", "ends", "minus1"])
def test_points_and_coefficients(kind):
    """z = 1, r - 1, roots of unity with z^L = 1 and z^T = 1 (every scan multiplier is 1, or returns to 1), random"""
    L, block = 4, 8
    T = L * block
    pyr = random.Random(len(kind))
    points = [1, R - 1, root_of_unity(L), root_of_unity(T), root_of_unity(2 * T), pyr.randrange(2, R), pyr.randrange(2, R)]
    for n in (1, 2, T + 1, 3 * T + 5):
        for i0 in x0_positions(n, L, T):
            for z in points:
                check(-i0, coefficients(kind, n, n), z, L, block)


@pytest.mark.parametrize("L", [2, 16])
def test_library_workgroup_size(L):
    """the same edges with 256 chunks per tile, as the kernels run them (the long case of the tile scan is left to the small workgroups)"""
    T = L * sw.BLOCK
    pyr = random.Random(L)
    for n in (T - 1, T + 1, 2 * T + 1):
        for i0 in (0, L + 1, T, n - 1):
            if i0 < n:
                check(-i0, coefficients("rand", n, n + i0), pyr.randrange(2, R), L, sw.BLOCK)
    assert sw.open_chunked(0, [5], 3, L) == (5, [])


def test_shape_rules():
    """the chunk length prove() takes (poly.hpp open_sweep_chunk) and the size rule of the carries: enough for any position of X^0"""
    assert [sw.sweep_chunk(n) for n in (1, 49157, 65536, 196609, 262143, 262144, 786437, 1 << 23)] == [2, 3, 4, 12, 15, 16, 16, 16]
    for L in (2, 3, 16):
        T = L * sw.BLOCK
        for n in (1, 2, T, T + 1, T + 2, 2 * T + 1, 5 * T + 7):
            for i0 in {0, 1, n // 2, n - 1} & set(range(n)):
                nb = -(-i0 // T) + -(-(n - 1 - i0) // T)
                assert nb * (sw.BLOCK + 1) + 2 * (sw.BLOCK + 1) <= sw.sweep_entries(n, L)
