"""The digit layer of the G1 MSM on the host: a Python mirror of DigitStream and of the even-width window layout (tests/util.py), the
digit-edge scalar families that tests/test_gpu_msm_paths.py feeds the kernels, and the closed-form reference those tests compare against.
Every family must produce exactly the signed digits it claims, and every layout must reconstruct its scalar with no carry out of the top
window: tables (c = 13, 16, 17, 20 as SRS.new picks them, srs_policy.hpp), the unfolded windows of sonic_msm_g1 (c = 4..16) and the
130-bit halves of the endomorphism split."""
import random

import numpy as np
import pytest

from util import (ENDO_BITS, HALF_R, LAM, NCPU, R, digit_families, digit_stream, digits_value, endo_split, fr_bytes, fr_ints,
                  msm_even_shift, msm_even_width, msm_path, msm_plan_points, rand_fr_array, root_of_unity, srs_exponent, table_widths)

TABLE_C = [13, 16, 17, 20]
POINT_C = list(range(4, 17))


def table_layout(c):
    W = (255 + c - 1) // c
    return W, table_widths(W)


def endo_layout(c):
    W = (ENDO_BITS + c - 1) // c
    return W, table_widths(W, ENDO_BITS)


def expected(D, negated):
    """claimed signed digits -> (magnitude, sign) as the recoding reports them (sign flips on a folded scalar)"""
    return [(abs(d), int((d < 0) != negated)) for d in D]


def same_digits(got, want):
    return all(g[0] == w[0] and (g[0] == 0 or g[1] == w[1]) for g, w in zip(got, want)) and len(got) == len(want)


def check_scalar(s, widths, fold):
    digs, neg, rest = digit_stream(s, widths, fold)
    assert rest == (0, 0), "carry or bits left over the top window"
    half = [1 << (c - 1) for c in widths]
    assert all(1 - h <= (-d if sg ^ neg else d) <= h or d == 0 for (d, sg), h in zip(digs, half))
    v = digits_value(digs, widths)
    assert v == (-(R - s) if neg else s)
    return digs, neg


def test_even_width_layout():
    for W in range(1, 33):
        for bits in (255, ENDO_BITS):
            ws = table_widths(W, bits)
            assert sum(ws) == bits and max(ws) - min(ws) <= 1 and ws == sorted(ws, reverse=True)
            assert all(msm_even_shift(W, w, bits) == sum(ws[:w]) for w in range(W))
    # the plans of the issue's table: d -> (c, W, widest window)
    for c, W in ((13, 20), (16, 16), (17, 15), (20, 13)):
        assert table_layout(c)[0] == W and max(table_layout(c)[1]) == c
    assert table_widths(13) == [20] * 8 + [19] * 5
    assert endo_layout(20) == (7, [19] * 4 + [18] * 3)
    assert msm_even_width(7, 0, ENDO_BITS) == 19


def test_points_plan_mirror():
    """the sizes of tests/test_gpu_msm_paths.py's caller-point cases land where that module claims"""
    want = {(1 << 9) + 3: (5, "seg_mul_small", 4), 1 << 13: (9, "seg_mul_small", 4), 1 << 14: (10, "seg_wave", 4),
            (1 << 17) + 5: (13, "seg_wave", 2), 1 << 18: (14, "seg_wave", 1), 500: (4, "seg_none", 4)}
    for n, (c, red, lanes) in want.items():
        cc, W = msm_plan_points(n)
        assert cc == c and W == (256 + c - 1) // c
        p = msm_path(W, 1 << (c - 1), shared=False)
        assert (p["reduction"], p["lanes"]) == (red, lanes), n


@pytest.mark.parametrize("kind,c", [("table", c) for c in TABLE_C] + [("points", c) for c in POINT_C] + [("endo", c) for c in TABLE_C])
def test_digit_families(kind, c):
    if kind == "table":
        widths, fold, limit = table_layout(c)[1], True, HALF_R
    elif kind == "points":
        widths, fold, limit = [c] * ((256 + c - 1) // c), False, R - 1
    else:
        widths, fold, limit = endo_layout(c)[1], False, LAM - 1
    fam = digit_families(widths, limit)
    assert set(fam) == {"half", "half+1", "all-ones", "top-max", "repeat"}
    half = [1 << (w - 1) for w in widths]
    for name, (s, D) in fam.items():
        assert 0 < s <= limit
        digs, neg = check_scalar(s, widths, fold)
        assert not neg and same_digits(digs, expected(D, False)), name
        k = sum(1 for d in D if d)                       # windows the pattern touches
        raw = [(s >> sum(widths[:w])) & ((1 << widths[w]) - 1) for w in range(len(widths))]
        if name == "half":
            assert raw[:k] == half[:k] and D[:k] == half[:k]
        if name == "half+1":
            kk = len([d for d in D if d < 0])
            assert raw[:kk] == [h + 1 for h in half[:kk]] and D[kk] == 1
        if name in ("all-ones", "top-max"):
            top = max(w for w in range(len(D)) if D[w])
            assert raw[:top] == [(1 << widths[w]) - 1 for w in range(top)] and D[top] > 0
        if name == "top-max":
            t = max(w for w in range(len(D)) if D[w])
            assert s + (1 << sum(widths[:t])) > limit or D[t] == half[t]       # the largest top digit that fits
        if name == "repeat":
            assert all(d == 3 for d in D[:k]) and k >= len(widths) - 1
        if fold:
            # the same pattern above (r-1)/2: folded onto the negated point, every digit's sign flips
            digs, neg = check_scalar(R - s, widths, fold)
            assert neg and same_digits(digs, expected(D, True)), name
        else:
            check_scalar(R - s if kind == "points" else limit - s, widths, fold)
    if kind == "endo":
        # scalars built from two half patterns: s = s1 + lambda s2 < r splits back into them
        for a, (s1, D1) in fam.items():
            lim2 = (R - 1 - s1) // LAM
            for b, (s2, D2) in digit_families(widths, lim2).items():
                s = s1 + LAM * s2
                assert s < R and endo_split(s) == (s1, s2)
                assert same_digits(digit_stream(s2, widths, False)[0], expected(D2, False)), (a, b)


@pytest.mark.parametrize("kind,c", [("table", c) for c in TABLE_C] + [("points", c) for c in POINT_C] + [("endo", c) for c in TABLE_C])
def test_reconstruction_uniform_and_value_edges(kind, c):
    pyr = random.Random(c * 7 + len(kind))
    edges = [0, 1, 2, R - 1, R - 2, HALF_R - 1, HALF_R, HALF_R + 1, HALF_R + 2, LAM, LAM - 1, LAM + 1, LAM * LAM % R, (1 << 128) - 1,
             1 << 253, (1 << 254) - 1]
    vals = edges + [pyr.randrange(R) for _ in range(300)]
    for s in vals:
        if kind == "table":
            check_scalar(s, table_layout(c)[1], True)
        elif kind == "points":
            check_scalar(s, [c] * ((256 + c - 1) // c), False)
        else:
            for h in endo_split(s):
                check_scalar(h, endo_layout(c)[1], False)


def test_fold_boundary():
    w = table_layout(20)[1]
    assert not digit_stream(HALF_R, w, True)[1] and digit_stream(HALF_R + 1, w, True)[1]
    assert digit_stream(R - 1, w, True)[0][0] == (1, 1)


@pytest.mark.parametrize("x", [1, R - 1, "w4", "w256"])
def test_closed_form_matches_oracle(orc, x):
    """srs_exponent (the reference of tests/test_gpu_msm_paths.py) against the oracle's Pippenger and its reference-shaped fold on small
    degenerate SRSs: x = 1 (every basis element is g: the reference's bench/Main.hs SRS), x = r - 1 (g, -g, g, ...), roots of unity"""
    x = {"w4": root_of_unity(2), "w256": root_of_unity(8)}.get(x, x)
    d, alpha = 300, 5
    o = orc.SRS(d, x, alpha, threads=min(NCPU, 16))
    g = orc.g1_gen()
    rng = np.random.default_rng(3)
    sc = rand_fr_array(rng, 2 * d + 1)
    sc[7] = 0
    ints = fr_ints(sc)
    for basis, e0, n in ((0, -d, 2 * d + 1), (1, -d, 2 * d + 1), (1, -5, 11), (0, 1, 200), (1, 0, 1)):
        want = orc.g1_mul(g, srs_exponent(x, alpha, basis, e0, ints[:n]))
        assert orc.msm_srs(o, basis, e0, sc[:n], 1, min(NCPU, 16)) == want, (basis, e0, n)
        assert orc.msm_srs(o, basis, e0, sc[:n], 0, min(NCPU, 16)) == want, (basis, e0, n)
    # equal scalars over x = 1 cancel to the point at infinity
    if x == 1:
        assert orc.msm_srs(o, 0, -2, fr_bytes([5, R - 5, 3, R - 3]), 1, 1) == bytes(96) == orc.g1_mul(g, srs_exponent(1, 5, 0, -2, [5, R - 5, 3, R - 3]))
