"""Every stage of the G2 MSM (sonic_amd/csrc/msm_g2.hip) over degenerate bases, at every window width, and the structure check and the
shared workspace on top of it.  Bytes and verdicts only; nothing rests on a tolerance.

References, none of them the MSM itself: over a string with known trapdoor the sum is (sum_i s_i k_i mod r) h, one g2_mul of
oracle/pairing.py; outside the subgroup it is the literal integer multiple (literal_mul of tests/test_gpu_msm_g2.py).

Which exceptional branch a case reaches is not guessed: util.g2_msm_mirror replays the chain on integers (tests/test_msm_g2_mirror.py
checks the mirror itself) and every case of part B asserts from it, before the GPU is called, the event it is named after at the stage
it is named after.  Stages and events are the mirror's (accum, combine, seg_run, seg_acc, seg_mul, seg_join, range, range_tree, range2,
range2_tree, fold; dbl, neg, p_inf, q_inf, both_inf, add).

Which width a chain ran at cannot be read off its result -- the sum is the same at every c -- so the cases that depend on the override
also count the launches of k_g2_sum through the library's kernel profiler (g2_sum_launches): one per chain up to c = 10, two from c = 11,
where nseg = 2^(c-4) exceeds 64 and g2_sum_ranges_enqueue takes its two-launch form.  An override that did not reach the G2 plan shows
there, and nowhere else.

Order inside a bucket: the sort of msm.hip places entries by atomic counters ("nothing needs to be stable"), so what a walk or a
bucket's chunks meet depends on an order the device does not fix.  Claims about accum and combine are therefore made only where the
mirror says order_free (at most two entries per bucket, or one value throughout a bucket: all points equal); the other cases (x = r - 1,
the roots of unity, the 256th root over two periods) claim only what follows from the buckets' sums -- seg_run onwards -- and say so.
That rules out the issue's "WM copies of P with WM/2 copies of 2P in different chunks": the same point in two Jacobian representations
meets g2_add instead in test_segments_caller_points_same_point_two_representations, across two buckets.

  A  the mirror                      tests/util.py, self-test in tests/test_msm_g2_mirror.py
  B  degenerate strings              test_accumulate_*, test_combine_*, test_segments_*, test_range_sum_*, test_horner_fold, test_outside_the_subgroup
  C  every window width              test_every_window_width, test_uniform_vectors
  D  the check                       test_check_*
  E  one workspace, two groups       test_one_workspace_serves_both_groups_in_turn

Sizes (WM = sonic_msm_g2_walk_max()): n = 65 for a walk, 2 WM / 2 WM + 1 / 3 WM for the combine, a handful of entries for the segment
and range constructions (c = 4, 7 by override: one and eight segments; c = 12, 16: four and 64 blocks per range, the second launch of
g2_sum_ranges_enqueue), n = 601 and 65 at every c = 4 .. 16.
"""
import ctypes as C
import random
from contextlib import contextmanager

import numpy as np
import pytest

from test_gpu_msm_g2 import R3, R4, SEED, cofactor_point, g2_bytes_array, literal_mul, neg, window_bits  # noqa: F401  (cofactor_point: a fixture)
from util import HALF_R, R, digit_families, digit_stream, g2_msm_mirror, root_of_unity, srs_exponent

pytestmark = pytest.mark.gpu

TRAPDOORS = {"x1": 1, "xneg1": R - 1, "root4": root_of_unity(2), "root256": root_of_unity(8)}
ALPHA = 0x5EED5EED5EED5EED
D = 300
D_BIG = 8200


def walk_max():
    from sonic_amd import _lib
    wm = _lib.lib().sonic_msm_g2_walk_max()
    assert 8 <= wm <= 4096
    return wm


@contextmanager
def window(c):
    """the MSM window override (sonic_msm_set_window), cleared whatever happens; c = 0: the automatic rule"""
    from sonic_amd import _lib
    _lib.lib().sonic_msm_set_window(c)
    try:
        yield
    finally:
        _lib.lib().sonic_msm_set_window(0)


def g2_sum_launches(call):
    """launches of k_g2_sum while call() runs, from the library's kernel profiler (sonic_profile_*).  The sum does not depend on the
    window width, so this is what shows which width a chain ran at: g2_sum_ranges_enqueue launches once per chain while nseg =
    2^(c-4) <= 64 and twice from c = 11."""
    from sonic_amd import _lib
    L = _lib.lib()
    _lib.check(L.sonic_profile_reset())
    _lib.check(L.sonic_profile_enable(1))
    try:
        call()
    finally:
        _lib.check(L.sonic_profile_enable(0))
    n = C.c_int64(-1)
    _lib.check(L.sonic_profile_get(b"k_g2_sum", None, C.byref(n)))
    return n.value


def g2_bytes_of(k):
    """the 192 bytes of k h"""
    from oracle import pairing as pr
    from sonic_amd import encoding as enc
    k %= R
    return enc.g2_to_bytes(pr.g2_mul(pr.G2_GEN, k) if k else None)


class Known:
    """a string of d with the trapdoor (x, alpha) in hand: k_e of both G2 bases (index e + d), their points on demand"""

    def __init__(self, sonic, d, x, alpha):
        self.d, self.n, self.x, self.alpha = d, 2 * d + 1, x, alpha
        self.srs = sonic.SRS.new(d, x, alpha)
        xinv = pow(x, -1, R)
        lo, hi = [1], [1]
        for _ in range(d):
            lo.append(lo[-1] * xinv % R)
            hi.append(hi[-1] * x % R)
        self._k = [lo[:0:-1] + hi, None]
        self._pts = {}

    def k(self, basis, e0=None, n=None):
        if self._k[1] is None:
            self._k[1] = [v * self.alpha % R for v in self._k[0]]
        ks = self._k[basis]
        return ks if e0 is None else ks[e0 + self.d:e0 + self.d + n]

    def exponent(self, basis, e0, scalars):
        return sum(s * k for s, k in zip(scalars, self.k(basis, e0, len(scalars)))) % R

    def points(self, basis):
        if basis not in self._pts:
            self._pts[basis] = self.srs.g2_points(basis, -self.d, self.n)
        return self._pts[basis]


_STRINGS = {}


@pytest.fixture
def known(sonic):
    def get(name, d=D):
        if (name, d) not in _STRINGS:
            if name == "honest":
                pyr = random.Random(d)
                x, alpha = pyr.randrange(2, R), pyr.randrange(2, R)
            else:
                x, alpha = TRAPDOORS[name], ALPHA
            _STRINGS[name, d] = Known(sonic, d, x, alpha)
        return _STRINGS[name, d]
    return get


def srs_case(sonic, S, basis, e0, sc, c=0):
    """mirror and closed form of msm_g2_srs(S, basis, e0, sc) under window width c (0: the rule); run() calls the GPU and compares"""
    cc = c or window_bits(len(sc))
    m = g2_msm_mirror(S.k(basis, e0, len(sc)), sc, cc, 255, True, walk_max())
    want = S.exponent(basis, e0, sc)
    assert m.total == want

    def run():
        with window(c):
            assert sonic.msm_g2_srs(S.srs, basis, e0, sc) == g2_bytes_of(want), (basis, e0, len(sc), c)
    return m, run


def points_case(sonic, pts, ks, sc, c=0):
    """the same for msm_g2 over caller points pts[i] = ks[i] h: 256 bits, nothing folded"""
    cc = c or window_bits(len(sc))
    m = g2_msm_mirror(ks, sc, cc, 256, False, walk_max())
    want = sum(s * k for s, k in zip(sc, ks)) % R
    assert m.total == want

    def run():
        with window(c):
            assert sonic.msm_g2(pts, sc) == g2_bytes_of(want), (len(sc), c)
    return m, run


# equal scalars, full width on both sides of (r - 1) / 2
EQUAL = {"below half": 0x1B5C9A1D3E4F60718293A4B5C6D7E8F90A1B2C3D4E5F60718293A4B5C6D7E8F9,
         "above half": R - 0x2F2E3D4C5B6A79880F1E2D3C4B5A69788796A5B4C3D2E1F00F1E2D3C4B5A6978}
assert 0 < EQUAL["below half"] < HALF_R < EQUAL["above half"] < R


# ---- B. accumulate ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", sorted(EQUAL))
@pytest.mark.parametrize("basis", (0, 1))
def test_accumulate_equal_points_meet_the_doubling(sonic, known, basis, which):
    """x = 1, n = 65 equal scalars: every bucket holds 65 copies of one point, so each walk is inf + P, P + P (g2_add_mixed's doubling),
    then generic additions -- order-free"""
    S = known("x1")
    sc = [EQUAL[which]] * 65
    m, run = srs_case(sonic, S, basis, -32, sc)
    nonempty = sum(1 for dg, _ in digit_stream(sc[0], [4] * 64, True)[0] if dg)
    assert m.order_free and nonempty > 30
    assert m["accum"]["dbl"] == nonempty == m["accum"]["p_inf"] and m["accum"]["neg"] == 0 and m["accum"]["add"] == 63 * nonempty
    run()
    # the same points as caller points: 256 bits, the scalar above (r - 1) / 2 stays literal
    m, run = points_case(sonic, S.points(basis)[:65], S.k(basis, -D, 65), sc)
    assert m.order_free and m["accum"]["dbl"] == sum(1 for dg, _ in digit_stream(sc[0], [4] * 64, False)[0] if dg) > 30
    run()


@pytest.mark.parametrize("name", ("xneg1", "root4", "root256"))
@pytest.mark.parametrize("basis", (0, 1))
def test_accumulate_cancelling_points(sonic, known, name, basis):
    """x = r - 1 (h and -h in turn), a 4th and a 256th root, n = 65 equal scalars.  In index order the walk of x = r - 1 is inf + P,
    P - P, inf + P, ...: it cancels and restarts.  The device's order inside a bucket is not fixed, so no accum count is claimed -- only
    that every bucket holds a point and its negative, whose second addition is a doubling or a cancellation in any order (x = r - 1), and
    the bucket sums, which no order changes."""
    S = known(name)
    for which in sorted(EQUAL):
        sc = [EQUAL[which]] * 65
        m, run = srs_case(sonic, S, basis, -32, sc)
        assert not m.order_free
        if name == "xneg1":
            assert m["accum"]["neg"] >= 32 and m["accum"]["add"] == 0          # (index order)
            # 33 of one sign and 32 of the other: every bucket's sum is a single +-P, so run meets equal and opposite buckets
            assert m["seg_run"]["dbl"] + m["seg_run"]["neg"] + m["seg_acc"]["dbl"] + m["seg_acc"]["neg"] > 0
        elif name == "root4":
            assert m["accum"]["neg"] > 0                                       # (index order: i P - i P)
        run()
        if name == "xneg1":
            m, run = points_case(sonic, S.points(basis)[D - 32:D + 33], S.k(basis, -32, 65), sc)
            assert not m.order_free and m["accum"]["neg"] >= 32
            run()


# ---- B. combine ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", ("2WM", "3WM", "2WM+1"))
def test_combine_equal_partial_sums(sonic, known, shape):
    """x = 1 and equal scalars over 2 WM, 3 WM and 2 WM + 1 terms: every bucket is cut into chunks that hold the same multiple of one
    point (order-free), so k_g2_bucket_combine doubles in g2_add, and then adds a single partial to the doubled one (3 WM: WM P to
    2 WM P; 2 WM + 1: P to 2 WM P)"""
    wm = walk_max()
    n = {"2WM": 2 * wm, "3WM": 3 * wm, "2WM+1": 2 * wm + 1}[shape]
    S = known("x1", D_BIG)
    assert n <= S.n
    for which in sorted(EQUAL):
        sc = [EQUAL[which]] * n
        for basis in (0, 1):
            m, run = srs_case(sonic, S, basis, -7, sc)
            nonempty = m["combine"]["p_inf"]
            assert m.order_free and nonempty > 20
            assert m["combine"]["dbl"] == nonempty and m["combine"]["neg"] == 0
            assert m["combine"]["add"] == (0 if shape == "2WM" else nonempty)
            run()
    m, run = points_case(sonic, S.points(0)[:n], S.k(0, -D_BIG, n), [EQUAL["above half"]] * n)
    assert m.order_free and m["combine"]["dbl"] == m["combine"]["p_inf"] > 20
    run()


def test_combine_buckets_that_sum_to_infinity(sonic, known):
    """the 256th root over 2 WM = two periods, equal scalars: every bucket's sum is infinity.  Were the order of entries kept, every
    partial sum would be infinity too; it is not kept (see the module docstring), so the claim is the order-independent one: the
    segments see nothing but infinity, and the sum is infinity"""
    wm = walk_max()
    n = 2 * wm
    assert n % 256 == 0
    S = known("root256", D_BIG)
    for basis in (0, 1):
        sc = [EQUAL["below half"]] * n
        m, run = srs_case(sonic, S, basis, -11, sc)
        assert not m.order_free and m.total == 0
        assert all(m[st][k] == 0 for st in ("seg_run", "seg_acc", "range", "fold") for k in ("add", "dbl", "neg", "p_inf", "q_inf"))
        run()


# ---- B. segments and the range sum ---------------------------------------------------------------------------------------------------------
def entry(c, w, digit, negative=False):
    """a scalar whose only non-zero digit is `digit` in window w, negative through the fold"""
    v = digit << (c * w)
    assert 0 < digit <= 1 << (c - 1) and v <= HALF_R
    return R - v if negative else v


def segment_constructions(c):
    """scalar lists over equal points, by name, each with the (stage, event) it must reach.  s: the top segment; its buckets hold digits
    s K + 1 .. s K + K.  All buckets hold at most two entries or equal ones: order-free."""
    NB = 1 << (c - 1)
    K = min(NB, 8)
    nseg = NB // K
    top = (nseg - 1) * K
    out = {
        # j + 1 and r - (j + 1) in one bucket: the walk cancels
        "cancel in one bucket": ([entry(c, 0, top + 3), entry(c, 0, top + 3, True), entry(c, 1, 1)], [("accum", "neg")]),
        # B_j = h, B_{j+1} = -h: run passes through infinity, and acc, finite, adds a run at infinity
        "adjacent opposite buckets": ([entry(c, 0, top + 1), entry(c, 0, top + 2, True)], [("seg_run", "neg"), ("seg_acc", "q_inf")]),
        # B_top = h, the bucket below -2h: acc = h meets run = -h
        "acc meets -run": ([entry(c, 0, top + K), entry(c, 0, top + K - 1, True), entry(c, 0, top + K - 1, True)], [("seg_acc", "neg"), ("accum", "dbl")]),
        # one bucket with an empty one below it: acc = run, the doubling of g2_add
        "acc meets run": ([entry(c, 0, top + K)], [("seg_acc", "dbl")] if K > 1 else []),
    }
    if nseg > 1:
        # an empty lowest segment beside a full top one: (s K) run by double-and-add with run finite (window 1: up = run, 2 run, 2 run +
        # run, ...) and, after h - h, with run at infinity below a finite acc (window 0: segres + up with up at infinity, which happens
        # in a segment s > 0 only when its run ended at infinity)
        out["segment multiple"] = ([entry(c, 0, top + 1), entry(c, 0, top + 2, True)] + [entry(c, 1, top + j) for j in range(1, K + 1)],
                                   [("seg_mul", "p_inf"), ("seg_mul", "add"), ("seg_mul", "dbl_op"), ("seg_join", "q_inf"), ("seg_join", "add")])
        # one entry in the top bucket of segment 1: acc = K B and the multiple (1 K) run = K B -- the last addition doubles
        out["acc meets the multiple"] = ([entry(c, 0, 2 * K)], [("seg_join", "dbl")])
    return out


@pytest.mark.parametrize("c", (4, 7, 12, 16))
def test_segments_over_equal_points(sonic, known, c):
    """x = 1, scalars chosen by digit so that chosen buckets hold chosen multiples of h (of alpha h): c = 4 (NB = 8, one segment), c = 7
    (eight segments, one block), and the same constructions under the two-launch range sum at c = 12 and 16"""
    S = known("x1")
    cons = segment_constructions(c)
    assert len(cons) == (4 if c == 4 else 6)
    for name, (sc, claims) in sorted(cons.items()):
        for basis in (0, 1):
            m, run = srs_case(sonic, S, basis, -3, sc, c)
            assert m.order_free and m.plan["nseg"] == max(1, 1 << (c - 4)), name
            for stage, event in claims:
                assert m[stage][event] >= 1, (name, stage, event, dict(m[stage]))
            assert (m.plan["blocks"] > 1) == (c >= 11)
            assert g2_sum_launches(run) == (2 if c >= 11 else 1)


def test_segments_caller_points_same_point_two_representations(sonic):
    """msm_g2 over P, P, 2P under scalars 1, 1, 2: bucket 1 holds 2P as the doubling of the walk left it (z = 2y), bucket 2 holds the
    affine 2P (z = 1).  run = B_2 + B_1 meets the same point in two Jacobian representations: U1 = U2 and S1 = S2 only after the
    cross-multiplication, the doubling branch of g2_add.  Two entries per bucket at most: order-free."""
    k = 0xFEEDFACE
    pts = np.frombuffer(g2_bytes_of(k) * 2 + g2_bytes_of(2 * k), np.uint8).reshape(3, 192)
    for c in (0, 7, 12):
        m, run = points_case(sonic, pts, [k, k, 2 * k], [1, 1, 2], c)
        assert m.order_free and m["accum"]["dbl"] == 1 and m["seg_run"]["dbl"] == 1 and m["seg_run"]["neg"] == 0
        run()


def range_construction(c):
    """scalars over equal points whose windows hold, in one call: two segment results that are equal and two that are opposite at the last
    level of the range sum's tree (buckets NB / 2 twice and NB once: segments nseg / 2 - 1 and nseg - 1 -- threads 3 and 7 of one block
    at c = 7, the last threads of blocks 1 and 3 (31 and 63) of the second launch at c = 12 (16)); where a range has 64 segments or more,
    the same in the first launch's tree (segments 0 and 32: bucket 2 132 times against bucket 264 once); a window whose buckets all cancel;
    an empty window between finite ones; a finite one"""
    NB = 1 << (c - 1)
    sc = [entry(c, 0, NB // 2)] * 2 + [entry(c, 0, NB)]
    sc += [entry(c, 1, NB // 2)] * 2 + [entry(c, 1, NB, True)]
    if NB // 8 >= 64:
        sc += [entry(c, 2, 2)] * 132 + [entry(c, 2, 264)]
        sc += [entry(c, 3, 2)] * 132 + [entry(c, 3, 264, True)]
    sc += [entry(c, 4, dg, sign) for dg in (1, 9, NB // 2 + 1, NB) for sign in (False, True)]
    sc += [entry(c, 6, 5)]
    return sc


@pytest.mark.parametrize("c", (7, 12, 16))
def test_range_sum_equal_opposite_and_infinite_segment_results(sonic, known, c):
    """k_g2_sum over the segment results of a window: its LDS tree and, from c = 11, the second launch over the block totals meet P + P,
    P - P and ranges that are all infinity (range_construction); c = 16 is nseg = 4096, 64 blocks per range"""
    S = known("x1")
    sc = range_construction(c)
    assert len(sc) <= S.n
    last = "range_tree" if c == 7 else "range2_tree"
    for basis in (0, 1):
        m, run = srs_case(sonic, S, basis, -D, sc, c)
        assert m.order_free and m.plan["blocks"] == {7: 1, 12: 4, 16: 64}[c]
        assert m[last]["dbl"] == 1 and m[last]["neg"] == 1
        if c >= 11:
            assert m["range_tree"]["dbl"] == 1 and m["range_tree"]["neg"] == 1 and m["range2"]["p_inf"] >= 4 and m["range2"]["both_inf"] > 0
        assert m.windows[1] == 0 and m.windows[4] == 0 and m.windows[5] == 0 and m.windows[0] and m.windows[6]
        assert m["fold"]["q_inf"] >= 3 and m["accum"]["neg"] == 4
        assert g2_sum_launches(run) == (2 if c >= 11 else 1)


# ---- B. the Horner fold -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", (0, 7, 13, 16))
def test_horner_fold(sonic, c):
    """msm_g2 over P = k h, Q = 2^c P, -Q and T: digit 1 for P in windows 6 and 3, for -Q in window 5, for Q in window 2, for T in window
    0.  From the top the host's fold holds P, shifts it to Q and adds -Q (infinity), doubles infinity through the empty window 4, takes P
    again, shifts it to Q and adds S_2 = Q (the doubling of g2_add), passes the empty window 1 with a finite accumulator and ends on T."""
    cc = c or window_bits(4)
    k, t = 0xABCDEF0123456789ABCDEF, 0x777
    ks = [k, (k << cc) % R, R - (k << cc) % R, t]
    sc = [(1 << 6 * cc) + (1 << 3 * cc), 1 << 2 * cc, 1 << 5 * cc, 1]
    pts = np.frombuffer(b"".join(g2_bytes_of(v) for v in ks), np.uint8).reshape(4, 192)
    m, run = points_case(sonic, pts, ks, sc, c)
    assert m.plan["c"] == cc and m.order_free
    assert m["fold"]["dbl"] == 1 and m["fold"]["neg"] == 1 and m["fold"]["q_inf"] == 1 and m["fold"]["p_inf"] == 2 and m["fold"]["add"] == 1
    assert m["fold"]["dbl_of_inf"] >= 2 * cc
    run()


# ---- B. outside the subgroup --------------------------------------------------------------------------------------------------------------
def test_outside_the_subgroup_through_chunks(sonic, cofactor_point):
    """2 WM + 5 copies of +-P, P of the twist outside the order-r subgroup, through msm_g2: the sum is the literal multiple by the integer
    sum_i +-s_i, not reduced modulo r.  The mirror runs over plain integers.  P goes with r - 1 and (r + 1) / 2, -P with two scalars
    whose digits fall where those two have none.  At c = 6 no window gives r - 1 and (r + 1) / 2 the same digit with opposite signs, so
    every bucket holds one point throughout (order-free, asserted): the 2 WM + 1 copies of P under r - 1 make three partial sums per
    bucket that the combine doubles and adds, far outside what a multiple modulo r would give.  At the automatic c = 5 window 25 has
    digit 11 of r - 1 and digit -11 of (r + 1) / 2 in one bucket, P among -P in an order the device does not fix: bytes only there."""
    from oracle import pairing as pr
    from sonic_amd import encoding as enc
    P = cofactor_point
    wm = walk_max()
    n = 2 * wm + 5
    for c, claim in ((6, True), (window_bits(n), False)):
        signed = [(1, R - 1)] * (2 * wm + 1) + [(1, (R + 1) // 2)] * 2 + [(-1, 3 << c), (-1, 7 << 7 * c)]
        assert len(signed) == n
        ks, sc = [s for s, _ in signed], [v for _, v in signed]
        m = g2_msm_mirror(ks, sc, c, 256, False, wm, mod=None)
        total = sum(k * s for k, s in signed)
        assert m.total == total > R and m.order_free == claim
        if claim:
            cut = sum(1 for dg, _ in digit_stream(R - 1, [c] * m.plan["W"], False)[0] if dg)
            assert m["combine"]["dbl"] == cut > 25 and m["combine"]["add"] == cut and m["accum"]["dbl"] >= cut
        want = enc.g2_to_bytes(literal_mul(pr, P, total))
        assert want != enc.g2_to_bytes(literal_mul(pr, P, total % R))
        pts = g2_bytes_array([P if k > 0 else neg(pr, P) for k in ks])
        with window(c if claim else 0):
            assert sonic.msm_g2(pts, sc) == want, c


# ---- C. every window width ----------------------------------------------------------------------------------------------------------------
def width_vector(c, bits, fold, n):
    """the digit-edge scalars of the layout [c] * W, the fixed boundary values, one that lives only in the top window, random fill"""
    W = -(-bits // c)
    limit = HALF_R if fold else R - 1
    fam = [s for s, _ in digit_families([c] * W, limit).values()]
    if fold:
        fam += [R - s for s in fam]
    top_only = 1 << (c * (W - 1))
    if top_only > limit:                       # (256 bits at c = 16: the top window starts at bit 240)
        top_only = 1 << (c * (W - 2))
    sc = fam + [0, 1, R - 1, HALF_R, HALF_R + 1, 1 << (c - 1), (1 << c) - 1, (1 << 252) - 1, 1 << 254, top_only]
    pyr = random.Random(1000 * c + bits)
    sc += [pyr.randrange(R) for _ in range(n - len(sc))]
    assert len(sc) == n
    return sc, W


def assert_carries(sc, c, W, fold):
    """from digit_stream: some scalar carries into the top window, none carries out of it.  A window hands a carry on exactly when it
    flips the digit's sign against the fold's (its digit went negative)."""
    into_top = 0
    for s in sc:
        digs, negated, over = digit_stream(s, [c] * W, fold)
        assert over == (0, 0), (hex(s), c)
        assert digs[W - 1][1] == int(negated), (hex(s), c)
        v = R - s if negated else s
        if digs[W - 2][1] != int(negated):
            into_top += 1
            assert digs[W - 1][0] == (v >> c * (W - 1)) + 1
    assert into_top > 0, c


@pytest.mark.parametrize("c", range(4, 17))
def test_every_window_width(sonic, known, c):
    """c = 4 .. 16 by override: the whole basis of d = 300 (n = 601, folded, 255 bits) and n = 65 caller points (literal, 256 bits) under
    the digit-edge families of that layout and the boundary scalars; the closed form is the reference"""
    S = known("honest")
    sc, W = width_vector(c, 255, True, S.n)
    assert_carries(sc, c, W, True)
    lit, Wl = width_vector(c, 256, False, 65)
    assert_carries(lit, c, Wl, False)
    want = [g2_bytes_of(S.exponent(b, -D, sc)) for b in (0, 1)]
    want_lit = g2_bytes_of(S.exponent(1, -D, lit))
    pts = S.points(1)[:65]

    def calls():
        for b in (0, 1):
            assert sonic.msm_g2_srs(S.srs, b, -D, sc) == want[b], (c, b)
        assert sonic.msm_g2(pts, lit) == want_lit, c

    with window(c):
        assert g2_sum_launches(calls) == 3 * (2 if c >= 11 else 1)          # the override reached all three chains
    assert window_bits(S.n) == 5 and window_bits(65) == 4
    assert g2_sum_launches(calls) == 3                                      # and the rule is back: c = 5, 5 and 4


@pytest.mark.parametrize("c", (9, 13, 16))
def test_uniform_vectors(sonic, known, c):
    """all 2^(c-1) (the largest positive digit, no carry) and all 2^252 - 1 (a carry through every window): c = 13 leaves an 8-bit top
    window at 255 bits, c = 16 fills 256 bits exactly"""
    S = known("honest")
    for v in (1 << (c - 1), (1 << 252) - 1):
        digs, _, over = digit_stream(v, [c] * -(-255 // c), True)
        assert over == (0, 0)
        want = [g2_bytes_of(S.exponent(1, -D, [v] * S.n)), g2_bytes_of(S.exponent(0, -D, [v] * 65))]
        with window(c):
            assert sonic.msm_g2_srs(S.srs, 1, -D, [v] * S.n) == want[0], (c, hex(v))
            assert sonic.msm_g2(S.points(0)[:65], [v] * 65) == want[1], (c, hex(v))


# ---- D. the check -------------------------------------------------------------------------------------------------------------------------
def check_both_settings(srs, monkeypatch):
    monkeypatch.setenv("SONIC_G2_MSM", "0")
    walk = srs.check(SEED)
    monkeypatch.delenv("SONIC_G2_MSM")
    return walk, srs.check(SEED)


@pytest.mark.parametrize("c", (0, 4, 16))
@pytest.mark.parametrize("name", sorted(TRAPDOORS))
def test_check_accepts_degenerate_strings(known, monkeypatch, name, c):
    """R0 .. R4 hold for every non-zero trapdoor: the degenerate strings are reference strings, under the walk and under the 129-bit MSM
    plan at the automatic width (c = 5) and at both ends of the override"""
    import srs_update_ref as uref
    S = known(name)
    # the check's own chains on integers: 128-bit randomizers under the 129-bit plan, nothing folded and no carry out of the top window
    # (the mirror asserts that).  Signed digits put P and -P into one bucket even over x = 1, in an order the device does not fix: the
    # only claim is that over the two-point bases (x = 1, r - 1) the buckets' sums, which no order changes, meet equal or opposite
    # operands further down
    rho = [uref.rho(SEED, i) for i in range(S.n)]
    for basis in (0, 1):
        m = g2_msm_mirror(S.k(basis), rho, c or window_bits(S.n), 129, True, walk_max())
        assert m.total == S.exponent(basis, -S.d, rho) != 0 and m.plan["W"] == -(-129 // (c or 5))
        late = ("seg_run", "seg_acc", "seg_join", "range", "range_tree", "range2_tree", "fold")
        assert name in ("root4", "root256") or sum(m[st]["dbl"] + m[st]["neg"] for st in late) > 0
    with window(c):
        assert check_both_settings(S.srs, monkeypatch) == ((True, 0), (True, 0))
        # the two G2 sums of the check ran at the override: two launches of k_g2_sum each from c = 11, one below
        assert g2_sum_launches(lambda: S.srs.check(SEED)) == (4 if c >= 11 else 2)


def test_check_accepts_x1_with_a_narrow_top_window(known, monkeypatch):
    """d = 8200: c = 10, thirteen windows over 129 bits, the top one 9 bits wide"""
    S = known("x1", D_BIG)
    assert window_bits(S.n) == 10 and 129 - 10 * (-(-129 // 10) - 1) == 9
    assert check_both_settings(S.srs, monkeypatch) == ((True, 0), (True, 0))


@pytest.mark.parametrize("which,mask", ((2, R3), (3, R4)))
def test_check_rejects_a_mutant_of_the_x1_string(sonic, known, monkeypatch, which, mask):
    """H[-d] := 2h over the x = 1 string (where swapping two elements changes nothing).  H0[-d] is a term of B = sum_e rho_e H0[e] and of
    no other relation -- R0 reads H0[0], R1 H0[1], R2 and R4 H1[0] -- and rho_0 != 0, so B moves by rho_0 h and R3 alone fails; H1[-d] is
    a term of C alone, which moves by rho_0 (2 - alpha) h != 0: R4 alone"""
    import srs_update_ref as uref
    S = known("x1")
    d = S.d
    assert uref.rho(SEED, 0) % R != 0 and (2 - ALPHA) % R != 0 and d > 1
    arrays = [S.srs.points(0, -d, S.n), S.srs.points(1, -d, S.n), S.points(0).copy(), S.points(1).copy()]
    arrays[which][0] = np.frombuffer(g2_bytes_of(2), np.uint8)
    bad = sonic.SRS.from_points(d, arrays[0], arrays[1])
    bad.set_g2_points(arrays[2], arrays[3])
    for c in (0, 16):
        with window(c):
            assert check_both_settings(bad, monkeypatch) == ((False, mask), (False, mask))
    bad.close()


# ---- E. one workspace, two groups ---------------------------------------------------------------------------------------------------------
def test_one_workspace_serves_both_groups_in_turn(sonic, orc, known):
    """G1 and G2 chains on different plans, one after the other in one process, sizes shrinking and growing: the shared digit-and-sort
    phase and the lease's workspace carry nothing from one group to the next"""
    from sonic_amd import _lib
    from sonic_amd.commitment import msm_g1_srs
    S, B = known("honest"), known("honest", D_BIG)
    pyr = random.Random(2025)
    sc601 = [pyr.randrange(R) for _ in range(S.n)]
    sc65 = [pyr.randrange(R) for _ in range(65)]
    scbig = [pyr.randrange(R) for _ in range(B.n)]
    sc20 = [pyr.randrange(R) for _ in range(20)]

    def plan(srs, n):
        c, w, sets = C.c_int(), C.c_int(), C.c_int()
        _lib.check(_lib.lib().sonic_msm_plan(srs._h, n, C.byref(c), C.byref(w), C.byref(sets)))
        return c.value, w.value, sets.value

    def g1(K, basis, e0, sc):
        return msm_g1_srs(K.srs, basis, e0, sc), orc.g1_mul(orc.g1_gen(), srs_exponent(K.x, K.alpha, basis, e0, sc))

    def g2(K, basis, e0, sc):
        return sonic.msm_g2_srs(K.srs, basis, e0, sc), g2_bytes_of(K.exponent(basis, e0, sc))

    assert plan(S.srs, S.n)[2] == 1                                   # window tables: one shared bucket set
    got = [g1(S, 0, -D, sc601), g2(S, 1, -D, sc601)]
    with window(13):
        assert plan(S.srs, S.n) == (13, 20, 20)                       # no tables: a bucket set per window
        got.append(g1(S, 1, -D, sc601))
    with window(16):
        want = g2_bytes_of(S.exponent(0, -D, sc65))
        got.append((sonic.msm_g2(S.points(0)[:65], sc65), want))
    got += [g1(S, 0, -D, sc601), g2(B, 0, -D_BIG, scbig), g1(S, 1, -9, sc20)]
    got += [g1(S, 0, -D, sc601), g2(S, 1, -D, sc601)]
    for i, (have, want) in enumerate(got):
        assert have == want, i
    assert got[4][0] == got[0][0] == got[7][0] and got[8][0] == got[1][0]
