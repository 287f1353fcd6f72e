"""The G2 MSM on the GPU (include/sonic_hip.h, sonic_msm_g2*): sums over the G2 half of a string and over caller-supplied points of the
twist, and the structure check that runs over it.  Bytes and verdicts only.

The expected sums need no slow reference: H0[e] = x^e h and H1[e] = alpha x^e h for a known trapdoor, so sum_e s_e H[e] is
(sum_e s_e k_e mod r) h -- integer arithmetic and one g2_mul of oracle/pairing.py.  Points outside the order-r subgroup are added term by
term with the oracle's g2_add.

Sizes, and what each crosses (window width c = floor(log2 n) - 4, at least 4; NB = 2^(c-1) buckets per window):
  n = 1, 2            the smallest sums
  n = 63, 64, 65      a wave of the bucket kernels
  n = 601             d = 300, the whole basis: c = 5, more than one 256-bucket sort partition per job
  n = 16401           d = 8200, the whole basis: c = 10, 512 buckets per window, 26 windows: more buckets than one workgroup
  n = 3 WALK_MAX + 5  equal scalars: one bucket per window with n entries, cut into four chunks
  n = 2^19 + 17       one term more than a slab and then some: two chains, the second at c = 4
Every c = 4 .. 16 by override, degenerate strings (x = 1, r - 1, roots of unity) through every stage with the exceptional branch each
case reaches asserted from an integer mirror, the check over those strings and G1 / G2 chains in turn on one workspace:
tests/test_gpu_msm_g2_paths.py.
"""
import ctypes as C
import random

import numpy as np
import pytest

from util import R

pytestmark = pytest.mark.gpu

SRS_INDEX, BAD_ENCODING, INVALID_ARG = 2, 3, 7
R3, R4 = 8, 16
SEED = bytes(range(100, 132))
D_SLAB = (1 << 19) + 3


def window_bits(n):
    return min(16, max(4, n.bit_length() - 1 - 4))


def trapdoor(d):
    pyr = random.Random(7000 * d + 18)
    return pyr.randrange(2, R), pyr.randrange(2, R)


class Str:
    """one honest string of d, made once, with the exponents' scalars k_e of both G2 bases (index e + d)"""

    def __init__(self, sonic, d):
        self.d, self.n = d, 2 * d + 1
        self.x, self.alpha = trapdoor(d)
        self.srs = sonic.SRS.new(d, self.x, self.alpha)
        xinv = pow(self.x, -1, R)
        neg, pos = [1], [1]
        for _ in range(d):
            neg.append(neg[-1] * xinv % R)
            pos.append(pos[-1] * self.x % R)
        self.k0 = neg[:0:-1] + pos
        self._k1 = None

    def k(self, basis):
        if basis == 0:
            return self.k0
        if self._k1 is None:
            self._k1 = [v * self.alpha % R for v in self.k0]
        return self._k1

    def want(self, basis, e0, scalars):
        """the 192 bytes of sum_i scalars[i] H_basis[e0 + i]"""
        from oracle import pairing as pr
        from sonic_amd import encoding as enc
        ks = self.k(basis)
        total = sum(s * ks[e0 + self.d + i] for i, s in enumerate(scalars)) % R
        return enc.g2_to_bytes(pr.g2_mul(pr.G2_GEN, total) if total else None)


_STRINGS = {}


@pytest.fixture
def string(sonic):
    def get(d):
        if d not in _STRINGS:
            _STRINGS[d] = Str(sonic, d)
        return _STRINGS[d]
    return get


def scalars_of(seed, n):
    pyr = random.Random(seed)
    return [pyr.randrange(R) for _ in range(n)]


# ---- correct sums -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("basis", (0, 1))
@pytest.mark.parametrize("d,n", [(300, 1), (300, 2), (300, 63), (300, 64), (300, 65), (300, 601), (8200, 16401)])
def test_sums_over_both_bases_at_every_size(sonic, string, d, n, basis):
    s = string(d)
    sc = scalars_of(31 * n + basis, n)
    assert sonic.msm_g2_srs(s.srs, basis, -d, sc) == s.want(basis, -d, sc)


@pytest.mark.parametrize("basis", (0, 1))
def test_a_range_from_a_negative_to_a_positive_exponent(sonic, string, basis):
    s = string(300)
    sc = scalars_of(77 + basis, 20)
    got = sonic.msm_g2_srs(s.srs, basis, -7, sc)
    assert got == s.want(basis, -7, sc) != bytes(192)
    assert got != sonic.msm_g2_srs(s.srs, basis, -8, sc)


def test_resident_scalars_give_the_host_scalar_sum(sonic, string):
    from sonic_amd import _lib, encoding as enc
    s = string(300)
    n = 601
    sc = scalars_of(5, n)
    arr = enc.fr_array(sc)
    L = _lib.lib()
    dp = C.c_void_p()
    _lib.check(L.sonic_dev_alloc(32 * n, C.byref(dp)))
    try:
        _lib.check(L.sonic_dev_upload(dp, arr.ctypes.data, 32 * n))
        got = sonic.msm_g2_srs(s.srs, 1, -300, (dp, n))
    finally:
        L.sonic_dev_free(dp)
    assert got == sonic.msm_g2_srs(s.srs, 1, -300, sc) == s.want(1, -300, sc)


@pytest.mark.parametrize("n", (1, 65, 601))
def test_caller_points_give_the_sum_over_the_string(sonic, string, n):
    s = string(300)
    sc = scalars_of(900 + n, n)
    pts = s.srs.g2_points(0, -300, n)
    assert sonic.msm_g2(pts, sc) == sonic.msm_g2_srs(s.srs, 0, -300, sc) == s.want(0, -300, sc)


# ---- boundary scalars ---------------------------------------------------------------------------------------------------------------------
N_B = 65
C_B = window_bits(N_B)                  # 4: 64 windows over 255 or 256 bits
W_B = -(-255 // C_B)
SPECIAL = {
    "0": 0, "1": 1, "r-1": R - 1, "(r-1)/2": (R - 1) // 2, "(r+1)/2": (R + 1) // 2,
    "2^c-1": (1 << C_B) - 1, "2^(c-1)": 1 << (C_B - 1),           # where the signed digit carries
    "2^128-1": (1 << 128) - 1, "2^128": 1 << 128, "2^254": 1 << 254,
    "every digit 1": sum(1 << (C_B * w) for w in range(W_B)),    # all of it in bucket 1 of every window
    "top window only": 3 << (C_B * (W_B - 1)),
}


def boundary_vectors():
    pyr = random.Random(65)
    mixed = list(SPECIAL.values()) + [pyr.randrange(R) for _ in range(N_B - len(SPECIAL))]
    out = {"mixed": mixed, "zeros": [0] * N_B}
    for name, v in SPECIAL.items():
        out["all " + name] = [v] * N_B
    # carries that run through every window: digits all 2^c - 1
    out["all ones up to 2^252"] = [(1 << 252) - 1] * N_B
    return out


BOUNDARY = boundary_vectors()


@pytest.mark.parametrize("name", sorted(BOUNDARY))
def test_boundary_scalars_folded_over_the_string_and_literal_over_caller_points(sonic, string, name):
    assert C_B == 4 and SPECIAL["every digit 1"] < (R - 1) // 2 and SPECIAL["top window only"] < (R - 1) // 2
    s = string(300)
    sc = BOUNDARY[name]
    want = s.want(1, -20, sc)
    assert sonic.msm_g2_srs(s.srs, 1, -20, sc) == want                      # 255 bits, scalars above (r-1)/2 folded
    assert sonic.msm_g2(s.srs.g2_points(1, -20, N_B), sc) == want           # 256 bits, nothing folded
    if name in ("zeros", "all 0"):
        assert want == bytes(192)


# ---- chunked walks ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("distinct", (1, 2))
def test_a_bucket_longer_than_the_walk_bound_is_cut_into_chunks(sonic, string, distinct):
    from sonic_amd import _lib
    wm = _lib.lib().sonic_msm_g2_walk_max()
    assert 1 <= wm <= 5000
    n = 3 * wm + 5
    s = string(8200)
    assert n <= s.n
    vals = scalars_of(4242, distinct)
    sc = [vals[i % distinct] for i in range(n)]           # equal scalars: every window has one bucket (or two) with all the entries
    for basis in (0, 1):
        assert sonic.msm_g2_srs(s.srs, basis, -8200, sc) == s.want(basis, -8200, sc)
    # exactly the bound, and one more
    for m in (wm, wm + 1):
        assert sonic.msm_g2_srs(s.srs, 0, -3, sc[:m]) == s.want(0, -3, sc[:m])


# ---- cancellation and doubling inside a bucket --------------------------------------------------------------------------------------------
def g2_bytes_array(points):
    from sonic_amd import encoding as enc
    return np.frombuffer(b"".join(enc.g2_to_bytes(p) for p in points), np.uint8).reshape(-1, 192)


def literal_mul(pr, p, k):
    """k p by double-and-add over the integer k itself: no reduction modulo r"""
    acc = None
    for bit in bin(k)[2:] if k else "":
        acc = pr.g2_add(acc, acc)
        if bit == "1":
            acc = pr.g2_add(acc, p)
    return acc


def literal_sum(pr, terms):
    acc = None
    for p, k in terms:
        acc = pr.g2_add(acc, literal_mul(pr, p, k))
    return acc


def neg(pr, p):
    return None if p is None else (p[0], pr.f2_neg(p[1]))


@pytest.mark.parametrize("k", (1, 5, R - 1, 0x1234567890ABCDEF1234567890ABCDEF))
def test_equal_and_opposite_points_in_one_bucket(sonic, k):
    from oracle import pairing as pr
    from sonic_amd import encoding as enc
    P = pr.g2_mul(pr.G2_GEN, 0xFACE)
    T = pr.g2_mul(pr.G2_GEN, 0xBEEF)
    cases = {"P+P": [P, P], "P-P": [P, neg(pr, P)], "P+P-P": [P, P, neg(pr, P)], "P-P+P+T": [P, neg(pr, P), P, T],
             "infinity among finite ones": [P, None, T, None], "only infinity": [None, None]}
    for name, pts in cases.items():
        want = enc.g2_to_bytes(literal_sum(pr, [(p, k) for p in pts if p is not None]))
        assert sonic.msm_g2(g2_bytes_array(pts), [k] * len(pts)) == want, name
    assert sonic.msm_g2(g2_bytes_array([P, neg(pr, P)]), [k, k]) == bytes(192)


# ---- literal multiples outside the subgroup -----------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def cofactor_point():
    """a point of the twist outside the order-r subgroup: the first small x whose right-hand side is a square"""
    from oracle import pairing as pr
    from sonic_amd import encoding as enc
    for x0 in range(1, 64):
        try:
            p = enc.g2_decompress(enc.g2_compress(((x0, 0), (0, 0))))
        except Exception:
            continue
        assert pr.g2_on_curve(p)
        if literal_mul(pr, p, R) is not None:
            return p
    raise AssertionError("no small x gives a point outside the subgroup")


def test_points_outside_the_subgroup_get_the_literal_multiple(sonic, cofactor_point):
    from oracle import pairing as pr
    from sonic_amd import encoding as enc
    P = cofactor_point
    S = pr.g2_mul(pr.G2_GEN, 0xC0DE)
    for k in (1, 2, R - 1, R - 2):
        assert sonic.msm_g2(g2_bytes_array([P]), [k]) == enc.g2_to_bytes(literal_mul(pr, P, k)), k
    assert literal_mul(pr, P, R - 1) != neg(pr, P)               # what a folding implementation would return
    mixed = [(P, 1), (S, R - 1), (P, R - 1), (S, 2), (P, 2), (P, R - 2), (S, (R + 1) // 2), (neg(pr, P), R - 1)]
    assert sonic.msm_g2(g2_bytes_array([p for p, _ in mixed]), [k for _, k in mixed]) == enc.g2_to_bytes(literal_sum(pr, mixed))


# ---- slab boundary ------------------------------------------------------------------------------------------------------------------------
def test_a_sum_across_the_slab_boundary(sonic):
    from sonic_amd import encoding as enc
    d, n = D_SLAB, (1 << 19) + 17
    s = Str(sonic, d)
    rs = np.random.default_rng(2019)
    arr = rs.integers(0, 256, size=(n, 32), dtype=np.uint8)
    arr[:, 31] &= 0x3F                                       # below 2^254 < r, on both sides of (r - 1) / 2
    sc = [int.from_bytes(row.tobytes(), "little") for row in arr]
    assert max(sc) > (R - 1) // 2
    for basis, e0 in ((0, -19), (1, d - n + 1)):             # up to d - 5, and up to d
        assert sonic.msm_g2_srs(s.srs, basis, e0, arr) == s.want(basis, e0, sc)
    assert enc.fr_array(sc[:3]).tobytes() == arr[:3].tobytes()


# ---- the check ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d", (12, 300, 8200))
def test_check_accepts_under_both_settings(string, monkeypatch, d):
    s = string(d)
    monkeypatch.setenv("SONIC_G2_MSM", "0")
    assert s.srs.check(SEED) == (True, 0)
    monkeypatch.delenv("SONIC_G2_MSM")
    assert s.srs.check(SEED) == (True, 0)


@pytest.mark.parametrize("which,mask", ((2, R3), (3, R4)))
def test_check_names_the_same_relation_under_both_settings(sonic, string, monkeypatch, which, mask):
    d = 300
    s = string(d)
    arrays = [s.srs.points(0, -d, s.n), s.srs.points(1, -d, s.n), s.srs.g2_points(0, -d, s.n), s.srs.g2_points(1, -d, s.n)]
    arrays[which] = arrays[which].copy()
    arrays[which][0] = arrays[which][1]                      # H[-d] := H[-d+1]: a term of B (R3) or of C (R4) and of nothing else
    bad = sonic.SRS.from_points(d, arrays[0], arrays[1])
    bad.set_g2_points(arrays[2], arrays[3])
    monkeypatch.setenv("SONIC_G2_MSM", "0")
    walk = bad.check(SEED)
    monkeypatch.delenv("SONIC_G2_MSM")
    assert bad.check(SEED) == walk == (False, mask)


def test_the_sums_of_the_check_are_the_msm_of_its_randomizers(sonic, string):
    import srs_update_ref as uref
    d = 300
    s = string(d)
    rho = [uref.rho(SEED, i) for i in range(s.n)]
    assert all(0 < v < 1 << 128 for v in rho)
    for basis in (0, 1):
        assert sonic.msm_g2_srs(s.srs, basis, -d, rho) == s.want(basis, -d, rho) != bytes(192)


# ---- refusals -----------------------------------------------------------------------------------------------------------------------------
def refused(sonic, code, call, *needles):
    with pytest.raises(sonic.SonicError) as e:
        call()
    assert e.value.code == code, (e.value.code, e.value.message)
    assert e.value.message, "a refusal carries a message"
    for needle in needles:
        assert needle in e.value.message, (needle, e.value.message)


def test_refusals_and_the_handle_afterwards(sonic, string):
    from sonic_amd import _lib, encoding as enc
    d = 300
    s = string(d)
    L = _lib.lib()
    out = C.create_string_buffer(192)
    sc = scalars_of(1, 4)
    arr = enc.fr_array(sc)
    pts = s.srs.g2_points(0, 0, 4)
    good = s.want(0, 0, sc)

    def after():
        assert sonic.msm_g2_srs(s.srs, 0, 0, sc) == good and sonic.msm_g2(pts, sc) == good

    # n = 0: infinity
    assert sonic.msm_g2_srs(s.srs, 0, 0, []) == bytes(192) and sonic.msm_g2(np.zeros((0, 192), np.uint8), []) == bytes(192)
    assert L.sonic_msm_g2_srs(s.srs._h, 0, d + 5, None, 0, out) == 0 and out.raw == bytes(192)
    # bad arguments
    for call in (lambda: L.sonic_msm_g2_srs(s.srs._h, 0, 0, arr.ctypes.data, -1, out), lambda: L.sonic_msm_g2_srs(None, 0, 0, arr.ctypes.data, 4, out),
                 lambda: L.sonic_msm_g2_srs(s.srs._h, 0, 0, None, 4, out), lambda: L.sonic_msm_g2_srs(s.srs._h, 0, 0, arr.ctypes.data, 4, None),
                 lambda: L.sonic_msm_g2_srs(s.srs._h, 2, 0, arr.ctypes.data, 4, out), lambda: L.sonic_msm_g2_srs_dev(s.srs._h, 0, 0, None, 4, out),
                 lambda: L.sonic_msm_g2(pts.ctypes.data, arr.ctypes.data, -1, out), lambda: L.sonic_msm_g2(None, arr.ctypes.data, 4, out),
                 lambda: L.sonic_msm_g2(pts.ctypes.data, None, 4, out), lambda: L.sonic_msm_g2(pts.ctypes.data, arr.ctypes.data, 4, None)):
        refused(sonic, INVALID_ARG, lambda: _lib.check(call()), "bad argument")
    after()
    # ranges outside [-d, d]: what sonic_msm_g1_srs answers for the same mistake
    with pytest.raises(sonic.SonicError) as g1:
        sonic.commitment.msm_g1_srs(s.srs, 0, d - 2, sc)
    assert g1.value.code == SRS_INDEX
    refused(sonic, SRS_INDEX, lambda: sonic.msm_g2_srs(s.srs, 0, d - 2, sc), "[%d, %d]" % (d - 2, d + 1))
    refused(sonic, SRS_INDEX, lambda: sonic.msm_g2_srs(s.srs, 1, -d - 1, sc), "[%d, %d]" % (-d - 1, -d + 2))
    after()
    # encodings
    big = arr.copy()                                                                       # (ints would be reduced on the way in)
    big[1] = np.frombuffer(R.to_bytes(32, "little"), np.uint8)
    refused(sonic, BAD_ENCODING, lambda: sonic.msm_g2_srs(s.srs, 0, 0, big), "non-canonical")
    big[1], big[3] = arr[1], np.frombuffer(((1 << 256) - 1).to_bytes(32, "little"), np.uint8)
    refused(sonic, BAD_ENCODING, lambda: sonic.msm_g2(pts, big), "non-canonical")
    bad = pts.copy()
    bad[2, :48] = np.frombuffer(enc.Q_MODULUS.to_bytes(48, "little"), np.uint8)            # x.c0 = q
    refused(sonic, BAD_ENCODING, lambda: sonic.msm_g2(bad, sc), "non-canonical")
    off = pts.copy()
    off[1, 96] ^= 1                                                                        # y.c0 moved: off the twist
    refused(sonic, BAD_ENCODING, lambda: sonic.msm_g2(off, sc), "twist")
    with pytest.raises(sonic.SonicError) as g1:                                            # the way sonic_msm_g1 refuses one
        sonic.msm_g1(np.ones((1, 96), np.uint8), [1])
    assert g1.value.code == BAD_ENCODING
    after()
    # a handle without a G2 half
    g1_only = sonic.SRS.from_points(d, s.srs.points(0, -d, s.n), s.srs.points(1, -d, s.n))
    assert not g1_only.has_g2()
    refused(sonic, INVALID_ARG, lambda: sonic.msm_g2_srs(g1_only, 0, 0, sc), "G2")
    after()


def test_a_view_serves_its_own_elements_and_nothing_else(sonic, string):
    from oracle import pairing as pr
    from sonic_amd import encoding as enc
    d, n = 300, 16
    s = string(d)
    view = s.srs.for_circuit(n, 2)
    k = 0xABCDEF0123456789
    held = {0: (n - d, 0), 1: (0, 1)}
    for basis, es in held.items():
        for e in es:
            elem = enc.g2_from_bytes(view.g2_points(basis, e, 1)[0].tobytes())
            assert sonic.msm_g2_srs(view, basis, e, [k]) == enc.g2_to_bytes(pr.g2_mul(elem, k)) == s.want(basis, e, [k])
    for basis, e, m in ((0, 1, 1), (0, n - d + 1, 1), (1, 2, 1), (1, 0, 2), (0, n - d, 2), (1, -1, 1)):
        refused(sonic, INVALID_ARG, lambda: sonic.msm_g2_srs(view, basis, e, [k] * m), "[%d, %d]" % (e, e + m - 1), "view")
    assert sonic.msm_g2_srs(view, 1, 1, [k]) == s.want(1, 1, [k])
