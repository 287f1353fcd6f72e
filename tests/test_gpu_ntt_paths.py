"""Every pass schedule, kernel build and table state of the Fr transform (sonic_amd/csrc/ntt.hip) behind sonic_ntt_fr and
sonic_poly_mul_fr[_dev] (poly_api.hip), by bytes against a reference that shares nothing with the kernels: the CPU oracle's transform
(orc.ntt), its schoolbook product (orc.poly_mul(use_ntt=False)), its NTT product at 2^20, and -- past what the oracle transforms in
seconds -- the copy identity a * (1 + X^e) = a + X^e a on a dense random a (ntt_paths_child.identity_operands), whose expected bytes
are copies of a and zeros.  Fr arithmetic is exact: no tolerance anywhere.

What ntt_run does with a transform of 2^L points (W = L - 11 wide stages, cut into ceil(W / 6) passes as even as possible), and the
cases that reach it.  [O] = against orc.ntt, [S] = against the schoolbook product, [N] = against the oracle's NTT product, [C] =
against the copied expectation; "down" / "up" / "mixed" are the orders of test_table_state, "builds" is
test_every_kernel_build_against_the_reference (the down order under each environment, then identity products at lg 16, 20, 21, 20).

  kernel            reached by
  k_ntt_small       L = 1 .. 10: dense_random_to_2p18 [O], extreme_inputs at 2, 5, 9, 10 [O], fused_product (2^1 .. 2^10) [S]
  k_ntt_local       L >= 11, default build: dense_random_to_2p18 11 .. 18 [O], dense_random_above_2p18 [O], copy_identity_product [C]
  k_ntt_local4      L >= 11 under SONIC_NTT_WAVES=2: builds [O, S, C]
  k_ntt_wide        L >= 12, default build: as k_ntt_local from 12
  k_ntt_wide4       L >= 12 under SONIC_NTT_WAVES=2: builds [O, C]
  k_ntt_wide_big    L = 20, 21 under SONIC_NTT_BIG=1 (nine, ten wide stages in one pass): builds, identity lg 20, 21, 20 [C]

  pass split        reached by
  1 .. 6 stages     L = 12 .. 17 in one pass: dense_random_to_2p18 [O]; fused_product at 2^12, 2^13 [S]; down, up, mixed [O]
  4 + 3             L = 18: dense_random_to_2p18 [O], extreme_inputs [O], down, up, mixed [O]
  4 + 4             L = 19: dense_random_above_2p18, both directions [O]
  5 + 4             L = 20: dense_random_above_2p18, both directions [O]; dense_product_2p20 [N]; builds, identity lg 20 [C]
  5 + 5             L = 21: dense_random_above_2p18, forward [O]; copy_identity_product lg 21 (forward twice, fused inverse) [C]
  6 + 5             L = 22: copy_identity_product lg 22 [C]
  6 + 6             L = 23: copy_identity_product lg 23 [C]
  5 + 4 + 4         L = 24: copy_identity_product lg 24 [C]

  tile loops        k_ntt_local walks several tiles per workgroup from 2^22 points, k_ntt_wide several blocks from 2^23:
                    copy_identity_product lg 22 .. 24 [C]; under SONIC_NTT_GRID=3 (5 with WAVES=2) both loop from 2^14 / 2^15 points:
                    builds [O at 14 .. 18, C at 2^16, 2^20, 2^21]

  tw_shift          0: up (every call regrows the tables) [O, S, C], mixed (18 and the first 12) [O]
                    non-zero: down (18 - L for every L below 18, the products, identity lg 16) [O, S, C], mixed (12, 5, 11 after 18) [O],
                    builds (identity lg 20 after 21: k_ntt_wide_big and 5 + 4 under a shift of 1) [C]

  fused product     (mul != nullptr in the inverse transform's first local stage)
                    k_ntt_small: fused_product 2^1 .. 2^10 [S]; k_ntt_local: fused_product 2^12, 2^13 [S], dense_product_2p20 [N],
                    copy_identity_product [C]; k_ntt_local4: builds, products 2^12, 2^13 [S] and identities [C]

The in-process cases run in whatever table state the tests before them left (a -k selection changes it); the table states themselves
are pinned by the fresh child processes of tests/ntt_paths_child.py.  Children run one at a time; after one that does not return 0 (an
abort, a fault, a time limit) no further child is started."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import ntt_paths_child as ch
from util import R

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
CHILD = os.path.join(HERE, "ntt_paths_child.py")
BAD_ENCODING, INVALID_ARG = 3, 7
TOP = np.frombuffer((R - 1).to_bytes(32, "little"), np.uint8)
ONE = np.frombuffer((1).to_bytes(32, "little"), np.uint8)


# ---- references, computed once ----------------------------------------------------------------------------------------------------------
_NTT_REF = {}


def ntt_ref(orc, log2n):
    """(input, forward transform, inverse transform) of the dense random input of 2^log2n points; the oracle runs once per size"""
    if log2n not in _NTT_REF:
        a = ch.ntt_input(log2n)
        _NTT_REF[log2n] = (a, orc.ntt(a, False), orc.ntt(a, True))
        for v in _NTT_REF[log2n]:
            v.setflags(write=False)
    return _NTT_REF[log2n]


_MUL_REF = {}


def mul_ref(orc, kind, na, nb):
    """(a, b, schoolbook product) of the operands the child uses for (kind, na, nb)"""
    if (kind, na, nb) not in _MUL_REF:
        a, b = (ch.product_operands if kind == "mul" else ch.edge_operands)(na, nb)
        _MUL_REF[kind, na, nb] = (a, b, orc.poly_mul(a, b, use_ntt=False))
    return _MUL_REF[kind, na, nb]


_IDENT_DIGEST = {}


def ident_digest(lg):
    if lg not in _IDENT_DIGEST:
        a, _, e = ch.identity_operands(lg)
        _IDENT_DIGEST[lg] = ch.digest_pieces(ch.identity_pieces(a, e))
    return _IDENT_DIGEST[lg]


def expected_lines(orc, order, sizes, identity):
    """what the child prints for (order, sizes, identity), with the oracle's digests"""
    want = []
    for log2n in sizes:
        _, fwd, inv = ntt_ref(orc, log2n)
        want.append("%s ntt %d 0 %s" % (order, log2n, ch.digest_pieces([fwd])))
        want.append("%s ntt %d 1 %s" % (order, log2n, ch.digest_pieces([inv])))
    for kind, pairs in (("mul", ch.PRODUCTS), ("edge", ch.EDGE_PRODUCTS)):
        for na, nb in pairs:
            want.append("%s %s %d %d %s" % (order, kind, na, nb, ch.digest_pieces([mul_ref(orc, kind, na, nb)[2]])))
    for lg in identity:
        want.append("%s ident %d %s" % (order, lg, ident_digest(lg)))
    return want


def run_ntt(data, log2n, inverse):
    from sonic_amd import _lib
    got = np.array(data, np.uint8, copy=True, order="C")
    _lib.check(_lib.lib().sonic_ntt_fr(got.ctypes.data, log2n, inverse))
    return got


def run_mul(a, b, fill=None):
    from sonic_amd import _lib
    na, nb = a.shape[0], b.shape[0]
    out = np.zeros((na + nb - 1, 32), np.uint8) if fill is None else np.full((na + nb - 1, 32), fill, np.uint8)
    _lib.check(_lib.lib().sonic_poly_mul_fr(a.ctypes.data, na, b.ctypes.data, nb, out.ctypes.data))
    return out


def first_difference(got, want):
    rows = np.flatnonzero((got != want).any(axis=1))
    return None if rows.size == 0 else (int(rows[0]), int(rows.size))


# ---- 1. sizes and schedules against the oracle -------------------------------------------------------------------------------------------
def test_product_shapes_hit_the_sizes_they_claim():
    """the (na, nb) lists of ntt_paths_child: a pair that fills and a pair just past the previous power of two, per transform size"""
    sizes = (1, 2, 4, 5, 6, 7, 9, 10, 12, 13)
    assert [ch.transform_log2(*p) for p in ch.PRODUCTS] == [k for k in sizes for _ in (0, 1)]
    for k, full, padded in zip(sizes, ch.PRODUCTS[::2], ch.PRODUCTS[1::2]):
        assert sum(full) - 1 == 1 << k and sum(padded) - 1 == (1 << (k - 1)) + 1
    assert [ch.transform_log2(*p) for p in ch.EDGE_PRODUCTS] == [10, 12] and [sum(p) - 1 for p in ch.EDGE_PRODUCTS] == [1 << 10, 1 << 12]


@pytest.mark.parametrize("log2n", range(19))
def test_dense_random_to_2p18(sonic, orc, log2n):
    """every size from one point to the first two-pass schedule: k_ntt_small at 1 .. 10 (at 2, two butterflies under 512 threads),
    one tile at 11, one pass of 1 .. 6 wide stages at 12 .. 17, 4 + 3 at 18"""
    a, fwd, inv = ntt_ref(orc, log2n)
    for inverse, want in ((0, fwd), (1, inv)):
        assert first_difference(run_ntt(a, log2n, inverse), want) is None, (log2n, inverse)


def _extreme(name, n):
    a = np.zeros((n, 32), np.uint8)
    if name == "all_top":
        a[:] = TOP
    elif name == "even_top":
        a[::2] = TOP
    elif name == "odd_top_even_one":
        a[1::2] = TOP
        a[::2] = ONE
    elif name == "half_block":
        a[: n // 2] = TOP
    elif name == "last_only":
        a[n - 1] = TOP
    else:
        a[(np.arange(n) // 1024) % 2 == 1] = TOP          # (all zero below 2^11 points)
    return a


@pytest.mark.parametrize("name", ["all_top", "even_top", "odd_top_even_one", "half_block", "last_only", "blocks_1024"])
@pytest.mark.parametrize("log2n", [2, 5, 9, 10, 18])
def test_extreme_inputs(sonic, orc, log2n, name):
    """the inputs of test_gpu_parity.test_ntt_extreme_inputs (all r - 1, zeros and r - 1 alternating, half blocks, one element, blocks of
    1024) through the C++ butterflies of k_ntt_small and through the first two-pass schedule, whose passes hand lazy values in [0, 2r)
    to each other"""
    a = _extreme(name, 1 << log2n)
    for inverse in (0, 1):
        assert first_difference(run_ntt(a, log2n, inverse), orc.ntt(a, bool(inverse))) is None, (log2n, name, inverse)


@pytest.mark.parametrize("log2n,inverse", [(19, 0), (19, 1), (20, 0), (20, 1), (21, 0)])
def test_dense_random_above_2p18(sonic, orc, log2n, inverse):
    """dense data beside the oracle where the suite had three-term inputs only: 4 + 4, 5 + 4 and 5 + 5 wide stages (2^21 is the last
    size the oracle transforms in a second or two, and it does so forward only here)"""
    a = ch.ntt_input(log2n)
    want = orc.ntt(a, bool(inverse))
    assert first_difference(run_ntt(a, log2n, inverse), want) is None, (log2n, inverse)


def _identity_overlap_case():
    """a * (1 + X^e) with e < na: the two copies overlap (no product of this module needs it; the branch of identity_pieces stays honest)"""
    a = ch.rand_fr(77, 300)
    b = np.zeros((120, 32), np.uint8)
    b[0, 0] = b[119, 0] = 1
    return a, b, 119


def test_copy_identity_matches_the_oracle(orc):
    """the expectation itself, before a GPU sees it (CPU only): the copied pieces are the oracle's product at lg = 16, filled and padded,
    and where the copies overlap"""
    for a, b, e in (ch.identity_operands(16), ch.identity_operands(16, padded=True), _identity_overlap_case()):
        assert b.shape[0] == e + 1 and np.flatnonzero(b.any(axis=1)).tolist() == [0, e]
        want = np.concatenate(ch.identity_pieces(a, e))
        assert want.shape[0] == a.shape[0] + e
        assert np.array_equal(want, orc.poly_mul(a, b, use_ntt=True))
    assert ch.transform_log2(1 << 14, ch.identity_operands(16)[2] + 1) == 16 == ch.transform_log2(1 << 14, ch.identity_operands(16, True)[2] + 1)
    assert ident_digest(16) == ch.digest_pieces([orc.poly_mul(*ch.identity_operands(16)[:2], use_ntt=True)])


@pytest.mark.parametrize("padded", [False, True], ids=["filled", "padded"])
@pytest.mark.parametrize("lg", [21, 22, 23, 24])
def test_copy_identity_product(sonic, lg, padded):
    """two forward transforms and the fused inverse on dense data through every stage of 5 + 5, 6 + 5, 6 + 6 and 5 + 4 + 4 (from 2^22
    k_ntt_local, from 2^23 k_ntt_wide walk several tiles per workgroup): a is dense, the transform of b = 1 + X^e is dense, and all
    na + e output coefficients are compared with copies of a and zeros"""
    a, b, e = ch.identity_operands(lg, padded)
    na = a.shape[0]
    assert ch.transform_log2(na, e + 1) == lg and na + e == ((1 << (lg - 1)) + 1 if padded else 1 << lg)
    out = run_mul(a, b, fill=0xA5)
    del b
    at = 0
    for piece in ch.identity_pieces(a, e):
        m = piece.shape[0]
        assert first_difference(out[at:at + m], piece) is None, (lg, padded, at)
        at += m
    assert at == out.shape[0]


@pytest.mark.parametrize("na,nb", ch.PRODUCTS)
def test_fused_product_matches_schoolbook(sonic, orc, na, nb):
    """the product folded into the inverse transform's first load, in k_ntt_small (2^1 .. 2^10) and k_ntt_local (2^12, 2^13), at the
    transform sizes test_gpu_parity.test_poly_mul_matches_schoolbook leaves out; per size one pair that fills the transform and one
    just past the previous power of two"""
    a, b, want = mul_ref(orc, "mul", na, nb)
    assert first_difference(run_mul(a, b, fill=0xA5), want) is None, (na, nb)


@pytest.mark.parametrize("na,nb", ch.EDGE_PRODUCTS)
def test_fused_product_all_r_minus_1(sonic, orc, na, nb):
    """every coefficient r - 1, at 2^10 (C++ butterflies) and 2^12 (generated butterflies, one wide stage)"""
    a, b, want = mul_ref(orc, "edge", na, nb)
    assert first_difference(run_mul(a, b, fill=0xA5), want) is None, (na, nb)


def test_dense_product_2p20(sonic, orc):
    """dense x dense at 2^20 (5 + 4 wide stages, forward and fused inverse) against the oracle's own NTT product"""
    a, b = ch.rand_fr(20, 1 << 19), ch.rand_fr(21, 1 << 19)
    want = orc.poly_mul(a, b, use_ntt=True)
    assert first_difference(run_mul(a, b, fill=0xA5), want) is None


def test_dev_product_reuses_its_scratch(sonic):
    """sonic_poly_mul_fr_dev keeps its two scratch arrays in the device context and only ever grows them: small products after large
    ones (2^14, 2^3, 2^11, 2^0, 2^14) run in scratch that still holds the earlier product, and must give sonic_poly_mul_fr's bytes"""
    from sonic_amd import _lib
    L = _lib.lib()
    for na, nb in [(9000, 7385), (3, 5), (1025, 1024), (1, 1), (5000, 7000)]:
        a, b = ch.rand_fr(3 * na + nb, na), ch.rand_fr(5 * na + nb, nb)
        rl = na + nb - 1
        want = run_mul(a, b)
        poison = np.full((rl, 32), 0xA5, np.uint8)
        ptrs = [C.c_void_p(), C.c_void_p(), C.c_void_p()]
        try:
            for p, arr in zip(ptrs, (a, b, poison)):
                _lib.check(L.sonic_dev_alloc(arr.size, C.byref(p)))
                _lib.check(L.sonic_dev_upload(p, arr.ctypes.data, arr.size))
            _lib.check(L.sonic_poly_mul_fr_dev(ptrs[0], na, ptrs[1], nb, ptrs[2]))
            got = np.zeros((rl, 32), np.uint8)
            _lib.check(L.sonic_dev_download(got.ctypes.data, ptrs[2], got.size))
        finally:
            for p in ptrs:
                if p.value:
                    L.sonic_dev_free(p)
        assert first_difference(got, want) is None, (na, nb)


# ---- refusals ---------------------------------------------------------------------------------------------------------------------------
BAD_VALUES = [R, R + 1, (1 << 256) - 1]


def _with(arr, pos, value):
    out = arr.copy()
    out[pos] = np.frombuffer(value.to_bytes(32, "little"), np.uint8)
    return out


@pytest.mark.parametrize("log2n", [3, 12])
def test_ntt_refuses_non_canonical_elements(sonic, orc, log2n):
    """r, r + 1 and 2^256 - 1 at the first or the last position: SONIC_ERR_BAD_ENCODING in both directions, the caller's buffer as it
    was, and the next correct call gives the oracle's bytes"""
    from sonic_amd import _lib
    L = _lib.lib()
    a, fwd, inv = ntt_ref(orc, log2n)
    for value in BAD_VALUES:
        for pos in (0, (1 << log2n) - 1):
            for inverse in (0, 1):
                bad = _with(a, pos, value)
                buf = bad.copy()
                assert L.sonic_ntt_fr(buf.ctypes.data, log2n, inverse) == BAD_ENCODING, (hex(value), pos, inverse)
                assert np.array_equal(buf, bad), (hex(value), pos, inverse)
            assert first_difference(run_ntt(a, log2n, 0), fwd) is None
    assert first_difference(run_ntt(a, log2n, 1), inv) is None


@pytest.mark.parametrize("na,nb", [(3, 5), (2000, 2097)], ids=["2p3", "2p12"])
def test_poly_mul_refuses_non_canonical_elements(sonic, orc, na, nb):
    """the same elements in either operand of sonic_poly_mul_fr: SONIC_ERR_BAD_ENCODING, operands and output buffer as they were"""
    from sonic_amd import _lib
    L = _lib.lib()
    a, b = ch.rand_fr(na, na), ch.rand_fr(nb, nb)
    want = orc.poly_mul(a, b, use_ntt=False)
    for value in BAD_VALUES:
        for which in (0, 1):
            for last in (False, True):
                ops = [a, b]
                ops[which] = _with(ops[which], ops[which].shape[0] - 1 if last else 0, value)
                before = [ops[0].copy(), ops[1].copy()]
                out = np.full((na + nb - 1, 32), 0xA5, np.uint8)
                rc = L.sonic_poly_mul_fr(ops[0].ctypes.data, na, ops[1].ctypes.data, nb, out.ctypes.data)
                assert rc == BAD_ENCODING, (hex(value), which, last)
                assert np.array_equal(ops[0], before[0]) and np.array_equal(ops[1], before[1]) and (out == 0xA5).all(), (hex(value), which, last)
        assert first_difference(run_mul(a, b, fill=0xA5), want) is None
    assert first_difference(run_mul(a, b), want) is None


def test_invalid_arguments(sonic, orc):
    """na = 0, nb = 0, negative counts and null pointers: SONIC_ERR_INVALID_ARG before anything is read or written"""
    from sonic_amd import _lib
    L = _lib.lib()
    a, b = ch.rand_fr(1, 3), ch.rand_fr(2, 5)
    out = np.full((7, 32), 0xA5, np.uint8)
    pa, pb, po = a.ctypes.data, b.ctypes.data, out.ctypes.data
    for args in [(pa, 0, pb, 5, po), (pa, 3, pb, 0, po), (pa, -1, pb, 5, po), (pa, 3, pb, -2, po), (None, 3, pb, 5, po), (pa, 3, None, 5, po), (pa, 3, pb, 5, None)]:
        assert L.sonic_poly_mul_fr(*args) == INVALID_ARG, args
    assert (out == 0xA5).all()
    assert L.sonic_ntt_fr(None, 3, 0) == INVALID_ARG and L.sonic_ntt_fr(None, 0, 1) == INVALID_ARG
    da = C.c_void_p()
    _lib.check(L.sonic_dev_alloc(32 * 8, C.byref(da)))
    try:
        for args in [(da, 0, da, 5, da), (da, 3, da, 0, da), (None, 3, da, 5, da), (da, 3, None, 5, da), (da, 3, da, 5, None)]:
            assert L.sonic_poly_mul_fr_dev(*args) == INVALID_ARG, args
    finally:
        L.sonic_dev_free(da)
    assert first_difference(run_mul(a, b), orc.poly_mul(a, b, use_ntt=False)) is None
    x, fwd, _ = ntt_ref(orc, 3)
    assert first_difference(run_ntt(x, 3, 0), fwd) is None


# ---- 2. table state, 3. kernel builds: fresh child processes ----------------------------------------------------------------------------
_CHILD_TROUBLE = []
NTT_KNOBS = ("SONIC_NTT_WAVES", "SONIC_NTT_GRID", "SONIC_NTT_BIG")


def run_child(order, sizes, identity, extra, timeout):
    """one child, on its own time limit; after a child that did not return 0 none is started"""
    assert not _CHILD_TROUBLE, "an earlier child did not return 0, nothing more is started on the GPU: %s" % _CHILD_TROUBLE
    env = {k: v for k, v in os.environ.items() if k not in NTT_KNOBS}
    env.update(extra)
    cmd = [sys.executable, CHILD, order, ",".join(map(str, sizes)), ",".join(map(str, identity)) or "-"]
    try:
        out = subprocess.run(cmd, capture_output=True, text=True, timeout=timeout, env=env)
    except subprocess.TimeoutExpired:
        _CHILD_TROUBLE.append((order, extra, "time limit"))
        raise
    if out.returncode != 0:
        _CHILD_TROUBLE.append((order, extra, out.returncode))
    assert out.returncode == 0 and out.stdout.endswith("ntt_paths_child ok\n"), (order, extra, out.returncode, out.stdout[-1500:], out.stderr[-3000:])
    return out.stdout.splitlines()[:-1]


def check_lines(got, want, extra):
    assert len(got) == len(want), (extra, len(got), len(want))
    wrong = [" ".join(w.split()[:-1]) for g, w in zip(got, want) if g != w]          # order, call, size (and direction)
    assert not wrong, (extra, wrong)


@pytest.mark.parametrize("order", list(ch.ORDERS))
def test_table_state(orc, order):
    """down: 2^18 first, then every smaller size through the 2^18 table (tw_shift = 18 - log2n in every kernel); up: every call frees and
    rebuilds the tables; mixed: the same size before and after a regrowth.  Then the schoolbook-sized products and one copy identity
    at 2^16, in the table state the transforms left"""
    sizes = ch.ORDERS[order]
    want = expected_lines(orc, order, sizes, [16])
    check_lines(run_child(order, sizes, [16], {}, 120), want, {})


BUILDS = [{}, {"SONIC_NTT_WAVES": "2"}, {"SONIC_NTT_GRID": "3"}, {"SONIC_NTT_WAVES": "2", "SONIC_NTT_GRID": "5"}, {"SONIC_NTT_BIG": "1"}]


@pytest.mark.parametrize("extra", BUILDS, ids=lambda e: "-".join("%s%s" % (k[10:].lower(), v) for k, v in e.items()) or "default")
def test_every_kernel_build_against_the_reference(orc, extra):
    """the environments of test_gpu_configs.test_ntt_kernel_variants_agree, each against the oracle and the copied expectation instead
    of against each other: the down order (every size to 2^18, shifted tables), the products, and the copy identity at lg 16, 20, 21
    and 20 again -- the sizes SONIC_NTT_BIG=1 sends through k_ntt_wide_big, the last one through the table of 2^21.  With
    SONIC_NTT_GRID=3 every wide and local kernel walks its tile loop from 2^14 / 2^15 points on.  (One case per environment: the five
    children in one case took 11.5 s.  run_child is what stops the sequence: after a child that did not return 0 the remaining cases
    fail before they start one.)"""
    sizes, identity = ch.ORDERS["down"], [16, 20, 21, 20]
    check_lines(run_child("down", sizes, identity, extra, 120), expected_lines(orc, "down", sizes, identity), extra)
