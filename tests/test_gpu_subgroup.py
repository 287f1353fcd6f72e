"""Subgroup membership on the GPU (include/sonic_hip.h, "Subgroup membership"; g1.hpp, g2.hpp): sonic_g1_subgroup_check and
sonic_g2_subgroup_check with both methods, and every loader, validator and decompressor that shares the endomorphism test.

THE YARDSTICK is tests/subgroup_ref.py: Python integers, which tests/test_subgroup_host.py pins to the definition r P = O on the same
adversarial sets -- points of small prime order, the generator plus such a point, [r](random point), random points without cofactor
clearing -- the inputs on which an endomorphism test could be unsound.  Every comparison is of bytes, bits or verdicts."""
import ctypes as C
import random

import numpy as np
import pytest

import subgroup_ref as sg
from sonic_amd import encoding as enc

pytestmark = pytest.mark.gpu

METHODS = ("endo", "walk")
INVALID_ARG, BAD_ENCODING = 7, 3


@pytest.fixture(scope="module")
def strings(sonic):
    """G1 and G2 points of two generated strings: d = 12 (every array of a handle) and d = 64 (129 points per basis)"""
    out = {}
    for d in (12, 64):
        s = sonic.SRS.new(d, 0x5eed + d, 0xa1fa + d)
        out[d] = dict(g0=s.points(0, -d, 2 * d + 1), g1=s.points(1, -d, 2 * d + 1), h0=s.g2_points(0, -d, 2 * d + 1), h1=s.g2_points(1, -d, 2 * d + 1))
        s.close()
    return out


def padded(cases, pad_rows, n, pinned, width):
    """n encodings: the adversarial cases named in `pinned` at the block boundaries 0, B - 1, B, n - 1, every other case spread between them,
    points of a generated string everywhere else"""
    rows = [bytes(pad_rows[i % len(pad_rows)]) for i in range(n)]
    B = 256 if width == 96 else 64
    at = [0, B - 1, B, n - 1]
    for i, name in zip(at, pinned):
        rows[i] = sg.case(cases, name)
    free = [i for i in range(1, n - 1, 3) if i not in at]
    others = [b for name, b, _ in cases if name not in pinned]
    assert len(others) <= len(free)
    for i, b in zip(free, others):
        rows[i] = b
    return rows


def as_array(rows, width):
    return np.frombuffer(b"".join(rows), np.uint8).reshape(-1, width).copy()


@pytest.fixture(scope="module")
def g1_input(strings):
    n = 2 * 256 + 3
    pad = [r for r in np.concatenate([strings[12]["g0"], strings[12]["g1"]]) if bytes(r) != bytes(96)]
    rows = padded(sg.g1_cases(), pad, n, ["G+T_11", "T_3", "G+T_52437899", "r*random"], 96)
    want = np.array([sg.g1_flag(b) for b in rows], np.uint8)
    assert set(want) == {0, 1, 2, 4}
    return rows, want


@pytest.fixture(scope="module")
def g2_input(strings):
    n = 2 * 64 + 3
    pad = list(np.concatenate([strings[12]["h0"], strings[12]["h1"]]))
    rows = padded(sg.g2_cases(), pad, n, ["H+T_13", "T_23", "H+T_262069", "H+r*random"], 192)
    want = np.array([sg.g2_flag(b) for b in rows], np.uint8)
    assert set(want) == {0, 1, 2, 4}
    return rows, want


# ---- 1, 2. the public calls, both methods ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("method", METHODS)
def test_g1_subgroup_check_gives_the_mirrors_flags(sonic, g1_input, method):
    rows, want = g1_input
    got = sonic.g1_subgroup_check(as_array(rows, 96), method=method)
    assert got.dtype == np.uint8 and got.shape == want.shape
    assert bytes(got) == bytes(want), [(i, int(g), int(w)) for i, (g, w) in enumerate(zip(got, want)) if g != w]
    for i in (0, 255, 256, len(rows) - 1):                 # the adversarial points at the block boundaries, one point per call
        assert want[i] == 4 and bytes(sonic.g1_subgroup_check(as_array(rows[i:i + 1], 96), method=method)) == b"\x04"
    assert bytes(sonic.g1_subgroup_check(as_array(rows[1:2], 96), method=method)) == bytes(want[1:2])
    assert sonic.g1_subgroup_check(np.zeros((0, 96), np.uint8), method=method).shape == (0,)


@pytest.mark.parametrize("method", METHODS)
def test_g2_subgroup_check_gives_the_mirrors_flags(sonic, g2_input, method):
    rows, want = g2_input
    got = sonic.g2_subgroup_check(as_array(rows, 192), method=method)
    assert got.dtype == np.uint8 and got.shape == want.shape
    assert bytes(got) == bytes(want), [(i, int(g), int(w)) for i, (g, w) in enumerate(zip(got, want)) if g != w]
    for i in (0, 63, 64, len(rows) - 1):
        assert want[i] == 4 and bytes(sonic.g2_subgroup_check(as_array(rows[i:i + 1], 192), method=method)) == b"\x04"
    assert bytes(sonic.g2_subgroup_check(as_array(rows[1:2], 192), method=method)) == bytes(want[1:2])
    assert sonic.g2_subgroup_check(np.zeros((0, 192), np.uint8), method=method).shape == (0,)


# ---- 3. every consumer gives the same verdicts on the same points ------------------------------------------------------------------------
def test_g1_validate_accepts_exactly_what_the_mirror_accepts(sonic, g1_input):
    from sonic_amd import _lib
    rows, want = g1_input
    a, fl = as_array(rows, 96), np.full(len(rows), 9, np.uint8)
    _lib.check(_lib.lib().sonic_g1_validate(a.ctypes.data, len(rows), fl.ctypes.data))
    assert bytes(fl) == bytes((want == 0).astype(np.uint8))


def test_decompressors_flag_exactly_the_points_outside_the_subgroup(sonic):
    for cases, flag, from_bytes, compress, decompress in ((sg.g1_cases(), sg.g1_flag, enc.g1_from_bytes, enc.g1_compress, sonic.g1_decompress),
                                                          (sg.g2_cases(), sg.g2_flag, enc.g2_from_bytes, enc.g2_compress, sonic.g2_decompress)):
        on_curve = [(name, b) for name, b, _ in cases if flag(b) in (0, 4)]
        z = np.frombuffer(b"".join(compress(from_bytes(b)) for _, b in on_curve), np.uint8)
        out, fl = decompress(z, check_subgroup=True, flags=True)
        want = [flag(b) for _, b in on_curve]
        assert 4 in want and 0 in want and list(fl) == want, [(n, int(g), w) for (n, _), g, w in zip(on_curve, fl, want) if g != w]
        for (name, b), row, w in zip(on_curve, out, want):      # an accepted point decodes to itself, a refused one to zeros
            assert bytes(row) == (b if w == 0 else bytes(len(b))), name
        _out, fl0 = decompress(z, check_subgroup=False, flags=True)
        assert not fl0.any()


def test_srs_loaders_refuse_a_generator_plus_a_small_order_point(sonic, strings):
    d = 12
    s = strings[d]
    good = sonic.SRS.from_points(d, s["g0"], s["g1"])
    good.set_g2_points(s["h0"], s["h1"])                       # the untouched string loads, both halves
    assert bytes(good.points(0, -d, 2 * d + 1)) == bytes(s["g0"]) and bytes(good.g2_points(1, -d, 2 * d + 1)) == bytes(s["h1"])
    good.close()
    bad_g = s["g0"].copy()
    bad_g[d + 3] = np.frombuffer(sg.case(sg.g1_cases(), "G+T_11"), np.uint8)
    with pytest.raises(sonic.SonicError, match="subgroup") as e:
        sonic.SRS.from_points(d, bad_g, s["g1"])
    assert e.value.code == BAD_ENCODING
    bad_h = s["h1"].copy()
    bad_h[5] = np.frombuffer(sg.case(sg.g2_cases(), "H+T_13"), np.uint8)
    g1only = sonic.SRS.from_points(d, s["g0"], s["g1"])
    with pytest.raises(sonic.SonicError, match="subgroup") as e:
        g1only.set_g2_points(s["h0"], bad_h)
    assert e.value.code == BAD_ENCODING
    g1only.close()


def test_verifiers_reject_a_proof_point_outside_the_subgroup(sonic, ref):
    from test_gpu_verify_batch import World, layout, put
    from sonic_amd import _lib
    n, Q, K = 2, 1, 3
    w = World(sonic, ref, n, Q, K)
    try:
        g1, _fr, _size = layout(Q)
        proofs = list(w.proofs)
        assert w.verifier(sonic, "dense").verify_batch(proofs, w.trs, seed=bytes(32), each=True) == (True, [True] * K)
        proofs[1] = put(proofs[1], g1[2], sg.case(sg.g1_cases(), "G+T_10177"))          # W_a
        assert w.verifier(sonic, "dense").verify_batch(proofs, w.trs, seed=bytes(32), each=True) == (False, [True, False, True])
        # sonic_verify refuses the encoding
        from sonic_amd.protocol import _circuit_args
        n_, Q_, suffix, args, _keep = _circuit_args(w.dense)
        y, z, yzs = w.trs[1]
        fr = lambda v: int(v).to_bytes(32, "little")      # noqa: E731
        ok = C.c_int(0)
        rc = getattr(_lib.lib(), "sonic_verify" + suffix)(w.srs._h, n_, Q_, *args, bytes(proofs[1]), fr(y), fr(z), b"".join(fr(a) + fr(b) for a, b in yzs), C.byref(ok))
        assert rc == BAD_ENCODING
        assert w.yard(sonic, proofs[0], w.trs[0]) is True
    finally:
        w.close()


# ---- 4. differential: the two methods against each other and against what is known by construction ---------------------------------------
def test_methods_agree_on_string_points_and_random_curve_points(sonic, strings):
    rng = random.Random(404)
    for width, inside, random_point, to_bytes, flag, check, m in (
            (96, strings[64]["g0"][:128], sg.g1_random_point, enc.g1_to_bytes, sg.g1_flag, sonic.g1_subgroup_check, 128),
            (192, strings[64]["h0"][:64], sg.g2_random_point, enc.g2_to_bytes, sg.g2_flag, sonic.g2_subgroup_check, 64)):
        rows = [(bytes(r), 0) for r in inside] + [(b, flag(b)) for b in (to_bytes(random_point(rng)) for _ in range(m))]
        assert len(rows) == 2 * m and sum(1 for _, f in rows[m:] if f == 4) >= m - 1        # a random point is outside but for a miracle
        rng.shuffle(rows)
        a = as_array([b for b, _ in rows], width)
        endo, walk = check(a, method="endo"), check(a, method="walk")
        assert bytes(endo) == bytes(walk) == bytes(f for _, f in rows)


# ---- 5. argument refusals ---------------------------------------------------------------------------------------------------------------------
def test_argument_refusals(sonic, g1_input, g2_input):
    from sonic_amd import _lib
    L = _lib.lib()
    for fn, rows, width in ((L.sonic_g1_subgroup_check, g1_input[0], 96), (L.sonic_g2_subgroup_check, g2_input[0], 192)):
        a, fl = as_array(rows[:4], width), np.full(4, 9, np.uint8)
        assert fn(a.ctypes.data, 4, 0, fl.ctypes.data) == 0 and fn(a.ctypes.data, 4, 1, fl.ctypes.data) == 0
        assert fn(None, 0, 0, None) == 0 and fn(None, 0, 1, None) == 0                 # n = 0 reads nothing
        for args in ((None, 4, 0, fl.ctypes.data), (a.ctypes.data, 4, 0, None), (a.ctypes.data, -1, 0, fl.ctypes.data),
                     (a.ctypes.data, (1 << 26) + 1, 0, fl.ctypes.data), (a.ctypes.data, 4, 2, fl.ctypes.data), (a.ctypes.data, 4, -1, fl.ctypes.data),
                     (None, 0, 2, None)):
            fl[:] = 9
            assert fn(*args) == INVALID_ARG, args
            assert "subgroup_check" in _lib.last_error() and bytes(fl) == b"\x09" * 4
    with pytest.raises(ValueError):
        sonic.g1_subgroup_check(np.zeros((1, 96), np.uint8), method="fast")
    with pytest.raises(ValueError):
        sonic.g2_subgroup_check(np.zeros((1, 192), np.uint8), method="")
