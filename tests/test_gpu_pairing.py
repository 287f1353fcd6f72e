"""Pairings on the GPU (include/sonic_hip.h, "Pairing"; pairing.hip): sonic_pairing_check with where = GPU against where = HOST and
against oracle/pairing.py.  The host and the device compile one copy of the formulas, so every comparison is of bytes or verdicts.
Points come from a generated string of d = 12 and from the adversarial sets of tests/subgroup_ref.py."""
import numpy as np
import pytest

import pairing_ref as pref
import subgroup_ref as sg
from oracle import pairing as pr
from oracle import sonic_ref as ref
from sonic_amd import encoding as enc

pytestmark = pytest.mark.gpu

INVALID_ARG = 7
WHERES = ("gpu", "host")


@pytest.fixture(scope="module")
def string(sonic):
    d = 12
    s = sonic.SRS.new(d, 0x5eed + d, 0xa1fa + d)
    out = dict(g0=s.points(0, -d, 2 * d + 1), g1=s.points(1, -d, 2 * d + 1), h0=s.g2_points(0, -d, 2 * d + 1), h1=s.g2_points(1, -d, 2 * d + 1))
    from sonic_amd import _lib
    import ctypes as C
    buf = C.create_string_buffer(576)
    _lib.check(_lib.lib().sonic_srs_pairing(s._h, buf))
    out["srs_pairing"] = buf.raw
    s.close()
    out["G1"] = [bytes(r) for r in np.concatenate([out["g0"], out["g1"]]) if bytes(r) != bytes(96)]
    out["G2"] = [bytes(r) for r in np.concatenate([out["h0"], out["h1"]])]
    return out


def arr(rows, width):
    return np.frombuffer(b"".join(rows), np.uint8).reshape(-1, width).copy() if rows else np.zeros((0, width), np.uint8)


def ends(sizes):
    return np.cumsum(np.array(sizes, np.int64)).astype(np.int64)


def test_gt_bytes_gpu_equal_host_over_uneven_groups(sonic, string):
    """328 pairs in groups of 0, 1, 2, 3, 5, 17, 0, 300: several blocks of 64 threads and three passes of the product"""
    sizes = [0, 1, 2, 3, 5, 17, 0, 300]
    n = sum(sizes)
    g1 = arr([string["G1"][(7 * i + 1) % len(string["G1"])] for i in range(n)], 96)
    g2 = arr([string["G2"][(5 * i + 3) % len(string["G2"])] for i in range(n)], 192)
    vg, tg = sonic.pairing_check(g1, g2, ends(sizes), where="gpu", gt=True)
    vh, th = sonic.pairing_check(g1, g2, ends(sizes), where="host", gt=True)
    assert vg.tolist() == vh.tolist() == [0, 1, 1, 1, 1, 1, 0, 1]
    for g in range(len(sizes)):
        assert tg[g].tobytes() == th[g].tobytes(), g
    assert tg[0].tobytes() == tg[6].tobytes() == pref.GT_ONE
    assert len({tg[g].tobytes() for g in range(len(sizes))}) == 7
    # without the values: the same verdicts
    assert sonic.pairing_check(g1, g2, ends(sizes), where="gpu").tolist() == vg.tolist()


@pytest.fixture(scope="module")
def one_groups(string):
    """groups that are one by construction: (a_i P, Q) ... (-(sum a_i) P, Q); pair indices 0, 63, 64 and n - 1 lie in groups 0, 2, 3, 5"""
    sizes = [3, 59, 2, 2, 4, 3]
    assert sum(sizes[:2]) == 62 and sum(sizes) == 73
    P = ref.G1_GEN
    rows1, rows2, scalars = [], [], []
    for g, m in enumerate(sizes):
        a = [1000 * g + 17 * i + 2 for i in range(m - 1)]
        a.append(-sum(a))
        scalars += a
        rows1 += [enc.g1_to_bytes(ref.g1_mul(P, x % pref.R)) for x in a]
        rows2 += [string["G2"][(3 * g + 1) % len(string["G2"])]] * m
    return sizes, rows1, rows2, scalars


@pytest.mark.parametrize("where", WHERES)
def test_groups_that_are_one_and_one_changed_scalar(sonic, one_groups, where):
    sizes, rows1, rows2, scalars = one_groups
    n = len(rows1)
    v, t = sonic.pairing_check(arr(rows1, 96), arr(rows2, 192), ends(sizes), where=where, gt=True)
    assert v.tolist() == [0] * len(sizes)
    assert all(t[g].tobytes() == pref.GT_ONE for g in range(len(sizes)))
    bad = list(rows1)
    for i in (0, 63, 64, n - 1):
        bad[i] = enc.g1_to_bytes(ref.g1_mul(ref.G1_GEN, (scalars[i] + 1) % pref.R))
    v, t = sonic.pairing_check(arr(bad, 96), arr(rows2, 192), ends(sizes), where=where, gt=True)
    assert v.tolist() == [1, 0, 1, 1, 0, 1]
    assert all((t[g].tobytes() == pref.GT_ONE) == (v[g] == 0) for g in range(len(sizes)))


def test_one_pair_equals_the_oracle_cubed_and_the_srs_pairing(sonic, string):
    """gt is oracle.pairing(P, Q) cubed.  sonic_srs_pairing is the textbook value e = 1 / f_{|x|}^((q^12 - 1) / r) (verify.hip), and gt is
    f_{|x|}^(3 (q^12 - 1) / r) = e^-3: the two are held together through that relation -- 1 / gt^(1/3 mod r) must be sonic_srs_pairing's
    bytes -- since as bytes e and e^-3 differ"""
    a, b = 0x1234567, 5
    P, Q = ref.g1_mul(ref.G1_GEN, a), pr.g2_mul(pr.G2_GEN, b)
    want = pref.oracle_value(((P, Q),))
    for where in WHERES:
        assert sonic.pairing(enc.g1_to_bytes(P), enc.g2_to_bytes(Q), where=where) == want, where
    g, h_alpha = bytes(string["g0"][12]), bytes(string["h1"][12])          # g^{x^0}, h^{alpha x^0}
    assert g == enc.g1_to_bytes(ref.G1_GEN)
    gt = sonic.pairing(g, h_alpha, where="gpu")
    assert gt == sonic.pairing(g, h_alpha, where="host")
    root = pr.f12_pow(pref.gt_from_bytes(gt), pow(3, -1, pref.R))
    assert pref.gt_bytes(pr.f12_inv(root)) == string["srs_pairing"]
    assert pref.gt_bytes(pref.cube(pr.f12_inv(pref.gt_from_bytes(string["srs_pairing"])))) == gt


@pytest.mark.parametrize("where", WHERES)
def test_infinity_in_either_slot_contributes_one(sonic, string, where):
    P, Q, Q2 = string["G1"][3], string["G2"][4], string["G2"][9]
    rows1 = [bytes(96), P, bytes(96), P, bytes(96), P]
    rows2 = [Q, bytes(192), bytes(192), Q, Q2, Q]
    v, t = sonic.pairing_check(arr(rows1, 96), arr(rows2, 192), [1, 2, 3, 5, 6], where=where, gt=True)
    assert v.tolist() == [0, 0, 0, 1, 1]
    assert t[0].tobytes() == t[1].tobytes() == t[2].tobytes() == pref.GT_ONE
    assert t[3].tobytes() == t[4].tobytes() != pref.GT_ONE          # (P, Q) (O, Q2) is (P, Q)


def test_flags_of_bad_points_and_the_other_groups_untouched(sonic, string):
    c1, c2 = sg.g1_cases(), sg.g2_cases()
    bad1 = {2: sg.case(c1, "x+q"), 4: sg.case(c1, "off-curve"), 8: sg.case(c1, "G+T_11")}
    bad2 = {2: sg.case(c2, "coordinate 3 + q"), 4: sg.case(c2, "off-twist"), 8: sg.case(c2, "H+T_13")}
    sizes = [2, 3, 1, 2, 4, 2, 3]
    n = sum(sizes)
    rows1 = [string["G1"][(2 * i + 5) % len(string["G1"])] for i in range(n)]
    rows2 = [string["G2"][(3 * i + 2) % len(string["G2"])] for i in range(n)]
    clean = {w: sonic.pairing_check(arr(rows1, 96), arr(rows2, 192), ends(sizes), where=w, gt=True) for w in WHERES}
    assert clean["gpu"][0].tolist() == clean["host"][0].tolist() == [1] * len(sizes)
    e = [0] + list(np.cumsum(sizes))
    b1, b2 = list(rows1), list(rows2)
    b1[e[0]] = bad1[2]; b1[e[2] - 1] = bad1[4]; b1[e[3]] = bad1[8]              # groups 0, 1, 3: one bad G1 point each
    b2[e[4]] = bad2[2]; b2[e[4] + 1] = bad2[4]; b1[e[4] + 2] = bad1[8]          # group 4: three kinds at once
    b2[e[6] + 1] = bad2[8]                                                      # group 6: a G2 point outside the subgroup
    want = [2, 4, 1, 8, 2 | 4 | 8, 1, 8]
    for w in WHERES:
        v, t = sonic.pairing_check(arr(b1, 96), arr(b2, 192), ends(sizes), where=w, gt=True)
        assert v.tolist() == want, w
        for g, x in enumerate(want):
            assert t[g].tobytes() == (clean[w][1][g].tobytes() if x == 1 else bytes(576)), (w, g)
    with pytest.raises(ValueError):
        sonic.pairing(bad1[8], rows2[0], where="gpu")


def test_empty_call_and_argument_errors(sonic, string):
    import ctypes as C
    from sonic_amd import _lib
    z1, z2 = np.zeros((0, 96), np.uint8), np.zeros((0, 192), np.uint8)
    for w in WHERES + ("auto",):
        assert sonic.pairing_check(z1, z2, [0, 0, 0], where=w).tolist() == [0, 0, 0]
        assert sonic.pairing_check(z1, z2, [], where=w).tolist() == []
    g1, g2 = arr(string["G1"][:4], 96), arr(string["G2"][:4], 192)
    for ge in ([2, 1, 4], [1, 2, 3], [1, 5], [-1, 4]):
        with pytest.raises(sonic.SonicError) as err:
            sonic.pairing_check(g1, g2, ge, where="gpu")
        assert err.value.code == INVALID_ARG and "sonic_pairing_check" in err.value.message and "group_end" in err.value.message
    L = _lib.lib()
    v, ge = np.zeros(1, np.uint8), np.array([4], np.int64)
    for args in ((None, g2.ctypes.data, 4, ge.ctypes.data, 1, 2, v.ctypes.data, None), (g1.ctypes.data, None, 4, ge.ctypes.data, 1, 2, v.ctypes.data, None),
                 (g1.ctypes.data, g2.ctypes.data, 4, None, 1, 2, v.ctypes.data, None), (g1.ctypes.data, g2.ctypes.data, 4, ge.ctypes.data, 1, 2, None, None),
                 (g1.ctypes.data, g2.ctypes.data, 4, ge.ctypes.data, 1, 3, v.ctypes.data, None), (g1.ctypes.data, g2.ctypes.data, -1, ge.ctypes.data, 1, 2, v.ctypes.data, None),
                 (g1.ctypes.data, g2.ctypes.data, 4, ge.ctypes.data, 0, 2, v.ctypes.data, None)):
        assert L.sonic_pairing_check(*args) == INVALID_ARG, args
        assert "sonic_pairing_check" in _lib.last_error()
    # auto gives what both give
    assert sonic.pairing_check(g1, g2, [4], where="auto").tolist() == sonic.pairing_check(g1, g2, [4], where="gpu").tolist() == [1]


def test_auto_takes_the_device_from_256_groups(sonic, monkeypatch):
    """PAIRING_GPU_MIN_GROUPS = 256 (pairing_device.hpp), seen through the profiler: k_final_exp runs for 256 (empty) groups and not for
    255; SONIC_PAIRING_GPU = 0 / 1 turns either round"""
    import ctypes as C
    from sonic_amd import _lib
    L = _lib.lib()
    z1, z2 = np.zeros((0, 96), np.uint8), np.zeros((0, 192), np.uint8)

    def final_exps(G):
        L.sonic_profile_enable(1)
        try:
            L.sonic_profile_reset()
            assert sonic.pairing_check(z1, z2, [0] * G, where="auto").tolist() == [0] * G
            cnt = C.c_int64(0)
            L.sonic_profile_get(b"k_final_exp", None, C.byref(cnt))
            return cnt.value
        finally:
            L.sonic_profile_reset()
            L.sonic_profile_enable(0)
    monkeypatch.delenv("SONIC_PAIRING_GPU", raising=False)
    assert final_exps(256) == 1 and final_exps(255) == 0 and final_exps(1) == 0
    monkeypatch.setenv("SONIC_PAIRING_GPU", "0")
    assert final_exps(256) == 0
    monkeypatch.setenv("SONIC_PAIRING_GPU", "1")
    assert final_exps(1) == 1
