"""Circuit-sized SRS views (sonic_srs_for_circuit, sonic_srs_load_for_circuit; sonic_amd/csrc/srs_view.hpp): a second kind of SRS handle
that holds only the exponent windows a circuit of (n, Q) touches, with tables sized for those windows and the window width of a string
of d = 8n.  The same d, the same Fiat-Shamir id, the same commitments and proofs: everything here is bit-exact -- against the whole
string's handle, against the C oracle, and through the trapdoor (tests/util.srs_exponent) -- and what a view does not hold is
SONIC_ERR_INVALID_ARG with its windows in the message, never a wrong point.

The shapes are the smallest where the plan of the view and of the whole string really differ, and where each geometry case occurs."""
import ctypes as C
import os
import random
import subprocess

import numpy as np
import pytest

from util import NCPU, R, circuit_arrays, fr_bytes, fr_ints, rand_fr_array, srs_exponent

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "tests", "host")
INVALID_ARG, SRS_INDEX = 7, 2

ROWS = {
    1: (1, 1, 12),                     # the minimum
    2: (2, 5, 16),                     # n + Q sets hi0
    3: (4, 20, 28),                    # merged windows
    4: (40, 2, 1 << 13),               # whole string c = 13 against view c = 9
    5: (300, 3, (1 << 15) + 3),        # c = 15 against c = 11
    6: (1000, 4, (1 << 16) + 17),      # both one chain per proof, different widths
}
# the window width srs_policy.hpp gives d (whole string) and 8n (view): floor(log2), at least 9, 2^15 .. 2^17 -> 15, 16, 16
WIDTHS = {1: (9, 9), 2: (9, 9), 3: (9, 9), 4: (13, 9), 5: (15, 11), 6: (16, 12)}


def _circuit(sonic, circ):
    return sonic.ArithCircuit(sonic.GateWeights(circ[0], circ[1], circ[2]), circ[3])


def _plan(srs, n):
    from sonic_amd import _lib
    c, w, sets = C.c_int(), C.c_int(), C.c_int()
    _lib.check(_lib.lib().sonic_msm_plan(srs._h, n, C.byref(c), C.byref(w), C.byref(sets)))
    return c.value, w.value, sets.value


def _host_windows(n, Q, d):
    subprocess.check_call(["make", "-C", HOST, "-f", "srs_view.mk", "-s", "srs_view_host"])
    out = subprocess.run([os.path.join(HOST, "srs_view_host")], input=f"geo {n} {Q} {d}\n", capture_output=True, text=True, timeout=60, check=True)
    return tuple(int(w) for w in out.stdout.split()[:4])


def _refused(sonic, code, call, *needles):
    """`call` raises SonicError `code`; every needle is in the message"""
    with pytest.raises(sonic.SonicError) as e:
        call()
    assert e.value.code == code, (e.value.code, e.value.message)
    for s in needles:
        assert str(s) in e.value.message, (s, e.value.message)
    return e.value.message


def _window_words(view):
    lo0, hi0, lo1, hi1 = view.windows
    return [f"[{lo0}, {hi0}]"] + ([f"[{lo1}, {hi1}]"] if hi1 >= lo1 else [])


class World:
    """one row: trapdoor, whole string, circuit, assignment, transcript, and the oracle's proof -- computed once"""

    def __init__(self, sonic, orc, ref, row):
        self.row = row
        self.n, self.Q, self.d = n, Q, d = ROWS[row]
        pyr = random.Random(7000 + row)
        self.x, self.alpha = pyr.randrange(2, R), pyr.randrange(2, R)
        self.full = sonic.SRS.new(d, self.x, self.alpha)
        self.circ, self.asg, enc = circuit_arrays(ref, pyr, n, Q)
        self.circuit = _circuit(sonic, self.circ)
        self.assignment = sonic.Assignment(*self.asg)
        self.tr_ints = [pyr.randrange(1, R) for _ in range(8 + 2 * Q)]
        self.tr = fr_bytes(self.tr_ints)
        o = orc.SRS(d, self.x, self.alpha, threads=NCPU)
        orc.set_mode(1, NCPU)
        self.want = orc.prove(o, n, Q, enc["wL"], enc["wR"], enc["wO"], enc["cs"], enc["aL"], enc["aR"], enc["aO"], self.tr, n >= 256)
        # (y, z, yzs) of the explicit transcript: blinders 0 .. 3, y, z, y_j, z_j, u, v
        t = self.tr_ints
        self.challenges = (t[4], t[5], [(t[6 + j], t[6 + Q + j]) for j in range(Q)])

    def prover(self, sonic, srs, prepare=False, circuit=None):
        p = sonic.Prover(srs, circuit or self.circuit, prepare=prepare)
        p.set_assignment(self.assignment)
        return p


_WORLDS = {}


@pytest.fixture
def world(sonic, orc, ref):
    def get(row):
        if row not in _WORLDS:
            _WORLDS[row] = World(sonic, orc, ref, row)
        return _WORLDS[row]
    return get


# ---- 1, 2. bytes ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("row", sorted(ROWS))
def test_a_view_proves_the_bytes_of_the_whole_string_and_of_the_oracle(sonic, orc, ref, row):
    w = World(sonic, orc, ref, row)               # (a world of its own: row 4 closes the whole string)
    n, Q = w.n, w.Q
    digest, seed = sonic.fs_circuit_digest(w.circuit), bytes(range(32))
    pf = w.prover(sonic, w.full)
    assert pf.prove_bytes(w.tr) == w.want
    full_fs = pf.prove_fs(digest, seed)
    pf.submit_fs(digest, seed)
    full_flight = pf.collect_fs()
    full_id = sonic.fs_srs_id(w.full)
    pf.close()
    view = w.full.for_circuit(n, Q)
    assert view.srsD == w.d and view.windows == _host_windows(n, Q, w.d)
    if row == 4:
        w.full.close()                             # the view owns copies of everything it holds
    assert sonic.fs_srs_id(view) == full_id
    for prepare in (True, False):
        p = w.prover(sonic, view, prepare)
        for _ in range(2):
            assert p.prove_bytes(w.tr) == w.want, prepare
        assert p.prove_fs(digest, seed) == full_fs, prepare
        p.submit_fs(digest, seed)
        assert p.collect_fs() == full_flight, prepare
        p.close()
    pr, _ = sonic.prove(view, w.assignment, w.circuit, transcript=w.tr_ints)
    assert pr.to_bytes() == w.want
    view.close()
    if row != 4:
        w.full.close()


# ---- 3. verification ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("row", [1, 3, 4])
def test_a_view_verifies(sonic, world, row):
    w = world(row)
    n, Q, d = w.n, w.Q, w.d
    view = w.full.for_circuit(n, Q)
    assert view.has_g2()
    p = w.prover(sonic, view)
    good = p.prove_bytes(w.tr)
    p.close()
    assert good == w.want
    bad = bytearray(good)
    bad[2 * 96] ^= 1                               # the evaluation a = r(z, 1), behind R and T: a flipped bit of a scalar
    y, z, yzs = w.challenges
    assert sonic.verify(view, w.circuit, sonic.Proof.from_bytes(good, Q), y, z, yzs) is True
    assert sonic.verify(view, w.circuit, sonic.Proof.from_bytes(bytes(bad), Q), y, z, yzs) is False
    v = sonic.Verifier(view, w.circuit)
    assert v.verify_batch([good, bytes(bad), good], [w.challenges] * 3, seed=bytes(range(32)), each=True) == (False, [True, False, True])
    assert v.verify_batch([good, good], [w.challenges] * 2, seed=bytes(range(32)), each=True) == (True, [True, True])
    v.close()
    assert view.srsPairing == w.full.srsPairing
    held = [(0, n - d), (0, 0), (1, 0), (1, 1)]
    for basis, e in held:
        assert view.g2_points(basis, e, 1).tobytes() == w.full.g2_points(basis, e, 1).tobytes(), (basis, e)
    for basis, e in [(0, 1), (0, -1), (0, n - d + 1), (1, -1), (1, 2), (1, n - d), (0, d), (1, -d)]:
        _refused(sonic, INVALID_ARG, lambda: view.g2_points(basis, e, 1), "not held", held[2 * basis][1], held[2 * basis + 1][1])
    _refused(sonic, INVALID_ARG, lambda: view.g2_points(1, 0, 2), "not held")
    _refused(sonic, SRS_INDEX, lambda: view.g2_points(0, d + 1, 1))
    _refused(sonic, SRS_INDEX, lambda: view.g2_points(0, -d - 1, 1))
    view.close()


# ---- 4. MSM and polynomial calls ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("row", [1, 4, 5])
def test_msms_and_polynomials_over_a_view(sonic, orc, world, row):
    from sonic_amd.commitment import msm_g1_srs
    w = world(row)
    n, Q, d = w.n, w.Q, w.d
    view = w.full.for_circuit(n, Q)
    lo0, hi0, lo1, hi1 = view.windows
    assert hi1 >= lo1 and hi0 + 1 < lo1
    rng = np.random.default_rng(row)
    gen = orc.g1_gen()
    ranges = [(lo0, hi0 - lo0 + 1), (lo1, hi1 - lo1 + 1), (-1, 3), (lo0, 1), (hi0, 1), (lo1, 1), (hi1, 1), (hi1 - 1, 2)]
    for basis in (0, 1):
        for e0, cnt in ranges:
            sc = rand_fr_array(rng, cnt)
            got = msm_g1_srs(view, basis, e0, sc)
            assert got == msm_g1_srs(w.full, basis, e0, sc), (basis, e0, cnt)
            assert got == orc.g1_mul(gen, srs_exponent(w.x, w.alpha, basis, e0, fr_ints(sc))), (basis, e0, cnt)
    words = _window_words(view)
    one = rand_fr_array(rng, lo1 - hi0 + 1)
    # across the gap, into it from either side, inside it
    for e0, cnt in [(hi0, lo1 - hi0 + 1), (hi0, 2), (lo1 - 1, 2), (hi0 + 1, 1), (lo0 - 1, 2)]:
        if e0 < -d:
            continue
        _refused(sonic, INVALID_ARG, lambda: msm_g1_srs(view, 1, e0, one[:cnt]), "not held", *words)
        _refused(sonic, INVALID_ARG, lambda: view.points(0, e0, cnt), "not held", *words)
    # beyond d: what it returns today
    with pytest.raises(sonic.SonicError) as full_err:
        msm_g1_srs(w.full, 0, d, one[:2])
    _refused(sonic, full_err.value.code, lambda: msm_g1_srs(view, 0, d, one[:2]))
    assert full_err.value.code == SRS_INDEX
    _refused(sonic, SRS_INDEX, lambda: view.points(1, -d - 1, 1))
    # points, table 0 and the diagnostics' window tables, are the whole string's where the view holds them
    for basis in (0, 1):
        for e0, cnt in ranges[:3]:
            assert view.points(basis, e0, cnt).tobytes() == w.full.points(basis, e0, cnt).tobytes()
    # commitPoly: max = d puts exponent e at e; a term inside each window commits as over the whole string, one in the gap is refused
    inside = {lo0 + 1: 5, -1: 7, hi0: 11}
    assert sonic.commit_poly(view, d, inside) == sonic.commit_poly(w.full, d, inside)
    high = {lo1: 3, hi1: 9}
    assert sonic.commit_poly(view, d, high) == sonic.commit_poly(w.full, d, high)
    _refused(sonic, INVALID_ARG, lambda: sonic.commit_poly(view, d, {hi0: 1, hi0 + 1: 2}), "not held", *words)
    _refused(sonic, INVALID_ARG, lambda: sonic.commit_poly(view, d, {hi0 + 1: 2}), "not held", *words)
    # openPoly reads the plain basis over the polynomial's own range
    f = {-2: 3, 0: 4, 3: 5}
    assert sonic.open_poly(view, 12345, f) == sonic.open_poly(w.full, 12345, f)
    _refused(sonic, INVALID_ARG, lambda: sonic.open_poly(view, 12345, {0: 1, hi0 + 2: 2}), "not held", *words)
    view.close()


# ---- 5. plan and memory ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("row", sorted(ROWS))
def test_plan_windows_and_memory(sonic, world, row):
    w = world(row)
    n, Q, d = w.n, w.Q, w.d
    view = w.full.for_circuit(n, Q)
    c_full, c_view = WIDTHS[row]
    assert _plan(w.full, n)[0] == c_full and _plan(w.full, n)[2] == 1
    assert _plan(view, n)[0] == c_view and _plan(view, n)[2] == 1 and _plan(view, 7 * n + 9)[0] == c_view
    assert view.windows == _host_windows(n, Q, d)
    assert w.full.windows == (-d, d, 1, 0)
    lo0, hi0, lo1, hi1 = view.windows
    npts = hi0 - lo0 + 1 + max(0, hi1 - lo1 + 1)
    pb = 128                                       # SONIC_SRS_POINT_BYTES
    W = lambda c: -(-255 // c)                     # noqa: E731
    assert w.full.device_bytes == pb * ((2 * d + 1) * (2 * W(c_full) + 1) + (d + 1) * W(c_full))
    assert view.device_bytes == pb * (npts * (2 * W(c_view) + 1) + (min(hi0, -lo0) + 1) * W(c_view))
    if row == 4:
        # by point count and window count the ratio is about 0.04: this fails on a view that kept the whole string's tables
        assert view.device_bytes <= w.full.device_bytes / 8
    view.close()


# ---- 6. files ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("compressed", [False, True])
def test_a_view_loaded_from_a_file(sonic, world, tmp_path, compressed):
    w = world(5)
    n, Q, d = w.n, w.Q, w.d
    path = str(tmp_path / "string.srs")
    w.full.save(path, g2=True, compressed=compressed)
    view = sonic.SRS.load(path, circuit=(n, Q))
    assert view.srsD == d and view.windows == w.full.for_circuit(n, Q).windows and view.has_g2()
    assert sonic.fs_srs_id(view) == sonic.fs_srs_id(w.full)
    p = w.prover(sonic, view)
    good = p.prove_bytes(w.tr)
    p.close()
    assert good == w.want
    y, z, yzs = w.challenges
    assert sonic.verify(view, w.circuit, sonic.Proof.from_bytes(good, Q), y, z, yzs) is True
    # a view is not a reference string
    for kw in (dict(), dict(compressed=True)):
        _refused(sonic, INVALID_ARG, lambda: view.save(str(tmp_path / "view.srs"), **kw), "view")
    assert not os.path.exists(str(tmp_path / "view.srs"))
    _refused(sonic, INVALID_ARG, lambda: view.set_g2_points(np.zeros((2 * d + 1, 192), np.uint8), np.zeros((2 * d + 1, 192), np.uint8)), "view")
    view.close()
    # the same file, one point short
    size = os.path.getsize(path)
    with open(path, "r+b") as f:
        f.truncate(size - (96 if compressed else 192))
    with pytest.raises(sonic.SonicError) as e:
        sonic.SRS.load(path, circuit=(n, Q))
    assert "truncated" in e.value.message
    # without a G2 half in the file: a view that proves and cannot verify, as any SRS without one
    w.full.save(path, g2=False, compressed=compressed)
    blind = sonic.SRS.load(path, circuit=(n, Q))
    assert not blind.has_g2()
    p = w.prover(sonic, blind, prepare=True)
    assert p.prove_bytes(w.tr) == w.want
    p.close()
    whole = sonic.SRS.load(path)
    with pytest.raises(sonic.SonicError) as whole_err:
        sonic.verify(whole, w.circuit, sonic.Proof.from_bytes(good, Q), y, z, yzs)
    _refused(sonic, whole_err.value.code, lambda: sonic.verify(blind, w.circuit, sonic.Proof.from_bytes(good, Q), y, z, yzs), "no G2 half")
    # ... and so is a view of a string that has none
    assert not whole.for_circuit(n, Q).has_g2()
    whole.close()
    blind.close()
    # a string too short for the circuit, and circuits that are none
    _refused(sonic, INVALID_ARG, lambda: sonic.SRS.load(path, circuit=(d // 7 + 1, 1)), d, 7 * (d // 7 + 1))
    _refused(sonic, INVALID_ARG, lambda: sonic.SRS.load(path, circuit=(0, 1)))
    _refused(sonic, INVALID_ARG, lambda: sonic.SRS.load(path, circuit=(1, 0)))


# ---- 7. containment ---------------------------------------------------------------------------------------------------------------------------
def test_views_of_views_smaller_circuits_and_replicas(sonic, orc, ref, world):
    w = world(4)
    n, Q, d = w.n, w.Q, w.d
    view = w.full.for_circuit(n, Q)
    words = _window_words(view)
    # a view of a view: (20, 2) lies inside (40, 2)
    pyr = random.Random(20)
    circ, asg, enc = circuit_arrays(ref, pyr, 20, 2)
    small = view.for_circuit(20, 2)
    assert small.windows == (-88, 60, d - 64, d)
    # its verifier would need h^{x^{20 - d}}, which a view for n = 40 does not hold: a source that cannot supply the four G2 elements
    # gives a view without a G2 half
    assert not small.has_g2()
    assert sonic.fs_srs_id(small) == sonic.fs_srs_id(w.full)
    o = orc.SRS(d, w.x, w.alpha, threads=NCPU)
    orc.set_mode(1, NCPU)
    want = orc.prove(o, 20, 2, enc["wL"], enc["wR"], enc["wO"], enc["cs"], enc["aL"], enc["aR"], enc["aO"], w.tr, False)
    for srs in (small, view):                      # ... and the smaller circuit proves under the larger view as well
        p = sonic.Prover(srs, _circuit(sonic, circ), prepare=False)
        p.set_assignment(sonic.Assignment(*asg))
        assert p.prove_bytes(w.tr) == want
        p.close()
    _refused(sonic, INVALID_ARG, lambda: sonic.Verifier(small, _circuit(sonic, circ)), "no G2 half")
    # a view's G2 half is for its own n: the whole string's view for n = 20 verifies that circuit, the view for n = 40 refuses the
    # verifier when it is made
    small.close()
    small = w.full.for_circuit(20, 2)
    assert small.has_g2()
    v = sonic.Verifier(small, _circuit(sonic, circ))
    t = w.tr_ints
    assert v.verify_batch([want], [(t[4], t[5], [(t[6], t[8]), (t[7], t[9])])], seed=bytes(range(32)), each=True) == (True, [True])
    v.close()
    _refused(sonic, INVALID_ARG, lambda: sonic.Verifier(view, _circuit(sonic, circ)), "not held")
    small.close()
    # (80, 2) does not: not as a view of the view, not as a prover over it
    _refused(sonic, INVALID_ARG, lambda: view.for_circuit(80, 2), "not held", *words)
    big, big_asg, _ = circuit_arrays(ref, pyr, 80, 2)
    _refused(sonic, INVALID_ARG, lambda: sonic.Prover(view, _circuit(sonic, big), prepare=False), "not held", *words)
    p = sonic.Prover(w.full, _circuit(sonic, big), prepare=False)          # (the whole string takes it)
    p.close()
    # n + Q' beyond hi0 = 3n = 120 although n' <= n
    wide, _, _ = circuit_arrays(ref, pyr, 40, 90)
    _refused(sonic, INVALID_ARG, lambda: sonic.Prover(view, _circuit(sonic, wide), prepare=False), "not held", *words)
    # the arguments
    _refused(sonic, INVALID_ARG, lambda: w.full.for_circuit(0, 1), "n = 0")
    _refused(sonic, INVALID_ARG, lambda: w.full.for_circuit(1, 0), "Q = 0")
    _refused(sonic, INVALID_ARG, lambda: w.full.for_circuit(d // 7 + 1, 1), d, 7 * (d // 7 + 1))
    tiny = sonic.SRS.new(11, 3, 5)
    _refused(sonic, INVALID_ARG, lambda: tiny.for_circuit(1, 1), 11, 12)
    tiny.close()
    # a replica of a view is a view
    rep = view.replicate(0)
    assert rep.windows == view.windows and rep.device_bytes == view.device_bytes and rep.has_g2()
    p = w.prover(sonic, rep)
    assert p.prove_bytes(w.tr) == w.want
    p.close()
    _refused(sonic, INVALID_ARG, lambda: rep.points(0, view.windows[1] + 1, 1), "not held", *words)
    rep.close()
    view.close()
