"""sonic_amd/csrc/srs_view.hpp says which exponents an SRS handle holds and where: the one window [-d, d] of a whole string, or the two
windows of a circuit-sized view -- low [-4n-8, max(3n, n+Q)], high [d-3n-4, d], merged where they touch.  A host program
(tests/host/srs_view_host.cpp, plain g++ and once more under ASan / UBSan) prints the geometry, the slots, the window width and the byte
ranges a view reads of both file containers; this file holds them against the exponents the literal restatement of the reference
(oracle/sonic_ref.prove) really asks its SRS for, and against values worked out by hand.  CPU only."""
import os
import random
import struct
import subprocess

import pytest

from oracle import sonic_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "tests", "host")

# (n, Q, d): tiny circuits under strings from the smallest that works to many times too large, Q below and above 2n
SHAPES = [(1, 1, 12), (1, 1, 40), (2, 5, 16), (2, 5, 100), (4, 8, 28), (4, 12, 28), (4, 20, 28), (5, 3, 35), (5, 3, 200), (8, 2, 56), (8, 2, 1000),
          (3, 30, 400)]


@pytest.fixture(scope="module", params=["srs_view_host", "srs_view_host_san"])
def ask(request):
    """ask(line) -> the words of the program's answer; the program built plain / under the sanitizers"""
    subprocess.check_call(["make", "-C", HOST, "-f", "srs_view.mk", "-s", request.param])
    env = {k: v for k, v in os.environ.items() if not k.startswith("SONIC_")}
    memo = {}

    def ask(line):
        if line not in memo:
            out = subprocess.run([os.path.join(HOST, request.param)], input=line + "\n", capture_output=True, text=True, timeout=60, env=env)
            assert out.returncode == 0 and not out.stderr, out.stdout[-2000:] + out.stderr[-3000:]
            memo[line] = out.stdout.split()
        return memo[line]
    return ask


def windows(ask, n, Q, d):
    lo0, hi0, lo1, hi1 = (int(w) for w in ask(f"geo {n} {Q} {d}")[:4])
    return (lo0, hi0), (lo1, hi1)


class RecordingSRS(ref.SRS):
    """every element prove asks for, as (basis, exponent); the group element itself is the empty sum: only the indices matter"""
    MAP = {"gNegativeX": (0, lambda k: -(k + 1)), "gPositiveX": (0, lambda k: k), "gNegativeAlphaX": (1, lambda k: -(k + 1)),
           "gPositiveAlphaX": (1, lambda k: k + 1)}

    def __init__(self, d):
        super().__init__(d, 3, 5)
        self.touched = set()

    def _get(self, name, k, length, scalar_fn):
        if not (0 <= k < length):
            raise IndexError(f"{name} is not long enough: {k} >= {length}")
        basis, exp = self.MAP[name]
        self.touched.add((basis, exp(k)))
        return ref.INF


_TOUCHED = {}


def touched(n, Q, d):
    if (n, Q, d) not in _TOUCHED:
        rng = random.Random(1000 * n + Q)
        circuit, assignment = ref.rnd_circuit(rng, n, Q)
        srs = RecordingSRS(d)
        ref.prove(srs, assignment, circuit, [rng.randrange(1, ref.R) for _ in range(8 + 2 * Q)])
        _TOUCHED[(n, Q, d)] = srs.touched
    return _TOUCHED[(n, Q, d)]


@pytest.mark.parametrize("n,Q,d", SHAPES)
def test_a_proof_touches_only_the_windows(ask, n, Q, d):
    (lo0, hi0), (lo1, hi1) = windows(ask, n, Q, d)
    got = touched(n, Q, d)
    assert len(got) > 7 * n
    for basis, e in got:
        in_low, in_high = lo0 <= e <= hi0, lo1 <= e <= hi1
        assert in_low or in_high, (basis, e)
        if basis == 0:
            # the plain basis never leaves the low window as the formulas give it (a merged window is wider)
            assert -4 * n - 8 <= e <= max(3 * n, n + Q), e
    # the windows are tight at their outer ends: t's lowest blinder and R's top coefficient are really read
    assert min(e for _, e in got) == lo0 and max(e for _, e in got) == (hi1 if hi1 >= lo1 else hi0)


@pytest.mark.parametrize("n,Q,d", SHAPES)
def test_the_windows_are_the_formulas(ask, n, Q, d):
    (lo0, hi0), (lo1, hi1) = windows(ask, n, Q, d)
    low, high = (-4 * n - 8, max(3 * n, n + Q)), (d - 3 * n - 4, d)
    if high[0] <= low[1] + 1:
        assert (lo0, hi0, lo1, hi1) == (low[0], high[1], 1, 0)
    else:
        assert (lo0, hi0, lo1, hi1) == (low[0], low[1], high[0], high[1])
    assert ask(f"need {n} {d}") == ["0"]


def test_merged_and_unmerged_and_the_d_rule(ask):
    assert windows(ask, 4, 20, 28) == ((-24, 28), (1, 0))
    # (4, 12, 28) merges as well: max(3n, n + Q) = 16 reaches past d - 3n - 4 = 12.  At d = 7n the high window starts at 4n - 4 and the
    # low one ends at 3n or later, so from n = 4 on every d = 7n merges; the unmerged forms are the small n and the large d
    assert windows(ask, 4, 12, 28) == ((-24, 28), (1, 0))
    assert windows(ask, 4, 8, 28) == ((-24, 28), (1, 0))            # touching: 12 and 12
    assert windows(ask, 1, 1, 12) == ((-12, 3), (5, 12))            # a gap of one exponent
    assert windows(ask, 2, 5, 16) == ((-16, 16), (1, 0))            # overlapping: 7 and 6
    assert windows(ask, 2, 5, 100) == ((-16, 7), (90, 100))
    assert windows(ask, 8, 2, 1000) == ((-40, 24), (972, 1000))
    # 7n <= d is not enough for tiny n: the blinders of t reach -4n - 8
    assert ask("need 1 7") == ["12"] and ask("need 1 11") == ["12"] and ask("need 1 12") == ["0"]
    assert ask("need 2 15") == ["16"] and ask("need 2 13") == ["14"] and ask("need 8 55") == ["56"] and ask("need 8 56") == ["0"]


@pytest.mark.parametrize("n,Q,d", SHAPES + [(0, 0, 12), (0, 0, 57)])
def test_slots_are_a_bijection_of_consecutive_runs(ask, n, Q, d):
    geo = [int(w) for w in ask(f"geo {n} {Q} {d}")]
    lo0, hi0, lo1, hi1, npts, centre, sym_n, full = geo
    pairs = [tuple(int(v) for v in w.split(":")) for w in ask(f"slots {n} {Q} {d}")]
    assert [e for e, _ in pairs] == list(range(-d, d + 1))
    held = [(e, s) for e, s in pairs if s >= 0]
    assert sorted(s for _, s in held) == list(range(npts))
    assert {e for e, _ in held} == set(range(lo0, hi0 + 1)) | set(range(lo1, hi1 + 1))
    slot = dict(held)
    for e, s in held:
        if e + 1 in slot and not (e == hi0 and hi1 >= lo1):
            assert slot[e + 1] == s + 1
    if hi1 >= lo1:
        assert slot[lo1] == slot[hi0] + 1          # the high window follows the low one
    assert slot[0] == centre == -lo0
    assert sym_n == min(hi0, -lo0) + 1
    if n == 0:
        assert full == 1 and all(s == e + d for e, s in pairs) and npts == 2 * d + 1 and sym_n == d + 1
    else:
        assert full == (1 if (lo0, hi0, lo1, hi1) == (-d, d, 1, 0) else 0)          # (2, 5, 16): the merged window is all of [-d, d]


def test_contains_rejects_what_crosses_the_gap(ask):
    n, Q, d = 8, 2, 1000                      # [-40, 24] and [972, 1000]
    yes = [(-40, 65), (-40, 1), (24, 1), (972, 29), (1000, 1), (0, 0), (500, 0), (-3, 10)]
    no = [(-41, 2), (24, 2), (25, 1), (500, 1), (971, 2), (971, 1), (1000, 2), (-40, 1041), (20, 960)]
    for e0, cnt in yes:
        assert ask(f"contains {n} {Q} {d} {e0} {cnt}") == ["1"], (e0, cnt)
    for e0, cnt in no:
        assert ask(f"contains {n} {Q} {d} {e0} {cnt}") == ["0"], (e0, cnt)
    assert ask("contains 0 0 1000 -1000 2001") == ["1"] and ask("contains 0 0 1000 -1001 2") == ["0"]


# floor(log2 8n) -> c by srs_policy.hpp's rule, W = ceil(255 / c), c = ceil(255 / W): worked out by hand
@pytest.mark.parametrize("n,c,W", [(1, 9, 29), (40, 9, 29), (300, 11, 24), (1 << 12, 15, 17), (1 << 18, 20, 13)])
def test_the_width_is_the_policys_at_8n(ask, n, c, W):
    assert [int(w) for w in ask(f"width {n}")] == [c, W, c, W]


def parse_ranges(words):
    return int(words[0]), [tuple(int(v) for v in w.split(":")) for w in words[1:]]


@pytest.mark.parametrize("z", [0, 1])
@pytest.mark.parametrize("g2", [0, 1])
@pytest.mark.parametrize("n,Q,d", [(1, 1, 12), (4, 20, 28), (8, 2, 1000), (1 << 12, 2, 1 << 21)])
def test_file_ranges_lie_inside_the_file(ask, z, g2, n, Q, d):
    total, ranges = parse_ranges(ask(f"ranges {z} {g2} {n} {Q} {d}"))
    p1, p2, cnt = (48, 96, 2 * d + 1) if z else (96, 192, 2 * d + 1)
    assert total == 24 + 2 * cnt * p1 + (2 * cnt * p2 if g2 else 0)
    (lo0, hi0), (lo1, hi1) = windows(ask, n, Q, d)
    want = []
    for b in range(2):
        want.append((b, lo0, hi0 - lo0 + 1, 24 + (b * cnt + lo0 + d) * p1, (hi0 - lo0 + 1) * p1))
        if hi1 >= lo1:
            want.append((b, lo1, hi1 - lo1 + 1, 24 + (b * cnt + lo1 + d) * p1, (hi1 - lo1 + 1) * p1))
    if g2:
        base = 24 + 2 * cnt * p1
        want += [(2 + b, e, 1, base + (b * cnt + e + d) * p2, p2) for b, e in ((0, n - d), (0, 0), (1, 0), (1, 1))]
    assert ranges == want
    for _, _, _, off, size in ranges:
        assert 24 <= off and off + size <= total


def write_file(path, z, g2, d, cut=0, extra=0, header_d=None):
    """a container whose point i of vector v starts with the u32 v << 24 | i (the reader does not look inside points)"""
    p1, p2, cnt = (48, 96, 2 * d + 1) if z else (96, 192, 2 * d + 1)
    body = bytearray()
    for v in range(4 if g2 else 2):
        for i in range(cnt):
            body += struct.pack("<I", v << 24 | i) + bytes((p1 if v < 2 else p2) - 4)
    head = (b"SONICSRZ" if z else b"SONICSRS") + struct.pack("<IIq", 1 if z else 2, 1 if g2 else 0, d if header_d is None else header_d)
    with open(path, "wb") as f:
        f.write(head + bytes(body[:len(body) - cut]) + bytes(extra))


@pytest.mark.parametrize("z", [0, 1])
@pytest.mark.parametrize("g2", [0, 1])
def test_the_reader_takes_the_windows_and_refuses_a_header_that_disagrees_with_the_file(ask, tmp_path, z, g2):
    n, Q, d = 2, 5, 40                       # [-16, 7] and [30, 40]
    path = str(tmp_path / f"s{z}{g2}.bin")
    write_file(path, z, g2, d)
    words = [int(w) for w in ask(f"read {path} {n} {Q}")]
    exps = list(range(-16, 8)) + list(range(30, 41))
    assert words[:5] == [0, z, g2, d, len(exps)]
    want = [b << 24 | (e + d) for b in range(2) for e in exps]
    if g2:
        want += [2 << 24 | (n - d + d), 2 << 24 | d, 3 << 24 | d, 3 << 24 | (d + 1)]
    assert words[5:] == want
    # one point short, one byte long, a header that promises another d: refused by the size check, before anything of the body is read
    for name, kw in (("cut", dict(cut=96 if not z else 48)), ("extra", dict(extra=1)), ("d", dict(header_d=d + 1)), ("dsmall", dict(header_d=d - 1))):
        bad = str(tmp_path / f"{name}{z}{g2}.bin")
        write_file(bad, z, g2, d, **kw)
        assert ask(f"read {bad} {n} {Q}") == ["3"], name
    # a string too short for the circuit, a file that is no container, a file that is not there
    assert ask(f"read {path} 6 1") == ["4"]
    junk = str(tmp_path / f"junk{z}{g2}.bin")
    with open(junk, "wb") as f:
        f.write(b"SONICSRX" + bytes(40))
    assert ask(f"read {junk} {n} {Q}") == ["2"]
    assert ask(f"read {tmp_path / 'absent'} {n} {Q}") == ["1"]
