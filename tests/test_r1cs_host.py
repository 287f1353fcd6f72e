"""R1CS front end, the parts that need no GPU (include/sonic_hip.h, "R1CS front end").  The mapping's own properties on the Python-integer
model (tests/r1cs_ref.py); the validation and the layouts of sonic_amd/csrc/r1cs.hpp, driven through a stand-alone program built plain and
under ASan / UBSan (tests/host/r1cs_host.cpp) and compared byte for byte with the model; the iden3 containers of sonic_amd/r1cs_io.py."""
import os
import random
import subprocess

import pytest

import r1cs_ref as ref
from r1cs_ref import R

HERE = os.path.dirname(os.path.abspath(__file__))
HOST = os.path.join(HERE, "host")
ENV = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
INVALID_ARG, BAD_ENCODING = 7, 3


def small_systems(count=200, seed=0x51C5):
    rng = random.Random(seed)
    for _ in range(count):
        m = rng.randrange(1, 13)
        N = rng.randrange(1, 14)
        n_pub = rng.randrange(0, min(3, N - 1) + 1)
        yield rng, m, N, n_pub, ref.random_r1cs(rng, m, N, n_pub)


# ---- the model's own properties ----
def test_shape_nnz_and_column_order():
    for rng, m, N, n_pub, (A, B, C, z) in small_systems():
        n, Q, g = ref.shape(m, N, n_pub)
        assert n == m + N // 2 and Q == 3 * m + n_pub and g == N // 2
        rows, cs = ref.compile_r1cs(m, N, n_pub, A, B, C)
        assert len(rows) == 3 * Q and len(cs) == Q
        assert sum(len(r) for r in rows) == ref.nnz_formula(m, n_pub, A, B, C)
        for r in rows:
            cols = [c for c, _ in r]
            assert all(0 <= c < n for c in cols) and all(a < b for a, b in zip(cols, cols[1:]))
            assert all(0 <= v < R for _, v in r)
        assert all(v == 0 for v in cs[3 * m:])


def test_honest_assignment_satisfies_and_one_changed_variable_breaks_exactly_when_it_should():
    for rng, m, N, n_pub, (A, B, C, z) in small_systems():
        n, Q, g = ref.shape(m, N, n_pub)
        rows, _ = ref.compile_r1cs(m, N, n_pub, A, B, C)
        aL, aR, aO, cs, bad = ref.assign(m, N, n_pub, A, B, C, z)
        assert ref.r1cs_holds(A, B, C, z) and bad == (0, -1)
        assert len(aL) == len(aR) == len(aO) == n
        assert ref.sonic_holds(Q, rows, cs, aL, aR, aO)
        if N == 1:
            continue
        j = rng.randrange(1, N)
        z2 = list(z)
        z2[j] = (z[j] + rng.randrange(1, R)) % R
        bL, bR, bO, _, bad2 = ref.assign(m, N, n_pub, A, B, C, z2)
        still = ref.r1cs_holds(A, B, C, z2)
        assert ref.sonic_holds(Q, rows, cs, bL, bR, bO) == (still and j > n_pub)
        # an unsatisfied row is a broken multiplication gate of the same index
        broken = [i for i in range(m) if ref.dot(A[i], z2) * ref.dot(B[i], z2) % R != ref.dot(C[i], z2)]
        assert bad2 == (len(broken), broken[0] if broken else -1)


def test_explicit_zeros_stay_entries_and_column_zero_goes_to_the_constants():
    A = [[(0, 5), (1, 0), (2, 7)]]
    B = [[(2, 0)]]
    C = [[]]
    rows, cs = ref.compile_r1cs(1, 3, 1, A, B, C)
    Q = 4
    assert rows[0] == [(0, 1), (1, 0)] and rows[Q + 0] == [(1, (R - 7) % R)]      # wL, wR of row 0: variable 1 at (L, gate 1), 2 at (R, gate 1)
    assert rows[1] == [] and rows[Q + 1] == [(0, 1), (1, 0)] and rows[2 * Q + 2] == [(0, 1)]
    assert rows[3] == [(1, 1)] and cs == [5, 0, 0, 0]
    assert sum(len(r) for r in rows) == ref.nnz_formula(1, 1, A, B, C) == 7


# ---- sonic_amd/csrc/r1cs.hpp through the stand-alone program ----
@pytest.fixture(scope="module")
def drivers():
    subprocess.check_call(["make", "-C", HOST, "-s", "-f", "r1cs.mk", "r1cs_host", "r1cs_host_san"])
    return {"plain": os.path.join(HOST, "r1cs_host"), "san": os.path.join(HOST, "r1cs_host_san")}


def hexle(v):
    return v.to_bytes(32, "little").hex()


def case_text(m, N, n_pub, mats):
    """mats: three raw (row_ptr, col, val) triples, as they are (a refusal case may break any rule)"""
    out = ["case %d %d %d" % (m, N, n_pub)]
    for rp, col, val in mats:
        out.append(" ".join([str(len(rp))] + [str(x) for x in rp]))
        out.append(" ".join([str(len(col))] + [str(x) for x in col]))
        out.append(" ".join([str(len(val))] + [hexle(x) for x in val]))
    return "\n".join(out) + "\n"


def expected_text(m, N, n_pub, A, B, C, T):
    n, Q, g = ref.shape(m, N, n_pub)
    rows, cs = ref.compile_r1cs(m, N, n_pub, A, B, C)
    rp, col, val = ref.csr_of(rows)
    stacked = A + B + C
    lines = ["ok %d %d %d %d" % (n, Q, len(col), g),
             " ".join(["row_ptr"] + [str(x) for x in rp]),
             " ".join(["col"] + [str(x) for x in col]),
             " ".join(["val"] + [hexle(x) for x in val]),
             " ".join(["cs"] + [hexle(x) for x in cs]),
             " ".join(["short"] + [str(i) for i, r in enumerate(stacked) if len(r) <= T]),
             " ".join(["long"] + [str(i) for i, r in enumerate(stacked) if len(r) > T])]
    return lines


def run_driver(path, text, tmp_path):
    f = tmp_path / "cases.txt"
    f.write_text(text)
    out = subprocess.run([path, str(f)], capture_output=True, text=True, timeout=600, env=ENV)
    assert out.returncode == 0 and out.stdout.endswith("r1cs_host ok\n"), out.stdout[-2000:] + out.stderr[-3000:]
    lines = out.stdout.splitlines()
    assert lines[0].startswith("chunk ")
    return int(lines[0].split()[1]), lines[1:-1]


def layout_cases():
    rng = random.Random(0xA11)
    full = lambda N: (N, N, N)      # noqa: E731
    cases = []
    # (m, N, n_pub, per-row lengths or None)
    for m, N, n_pub, lengths in [
            (1, 1, 0, [(1, 1, 1)]),                                  # m = 1, N = 1: only the constant column
            (1, 1, 0, [(0, 0, 0)]),
            (3, 7, 0, None), (3, 8, 0, None),                        # N odd and even, no public input
            (4, 7, 6, None), (4, 8, 7, None),                        # n_pub = N - 1
            (5, 9, 2, [(0, 0, 0), (2, 0, 3), full(9), (1, 1, 1), (0, 4, 0)]),      # an empty row, a row over all columns
            (2, 70, 1, [full(70), (33, 32, 31)]),                    # rows on both sides of the row chunk
            (12, 13, 3, None)]:
        A, B, C, z = ref.random_r1cs(rng, m, N, n_pub, lengths)
        cases.append((m, N, n_pub, A, B, C))
    # a column-0 entry in each matrix, one at a time and together
    for where in ((0,), (1,), (2,), (0, 1, 2)):
        mats = [[[(1, 3), (2, R - 1)]], [[(2, 1)]], [[(1, 0), (3, 9)]]]
        for k in where:
            mats[k][0] = [(0, 11 + k)] + mats[k][0]
        cases.append((1, 4, 1, mats[0], mats[1], mats[2]))
    return cases


@pytest.mark.parametrize("build", ["plain", "san"])
def test_layout_matches_the_model_byte_for_byte(drivers, build, tmp_path):
    cases = layout_cases()
    text = "".join(case_text(m, N, l, [ref.matrix_csr(M) for M in (A, B, C)]) for m, N, l, A, B, C in cases)
    T, got = run_driver(drivers[build], text, tmp_path)
    assert T >= 1
    want = []
    for m, N, l, A, B, C in cases:
        want += expected_text(m, N, l, A, B, C, T)
    assert got == want


REFUSALS = [
    # name, m, N, n_pub, matrices (A; B and C are one empty row each unless given), status, a word of the message
    ("row_ptr decreases", 2, 3, 0, ([0, 2, 1], [0, 1], [1, 1]), INVALID_ARG, "row_ptr decreases at row 1"),
    ("row_ptr[0] != 0", 1, 3, 0, ([1, 1], [], []), INVALID_ARG, "row_ptr[0]"),
    ("column out of range", 1, 3, 0, ([0, 1], [3], [1]), INVALID_ARG, "column 3 outside [0, 3)"),
    ("negative column", 1, 3, 0, ([0, 1], [-1], [1]), INVALID_ARG, "column -1 outside"),
    ("repeated column", 1, 3, 0, ([0, 2], [1, 1], [1, 1]), INVALID_ARG, "not strictly increasing"),
    ("decreasing column", 1, 3, 0, ([0, 2], [2, 1], [1, 1]), INVALID_ARG, "not strictly increasing"),
    ("value = r", 1, 3, 0, ([0, 1], [1], [R]), BAD_ENCODING, "non-canonical"),
    ("value = 2^256 - 1", 1, 3, 0, ([0, 1], [1], [(1 << 256) - 1]), BAD_ENCODING, "non-canonical"),
    ("n_pub > N - 1", 1, 3, 3, ([0, 0], [], []), INVALID_ARG, "n_pub = 3"),
    ("n_pub < 0", 1, 3, -1, ([0, 0], [], []), INVALID_ARG, "n_pub = -1"),
    ("m = 0", 0, 3, 0, ([0], [], []), INVALID_ARG, "m >= 1"),
    ("N = 0", 1, 0, 0, ([0, 0], [], []), INVALID_ARG, "N >= 1"),
]


@pytest.mark.parametrize("build", ["plain", "san"])
def test_every_refusal_has_its_status_and_names_the_place(drivers, build, tmp_path):
    for which in range(3):          # the broken matrix as A, as B, as C
        text = ""
        for name, m, N, l, bad, status, word in REFUSALS:
            empty = ([0] * (m + 1), [], [])
            mats = [empty, empty, empty]
            mats[which] = bad
            text += case_text(m, N, l, mats)
        _, got = run_driver(drivers[build], text, tmp_path)
        assert len(got) == len(REFUSALS)
        for (name, m, N, l, bad, status, word), line in zip(REFUSALS, got):
            assert line.startswith("refused %d " % status) and word in line, (name, line)
            if "row" in word or "column" in word or "non-canonical" in word:
                assert (" %s: " % "ABC"[which]) in line, (name, line)


# ---- the iden3 containers ----
def test_r1cs_and_wtns_files_round_trip(tmp_path):
    from sonic_amd import r1cs_io
    rng = random.Random(7)
    m, N, n_pub = 9, 11, 3
    A, B, C, z = ref.random_r1cs(rng, m, N, n_pub)
    f = r1cs_io.R1csFile(N, 1, 2, N - 4, [dict(r) for r in A], [dict(r) for r in B], [dict(r) for r in C], n_labels=N + 5, labels=list(range(5, N + 5)))
    path = tmp_path / "sys.r1cs"
    r1cs_io.write_r1cs(path, f)
    g = r1cs_io.read_r1cs(path)
    assert (g.n_wires, g.n_pub_out, g.n_pub_in, g.n_prv_in, g.n_labels, g.labels) == (N, 1, 2, N - 4, N + 5, list(range(5, N + 5)))
    assert g.n_pub == n_pub and g.m == m and g.prime == R
    assert [sorted(d.items()) for d in g.A] == A and [sorted(d.items()) for d in g.B] == B and [sorted(d.items()) for d in g.C] == C
    raw = path.read_bytes()
    assert raw[:4] == b"r1cs" and raw[4:12] == (1).to_bytes(4, "little") + (3).to_bytes(4, "little")
    assert raw[12:24] == (1).to_bytes(4, "little") + (64).to_bytes(8, "little") and raw[24:28] == (32).to_bytes(4, "little")
    assert raw[28:60] == R.to_bytes(32, "little")
    # terms out of order and a wire named twice: sorted and summed when read
    f2 = r1cs_io.R1csFile(4, 0, 1, 2, [[(3, 5), (1, 2), (3, R - 1), (0, 9)]], [[]], [[(2, 1), (2, R - 1)]])
    r1cs_io.write_r1cs(path, f2)
    g2 = r1cs_io.read_r1cs(path)
    assert list(g2.A[0].items()) == [(0, 9), (1, 2), (3, 4)] and g2.B == [{}] and g2.C == [{2: 0}]
    wpath = tmp_path / "w.wtns"
    r1cs_io.write_wtns(wpath, z)
    assert r1cs_io.read_wtns(wpath) == z
    raw = wpath.read_bytes()
    assert raw[:4] == b"wtns" and raw[4:12] == (2).to_bytes(4, "little") + (2).to_bytes(4, "little")
    assert raw[12:24] == (1).to_bytes(4, "little") + (40).to_bytes(8, "little")


def test_a_file_over_another_prime_is_refused_and_both_primes_are_named(tmp_path):
    from sonic_amd import r1cs_io
    bn254 = 21888242871839275222246405745257275088548364400416034343698204186575808495617
    path = tmp_path / "bn.r1cs"
    r1cs_io.write_r1cs(path, r1cs_io.R1csFile(3, 0, 1, 1, [{1: 1}], [{1: 1}], [{2: 1}], prime=bn254))
    with pytest.raises(ValueError) as e:
        r1cs_io.read_r1cs(path)
    assert hex(bn254) in str(e.value) and hex(R) in str(e.value)
    wpath = tmp_path / "bn.wtns"
    r1cs_io.write_wtns(wpath, [1, 2, 3], prime=bn254)
    with pytest.raises(ValueError) as e:
        r1cs_io.read_wtns(wpath)
    assert hex(bn254) in str(e.value) and hex(R) in str(e.value)
    with pytest.raises(ValueError):
        (tmp_path / "junk.r1cs").write_bytes(b"wtns" + bytes(8))
        r1cs_io.read_r1cs(tmp_path / "junk.r1cs")
