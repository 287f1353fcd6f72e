"""One resident circuit, many statements, on the GPU (include/sonic_hip.h, "One circuit, many statements"; sonic_amd/csrc/statement.hip):
sonic_prover_eval_constraints, sonic_prover_set_constants, sonic_prove_batch_statements and the batched verifier's `_cs` forms.

Every comparison is byte (or integer) equality: Fr sums are exact.  The yardsticks are Python integers for the constants and the gate
check, a FRESH handle made with the constants (and the C oracle, as the parity tests use it) for proof bytes, and the per-equation host
verifier sonic_verify / sonic_verify_fs with each proof's own cs for verdicts -- never the code under test.

Reference: cs = wL.aL + wR.aR + wO.aO (test/Test/Reference.hs:138); Sonic.Protocol.prove / verify (src/Sonic/Protocol.hs:47-130)."""
import ctypes as C
import hashlib
import os
import random

import numpy as np
import pytest

from util import NCPU, R, circuit_arrays, fr_bytes

pytestmark = pytest.mark.gpu

D = 7 * 1000 + 24
SEED = bytes(range(32))


@pytest.fixture(scope="module")
def srs_pair(sonic, orc):
    pyr = random.Random(77)
    x, alpha = pyr.randrange(2, R), pyr.randrange(2, R)
    g = sonic.SRS.new(D, x, alpha)
    yield g, orc.SRS(D, x, alpha, threads=NCPU)
    g.close()


# ---- statements in Python integers -----------------------------------------------------------------------------------------------------
def rand_assignment(pyr, n):
    aL = [pyr.randrange(R) for _ in range(n)]
    aR = [pyr.randrange(R) for _ in range(n)]
    return aL, aR, [a * b % R for a, b in zip(aL, aR)]


def cs_of(rows, Q, asg):
    """rows: 3Q mappings {gate: weight} (wL, wR, wO stacked) -> the Q constants of the assignment"""
    return [sum(w * asg[m][i] for m in range(3) for i, w in rows[m * Q + q].items()) % R for q in range(Q)]


def dense_rows(pyr, n, Q):
    return [{i: pyr.randrange(R) for i in range(n)} for _ in range(3 * Q)]


def skewed_rows(pyr, n, Q=3):
    """rows of 0 entries, rows of n entries (longer than one chunk at n = 1000) and rows of at most 4"""
    few = lambda: {i: pyr.randrange(1, R) for i in pyr.sample(range(n), min(n, pyr.randrange(1, 5)))}      # noqa: E731
    full = lambda: {i: pyr.randrange(1, R) for i in range(n)}                                              # noqa: E731
    return [full(), {}, few(),  {}, {}, few(),  few(), full(), {}]


def short_rows(pyr, n, Q):
    return [{i: pyr.randrange(R) for i in pyr.sample(range(n), min(n, pyr.randrange(0, 5)))} for _ in range(3 * Q)]


def circuit_of(sonic, form, n, Q, rows, cs):
    if form == "csr":
        return sonic.SparseCircuit.from_rows(n, rows[:Q], rows[Q:2 * Q], rows[2 * Q:], cs)
    mats = [[[row.get(i, 0) for i in range(n)] for row in rows[m * Q:(m + 1) * Q]] for m in range(3)]
    return sonic.ArithCircuit(sonic.GateWeights(*mats), cs)


EVAL_CASES = [("dense", 1, 1, dense_rows), ("dense", 255, 2, dense_rows), ("dense", 256, 2, dense_rows), ("dense", 257, 5, dense_rows), ("dense", 1000, 64, dense_rows),
              ("csr", 1, 3, skewed_rows), ("csr", 255, 3, skewed_rows), ("csr", 256, 3, skewed_rows), ("csr", 257, 3, skewed_rows), ("csr", 1000, 3, skewed_rows),
              ("csr", 1000, 64, short_rows)]


@pytest.mark.parametrize("form,n,Q,make", EVAL_CASES, ids=["%s-%d-%d" % c[:3] for c in EVAL_CASES])
def test_eval_constraints_against_python_integers(sonic, srs_pair, form, n, Q, make):
    from sonic_amd import _lib
    pyr = random.Random(1000 * n + Q)
    rows = make(pyr, n, Q)
    asgs = [rand_assignment(pyr, n) for _ in range(3)]
    want = [cs_of(rows, Q, a) for a in asgs]
    p = sonic.Prover(srs_pair[0], circuit_of(sonic, form, n, Q, rows, want[0]), prepare=False)
    try:
        with pytest.raises(_lib.SonicError) as e:                  # the resident form with no assignment set: what prove says
            p.eval_constraints()
        assert e.value.code == 7
        A = [sonic.Assignment(*a) for a in asgs]
        for B in (1, 3):
            cs, gates = p.eval_constraints(A[:B])
            print(form, n, Q, "B =", B, "first constants", [hex(c)[:12] for c in cs[0][:2]], "gates", gates)
            assert cs == want[:B]
            assert gates == [(0, -1)] * B
        p.set_assignment(A[1])
        assert p.eval_constraints() == ([want[1]], [(0, -1)])
        # the gate check: aO corrupted at index 0, at index n - 1, and at two indices at once (one assignment each, one call)
        def broken(idx):
            aO = list(asgs[2][2])
            for i in idx:
                aO[i] = (aO[i] + 1) % R
            return (asgs[2][0], asgs[2][1], aO)
        cases = [[0], [n - 1]] + ([[n // 3, n - 1]] if n >= 3 else [])
        bad = [broken(idx) for idx in cases]
        cs, gates = p.eval_constraints([sonic.Assignment(*a) for a in bad])
        print(form, n, Q, "broken gates", gates)
        assert gates == [(len(set(idx)), min(idx)) for idx in cases]
        assert cs == [cs_of(rows, Q, a) for a in bad]              # (the constants of what was given, satisfied gates or not)
        # a non-canonical input is refused
        raw = [np.ascontiguousarray(fr_bytes(v)) for v in asgs[0]]
        raw[1][n - 1] = np.frombuffer(R.to_bytes(32, "little"), np.uint8)
        out, g2 = np.zeros((1, Q, 32), np.uint8), np.zeros((1, 2), np.int64)
        rc = _lib.lib().sonic_prover_eval_constraints(p._h, 1, raw[0].ctypes.data, raw[1].ctypes.data, raw[2].ctypes.data, out.ctypes.data, g2.ctypes.data)
        assert rc == 3, _lib.last_error()
        assert _lib.lib().sonic_prover_eval_constraints(p._h, 0, raw[0].ctypes.data, raw[0].ctypes.data, raw[0].ctypes.data, out.ctypes.data, None) == 7
        assert _lib.lib().sonic_prover_eval_constraints(p._h, (1 << 26) // n + 1, raw[0].ctypes.data, raw[0].ctypes.data, raw[0].ctypes.data, out.ctypes.data, None) == 7
        assert p.eval_constraints() == ([want[1]], [(0, -1)])      # the handle's own assignment was left alone
    finally:
        p.close()


def test_eval_constraints_refuses_a_handle_in_flight(sonic, ref, srs_pair):
    from sonic_amd import _lib
    pyr = random.Random(5)
    circ, asg, enc = circuit_arrays(ref, pyr, 16, 2)
    p = sonic.Prover(srs_pair[0], sonic.ArithCircuit(sonic.GateWeights(circ[0], circ[1], circ[2]), circ[3]), prepare=False)
    p.set_assignment(sonic.Assignment(*asg))
    p.submit([pyr.randrange(1, R) for _ in range(12)])
    try:
        for call in (p.eval_constraints, lambda: p.set_constants(circ[3])):
            with pytest.raises(_lib.SonicError) as e:
                call()
            assert e.value.code == 7
    finally:
        p.collect()
        p.close()


# ---- set_constants ---------------------------------------------------------------------------------------------------------------------
def two_statements(sonic, ref, pyr, n, Q, form):
    circ, asg, enc = circuit_arrays(ref, pyr, n, Q)
    dense = sonic.ArithCircuit(sonic.GateWeights(enc["wL"], enc["wR"], enc["wO"]), enc["cs"])
    circuit = sonic.SparseCircuit.from_circuit(dense) if form == "csr" else dense
    rows = [{i: w for i, w in enumerate(row) if w} for m in circ[:3] for row in m]
    a2 = rand_assignment(pyr, n)
    return circ, asg, enc, circuit, a2, cs_of(rows, Q, a2)


def with_constants(sonic, circuit, cs):
    if isinstance(circuit, sonic.SparseCircuit):
        return sonic.SparseCircuit(circuit.n, circuit.Q, circuit.row_ptr, circuit.col, circuit.val, fr_bytes(cs))
    return sonic.ArithCircuit(circuit.weights, fr_bytes(cs))


def fresh_proof(sonic, srs, circuit, cs, asg, tr):
    q = sonic.Prover(srs, with_constants(sonic, circuit, cs), prepare=False)
    try:
        q.set_assignment(sonic.Assignment(*asg))
        return q.prove_bytes(tr)
    finally:
        q.close()


@pytest.mark.parametrize("form", ["dense", "csr"])
@pytest.mark.parametrize("prepare", [False, True], ids=["unprepared", "prepared"])
def test_set_constants_proves_the_second_statement(sonic, orc, ref, srs_pair, form, prepare):
    from sonic_amd import _lib
    g, o = srs_pair
    n, Q = 257, 5
    pyr = random.Random(257 + prepare)
    circ, asg, enc, circuit, a2, cs2 = two_statements(sonic, ref, pyr, n, Q, form)
    tr1, tr2 = ([pyr.randrange(1, R) for _ in range(8 + 2 * Q)] for _ in range(2))
    p = sonic.Prover(g, circuit, prepare=prepare)
    try:
        p.set_assignment(sonic.Assignment(*asg))
        first = p.prove_bytes(tr1)
        assert first == fresh_proof(sonic, g, circuit, circ[3], asg, tr1)
        p.set_assignment(sonic.Assignment(*a2))
        with pytest.raises(_lib.SonicError) as e:                  # the new assignment against the OLD constants: t(X, y) keeps a constant term
            p.prove_bytes(tr2)
        assert e.value.code == 2
        got_cs, gates = p.eval_constraints()
        assert got_cs == [cs2] and gates == [(0, -1)]
        with pytest.raises(_lib.SonicError) as e:                  # a refused cs leaves the old constants
            p.set_constants([R] + cs2[1:])
        assert e.value.code == 3
        with pytest.raises(_lib.SonicError) as e:
            p.prove_bytes(tr2)
        assert e.value.code == 2
        p.set_constants(got_cs[0])
        second = p.prove_bytes(tr2)
        assert second == fresh_proof(sonic, g, circuit, cs2, a2, tr2)
        if form == "dense" and not prepare:
            assert second == orc.prove(o, n, Q, enc["wL"], enc["wR"], enc["wO"], fr_bytes(cs2), fr_bytes(a2[0]), fr_bytes(a2[1]), fr_bytes(a2[2]), fr_bytes(tr2))
        # and back: the first statement again on the same handle
        p.set_assignment(sonic.Assignment(*asg))
        p.set_constants(circ[3])
        assert p.prove_bytes(tr1) == first
    finally:
        p.close()


def test_set_constants_under_graph_replay(sonic, ref, srs_pair):
    """SONIC_PROVE_GRAPH=1 (turned on as test_prove_graph_replay does): proof 2 is captured, later proofs replay it; the constants change
    between the captured proof and a replayed one, in place, and the replay must read the new ones"""
    g, _ = srs_pair
    n, Q = 40, 2
    pyr = random.Random(4040)
    circ, asg, enc, circuit, a2, cs2 = two_statements(sonic, ref, pyr, n, Q, "dense")
    os.environ["SONIC_PROVE_GRAPH"] = "1"
    try:
        p = sonic.Prover(g, circuit)
    finally:
        del os.environ["SONIC_PROVE_GRAPH"]
    try:
        p.set_assignment(sonic.Assignment(*asg))
        trs = [[pyr.randrange(1, R) for _ in range(8 + 2 * Q)] for _ in range(5)]
        for k in range(3):                                          # grows the workspaces, is captured, is replayed
            assert p.prove_bytes(trs[k]) == fresh_proof(sonic, g, circuit, circ[3], asg, trs[k]), k
        p.set_assignment(sonic.Assignment(*a2))
        p.set_constants(p.eval_constraints()[0][0])
        for k in (3, 4):
            assert p.prove_bytes(trs[k]) == fresh_proof(sonic, g, circuit, cs2, a2, trs[k]), k
    finally:
        p.close()


# ---- sonic_prove_batch_statements ------------------------------------------------------------------------------------------------------
def test_prove_batch_statements(sonic, ref, srs_pair):
    from sonic_amd import _lib
    g, _ = srs_pair
    n, Q, K = 64, 3, 5
    pyr = random.Random(643)
    circ, asg, enc, circuit, _, _ = two_statements(sonic, ref, pyr, n, Q, "dense")
    rows = [{i: w for i, w in enumerate(row) if w} for m in circ[:3] for row in m]
    asgs = [rand_assignment(pyr, n) for _ in range(K)]
    css = [cs_of(rows, Q, a) for a in asgs]
    assert len({tuple(c) for c in css}) == K
    trs = [[pyr.randrange(1, R) for _ in range(8 + 2 * Q)] for _ in range(K)]
    want = [fresh_proof(sonic, g, circuit, css[k], asgs[k], trs[k]) for k in range(K)]
    provers = [sonic.Prover(g, circuit) for _ in range(2)]
    try:
        A = [sonic.Assignment(*a) for a in asgs]
        assert sonic.prove_batch(provers, trs, A, constants=css) == want
        # each handle holds the constants (and assignment) of the last proof it ran: proofs 4 and 3
        assert provers[0].prove_bytes(trs[4]) == want[4] and provers[1].prove_bytes(trs[3]) == want[3]
        # proof 2 with proof 0's constants: its own status, the others' bytes, and the return value is that status
        wrong = list(css)
        wrong[2] = css[0]
        L = _lib.lib()
        psz = L.sonic_proof_size(Q)
        enc3 = [np.ascontiguousarray(np.stack([fr_bytes(a[m]) for a in asgs])) for m in range(3)]
        tr = np.ascontiguousarray(np.stack([fr_bytes(t) for t in trs]))
        cs = np.ascontiguousarray(np.stack([fr_bytes(c) for c in wrong]))
        out = np.zeros((K, psz), np.uint8)
        status = (C.c_int * K)()
        arr = (C.c_void_p * 2)(*[p._h for p in provers])
        rc = L.sonic_prove_batch_statements(arr, 2, K, enc3[0].ctypes.data, enc3[1].ctypes.data, enc3[2].ctypes.data, cs.ctypes.data, tr.ctypes.data, out.ctypes.data, status)
        assert rc == 2 and list(status) == [0, 0, 2, 0, 0]
        assert [out[k].tobytes() for k in (0, 1, 3, 4)] == [want[k] for k in (0, 1, 3, 4)]
        # a non-canonical constant: that proof's status, before anything of it is queued
        cs[1, 0] = np.frombuffer(R.to_bytes(32, "little"), np.uint8)
        cs[2] = fr_bytes(css[2])
        rc = L.sonic_prove_batch_statements(arr, 2, K, enc3[0].ctypes.data, enc3[1].ctypes.data, enc3[2].ctypes.data, cs.ctypes.data, tr.ctypes.data, out.ctypes.data, status)
        assert rc == 3 and list(status) == [0, 3, 0, 0, 0]
        assert [out[k].tobytes() for k in (0, 2, 3, 4)] == [want[k] for k in (0, 2, 3, 4)]
    finally:
        for p in provers:
            p.close()


# ---- the batched verifier with per-proof constants -------------------------------------------------------------------------------------
class Statements:
    """K statements of one circuit (n = 16, Q = 3) and their proofs, plain and Fiat-Shamir, made once"""

    def __init__(self, sonic, ref, srs):
        pyr = random.Random(163)
        self.n, self.Q, self.K, self.srs = 16, 3, 6, srs
        circ, asg, enc, self.circuit, _, _ = two_statements(sonic, ref, pyr, self.n, self.Q, "dense")
        self.cs0 = circ[3]
        rows = [{i: w for i, w in enumerate(row) if w} for m in circ[:3] for row in m]
        self.asgs = [rand_assignment(pyr, self.n) for _ in range(self.K)]
        self.css = [cs_of(rows, self.Q, a) for a in self.asgs]
        Q = self.Q
        trs = [[pyr.randrange(1, R) for _ in range(8 + 2 * Q)] for _ in range(self.K)]
        p = sonic.Prover(srs, self.circuit)
        self.proofs = sonic.prove_batch([p], trs, [sonic.Assignment(*a) for a in self.asgs], constants=self.css)
        p.close()
        self.trs = [(t[4], t[5], list(zip(t[6:6 + Q], t[6 + Q:6 + 2 * Q]))) for t in trs]
        # Fiat-Shamir: per statement, prove_fs with the resumed digest after set_constants
        mid = sonic.fs_circuit_midstate(self.circuit)
        p = sonic.Prover(srs, self.circuit, prepare=False)
        self.fs_proofs = []
        for k in range(self.K):
            p.set_assignment(sonic.Assignment(*self.asgs[k]))
            p.set_constants(self.css[k])
            digest = sonic.fs_circuit_digest_resume(mid, self.css[k])
            assert digest == sonic.fs_circuit_digest(with_constants(sonic, self.circuit, self.css[k]))
            self.fs_proofs.append(p.prove_fs(digest, hashlib.sha256(b"blind%d" % k).digest())[0])
        p.close()
        self.verifier = sonic.Verifier(srs, self.circuit)

    def yard(self, sonic, raw, tr, cs):
        """sonic_verify on one proof with the given constants (a refused encoding reads as rejected)"""
        from sonic_amd import _lib
        from sonic_amd.protocol import _circuit_args
        n, Q, suffix, args, _keep = _circuit_args(self.circuit)
        csb = b"".join(int(c).to_bytes(32, "little") for c in cs)
        y, z, yzs = tr
        fr = lambda v: int(v).to_bytes(32, "little")      # noqa: E731
        ok = C.c_int(0)
        rc = _lib.lib().sonic_verify(self.srs._h, n, Q, *args[:3], csb, bytes(raw), fr(y), fr(z), b"".join(fr(a) + fr(b) for a, b in yzs), C.byref(ok))
        assert rc in (0, 3), (rc, _lib.last_error())
        return rc == 0 and bool(ok.value)

    def yard_fs(self, sonic, raw, cs):
        from sonic_amd import _lib
        from sonic_amd.protocol import _circuit_args
        n, Q, suffix, args, _keep = _circuit_args(self.circuit)
        csb = b"".join(int(c).to_bytes(32, "little") for c in cs)
        ok = C.c_int(0)
        rc = _lib.lib().sonic_verify_fs(self.srs._h, n, Q, *args[:3], csb, bytes(raw), C.byref(ok))
        assert rc in (0, 3), (rc, _lib.last_error())
        return rc == 0 and bool(ok.value)


@pytest.fixture(scope="module")
def statements(sonic, ref, srs_pair):
    s = Statements(sonic, ref, srs_pair[0])
    yield s
    s.verifier.close()


def both_encodings(sonic, proofs, Q):
    return [("plain", proofs), ("compressed", [sonic.Proof.from_bytes(p, Q).to_bytes(compressed=True) for p in proofs])]


def test_verify_batch_cs(sonic, statements):
    s, v = statements, statements.verifier
    K = s.K
    assert [s.yard(sonic, s.proofs[k], s.trs[k], s.css[k]) for k in range(K)] == [True] * K
    swapped = list(s.css)
    swapped[1], swapped[4] = s.css[4], s.css[1]
    yard_swapped = [s.yard(sonic, s.proofs[k], s.trs[k], swapped[k]) for k in range(K)]
    assert yard_swapped == [k not in (1, 4) for k in range(K)]
    bad = [b"".join(int(c).to_bytes(32, "little") for c in cs) for cs in s.css]
    bad[2] = bad[2][:32] + R.to_bytes(32, "little") + bad[2][64:]
    for name, proofs in both_encodings(sonic, s.proofs, s.Q):
        assert v.verify_batch(proofs, s.trs, seed=SEED, each=True, constants=s.css) == (True, [True] * K), name
        assert v.verify_batch(proofs, s.trs, seed=SEED, constants=s.css) is True, name
        assert v.verify_batch(proofs, s.trs, seed=SEED, each=True, constants=swapped) == (False, yard_swapped), name
        assert v.verify_batch(proofs, s.trs, seed=SEED, constants=swapped) is False, name
        assert v.verify_batch(proofs, s.trs, seed=SEED, each=True, constants=bad) == (False, [k != 2 for k in range(K)]), name
        # the handle's own constants for every proof: the verdicts of verify_batch (these proofs are of other statements: rejected alike)
        own = [s.cs0] * K
        assert v.verify_batch(proofs, s.trs, seed=SEED, each=True, constants=own) == v.verify_batch(proofs, s.trs, seed=SEED, each=True), name


def test_verify_batch_cs_equals_verify_batch_on_the_handles_statement(sonic, ref, srs_pair):
    g, _ = srs_pair
    n, Q, K = 16, 3, 3
    pyr = random.Random(1603)
    circ, asg, enc, circuit, _, _ = two_statements(sonic, ref, pyr, n, Q, "dense")
    p = sonic.Prover(g, circuit)
    p.set_assignment(sonic.Assignment(*asg))
    trs = [[pyr.randrange(1, R) for _ in range(8 + 2 * Q)] for _ in range(K)]
    proofs = [p.prove_bytes(t) for t in trs]
    p.close()
    proofs[1] = proofs[1][:96 + 96] + int((int.from_bytes(proofs[1][192:224], "little") + 1) % R).to_bytes(32, "little") + proofs[1][224:]      # a changed: rejected
    ch = [(t[4], t[5], list(zip(t[6:6 + Q], t[6 + Q:6 + 2 * Q]))) for t in trs]
    v = sonic.Verifier(g, circuit)
    try:
        want = v.verify_batch(proofs, ch, seed=SEED, each=True)
        assert want == (False, [True, False, True])
        assert v.verify_batch(proofs, ch, seed=SEED, each=True, constants=[circ[3]] * K) == want
    finally:
        v.close()


def test_fiat_shamir_statements(sonic, statements):
    s, v = statements, statements.verifier
    K = s.K
    assert [s.yard_fs(sonic, s.fs_proofs[k], s.css[k]) for k in range(K)] == [True] * K
    moved = s.css[1:] + s.css[:1]                                    # every proof against another statement's constants
    assert [s.yard_fs(sonic, s.fs_proofs[k], moved[k]) for k in range(K)] == [False] * K
    one = list(s.css)
    one[3] = s.css[0]
    for name, proofs in both_encodings(sonic, s.fs_proofs, s.Q):
        assert v.verify_fs_batch(proofs, seed=SEED, each=True, constants=s.css) == (True, [True] * K), name
        assert v.verify_fs_batch(proofs, seed=SEED, each=True, constants=one) == (False, [k != 3 for k in range(K)]), name
        assert v.verify_fs_batch(proofs, seed=SEED, constants=moved) is False, name
