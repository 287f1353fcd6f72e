"""Fiat-Shamir proofs in flight on the GPU (include/sonic_hip.h, "Fiat-Shamir proofs in flight"): witness digest v2 from the kernels of
witness.hip against the hashlib restatement (tests/fs_stream_ref.py), sonic_prover_submit_fs / collect_fs against the restated blinders,
the one-pass prover, the C oracle and the verifier, two handles in flight from one host thread, the error contract, and
sonic_prove_batch_fs.  Every comparison is byte equality."""
import ctypes as C
import hashlib
import random

import numpy as np
import pytest

import fs_stream_ref as fref
from util import NCPU, R, big_circuit, circuit_arrays, fr_bytes

pytestmark = pytest.mark.gpu

TREE_NS = [1, 10, 11, 32, 341, 342, 10922, 10923]


def seed_of(tag) -> bytes:
    return hashlib.sha256(b"fs-stream-%s" % str(tag).encode()).digest()


# ---- witness digest ----
@pytest.fixture(scope="module")
def wide_srs(sonic):
    g = sonic.SRS.new(7 * max(TREE_NS), 0x1234567891, 0x987654321)
    yield g
    g.close()


@pytest.mark.parametrize("n", TREE_NS)
def test_witness_digest_matches_the_restatement(sonic, wide_srs, n):
    one = np.zeros((n, 32), np.uint8)
    one[:, 0] = 1
    p = sonic.Prover(wide_srs, sonic.ArithCircuit(sonic.GateWeights(one, one, one), [5]), prepare=False)
    try:
        seen = []
        for k in range(2):                    # a second set_assignment: the cached digest goes, the new one differs
            a = fref.assignment_values(n, seed=k)
            p.set_assignment(sonic.Assignment(*[fr_bytes(v) for v in a]))
            got = p.witness_digest()
            assert got == fref.witness_digest_v2(*a), (n, k)
            assert p.witness_digest() == got
            seen.append(got)
        assert seen[0] != seen[1]
    finally:
        p.close()


def test_witness_digest_needs_an_assignment(sonic, wide_srs):
    from sonic_amd import _lib
    one = np.zeros((4, 32), np.uint8)
    p = sonic.Prover(wide_srs, sonic.ArithCircuit(sonic.GateWeights(one, one, one), [5]), prepare=False)
    with pytest.raises(_lib.SonicError) as e:
        p.witness_digest()
    assert e.value.code == 7
    p.close()


# ---- proof parity ----
@pytest.mark.parametrize("prepare", [False, True], ids=["unprepared", "prepared"])
@pytest.mark.parametrize("n,Q", [(1, 1), (5, 3), (64, 2)])
def test_collect_fs_parity(sonic, orc, ref, n, Q, prepare):
    pyr = random.Random(1000 * n + Q)
    d = max(7 * n, 4 * n + 8) + pyr.randrange(0, 9)          # n = 1 needs d >= 4n + 8: t(X,y) reaches X^{-4n-8}
    x, alpha = pyr.randrange(1, R), pyr.randrange(1, R)
    srs = sonic.SRS.new(d, x, alpha)
    circ, asg, enc = circuit_arrays(ref, pyr, n, Q)
    circuit = sonic.ArithCircuit(sonic.GateWeights(circ[0], circ[1], circ[2]), circ[3])
    digest, srs_id = sonic.fs_circuit_digest(circuit), sonic.fs_srs_id(srs)
    assert digest == ref.fs_circuit_digest(circ)
    seed = seed_of((n, Q))
    p = sonic.Prover(srs, circuit, prepare=prepare)
    try:
        p.set_assignment(sonic.Assignment(*asg))
        p.submit_fs(digest, seed)
        raw, tr = p.collect_fs()
        assert p.witness_digest() == fref.witness_digest_v2(*asg)
        assert tr[:4] == fref.blinders(seed, digest, srs_id, fref.witness_digest_v2(*asg))
        assert tr[:4] != ref.fs_blinders(seed, digest, srs_id, ref.fs_witness_digest(asg))      # (v1's: what prove_fs uses)
        y, z, ys, zs, u, v = ref.fs_challenges_of_proof(n, Q, d, digest, srs_id, raw)
        assert tr[4:] == [y, z] + ys + zs + [u, v]
        assert p.prove_bytes(tr) == raw
        want = orc.prove(orc.SRS(d, x, alpha, threads=NCPU), n, Q, enc["wL"], enc["wR"], enc["wO"], enc["cs"], enc["aL"], enc["aR"], enc["aO"], fr_bytes(tr))
        assert raw == want
        assert sonic.verify_fs(srs, circuit, sonic.Proof.from_bytes(raw, Q))
        # the same inputs again: the same bytes; another seed: other bytes, still accepted
        p.submit_fs(digest, seed)
        assert p.collect_fs() == (raw, tr)
        p.submit_fs(digest, bytes(32))
        raw2, tr2 = p.collect_fs()
        assert raw2 != raw and not set(tr2[:4]) & set(tr[:4]) and sonic.verify_fs(srs, circuit, sonic.Proof.from_bytes(raw2, Q))
        # the blocking call on the same handle is what it was: v1 blinders
        raw1, tr1 = p.prove_fs(digest, seed)
        assert tr1[:4] == ref.fs_blinders(seed, digest, srs_id, ref.fs_witness_digest(asg)) and sonic.verify_fs(srs, circuit, sonic.Proof.from_bytes(raw1, Q))
    finally:
        p.close()
        srs.close()


# ---- two handles in flight, one host thread ----
@pytest.fixture(scope="module")
def mid_size(sonic):
    n, Q = 1 << 12, 2
    srs = sonic.SRS.new(8 * n, 0x1234567891, 0x987654321)
    cases = []
    for s in (5, 6):
        c = big_circuit(s, n, Q)
        circuit = sonic.ArithCircuit(sonic.GateWeights(c["wL"], c["wR"], c["wO"]), c["cs"])
        cases.append((c, circuit, sonic.fs_circuit_digest(circuit)))
    yield n, Q, srs, cases
    srs.close()


def test_two_handles_in_flight(sonic, mid_size):
    n, Q, srs, cases = mid_size
    provers = []
    for c, circuit, _ in cases:
        p = sonic.Prover(srs, circuit)
        p.set_assignment(sonic.Assignment(c["aL"], c["aR"], c["aO"]))
        provers.append(p)
    (_, circA, dA), (_, circB, dB) = cases
    A, B = provers
    try:
        alone = []
        for r in range(3):
            A.submit_fs(dA, seed_of(("A", r)))
            a = A.collect_fs()
            B.submit_fs(dB, seed_of(("B", r)))
            alone.append((a, B.collect_fs()))
        for r in range(3):
            A.submit_fs(dA, seed_of(("A", r)))
            B.submit_fs(dB, seed_of(("B", r)))
            b = B.collect_fs()
            a = A.collect_fs()
            assert (a, b) == alone[r], r
            assert sonic.verify_fs(srs, circA, sonic.Proof.from_bytes(a[0], Q)) and sonic.verify_fs(srs, circB, sonic.Proof.from_bytes(b[0], Q))
        assert len({a[0] for a, _ in alone} | {b[0] for _, b in alone}) == 6
    finally:
        for p in provers:
            p.close()


# ---- error contract ----
def test_error_contract(sonic, mid_size):
    from sonic_amd import _lib
    n, Q, srs, cases = mid_size
    c, circuit, digest = cases[0]
    asg = sonic.Assignment(c["aL"], c["aR"], c["aO"])
    seed = seed_of("errors")
    tr0 = [7 + k for k in range(8 + 2 * Q)]
    p = sonic.Prover(srs, circuit)

    def refused(call):
        with pytest.raises(_lib.SonicError) as e:
            call()
        assert e.value.code == 7 and e.value.message, call
    try:
        refused(p.collect_fs)                                        # nothing in flight
        refused(lambda: p.submit_fs(digest, seed))                   # no assignment
        p.set_assignment(asg)
        p.submit_fs(digest, seed)
        good = p.collect_fs()
        assert sonic.verify_fs(srs, circuit, sonic.Proof.from_bytes(good[0], Q))
        # an unsatisfied assignment: the pass that commits T reports it, on the collecting thread
        aO = c["aO"].copy()
        aO[0, 0] ^= 1
        p.set_assignment(sonic.Assignment(c["aL"], c["aR"], aO))
        p.submit_fs(digest, seed)
        with pytest.raises(_lib.SonicError) as e:
            p.collect_fs()
        assert e.value.code == 2 and "SRS element" in e.value.message
        refused(p.collect_fs)                                        # the flight ended with the failed collect
        p.set_assignment(asg)
        p.submit_fs(digest, seed)
        # ... and while a Fiat-Shamir proof is in flight: every call a transcript flight refuses, and the wrong collects; the flight stays
        for call in (lambda: p.submit_fs(digest, seed), lambda: p.submit(tr0), p.collect, p.collect_share, lambda: p.set_assignment(asg),
                     lambda: p.set_constants(c["cs_ints"]), lambda: p.prove_fs(digest, seed), lambda: p.prove_bytes(tr0), p.witness_digest,
                     lambda: p.set_share(0, 2), p.eval_constraints):
            refused(call)
        assert p.collect_fs() == good                                # the handle proves correctly afterwards, and the flight was intact
        # a transcript flight is not collect_fs's
        p.submit(tr0)
        refused(p.collect_fs)
        assert p.collect() == p.prove_bytes(tr0)
        # one rank's share of a proof: refused, as by prove_fs
        p.set_share(0, 2)
        refused(lambda: p.submit_fs(digest, seed))
        p.set_share(0, 1)
        p.submit_fs(digest, seed)
        assert p.collect_fs() == good
        with pytest.raises(ValueError):
            p.submit_fs(digest[:31], seed)                           # short inputs never reach the C side
        # close() with a proof in flight returns once the job has ended
        p.submit_fs(digest, seed)
    finally:
        p.close()
    assert p._h is None


# ---- batch ----
def test_prove_batch_fs(sonic, ref):
    from sonic_amd import _lib
    n, Q, K = 64, 2, 6
    pyr = random.Random(6402)
    d = 7 * n + 3
    srs = sonic.SRS.new(d, pyr.randrange(1, R), pyr.randrange(1, R))
    circ, _, enc = circuit_arrays(ref, pyr, n, Q)
    circuit = sonic.ArithCircuit(sonic.GateWeights(enc["wL"], enc["wR"], enc["wO"]), enc["cs"])
    mid = sonic.fs_circuit_midstate(circuit)
    asgs = []
    for _ in range(K):
        aL, aR = [pyr.randrange(R) for _ in range(n)], [pyr.randrange(R) for _ in range(n)]
        asgs.append((aL, aR, [a * b % R for a, b in zip(aL, aR)]))
    css = [[sum(circ[m][q][i] * a[m][i] for m in range(3) for i in range(n)) % R for q in range(Q)] for a in asgs]
    assert len({tuple(c) for c in css}) == K
    digests = [sonic.fs_circuit_digest_resume(mid, cs) for cs in css]
    seeds = [seed_of(("batch", k)) for k in range(K)]
    A = [sonic.Assignment(*a) for a in asgs]
    one = sonic.Prover(srs, circuit)
    provers = [sonic.Prover(srs, circuit) for _ in range(2)]
    verifier = sonic.Verifier(srs, circuit)
    try:
        want = []
        for k in range(K):
            one.set_assignment(A[k])
            one.set_constants(css[k])
            one.submit_fs(digests[k], seeds[k])
            want.append(one.collect_fs())
        got = sonic.prove_batch_fs(provers, digests, seeds, assignments=A, constants=css)
        assert got == want
        assert verifier.verify_fs_batch([raw for raw, _ in got], seed=bytes(range(32)), each=True, constants=css) == (True, [True] * K)
        # each handle keeps the assignment, the constants and the cached digest of the last proof it ran: proofs 4 and 5
        assert provers[0].witness_digest() == fref.witness_digest_v2(*asgs[4]) and provers[1].witness_digest() == fref.witness_digest_v2(*asgs[5])
        assert sonic.prove_batch_fs(provers, [digests[4], digests[5]], [seeds[4], seeds[5]]) == [want[4], want[5]]
        # one broken assignment: that proof's status, the other five unchanged
        L = _lib.lib()
        psz, tl = L.sonic_proof_size(Q), 8 + 2 * Q
        enc3 = [np.ascontiguousarray(np.stack([fr_bytes(a[m]) for a in asgs])) for m in range(3)]
        enc3[2][2, 0, 0] ^= 1
        cs = np.ascontiguousarray(np.stack([fr_bytes(c) for c in css]))
        out, trs = np.zeros((K, psz), np.uint8), np.zeros((K, tl, 32), np.uint8)
        status = (C.c_int * K)()
        arr = (C.c_void_p * 2)(*[p._h for p in provers])
        rc = L.sonic_prove_batch_fs(arr, 2, K, enc3[0].ctypes.data, enc3[1].ctypes.data, enc3[2].ctypes.data, cs.ctypes.data, b"".join(digests), b"".join(seeds),
                                    out.ctypes.data, trs.ctypes.data, status)
        assert rc == 2 and list(status) == [0, 0, 2, 0, 0, 0] and "proof 2" in _lib.last_error()
        assert [out[k].tobytes() for k in (0, 1, 3, 4, 5)] == [want[k][0] for k in (0, 1, 3, 4, 5)]
        # without a transcript buffer, and nothing to prove
        rc = L.sonic_prove_batch_fs(arr, 2, 2, enc3[0].ctypes.data, enc3[1].ctypes.data, enc3[2].ctypes.data, cs.ctypes.data, b"".join(digests), b"".join(seeds),
                                    out.ctypes.data, None, None)
        assert rc == 0 and [out[k].tobytes() for k in (0, 1)] == [want[k][0] for k in (0, 1)]
        assert sonic.prove_batch_fs(provers, [], []) == []
    finally:
        for p in provers + [one]:
            p.close()
        verifier.close()
        srs.close()
