"""Core proofs on the GPU (include/sonic_hip.h, "Core proofs"): the prover's head-only pass against the full proof and the CPU oracle, the
flights and their error contract, the unhelped verifier -- s(z, y) evaluated, then the three equations of the head -- alone and batched, the
forgery that the reference-shaped verifier accepts and this one rejects, and the Fiat-Shamir form against a hashlib transcript
(tests/core_proof_ref.py).  Every comparison is byte equality or a verdict."""
import hashlib
import json
import os
import random
import subprocess

import numpy as np
import pytest

import core_proof_ref as cref
import fs_stream_ref as fref
from util import NCPU, R, big_circuit, circuit_arrays, fr_bytes

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
SMALL_NS, SMALL_QS = [1, 2, 5, 257], [1, 2, 5]
SMALL_D = 7 * 257 + 6          # one string for every small shape (n = 1 needs d >= 4n + 8)
X, ALPHA = 0x1234567891, 0x987654321
INVALID_ARG, BAD_ENCODING, INEXACT_DIVISION = 7, 3, 4


def seed_of(tag) -> bytes:
    return hashlib.sha256(b"core-proofs-%s" % str(tag).encode()).digest()


def refused(sonic, code, fn):
    from sonic_amd import _lib
    with pytest.raises(_lib.SonicError) as e:
        fn()
    assert e.value.code == code, e.value
    return True


def rejects(fn) -> bool:
    """a verifier's "no": False, or the BAD_ENCODING status that the one-proof calls give a malformed proof"""
    from sonic_amd import _lib
    try:
        return fn() is False
    except _lib.SonicError as e:
        return e.code == BAD_ENCODING


# ---- the small shapes: one string, one oracle proof per shape, shared ----
@pytest.fixture(scope="module")
def small_srs(sonic):
    g = sonic.SRS.new(SMALL_D, X, ALPHA)
    yield g
    g.close()


@pytest.fixture(scope="module")
def small_cases(sonic, orc, ref):
    osrs = orc.SRS(SMALL_D, X, ALPHA, threads=NCPU)
    out = {}
    for n in SMALL_NS:
        for Q in SMALL_QS:
            pyr = random.Random(7000 * n + Q)
            circ, asg, enc = circuit_arrays(ref, pyr, n, Q)
            tr = [pyr.randrange(1, R) for _ in range(8 + 2 * Q)]
            want = orc.prove(osrs, n, Q, enc["wL"], enc["wR"], enc["wO"], enc["cs"], enc["aL"], enc["aR"], enc["aO"], fr_bytes(tr))
            out[(n, Q)] = dict(circ=circ, asg=asg, tr=tr, oracle=bytes(want),
                               circuit=sonic.ArithCircuit(sonic.GateWeights(circ[0], circ[1], circ[2]), circ[3]))
    return out


# ---- head equality and alternation ----
@pytest.mark.parametrize("Q", SMALL_QS)
@pytest.mark.parametrize("n", SMALL_NS)
def test_core_is_the_head_of_the_full_proof_and_of_the_oracle(sonic, small_srs, small_cases, n, Q):
    c = small_cases[(n, Q)]
    head = c["oracle"][:cref.CORE_SIZE]
    for form in ("dense", "csr"):
        circuit = c["circuit"] if form == "dense" else sonic.SparseCircuit.from_circuit(c["circuit"])
        for prepare in (False, True):
            p = sonic.Prover(small_srs, circuit, prepare=prepare)
            try:
                p.set_assignment(sonic.Assignment(*c["asg"]))
                core = p.prove_core_bytes(c["tr"][:6])                      # (first on the handle: nothing of a full proof to lean on)
                assert core == head, (form, prepare)
                # full, core, full, core: neither disturbs the other
                for _ in range(2):
                    assert p.prove_bytes(c["tr"]) == c["oracle"], (form, prepare)
                    assert p.prove_core_bytes(c["tr"][:6]) == head, (form, prepare)
                # the elements a core proof never draws do not reach it
                other = c["tr"][:6] + [v + 1 for v in c["tr"][6:]]
                assert p.prove_bytes(other)[:cref.CORE_SIZE] == head and p.prove_core_bytes(other[:6]) == head
            finally:
                p.close()


def test_core_on_a_group_wise_plan_and_over_an_srs_view(sonic, small_srs, small_cases, monkeypatch):
    n, Q = 257, 2
    c = small_cases[(n, Q)]
    head = c["oracle"][:cref.CORE_SIZE]
    monkeypatch.setenv("SONIC_PROVE_FUSED", "0")             # one chain per group instead of one per proof
    p = sonic.Prover(small_srs, c["circuit"], prepare=False)
    try:
        p.set_assignment(sonic.Assignment(*c["asg"]))
        assert p.prove_core_bytes(c["tr"][:6]) == head
        assert p.prove_bytes(c["tr"]) == c["oracle"]
        assert p.prove_core_bytes(c["tr"][:6]) == head
    finally:
        p.close()
    monkeypatch.delenv("SONIC_PROVE_FUSED")
    view = small_srs.for_circuit(n, Q)
    p = sonic.Prover(view, c["circuit"])
    try:
        p.set_assignment(sonic.Assignment(*c["asg"]))
        assert p.prove_core_bytes(c["tr"][:6]) == head
        assert p.prove_bytes(c["tr"]) == c["oracle"]
    finally:
        p.close()
        view.close()


def test_core_between_the_replays_of_a_captured_proof(sonic, small_srs, small_cases, monkeypatch):
    """SONIC_PROVE_GRAPH=1: the handle captures a full proof's enqueue and replays it; core proofs run by direct launches between the
    replays, and neither disturbs the other"""
    n, Q = 257, 2
    c = small_cases[(n, Q)]
    head = c["oracle"][:cref.CORE_SIZE]
    monkeypatch.setenv("SONIC_PROVE_GRAPH", "1")
    p = sonic.Prover(small_srs, c["circuit"])
    monkeypatch.delenv("SONIC_PROVE_GRAPH")
    try:
        p.set_assignment(sonic.Assignment(*c["asg"]))
        assert p.prove_core_bytes(c["tr"][:6]) == head              # the handle's first proof
        for _ in range(3):                                          # full: direct, captured, replayed -- a core proof after each
            assert p.prove_bytes(c["tr"]) == c["oracle"]
            assert p.prove_core_bytes(c["tr"][:6]) == head
        p.submit_core(c["tr"][:6])
        assert p.collect_core() == head
        assert p.prove_bytes(c["tr"]) == c["oracle"]
    finally:
        p.close()


def test_core_at_a_multi_tile_size(sonic):
    """n = 3 * 4096 + 5, Q = 2 against the oracle's head stored in tests/golden (tools/gen_core_golden.py: ~25 s of CPU per run otherwise)"""
    g = json.load(open(os.path.join(HERE, "golden", "core_head_big.json")))
    n, Q, head = g["n"], g["Q"], bytes.fromhex(g["head"])
    assert n == 3 * 4096 + 5 and Q == 2 and len(head) == cref.CORE_SIZE
    pyr = random.Random(g["transcript_seed"])
    tr = [pyr.randrange(1, R) for _ in range(8 + 2 * Q)]
    c = big_circuit(g["circuit_seed"], n, Q)
    srs = sonic.SRS.new(g["d"], g["x"], g["alpha"])
    circuit = sonic.ArithCircuit(sonic.GateWeights(c["wL"], c["wR"], c["wO"]), c["cs"])
    try:
        for circ, prepare in ((circuit, False), (circuit, True), (sonic.SparseCircuit.from_circuit(circuit), False)):
            p = sonic.Prover(srs, circ, prepare=prepare)
            try:
                p.set_assignment(sonic.Assignment(c["aL"], c["aR"], c["aO"]))
                core = p.prove_core_bytes(tr[:6])
                assert core == head
                assert p.prove_bytes(tr)[:cref.CORE_SIZE] == head
                assert p.prove_core_bytes(tr[:6]) == head
            finally:
                p.close()
        assert sonic.verify_core(srs, circuit, head, tr[4], tr[5])
    finally:
        srs.close()


# ---- flights ----
def random_statements(sonic, prover, n, K, seed):
    """K assignments with aO = aL * aR and the constants each satisfies under the handle's weights"""
    pyr = random.Random(seed)
    asgs = []
    for _ in range(K):
        aL, aR = [pyr.randrange(R) for _ in range(n)], [pyr.randrange(R) for _ in range(n)]
        asgs.append(sonic.Assignment(aL, aR, [a * b % R for a, b in zip(aL, aR)]))
    cs, gates = prover.eval_constraints(asgs)
    assert all(g == (0, -1) for g in gates)
    return asgs, cs


def test_submit_and_collect_core_over_two_handles(sonic, small_srs, small_cases):
    n, Q = 5, 2
    c = small_cases[(n, Q)]
    A, B = sonic.Prover(small_srs, c["circuit"]), sonic.Prover(small_srs, c["circuit"], prepare=False)
    try:
        asgs, cs = random_statements(sonic, A, n, 4, 31)
        pyr = random.Random(32)
        trs = [[pyr.randrange(1, R) for _ in range(6)] for _ in range(4)]
        alone = []
        for k in range(4):                          # one at a time, blocking
            p = (A, B)[k % 2]
            p.set_assignment(asgs[k]); p.set_constants(cs[k])
            alone.append(p.prove_core_bytes(trs[k]))
        assert len(set(alone)) == 4
        for k in (0, 2):                            # two in flight, collected in the other order
            A.set_assignment(asgs[k]); A.set_constants(cs[k]); A.submit_core(trs[k])
            B.set_assignment(asgs[k + 1]); B.set_constants(cs[k + 1]); B.submit_core(trs[k + 1])
            assert B.collect_core() == alone[k + 1] and A.collect_core() == alone[k]
        # each is the head of the full proof of its statement
        full_tr = trs[3] + [pyr.randrange(1, R) for _ in range(2 + 2 * Q)]
        assert B.prove_bytes(full_tr)[:cref.CORE_SIZE] == alone[3]
        for k in range(4):
            stmt = sonic.ArithCircuit(c["circuit"].weights, cs[k])
            assert sonic.verify_core(small_srs, stmt, alone[k], trs[k][4], trs[k][5])
    finally:
        A.close(); B.close()


def test_flight_misuse_is_refused_and_the_flight_survives(sonic, small_srs, small_cases):
    n, Q = 5, 2
    c = small_cases[(n, Q)]
    head = c["oracle"][:cref.CORE_SIZE]
    p = sonic.Prover(small_srs, c["circuit"])
    try:
        p.set_assignment(sonic.Assignment(*c["asg"]))
        assert refused(sonic, INVALID_ARG, p.collect_core)                     # nothing in flight
        # a core flight: the other collects refuse it and leave it
        p.submit_core(c["tr"][:6])
        for other in (p.collect, p.collect_share, p.collect_fs):
            assert refused(sonic, INVALID_ARG, other)
        assert refused(sonic, INVALID_ARG, lambda: p.submit_core(c["tr"][:6]))   # one proof in flight per handle
        assert refused(sonic, INVALID_ARG, lambda: p.prove_core_bytes(c["tr"][:6]))
        assert refused(sonic, INVALID_ARG, lambda: p.set_assignment(sonic.Assignment(*c["asg"])))
        assert p.collect_core() == head
        assert refused(sonic, INVALID_ARG, p.collect_core)
        # a transcript flight and a Fiat-Shamir flight: collect_core refuses them and leaves them
        p.submit(c["tr"])
        assert refused(sonic, INVALID_ARG, p.collect_core)
        assert p.collect() == c["oracle"]
        digest = sonic.fs_circuit_digest(c["circuit"])
        p.submit_fs(digest, seed_of("misuse"))
        assert refused(sonic, INVALID_ARG, p.collect_core)
        raw, _ = p.collect_fs()
        assert sonic.verify_fs(small_srs, c["circuit"], sonic.Proof.from_bytes(raw, Q))
        # a zero challenge is the status of a full proof's
        assert refused(sonic, INEXACT_DIVISION, lambda: p.prove_core_bytes(c["tr"][:4] + [0, c["tr"][5]]))
        assert refused(sonic, INEXACT_DIVISION, lambda: p.prove_core_bytes(c["tr"][:5] + [0]))
        assert p.prove_core_bytes(c["tr"][:6]) == head
        # share mode refuses core calls; back in whole-proof mode they work again
        p.set_share(0, 2)
        assert refused(sonic, INVALID_ARG, lambda: p.prove_core_bytes(c["tr"][:6]))
        assert refused(sonic, INVALID_ARG, lambda: p.submit_core(c["tr"][:6]))
        assert refused(sonic, INVALID_ARG, lambda: p.prove_core_fs(digest, seed_of("share")))
        assert refused(sonic, INVALID_ARG, lambda: sonic.prove_core_batch([p], [c["tr"][:6]]))
        p.set_share(0, 1)
        assert p.prove_core_bytes(c["tr"][:6]) == head
    finally:
        p.close()


# ---- verification ----
def other_points(sonic, srs, k):
    """k valid points that no proof here holds: g^{x^e}"""
    return [sonic.g1_from_bytes(b.tobytes()) for b in srs.points(0, 1, k)]


def test_verify_core_accepts_the_head_and_rejects_every_change(sonic, small_srs, small_cases):
    n, Q = 5, 2
    c = small_cases[(n, Q)]
    y, z = c["tr"][4], c["tr"][5]
    full = sonic.Proof.from_bytes(c["oracle"], Q)
    core = full.core()
    assert core.to_bytes() == c["oracle"][:cref.CORE_SIZE] == sonic.CoreProof.from_bytes(core.to_bytes(compressed=True)).to_bytes()
    assert len(core.to_bytes(compressed=True)) == cref.CORE_SIZE_Z
    sparse = sonic.SparseCircuit.from_circuit(c["circuit"])
    for circuit in (c["circuit"], sparse):
        assert sonic.verify_core(small_srs, circuit, core, y, z)
        assert sonic.verify_core(small_srs, circuit, full, y, z)                  # the recipe for an existing full proof
        assert sonic.verify_core(small_srs, circuit, core.to_bytes(compressed=True), y, z)
    from dataclasses import replace
    for field in ("prS", "prA", "prB"):
        assert sonic.verify_core(small_srs, c["circuit"], replace(core, **{field: (getattr(core, field) + 1) % R}), y, z) is False, field
    for field, pt in zip(("prR", "prT", "prWa", "prWb", "prWt"), other_points(sonic, small_srs, 5)):
        assert sonic.verify_core(small_srs, c["circuit"], replace(core, **{field: pt}), y, z) is False, field
        assert sonic.verify_core(small_srs, sparse, replace(core, **{field: pt}), y, z) is False, field
    assert sonic.verify_core(small_srs, c["circuit"], core, (y + 1) % R, z) is False
    assert sonic.verify_core(small_srs, c["circuit"], core, y, (z + 1) % R) is False
    assert sonic.verify_core(small_srs, c["circuit"], core, z, y) is False
    # another statement of the same weights
    assert sonic.verify_core(small_srs, sonic.ArithCircuit(c["circuit"].weights, [c["circ"][3][0] + 1] + c["circ"][3][1:]), core, y, z) is False
    assert refused(sonic, INEXACT_DIVISION, lambda: sonic.verify_core(small_srs, c["circuit"], core, 0, z))
    assert refused(sonic, INEXACT_DIVISION, lambda: sonic.verify_core(small_srs, c["circuit"], core, y, 0))
    assert refused(sonic, BAD_ENCODING, lambda: sonic.verify_core(small_srs, c["circuit"], replace(core, prS=R), y, z))


def forge(sonic, srs, n, cs, y, z, pyr):
    """A head that satisfies the three pcV equations of `verify` for ANY statement, without a witness: any r(X) on R's support and any
    t'(X) without a constant term, committed and opened honestly, and s SOLVED from t'(z) = a (b + s) - k(y)."""
    r = {e: pyr.randrange(1, R) for e in range(-2 * n - 4, n + 1) if e != 0}
    t = {e: pyr.randrange(1, R) for e in range(-4 * n - 8, 3 * n + 1) if e != 0}
    d = srs.srsD
    cR, cT = sonic.commit_poly(srs, n, r), sonic.commit_poly(srs, d, t)
    a, wa = sonic.open_poly(srs, z, r)
    b, wb = sonic.open_poly(srs, y * z % R, r)
    tz, wt = sonic.open_poly(srs, z, t)
    ky = sum(c * pow(y, n + 1 + q, R) for q, c in enumerate(cs)) % R
    s = ((tz + ky) * pow(a, -1, R) - b) % R
    return sonic.CoreProof(cR, cT, a, wa, b, wb, wt, s)


def test_the_forgery_that_verify_accepts_is_rejected(sonic, orc, ref):
    """n = 2, Q = 2, d = 22, a statement the assignment does not satisfy.  sonic_verify ACCEPTS the forged proof -- the reference's
    behaviour (Protocol.hs:119-126 reads prS once, and the signature is made at pairs drawn independently of y, z), byte-faithfully kept,
    and the reason core proofs exist.  verify_core and verify_core_batch reject it."""
    n, Q, d = 2, 2, 22
    pyr = random.Random(2022)
    circ, asg, enc = circuit_arrays(ref, pyr, n, Q)
    tr = [pyr.randrange(1, R) for _ in range(8 + 2 * Q)]
    y, z, yzs = tr[4], tr[5], list(zip(tr[6:6 + Q], tr[6 + Q:6 + 2 * Q]))
    srs = sonic.SRS.new(d, X, ALPHA)
    honest_circuit = sonic.ArithCircuit(sonic.GateWeights(circ[0], circ[1], circ[2]), circ[3])
    false_cs = [(circ[3][0] + 5) % R, (circ[3][1] + 11) % R]
    false_circuit = sonic.ArithCircuit(honest_circuit.weights, false_cs)
    try:
        honest, _ = sonic.prove(srs, sonic.Assignment(*asg), honest_circuit, transcript=tr)
        assert sonic.verify(srs, honest_circuit, honest, y, z, yzs) and sonic.verify_core(srs, honest_circuit, honest, y, z)
        # the assignment does not satisfy the false statement, and an honest proof of the true one does not pass for it
        assert [sum(w * a for w, a in zip(circ[0][q] + circ[1][q] + circ[2][q], asg[0] + asg[1] + asg[2])) % R for q in range(Q)] == circ[3] != false_cs
        assert sonic.verify(srs, false_circuit, honest, y, z, yzs) is False
        head = forge(sonic, srs, n, false_cs, y, z, pyr)
        forged = sonic.Proof(head.prR, head.prT, head.prA, head.prWa, head.prB, head.prWb, head.prWt, head.prS, honest.prHscProof)
        v = sonic.Verifier(srs, false_circuit)
        try:
            s_true = v.eval_s([(z, y)])[0]
            assert head.prS != s_true
            # the gap: every check of the reference-shaped verifiers holds
            assert sonic.verify(srs, false_circuit, forged, y, z, yzs) is True
            assert v.verify_batch([forged], [(y, z, yzs)]) is True
            # closed
            assert sonic.verify_core(srs, false_circuit, head, y, z) is False
            assert sonic.verify_core(srs, false_circuit, forged, y, z) is False
            assert v.verify_core_batch([head], [(y, z)], each=True) == (False, [False])
            assert v.verify_core_batch([forged.core().to_bytes(compressed=True)], [(y, z)], seed=seed_of("forged")) is False
            # (with the true s in its place the equations fail instead: the forger cannot have both)
            from dataclasses import replace
            assert sonic.verify_core(srs, false_circuit, replace(head, prS=s_true), y, z) is False
        finally:
            v.close()
    finally:
        srs.close()


# ---- batched ----
@pytest.fixture(scope="module")
def batch17(sonic, small_srs, small_cases):
    """17 core proofs of 17 statements of one circuit (n = 5, Q = 2), made by prove_core_batch over two handles"""
    n, Q, K = 5, 2, 17
    c = small_cases[(n, Q)]
    A, B = sonic.Prover(small_srs, c["circuit"]), sonic.Prover(small_srs, c["circuit"])
    try:
        asgs, cs = random_statements(sonic, A, n, K, 51)
        pyr = random.Random(52)
        trs = [[pyr.randrange(1, R) for _ in range(6)] for _ in range(K)]
        proofs = sonic.prove_core_batch([A, B], trs, assignments=asgs, constants=cs)
        # the same through one handle, statement by statement, and from a WitnessBatch of the resident kind
        for k in (0, 16):
            A.set_assignment(asgs[k]); A.set_constants(cs[k])
            assert A.prove_core_bytes(trs[k]) == proofs[k]
        A.set_constants(cs[3]); A.set_assignment(asgs[3])
        assert sonic.prove_core_batch([A], [trs[3]]) == [proofs[3]]                   # (the resident assignment and constants)
    finally:
        A.close(); B.close()
    yzs = [(t[4], t[5]) for t in trs]
    return dict(n=n, Q=Q, K=K, c=c, proofs=proofs, yzs=yzs, cs=cs, pyr=pyr)


@pytest.mark.parametrize("K", [1, 3, 17])
def test_verify_core_batch_equals_per_proof_verify_core(sonic, small_srs, batch17, K):
    b = batch17
    c, Q = b["c"], b["Q"]
    proofs, yzs, cs = b["proofs"][:K], b["yzs"][:K], b["cs"][:K]
    v = sonic.Verifier(small_srs, c["circuit"])
    try:
        for k in range(K):
            assert sonic.verify_core(small_srs, sonic.ArithCircuit(c["circuit"].weights, cs[k]), proofs[k], *yzs[k])
        zs = [sonic.CoreProof.from_bytes(p).to_bytes(compressed=True) for p in proofs]
        for form in (proofs, zs):
            assert v.verify_core_batch(form, yzs, constants=cs) is True
            assert v.verify_core_batch(form, yzs, constants=cs, each=True, seed=seed_of(K)) == (True, [True] * K)
        # against the handle's own constants every proof of another statement fails, and only those
        own = [sonic.verify_core(small_srs, c["circuit"], proofs[k], *yzs[k]) for k in range(K)]
        assert not any(own)
        assert v.verify_core_batch(proofs, yzs, each=True) == (False, own)
        if K < 3:
            return
        # one forged, one with a non-canonical s, one with a point off the curve, one with a point outside the subgroup: each rejects
        # its own proof only, in either encoding of the rest
        bad = list(proofs)
        forged = forge(sonic, small_srs, b["n"], cs[0], *yzs[0], random.Random(53))
        bad[0] = forged.to_bytes()
        bad[1] = proofs[1][:544] + R.to_bytes(32, "little")
        want = [False, False] + [True] * (K - 2)
        if K > 3:
            bad[2] = proofs[2][:96] + (1).to_bytes(48, "little") + (1).to_bytes(48, "little") + proofs[2][192:]           # T = (1, 1): not on the curve
            bad[4] = proofs[4][:448] + (0).to_bytes(48, "little") + (2).to_bytes(48, "little") + proofs[4][544:]          # W_t = (0, 2): order 3
            want[2] = want[4] = False
        for k in range(K):
            stmt = sonic.ArithCircuit(c["circuit"].weights, cs[k])
            assert rejects(lambda: sonic.verify_core(small_srs, stmt, bad[k], *yzs[k])) == (not want[k]), k
        first = v.verify_core_batch(bad, yzs, constants=cs, each=True, seed=seed_of("bad"))
        assert first == (False, want)
        assert v.verify_core_batch(bad, yzs, constants=cs, each=True, seed=seed_of("bad")) == first                      # a fixed seed: the same verdicts
        assert v.verify_core_batch(bad, yzs, constants=cs, each=True) == first                                          # and a drawn one
        assert v.verify_core_batch(bad, yzs, constants=cs) is False
        # compressed: the forged proof and the one with the non-canonical s travel as they are (their points are valid)
        zbad = [sonic.CoreProof.from_bytes(p).to_bytes(compressed=True) for p in proofs]
        zbad[0] = forged.to_bytes(compressed=True)
        zbad[1] = zs[1][:304] + R.to_bytes(32, "little")
        zbad[2] = zs[2][:48] + bytes([0x80 | 0x1f]) + b"\xff" * 47 + zs[2][96:]                                          # x >= q: malformed
        assert v.verify_core_batch(zbad, yzs, constants=cs, each=True, seed=seed_of("zbad")) == (False, [False] * 3 + [True] * (K - 3))
        # a non-canonical cs_k, a zero y_k and a zero z_k reject proof k and fail nothing
        cs_bad = [list(k) for k in cs]
        cs_bad[1] = R.to_bytes(32, "little") + int(cs[1][1]).to_bytes(32, "little")
        assert v.verify_core_batch(proofs, yzs, constants=cs_bad, each=True) == (False, [True, False] + [True] * (K - 2))
        yz0 = list(yzs)
        yz0[0], yz0[2] = (0, yzs[0][1]), (yzs[2][0], 0)
        assert v.verify_core_batch(proofs, yz0, constants=cs, each=True) == (False, [False, True, False] + [True] * (K - 3))
        # swapped challenges of two good proofs: both rejected, the rest stand
        yzx = [yzs[1], yzs[0]] + yzs[2:]
        assert v.verify_core_batch(proofs, yzx, constants=cs, each=True) == (False, [False, False] + [True] * (K - 2))
    finally:
        v.close()


# ---- Fiat-Shamir ----
def test_core_fs_matches_a_hashlib_transcript_and_verifies(sonic, small_srs, small_cases):
    n, Q = 5, 2
    c = small_cases[(n, Q)]
    circuit, d = c["circuit"], SMALL_D
    digest, srs_id = sonic.fs_circuit_digest(circuit), sonic.fs_srs_id(small_srs)
    seed = seed_of("fs")
    p = sonic.Prover(small_srs, circuit)
    v = sonic.Verifier(small_srs, circuit)
    try:
        p.set_assignment(sonic.Assignment(*c["asg"]))
        raw, y, z = p.prove_core_fs(digest, seed)
        assert p.witness_digest() == fref.witness_digest_v2(*c["asg"])
        # the test's own walk: blinders from witness digest v2, R -> y, T -> z, each from a core proof driven with what is known so far
        bl = fref.blinders(seed, digest, srs_id, p.witness_digest())
        R_bytes = p.prove_core_bytes(bl + [1, 1])[:96]
        t = cref.Transcript(b"sonic-hip/fs-core/v1", n, Q, d, digest, srs_id)
        t.absorb(b"R", R_bytes)
        y1 = t.challenge(b"y")
        T_bytes = p.prove_core_bytes(bl + [y1, 1])[96:192]
        t.absorb(b"T", T_bytes)
        z1 = t.challenge(b"z")
        assert (y, z) == (y1, z1) == cref.core_challenges(n, Q, d, digest, srs_id, raw) == sonic.fs_core_challenges(small_srs, circuit, raw)
        assert raw == p.prove_core_bytes(bl + [y1, z1])
        assert p.prove_core_fs(digest, seed) == (raw, y, z)
        assert sonic.verify_core_fs(small_srs, circuit, raw) and sonic.verify_core(small_srs, circuit, raw, y, z)
        assert sonic.verify_core_fs(small_srs, sonic.SparseCircuit.from_circuit(circuit), sonic.CoreProof.from_bytes(raw))
        assert v.verify_core_fs_batch([raw], each=True) == (True, [True])
        # one byte of R changed: no longer a point of the subgroup, or another transcript -- rejected either way
        flipped = bytes([raw[0] ^ 1]) + raw[1:]
        assert rejects(lambda: sonic.verify_core_fs(small_srs, circuit, flipped))
        assert v.verify_core_fs_batch([flipped, raw], each=True) == (False, [False, True])
        # R replaced by another valid point: well-formed, another y, rejected
        swapped = sonic.CoreProof.from_bytes(raw)
        swapped.prR = other_points(sonic, small_srs, 1)[0]
        assert sonic.verify_core_fs(small_srs, circuit, swapped) is False
        assert sonic.fs_core_challenges(small_srs, circuit, swapped)[0] != y
        # not the head of the full Fiat-Shamir proof for the same seed: the same blinders, so the same R -- and another label, another y
        p.submit_fs(digest, seed)
        full, ftr = p.collect_fs()
        assert ftr[:4] == bl and full[:96] == raw[:96]
        assert ftr[4] != y and full[:cref.CORE_SIZE] != raw
        assert ftr[4:6] == list(cref.full_challenges_yz(n, Q, d, digest, srs_id, full))
        # so neither passes for the other: the full proof's head is no core Fiat-Shamir proof (it IS sound under its own y, z) ...
        assert sonic.verify_core_fs(small_srs, circuit, full[:cref.CORE_SIZE]) is False
        assert sonic.verify_core(small_srs, circuit, sonic.Proof.from_bytes(full, Q), ftr[4], ftr[5])
        # ... and the core proof, completed with the full proof's signature, is no full Fiat-Shamir proof
        assert sonic.verify_fs(small_srs, circuit, sonic.Proof.from_bytes(raw + full[cref.CORE_SIZE:], Q)) is False
    finally:
        p.close(); v.close()


def test_prove_core_batch_fs_equals_the_per_proof_calls(sonic, small_srs, small_cases):
    n, Q, K = 5, 2, 5
    c = small_cases[(n, Q)]
    A, B = sonic.Prover(small_srs, c["circuit"]), sonic.Prover(small_srs, c["circuit"], prepare=False)
    v = sonic.Verifier(small_srs, c["circuit"])
    try:
        asgs, cs = random_statements(sonic, A, n, K, 61)
        mid = sonic.fs_circuit_midstate(c["circuit"])
        digests = [sonic.fs_circuit_digest_resume(mid, k) for k in cs]
        seeds = [seed_of(("batch", k)) for k in range(K)]
        got = sonic.prove_core_batch_fs([A, B], digests, seeds, assignments=asgs, constants=cs)
        for k in range(K):
            A.set_assignment(asgs[k]); A.set_constants(cs[k])
            assert A.prove_core_fs(digests[k], seeds[k]) == got[k], k
            stmt = sonic.ArithCircuit(c["circuit"].weights, cs[k])
            assert sonic.verify_core_fs(small_srs, stmt, got[k][0])
            assert (got[k][1], got[k][2]) == sonic.fs_core_challenges(small_srs, stmt, got[k][0])
        assert len({g[0] for g in got}) == K
        assert v.verify_core_fs_batch([g[0] for g in got], constants=cs, each=True) == (True, [True] * K)
        assert v.verify_core_batch([g[0] for g in got], [(g[1], g[2]) for g in got], constants=cs) is True
        # under the handle's own constants the transcripts are others: every proof rejected
        assert v.verify_core_fs_batch([g[0] for g in got], each=True) == (False, [False] * K)
        # a WitnessBatch of numpy arrays: the same proofs
        wb = sonic.WitnessBatch(*[np.stack([fr_bytes(getattr(a, k)) for a in asgs]) for k in ("aL", "aR", "aO")])
        assert sonic.prove_core_batch_fs([B, A], digests, seeds, assignments=wb, constants=cs) == got
    finally:
        A.close(); B.close(); v.close()


# ---- the boundary from plain C99 ----
def test_c99_harness(sonic, tmp_path):
    """core proofs through include/sonic_hip.h alone (tests/host/core_proof_harness.c): prove_core, the flights, verify_core, the error contract"""
    root = os.path.dirname(HERE)
    exe = str(tmp_path / "core_proof_harness")
    subprocess.check_call(["gcc", "-std=c99", "-pedantic", "-Wall", "-Wextra", "-Werror", "-I" + os.path.join(root, "include"),
                           os.path.join(HERE, "host", "core_proof_harness.c"), "-L" + os.path.join(root, "sonic_amd", "csrc"), "-lsonic_hip",
                           "-Wl,-rpath," + os.path.join(root, "sonic_amd", "csrc"), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and "core_proof_harness: OK" in out.stdout, out.stdout + out.stderr
