"""Circuits with Q ~ n on the GPU (include/sonic_hip.h, "Circuits with Q ~ n"): weights digest v2 from the resident CSR of a prover and of a
verifier handle against the hashlib restatement (tests/weights_digest_ref.py) at every tree and row shape of the host test; verifier handles
of digest kind 1 and 2 under Fiat-Shamir core proofs and helped batches; the prover's per-pair state, which appears with the first full
proof and changes no byte; and a compiled R1CS with n < Q end to end under the v2 digests.  Every comparison is byte equality.

Shapes: n <= 64 for the digests except nnz = 16385 (n = 128, Q = 43); n = 8, Q = 5 for the Fiat-Shamir and helped cases.  The lazy-state
cases use n = 2048, not 256: a fresh handle keeps 5 Q + 8 MSM slots of 12 304 bytes, so two handles of Q = 64 and Q = 128 differ by 3.9 MB
in O(Q) buffers alone, above the bound 32 * 64 * (3n + 1) / 2 at n = 256 (0.79 MB) and below it at n = 2048 (6.3 MB); the Q n term that the
bound is about would be 12.6 MB there.
"""
import ctypes as C
import random

import numpy as np
import pytest

import r1cs_ref as rref
import weights_digest_ref as wref
from weights_digest_ref import CASES
from util import R

pytestmark = pytest.mark.gpu

INVALID_ARG = 7


@pytest.fixture(scope="module")
def srs(sonic):
    rng = random.Random(71)
    s = sonic.SRS.new(1024, rng.randrange(2, R), rng.randrange(2, R))      # d >= 7 n for n <= 128
    yield s
    s.close()


def sparse_of(sonic, c):
    return sonic.SparseCircuit(c.n, c.Q, c.row_ptr, c.col, c.val, c.cs)


def random_rows(rng, n, Q, max_len, zeros=True):
    """3Q rows of at most max_len entries as {gate: value}; with `zeros` some values are explicit zeros, and some rows are empty"""
    pick = lambda: rng.choice([0, 1, R - 1, rng.randrange(R)]) if zeros else rng.randrange(1, R)      # noqa: E731
    rows = [{j: pick() for j in rng.sample(range(n), rng.randrange(0, max_len + 1))} for _ in range(3 * Q)]
    return rows[:Q], rows[Q:2 * Q], rows[2 * Q:]


def statement(rng, n, rows):
    """a random assignment with aO = aL aR and the constants it satisfies under the rows"""
    aL, aR = [rng.randrange(R) for _ in range(n)], [rng.randrange(R) for _ in range(n)]
    aO = [a * b % R for a, b in zip(aL, aR)]
    wL, wR, wO = rows
    cs = [(sum(v * aL[j] for j, v in wL[q].items()) + sum(v * aR[j] for j, v in wR[q].items()) + sum(v * aO[j] for j, v in wO[q].items())) % R for q in range(len(wL))]
    return (aL, aR, aO), cs


# ---- digests ----
@pytest.mark.parametrize("case", CASES, ids=[c.name for c in CASES])
def test_handles_compute_the_restatements_digest(sonic, srs, case):
    want = case.digest()
    sp = sparse_of(sonic, case)
    p = sonic.Prover(srs, sp, prepare=False)
    assert p.weights_digest_v2() == want
    p.close()
    for kind in (1, 2):
        v = sonic.Verifier(srs, sp, digest=kind)
        assert v.digest_kind == kind and v.weights_digest_v2() == want, kind
        v.close()


def test_a_dense_prover_handle_is_refused_and_the_value_is_cached(sonic, srs):
    from sonic_amd import _lib
    case = next(c for c in CASES if c.name == "nnz513")
    sp = sparse_of(sonic, case)
    dense = sonic.Prover(srs, sp.to_dense(), prepare=False)
    with pytest.raises(sonic.SonicError) as e:
        dense.weights_digest_v2()
    assert e.value.code == INVALID_ARG and "from CSR" in str(e.value)
    dense.close()
    # a verifier made from the dense weights holds their non-zero entries: the digest of SparseCircuit.from_circuit
    v = sonic.Verifier(srs, sp.to_dense())
    assert v.digest_kind == 1 and v.weights_digest_v2() == sonic.fs_weights_digest_v2(sp.to_dense()) != case.digest()
    v.close()
    p = sonic.Prover(srs, sp, prepare=False)
    L = _lib.lib()
    assert L.sonic_profile_reset() == 0 and L.sonic_profile_enable(1) == 0
    try:
        first, second = p.weights_digest_v2(), p.weights_digest_v2()
        ms, launches = C.c_double(0), C.c_int64(0)
        assert L.sonic_profile_get(b"k_weights_leaves", C.byref(ms), C.byref(launches)) == 0
    finally:
        L.sonic_profile_enable(0)
    assert first == second == case.digest() and launches.value == 1      # the second call launched nothing
    p.close()


# ---- Fiat-Shamir core proofs and helped batches under both kinds, n = 8, Q = 5 ----
@pytest.fixture(scope="module")
def small(sonic, srs):
    rng = random.Random(85)
    n, Q = 8, 5
    rows = random_rows(rng, n, Q, 4)
    rows[0][0][3] = 0                                          # (an explicit zero, whatever the draws were)
    stm = [statement(rng, n, rows) for _ in range(2)]
    sp = sonic.SparseCircuit.from_rows(n, *rows, stm[0][1])
    assert 0 in [int.from_bytes(bytes(v), "little") for v in sp.val]      # (explicit zeros are entries)
    wd2 = wref.weights_digest_v2(n, Q, sp.row_ptr.tolist(), sp.col.tolist(), [int.from_bytes(bytes(v), "little") for v in sp.val])
    p = sonic.Prover(srs, sp, prepare=False)
    assert p.weights_digest_v2() == wd2 == sonic.fs_weights_digest_v2(sp)
    mid = sonic.fs_circuit_midstate(sp)
    out = {"n": n, "Q": Q, "sp": sp, "wd2": wd2, "wd1": sonic.fs_weights_digest(sp), "cs": [s[1] for s in stm], "proofs": {1: [], 2: []}}
    for k, (asg, cs) in enumerate(stm):
        p.set_assignment(sonic.Assignment(*asg))
        p.set_constants(cs)
        cd2 = wref.circuit_digest_v2(wd2, cs)
        assert cd2 == sonic.fs_circuit_digest_v2(wd2, cs)
        out["proofs"][2].append(p.prove_core_fs(cd2, bytes([k + 1]) * 32))
        out["proofs"][1].append(p.prove_core_fs(sonic.fs_circuit_digest_resume(mid, cs), bytes([k + 1]) * 32))
    out["agg"] = {}
    for kind, wd in ((1, out["wd1"]), (2, wd2)):
        out["agg"][kind] = p.aggregate_core([(y, z) for _, y, z in out["proofs"][kind]], weights_digest=wd)
    p.close()
    return out


def test_digest_kind_1_is_the_verifier_of_today_and_kind_2_the_same_over_digest_v2(sonic, srs, small):
    from sonic_amd import _lib
    sp, cs = small["sp"], small["cs"]
    today, v1, v2 = sonic.Verifier(srs, sp), sonic.Verifier(srs, sp, digest=1), sonic.Verifier(srs, sp, digest=2)
    # (Verifier(digest=1) goes through sonic_verifier_new_csr: the new entry point with digest_kind = 1, through the C ABI, as a handle of its own)
    v1_abi = sonic.Verifier.__new__(sonic.Verifier)
    v1_abi.n, v1_abi.Q, v1_abi._srs, v1_abi._h = sp.n, sp.Q, srs, C.c_void_p()
    _lib.check(_lib.lib().sonic_verifier_new_digest(srs._h, sp.n, sp.Q, *sp._args(), sp.cs.ctypes.data, 1, C.byref(v1_abi._h)))
    assert (today.digest_kind, v1.digest_kind, v1_abi.digest_kind, v2.digest_kind) == (1, 1, 1, 2)
    with pytest.raises(ValueError):
        sonic.Verifier(srs, sp, digest=3)
    h = C.c_void_p()
    assert _lib.lib().sonic_verifier_new_digest(srs._h, sp.n, sp.Q, *sp._args(), sp.cs.ctypes.data, 3, C.byref(h)) == INVALID_ARG and not h
    seed = b"\x05" * 32
    for kind, v in ((1, today), (1, v1), (1, v1_abi), (2, v2)):
        own, other = [pf for pf, _, _ in small["proofs"][kind]], [pf for pf, _, _ in small["proofs"][3 - kind]]
        # the handle's statement is statement 0; with constants, each proof against its own
        assert v.verify_core_fs_batch(own[:1], seed=seed, each=True) == (True, [True])
        assert v.verify_core_fs_batch(own, seed=seed, each=True, constants=cs) == (True, [True, True])
        # statement 1's proof under the handle's constants, a flipped byte, and the bytes made under the other kind: rejected, not an error
        assert v.verify_core_fs_batch(own[1:], seed=seed, each=True) == (False, [False])
        bent = bytearray(own[0]); bent[200] ^= 1
        assert v.verify_core_fs_batch([bytes(bent), own[1]], seed=seed, each=True, constants=cs) == (False, [False, True])
        assert v.verify_core_fs_batch(other[:1], seed=seed, each=True) == (False, [False])
        assert v.verify_core_fs_batch(other, seed=seed, each=True, constants=cs) == (False, [False, False])
        # with the challenges given, the proof's bytes verify under either kind: the kinds differ in the digests alone
        yzs = [(y, z) for _, y, z in small["proofs"][3 - kind]]
        assert v.verify_core_batch(other, yzs, seed=seed, each=True, constants=cs) == (True, [True, True])
    # (A handle does not give out the batch digest it folds under, so this file cannot hold it against sonic_verify_core_batch_digest.
    # What the cases above pin is the circuit digest the handle derives -- the Fiat-Shamir challenges come from it, and the batch digest is
    # fs_core_batch_digest over the same field of the handle.)
    for v in (today, v1, v1_abi, v2):
        v.close()


def test_helped_batches_bind_the_weights_digest_of_the_handles_kind(sonic, srs, small):
    sp, cs = small["sp"], small["cs"]
    seed = b"\x06" * 32
    for kind in (1, 2):
        v = sonic.Verifier(srs, sp, digest=kind)
        proofs = [pf for pf, _, _ in small["proofs"][kind]]
        yzs = [(y, z) for _, y, z in small["proofs"][kind]]
        assert v.verify_core_batch_helped(proofs, yzs, small["agg"][kind], seed=seed, each=True, constants=cs) == (True, [True, True])
        assert v.verify_core_fs_batch_helped(proofs, small["agg"][kind], seed=seed, each=True, constants=cs) == (True, [True, True])
        # the aggregate made under the other kind's weights digest, over the same pairs: every proof rejected
        from_other = sonic.Prover(srs, sp, prepare=False)
        agg = from_other.aggregate_core(yzs, weights_digest=small["wd1" if kind == 2 else "wd2"])
        from_other.close()
        assert v.verify_core_batch_helped(proofs, yzs, agg, seed=seed, each=True, constants=cs) == (False, [False, False])
        v.close()


# ---- the per-pair state ----
LAZY_N = 2048


@pytest.fixture(scope="module")
def lazy(sonic):
    rng = random.Random(93)
    s = sonic.SRS.new(7 * LAZY_N, rng.randrange(2, R), rng.randrange(2, R))
    out = {"srs": s}
    for Q in (64, 128):
        rows = random_rows(rng, LAZY_N, Q, 4, zeros=False)
        asg, cs = statement(rng, LAZY_N, rows)
        out[Q] = (sonic.SparseCircuit.from_rows(LAZY_N, *rows, cs), sonic.Assignment(*asg))
    out["tr"] = [[rng.randrange(1, R) for _ in range(8 + 2 * 64)] for _ in range(2)]
    yield out
    s.close()


def test_fresh_handles_hold_nothing_proportional_to_q_times_n(sonic, lazy):
    n = LAZY_N
    fresh = {}
    for Q in (64, 128):
        p = sonic.Prover(lazy["srs"], lazy[Q][0], prepare=False)
        fresh[Q] = p.device_bytes
        p.close()
    assert 0 < fresh[64] <= fresh[128]
    assert fresh[128] - fresh[64] < 32 * 64 * (3 * n + 1) // 2, fresh


@pytest.mark.parametrize("form", ["csr", "dense", "prepared"])
def test_pair_state_appears_with_the_first_full_proof_and_changes_no_byte(sonic, lazy, form):
    n, Q = LAZY_N, 64
    sp, asg = lazy[Q]
    circuit = sp.to_dense() if form == "dense" else sp
    tr = lazy["tr"]

    def handle():
        p = sonic.Prover(lazy["srs"], circuit, prepare=(form == "prepared"))
        p.set_assignment(asg)
        return p

    a = handle()
    core0 = a.prove_core_bytes(tr[0][:6])
    after_first = a.device_bytes
    others = [a.prove_core_bytes(tr[k][:6]) for k in (1, 0, 1)]
    assert others[1] == core0 and others[0] == others[2] != core0
    assert a.device_bytes == after_first                       # three more core proofs: not one byte more
    full0 = a.prove_bytes(tr[0])
    assert a.device_bytes - after_first >= 32 * Q * (3 * n + 1)
    # core, full, core, full on one handle
    assert core0 == full0[:576]
    core1 = a.prove_core_bytes(tr[0][:6])
    full1 = a.prove_bytes(tr[0])
    assert core1 == core0 == full1[:576] and full1 == full0
    a.close()
    # a second handle that makes a full proof first
    b = handle()
    assert b.prove_bytes(tr[0]) == full0
    assert b.prove_core_bytes(tr[0][:6]) == core0
    b.close()


# ---- a compiled R1CS with n < Q, end to end under the v2 digests ----
def always_satisfiable(rng, n_in, m, N):
    """z = (1, n_in inputs, N - 1 - n_in products): row i < P multiplies two combinations of earlier columns into column 1 + n_in + i; the
    rows behind are <a, z> * 1 = <a, z>.  Every choice of inputs has its witness."""
    P = N - 1 - n_in
    A, B, Cm = [], [], []
    for i in range(m):
        if i < P:
            top = 1 + n_in + i
            a = rref.random_row(rng, top, rng.randrange(1, 4))
            if i == 0:
                a = sorted(dict(a + [(1, 1), (2, 1)]).items())      # (both public inputs are read)
            A.append(a); B.append(rref.random_row(rng, top, rng.randrange(1, 4))); Cm.append([(top, 1)])
        else:
            a = rref.random_row(rng, N, rng.randrange(1, 4))
            A.append(a); B.append([(0, 1)]); Cm.append(list(a))

    def solve(inputs):
        z = [1] + [v % R for v in inputs]
        for i in range(P):
            z.append(rref.dot(A[i], z) * rref.dot(B[i], z) % R)
        return z
    return A, B, Cm, solve


def test_end_to_end_compiled_r1cs_under_digest_v2(sonic, srs):
    import torch
    rng = random.Random(97)
    m, N, n_in, n_pub, K = 64, 40, 9, 2, 3
    A, B, Cm, solve = always_satisfiable(rng, n_in, m, N)
    r = sonic.R1CS.from_rows(N, n_pub, [dict(x) for x in A], [dict(x) for x in B], [dict(x) for x in Cm])
    assert (r.n, r.Q) == (84, 194) and r.n < r.Q
    # three witnesses: witness 1 has one changed PUBLIC input, witness 2 one changed private input; each is solved for, so each satisfies
    inputs = [rng.randrange(R) for _ in range(n_in)]
    zs = [solve(inputs), solve([(inputs[0] + 1) % R] + inputs[1:]), solve(inputs[:5] + [(inputs[5] + 1) % R] + inputs[6:])]
    za = np.frombuffer(b"".join(v.to_bytes(32, "little") for z in zs for v in z), np.uint8).reshape(K, N, 32)
    wb, cs, bad = r.assign(torch.from_numpy(za.copy()).to(f"cuda:{r.device}"))
    assert bad == [(0, -1)] * K
    assert [c[3 * m:] for c in cs] == [z[1:3] for z in zs] and cs[0] == cs[2] != cs[1]
    circuit = r.circuit(public=zs[0][1:3])
    p = sonic.Prover(srs, circuit, prepare=False)
    wd2 = p.weights_digest_v2()
    assert wd2 == sonic.fs_weights_digest_v2(circuit) == wref.weights_digest_v2(r.n, r.Q, circuit.row_ptr.tolist(), circuit.col.tolist(),
                                                                                 [int.from_bytes(bytes(v), "little") for v in circuit.val])
    digests = [sonic.fs_circuit_digest_v2(wd2, c) for c in cs]
    seeds = [bytes([k + 9]) * 32 for k in range(K)]
    proofs = sonic.prove_core_batch_fs([p], digests, seeds, wb, constants=cs)
    v = sonic.Verifier(srs, circuit, digest=2)
    assert v.weights_digest_v2() == wd2
    raws = [pf for pf, _, _ in proofs]
    assert v.verify_core_fs_batch(raws, seed=b"\x07" * 32, each=True, constants=cs) == (True, [True, True, True])
    # every proof held against the public inputs of witness 0: exactly the proof of the witness whose public input differs is rejected
    assert v.verify_core_fs_batch(raws, seed=b"\x07" * 32, each=True, constants=[cs[0]] * K) == (False, [True, False, True])
    assert v.verify_core_fs_batch(raws, seed=b"\x07" * 32, each=True) == (False, [True, False, True])      # (the handle's own statement is witness 0's)
    # the same bytes on a verifier of kind 1: rejected
    v1 = sonic.Verifier(srs, circuit, digest=1)
    assert v1.verify_core_fs_batch(raws, seed=b"\x07" * 32, each=True, constants=cs) == (False, [False, False, False])
    for h in (v, v1, p, r):
        h.close()


def test_the_digest_v2_example_runs(sonic):
    import os
    import sys
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "examples"))
    try:
        import r1cs_digest_v2
    finally:
        sys.path.pop(0)
    assert r1cs_digest_v2.run_example() is True
