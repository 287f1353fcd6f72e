"""Gate weights as CSR on the GPU (include/sonic_hip.h, "gate weights as CSR"): a CSR handle, the one-shot sonic_prove_csr and the sparse
verifiers give the bytes and answers of the dense path for the densified circuit -- against the CPU oracle at small shapes, against the
dense handle (which the rest of the suite pins to the oracle) at n = 2^14 -- and a shape that dense input cannot reasonably reach
(n = 2^16, Q = 128: 805 MB of dense weights) proves and verifies.

Reference: Sonic.Protocol.prove / verify (src/Sonic/Protocol.hs:47-130), sPoly (src/Sonic/Constraints.hs:34-53)."""
import ctypes as C
import random

import numpy as np
import pytest

from util import NCPU, R, big_circuit, fr_bytes, rand_fr_array

pytestmark = pytest.mark.gpu


def _ints(a):
    return [int.from_bytes(a[i].tobytes(), "little") for i in range(a.shape[0])]


def _satisfied(sonic, n, Q, row_ptr, col, val, seed):
    """a SparseCircuit over the given rows whose constants make a random assignment (aO = aL aR) satisfy it"""
    rng = np.random.default_rng(seed)
    aL, aR = rand_fr_array(rng, n), rand_fr_array(rng, n)
    la, lb = _ints(aL), _ints(aR)
    lo = [a * b % R for a, b in zip(la, lb)]
    vals = _ints(val) if len(val) else []
    cs = [0] * Q
    for r in range(3 * Q):
        m, q = divmod(r, Q)
        a = (la, lb, lo)[m]
        for k in range(int(row_ptr[r]), int(row_ptr[r + 1])):
            cs[q] = (cs[q] + vals[k] * a[int(col[k])]) % R
    sp = sonic.SparseCircuit(n, Q, row_ptr, col, val, fr_bytes(cs))
    return sp, sonic.Assignment(aL, aR, fr_bytes(lo))


def _random_rows(n, Q, k, seed):
    rng = np.random.default_rng(seed)
    counts = rng.integers(0, min(k, n) + 1, size=3 * Q)
    rp = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
    col = np.concatenate([np.sort(rng.choice(n, size=int(c), replace=False)) for c in counts]).astype(np.int64)
    return rp, col, rand_fr_array(rng, int(rp[-1]))


def _edge_rows(kind, n, Q, seed):
    rng = np.random.default_rng(seed)
    if kind == "empty":
        return np.zeros(3 * Q + 1, np.int64), np.zeros(0, np.int64), np.zeros((0, 32), np.uint8)
    if kind == "dense_row":                      # one fully dense row of wO, every other row empty
        rp = np.zeros(3 * Q + 1, np.int64); rp[2 * Q + 1:] = n
        return rp, np.arange(n, dtype=np.int64), rand_fr_array(rng, n)
    if kind == "one_gate":                       # gate n // 2 in every row
        return np.arange(3 * Q + 1, dtype=np.int64), np.full(3 * Q, n // 2, np.int64), rand_fr_array(rng, 3 * Q)
    if kind == "zeros":                          # explicit zero values among the entries
        rp, col, val = _random_rows(n, Q, 4, seed)
        val[::2] = 0
        return rp, col, val
    raise ValueError(kind)


def _dense_args(sp):
    d = sp.to_dense()
    w = d.weights
    return [np.ascontiguousarray(x).reshape(-1, 32) for x in (w.wL, w.wR, w.wO)] + [np.ascontiguousarray(d.cs)]


def _tr(Q, seed):
    pyr = random.Random(seed)
    return [pyr.randrange(1, R) for _ in range(8 + 2 * Q)]


CASES = [(1, 1, "random"), (7, 3, "random"), (257, 16, "random"), (5000, 3, "random"), (257, 3, "empty"), (257, 3, "dense_row"),
         (257, 3, "one_gate"), (257, 3, "zeros"), (7, 16, "one_gate")]


@pytest.mark.parametrize("n,Q,kind", CASES)
def test_csr_handle_matches_the_oracle(sonic, orc, n, Q, kind):
    """prepared and unprepared CSR handles, prove and submit / collect, against the oracle on the densified circuit"""
    seed = 1000 * n + 10 * Q + len(kind)
    rows = _random_rows(n, Q, 4, seed) if kind == "random" else _edge_rows(kind, n, Q, seed)
    sp, asg = _satisfied(sonic, n, Q, *rows, seed)
    pyr = random.Random(seed)
    d = 7 * n + 12 + pyr.randrange(20)
    x, alpha = pyr.randrange(2, R), pyr.randrange(2, R)
    g = sonic.SRS.new(d, x, alpha)
    o = orc.SRS(d, x, alpha, threads=NCPU)
    tr = _tr(Q, seed)
    wL, wR, wO, cs = _dense_args(sp)
    orc.set_mode(1, NCPU)
    want = orc.prove(o, n, Q, wL, wR, wO, cs, asg.aL, asg.aR, asg.aO, fr_bytes(tr), n >= 256)
    for prepare in (True, False):
        p = sonic.Prover(g, sp, prepare=prepare)
        p.set_assignment(asg)
        assert p.prove_bytes(tr) == want, prepare
        p.submit(tr)
        assert p.collect() == want, prepare
        p.close()
    g.close()


@pytest.mark.parametrize("kind,Q", [("rnd", 2), ("sparse", 16), ("sparse", 64)])
def test_csr_handle_matches_the_dense_handle_at_2_14(sonic, kind, Q):
    from sonic_amd import workload
    n = 1 << 14
    if kind == "rnd":                              # rndCircuit: one row of n ones per matrix (the worst skew for the row sums)
        b = big_circuit(77, n, Q)
        rp, col, val = workload.csr_from_dense(b["wL"], b["wR"], b["wO"], n, Q)
        sp = sonic.SparseCircuit(n, Q, rp, col, val, b["cs"])
        asg = sonic.Assignment(b["aL"], b["aR"], b["aO"])
    else:
        c = workload.sparse_circuit(Q, n, Q, 4)
        sp = sonic.SparseCircuit(n, Q, c["row_ptr"], c["col"], c["val"], c["cs"])
        asg = sonic.Assignment(c["aL"], c["aR"], c["aO"])
    g = sonic.SRS.new(7 * n + 9, 3, 5)
    tr = _tr(Q, n + Q)
    dense = sonic.Prover(g, sp.to_dense(), prepare=True)
    dense.set_assignment(asg)
    want = dense.prove_bytes(tr)
    dense.close()
    for prepare in (True, False):
        p = sonic.Prover(g, sp, prepare=prepare)
        p.set_assignment(asg)
        assert p.prove_bytes(tr) == want, prepare
        p.close()
    g.close()


def test_other_handle_operations_match_dense(sonic):
    """hsc_prove, prove_fs (proof and transcript), prove_shared over two handles of one GPU and prove_batch on CSR handles"""
    n, Q = 300, 3
    rows = _random_rows(n, Q, 4, 5)
    sp, asg = _satisfied(sonic, n, Q, *rows, 5)
    dc = sp.to_dense()
    g = sonic.SRS.new(7 * n + 9, 11, 13)
    pd, pc = sonic.Prover(g, dc, prepare=False), sonic.Prover(g, sp, prepare=False)
    for p in (pd, pc):
        p.set_assignment(asg)
    yzs = [(7, 9), (11, 13), (17, 19), (23, 29)]
    assert pc.hsc_prove(yzs, 31, 37) == pd.hsc_prove(yzs, 31, 37)
    digest = sonic.fs_circuit_digest(dc)
    assert sonic.fs_circuit_digest(sp) == digest
    seed = bytes(range(32))
    assert pc.prove_fs(digest, seed) == pd.prove_fs(digest, seed)
    tr = _tr(Q, 99)
    want = pd.prove_bytes(tr)
    assert pc.prove_bytes(tr) == want
    pc2 = sonic.Prover(g, sp, prepare=False)                        # (the ranks of one proof plan alike: both unprepared)
    pc2.set_assignment(asg)
    assert sonic.prove_shared([pc, pc2], tr) == want
    trs = [_tr(Q, 100 + i) for i in range(3)]
    for p in (pc, pc2):
        p.set_share(0, 1)
    assert sonic.prove_batch([pc, pc2], trs) == sonic.prove_batch([pd], trs)
    for p in (pd, pc, pc2):
        p.close()
    g.close()


def test_sparse_verifiers(sonic):
    """verify_csr / verify_fs_csr accept the proofs of a CSR handle and reject a flipped byte; the dense verify_fs accepts a CSR handle's
    prove_fs proof (one digest for both forms)"""
    n, Q = 200, 3
    rows = _random_rows(n, Q, 4, 21)
    sp, asg = _satisfied(sonic, n, Q, *rows, 21)
    g = sonic.SRS.new(7 * n + 9, 41, 43)
    tr = _tr(Q, 21)
    proof, oracle = sonic.prove(g, asg, sp, transcript=tr)
    assert sonic.verify(g, sp, proof, oracle.rndOracleY, oracle.rndOracleZ, oracle.rndOracleYZs)
    assert sonic.verify(g, sp.to_dense(), proof, oracle.rndOracleY, oracle.rndOracleZ, oracle.rndOracleYZs)
    raw = bytearray(proof.to_bytes())
    raw[200] ^= 1                                                    # inside a
    bad = sonic.Proof.from_bytes(bytes(raw), Q)
    assert not sonic.verify(g, sp, bad, oracle.rndOracleY, oracle.rndOracleZ, oracle.rndOracleYZs)
    fproof, _ = sonic.prove_fs(g, asg, sp, blinder_seed=bytes(32))
    assert sonic.verify_fs(g, sp, fproof) and sonic.verify_fs(g, sp.to_dense(), fproof)
    raw = bytearray(fproof.to_bytes())
    raw[200] ^= 1
    assert not sonic.verify_fs(g, sp, sonic.Proof.from_bytes(bytes(raw), Q))
    g.close()


def test_one_shot_alternates_dense_and_csr_over_parked_shells(sonic, orc):
    from sonic_amd import _lib
    n, Q = 257, 3
    pyr = random.Random(5)
    d = 7 * n + 20
    x, alpha = pyr.randrange(2, R), pyr.randrange(2, R)
    g = sonic.SRS.new(d, x, alpha)
    o = orc.SRS(d, x, alpha, threads=NCPU)
    orc.set_mode(1, NCPU)
    _lib.lib().sonic_one_shot_trim(-1)
    for i in range(6):
        rows = _random_rows(n, Q, 4, 50 + i) if i % 3 else _edge_rows("dense_row", n, Q, 50 + i)
        sp, asg = _satisfied(sonic, n, Q, *rows, 50 + i)
        tr = _tr(Q, 50 + i)
        wL, wR, wO, cs = _dense_args(sp)
        want = orc.prove(o, n, Q, wL, wR, wO, cs, asg.aL, asg.aR, asg.aO, fr_bytes(tr), True)
        circ = sp if i % 2 == 0 else sp.to_dense()                  # CSR, dense, CSR, ... on the same (n, Q)
        pr, _ = sonic.prove(g, asg, circ, transcript=tr)
        assert pr.to_bytes() == want, i
    g.close()


def test_error_contract(sonic):
    from sonic_amd import _lib
    L = _lib.lib()
    n, Q = 40, 2
    rows = _random_rows(n, Q, 4, 3)
    sp, asg = _satisfied(sonic, n, Q, *rows, 3)
    h = C.c_void_p()
    small = sonic.SRS.new(7 * n - 1, 3, 5)                          # d too small
    assert L.sonic_prover_new_csr(small._h, n, Q, *sp._args(), sp.cs.ctypes.data, C.byref(h)) == 1
    a = np.ascontiguousarray(asg.aL)
    out = C.create_string_buffer(L.sonic_proof_size(Q))
    trb = fr_bytes(_tr(Q, 1))
    assert L.sonic_prove_csr(small._h, n, Q, *sp._args(), sp.cs.ctypes.data, a.ctypes.data, a.ctypes.data, a.ctypes.data, trb.ctypes.data, out) == 1
    small.close()
    g = sonic.SRS.new(7 * n, 3, 5)                                  # d = 7n exactly: every P_q term is inside [-d, d]
    bad_rp = sp.row_ptr.copy(); bad_rp[0] = 1
    assert L.sonic_prover_new_csr(g._h, n, Q, bad_rp.ctypes.data, sp._args()[1], sp._args()[2], sp.cs.ctypes.data, C.byref(h)) == 7
    assert "row 0" in _lib.last_error()
    assert L.sonic_prove_csr(g._h, n, Q, bad_rp.ctypes.data, sp._args()[1], sp._args()[2], sp.cs.ctypes.data, a.ctypes.data, a.ctypes.data,
                             a.ctypes.data, trb.ctypes.data, out) == 7
    nc = sp.val.copy()
    if nc.shape[0]:
        nc[0] = np.frombuffer(R.to_bytes(32, "little"), np.uint8)
        assert L.sonic_prover_new_csr(g._h, n, Q, sp.row_ptr.ctypes.data, sp.col.ctypes.data, nc.ctypes.data, sp.cs.ctypes.data, C.byref(h)) == 3
    # prepare at d = 7n: dense and CSR agree (both succeed: no P_q term leaves the SRS)
    pc, pd = sonic.Prover(g, sp, prepare=True), sonic.Prover(g, sp.to_dense(), prepare=True)
    for p in (pc, pd):
        p.set_assignment(asg)
    tr = _tr(Q, 2)
    assert pc.prove_bytes(tr) == pd.prove_bytes(tr)
    zero = list(tr); zero[5] = 0                                     # a zero transcript element (z)
    for p in (pc, pd):
        with pytest.raises(sonic.SonicError) as e:
            p.prove_bytes(zero)
        assert e.value.code == 4
    pc.close(); pd.close()
    g.close()


def test_a_shape_dense_input_cannot_reasonably_reach(sonic):
    """n = 2^16, Q = 128, <= 4 entries per row: dense weights would be 3 Q n 32 B = 805 MB; the CSR holds ~1.5 K entries"""
    from sonic_amd import workload
    n, Q = 1 << 16, 128
    c = workload.sparse_circuit(2026, n, Q, 4)
    sp = sonic.SparseCircuit(n, Q, c["row_ptr"], c["col"], c["val"], c["cs"])
    g = sonic.SRS.new(7 * n + 9, 7, 9)
    p = sonic.Prover(g, sp, prepare=True)
    p.set_assignment(sonic.Assignment(c["aL"], c["aR"], c["aO"]))
    tr = _tr(Q, 7)
    proof = sonic.Proof.from_bytes(p.prove_bytes(tr), Q)
    p.close()
    t = [v % R for v in tr]
    assert sonic.verify(g, sp, proof, t[4], t[5], list(zip(t[6:6 + Q], t[6 + Q:6 + 2 * Q])))
    g.close()
