"""Helped verification on the GPU (include/sonic_hip.h, "Helped verification").  The helper: sonic_prover_aggregate_core against
sonic_prover_hsc_prove on the same handle -- with u, v from the hashlib transcript of tests/aggregate_ref.py -- against sonic_hsc_verify and
against the CPU oracle's hsc_prove; the tile and group edges, both SONIC_AGG_KEEP settings, an SRS view, and the error contract.  The helped
verifier: its verdicts against verify_core_batch and against the slow composition from calls that existed before, both point encodings,
per-proof constants, the Fiat-Shamir form, the digest its randomizers bind, and the rejections, each with its exact `each` vector.  Every
comparison is byte equality or a verdict.  The small shapes and the one string of tests/test_gpu_core_proofs.py."""
import os
import random
import subprocess
import sys

import pytest

import aggregate_ref as aref
from util import R, circuit_arrays

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SMALL_NS, SMALL_QS = [1, 2, 5, 257], [1, 2, 5]
SMALL_D = 7 * 257 + 6
X, ALPHA = 0x1234567891, 0x987654321
INVALID_ARG, BAD_ENCODING, INEXACT_DIVISION = 7, 3, 4


def refused(code, fn):
    from sonic_amd import _lib
    with pytest.raises(_lib.SonicError) as e:
        fn()
    assert e.value.code == code, e.value
    return True


@pytest.fixture(scope="module")
def small_srs(sonic):
    g = sonic.SRS.new(SMALL_D, X, ALPHA)
    yield g
    g.close()


def circuit_of(sonic, ref, n, Q):
    pyr = random.Random(9000 * n + Q)
    circ, asg, _enc = circuit_arrays(ref, pyr, n, Q)
    return sonic.ArithCircuit(sonic.GateWeights(circ[0], circ[1], circ[2]), circ[3]), asg, circ


def pairs(seed, K):
    pyr = random.Random(seed)
    return [(pyr.randrange(1, R), pyr.randrange(1, R)) for _ in range(K)]


def challenges(sonic, srs, circuit, n, Q, yzs, agg):
    """u, v of an aggregate by the hashlib restatement, from what a verifier holds"""
    wd = aref.weights_digest(sonic.fs_circuit_midstate(circuit))
    return aref.aggregate_challenges(n, Q, srs.srsD, wd, sonic.fs_srs_id(srs), yzs, agg)


def hsc_bytes(sonic, prover, yzs, u, v):
    from sonic_amd.protocol import _hsc_to_bytes
    return _hsc_to_bytes(prover.hsc_prove(yzs, u, v))


def check_aggregate(sonic, srs, circuit, prover, n, Q, yzs, what):
    """the aggregate's u, v are its transcript's, and sonic_prover_hsc_prove with them reproduces it byte for byte"""
    K = len(yzs)
    agg = prover.aggregate_core(yzs)
    assert len(agg) == aref.aggregate_size(K), what
    u, v = challenges(sonic, srs, circuit, n, Q, yzs, agg)
    p = aref.parts(K, agg)
    assert (p["u"], p["v"]) == (aref.fr(u), aref.fr(v)), what
    assert agg == hsc_bytes(sonic, prover, yzs, u, v), what
    return agg


# ---- bytes ----
@pytest.mark.parametrize("Q", SMALL_QS)
@pytest.mark.parametrize("n", SMALL_NS)
def test_aggregate_is_hsc_prove_under_its_own_transcript(sonic, ref, small_srs, n, Q):
    """dense and CSR, prepared and not (a prepared handle commits S_j as the diagonal part plus the Q-term sum over the C_q): one aggregate,
    which sonic_hsc_verify accepts and which the library's own transcript call and the Python one agree on"""
    from sonic_amd.protocol import _hsc_from_bytes
    circuit, _asg, _circ = circuit_of(sonic, ref, n, Q)
    K = 3
    yzs = pairs(100 * n + Q, K)
    seen = set()
    for form in ("dense", "csr"):
        c = circuit if form == "dense" else sonic.SparseCircuit.from_circuit(circuit)
        for prepare in (False, True):
            p = sonic.Prover(small_srs, c, prepare=prepare)
            try:
                seen.add(check_aggregate(sonic, small_srs, circuit, p, n, Q, yzs, (form, prepare)))
            finally:
                p.close()
    assert len(seen) == 1
    agg = seen.pop()
    assert sonic.hsc_verify(small_srs, circuit, yzs, _hsc_from_bytes(agg, K))
    u, v = sonic.fs_aggregate_challenges(small_srs, circuit, yzs, agg)
    assert (aref.fr(u), aref.fr(v)) == (aref.parts(K, agg)["u"], aref.parts(K, agg)["v"])
    # another order of the same pairs is another aggregate: u binds the order
    other = list(reversed(yzs))
    assert sonic.fs_aggregate_challenges(small_srs, circuit, other, agg) != (u, v)


@pytest.mark.parametrize("K", [1, 7, 8, 9, 15, 16, 17, 33])
def test_tile_and_group_edges(sonic, ref, small_srs, K):
    """tiles of 8 pairs, chains of 16 jobs, six lanes: a tile that is not full, exactly one, one pair into the next, and more tiles than lanes"""
    n, Q = 5, 2
    circuit, _asg, _circ = circuit_of(sonic, ref, n, Q)
    yzs = pairs(500 + K, K)
    for c, prepare in ((circuit, True), (sonic.SparseCircuit.from_circuit(circuit), False)):
        p = sonic.Prover(small_srs, c, prepare=prepare)
        try:
            agg = check_aggregate(sonic, small_srs, circuit, p, n, Q, yzs, (K, prepare))
            assert p.aggregate_core(yzs) == agg                      # and again on the same handle: nothing of the first call is left behind
        finally:
            p.close()


CHILD = r"""
import random, sys
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, sys.argv[1] + "/tests")
import sonic_amd as sonic
from oracle import sonic_ref as ref
from util import R, circuit_arrays
n, Q, K, d = 257, 2, 17, int(sys.argv[2])
circ, asg, enc = circuit_arrays(ref, random.Random(9000 * n + Q), n, Q)
circuit = sonic.ArithCircuit(sonic.GateWeights(circ[0], circ[1], circ[2]), circ[3])
pyr = random.Random(77)
yzs = [(pyr.randrange(1, R), pyr.randrange(1, R)) for _ in range(K)]
srs = sonic.SRS.new(d, 0x1234567891, 0x987654321)
for c, prepare in ((circuit, True), (circuit, False), (sonic.SparseCircuit.from_circuit(circuit), False)):
    p = sonic.Prover(srs, c, prepare=prepare)
    print("agg", p.aggregate_core(yzs).hex())
    p.close()
"""


def test_both_keep_settings_give_the_same_bytes(sonic, ref, small_srs):
    """SONIC_AGG_KEEP=1 keeps the polynomials of pass 1 for pass 2, =0 recomputes them tile by tile: each in a fresh process of its own"""
    n, Q, K = 257, 2, 17
    circuit, _asg, _circ = circuit_of(sonic, ref, n, Q)
    pyr = random.Random(77)
    yzs = [(pyr.randrange(1, R), pyr.randrange(1, R)) for _ in range(K)]
    p = sonic.Prover(small_srs, circuit)
    try:
        want = check_aggregate(sonic, small_srs, circuit, p, n, Q, yzs, "parent").hex()
    finally:
        p.close()
    for keep in ("0", "1"):
        out = subprocess.run(["timeout", "-k", "10", "120", sys.executable, "-c", CHILD, ROOT, str(SMALL_D)], capture_output=True, text=True,
                             env=dict(os.environ, SONIC_AGG_KEEP=keep))
        assert out.returncode == 0, (keep, out.stdout[-500:], out.stderr[-2000:])
        got = [ln.split()[1] for ln in out.stdout.splitlines() if ln.startswith("agg ")]
        assert got == [want] * 3, keep


def test_against_the_cpu_oracle(sonic, ref):
    """n = 2, Q = 2, K = 3 over a string of d = 20: oracle/sonic_ref.py's hsc_prove with the aggregate's u, v"""
    n, Q, K, d = 2, 2, 3, 20
    circuit, _asg, circ = circuit_of(sonic, ref, n, Q)
    yzs = pairs(31, K)
    srs = sonic.SRS.new(d, X, ALPHA)
    p = sonic.Prover(srs, circuit)
    try:
        agg = check_aggregate(sonic, srs, circuit, p, n, Q, yzs, "oracle")
    finally:
        p.close()
        srs.close()
    u, v = (int.from_bytes(aref.parts(K, agg)[k], "little") for k in ("u", "v"))
    w = ref.hsc_prove(ref.SRS(d, X, ALPHA), ref.s_poly(circ[0], circ[1], circ[2]), yzs, u, v)
    G, F = ref.g1_to_bytes, ref.fr_to_bytes
    want = b"".join(G(cm) + F(fz) + G(W) for cm, (fz, W) in w["hscS"]) + b"".join(F(sp) + G(wp) + G(q) for sp, wp, q in w["hscW"]) \
        + G(w["hscQv"]) + G(w["hscC"]) + F(w["hscU"]) + F(w["hscV"])
    assert agg == want


def test_over_an_srs_view(sonic, ref, small_srs):
    from sonic_amd.protocol import _hsc_from_bytes
    n, Q, K = 257, 2, 9
    circuit, _asg, _circ = circuit_of(sonic, ref, n, Q)
    yzs = pairs(41, K)
    view = small_srs.for_circuit(n, Q)
    p = sonic.Prover(view, circuit)
    try:
        agg = check_aggregate(sonic, view, circuit, p, n, Q, yzs, "view")
    finally:
        p.close()
        view.close()
    assert sonic.hsc_verify(small_srs, circuit, yzs, _hsc_from_bytes(agg, K))


# ---- what a helper ships ----
def test_aggregate_links_to_the_core_proofs_and_lists_the_mismatched(sonic, ref, small_srs):
    """s_k of the aggregate is s(z_k, y_k): the s of an honest core proof made at (y_k, z_k).  sonic_amd.aggregate_core lists the proofs
    whose s differs, and the slow composition from existing calls -- the transcript, hsc_verify, s equality, verify_core -- accepts the rest"""
    from sonic_amd.protocol import _hsc_from_bytes
    n, Q, K = 5, 2, 3
    circuit, asg, _circ = circuit_of(sonic, ref, n, Q)
    pyr = random.Random(51)
    trs = [[pyr.randrange(1, R) for _ in range(6)] for _ in range(K)]
    yzs = [(tr[4], tr[5]) for tr in trs]
    p = sonic.Prover(small_srs, circuit)
    try:
        p.set_assignment(sonic.Assignment(*asg))
        proofs = [p.prove_core_bytes(tr) for tr in trs]
        agg, mismatched = sonic.aggregate_core(p, proofs, yzs)
        assert mismatched == [] and [aref.s_of(K, agg, k) for k in range(K)] == [pf[544:576] for pf in proofs]
        forged = bytearray(proofs[1])
        forged[544] ^= 1
        agg2, mismatched = sonic.aggregate_core(p, [proofs[0], bytes(forged), proofs[2]], yzs)
        assert agg2 == agg and mismatched == [1]
    finally:
        p.close()
    u, v = sonic.fs_aggregate_challenges(small_srs, circuit, yzs, agg)
    assert aref.fr(u) + aref.fr(v) == agg[-64:]
    assert sonic.hsc_verify(small_srs, circuit, yzs, _hsc_from_bytes(agg, K))
    assert all(sonic.verify_core(small_srs, circuit, pf, y, z) for pf, (y, z) in zip(proofs, yzs))
    # a signature over other pairs does not vouch for these proofs: its transcript differs and so does its s_k
    swapped = [yzs[1], yzs[0], yzs[2]]
    assert sonic.fs_aggregate_challenges(small_srs, circuit, swapped, agg) != (u, v)
    assert not sonic.hsc_verify(small_srs, circuit, swapped, _hsc_from_bytes(agg, K))


# ---- the error contract ----
def test_refusals(sonic, ref, small_srs):
    n, Q = 5, 2
    circuit, asg, _circ = circuit_of(sonic, ref, n, Q)
    yzs = pairs(61, 3)
    p = sonic.Prover(small_srs, circuit)
    try:
        for bad in ([(0, 5)] + yzs, yzs + [(7, 0)]):
            assert refused(INEXACT_DIVISION, lambda: p.aggregate_core(bad))
        from sonic_amd import _lib
        out = bytes(aref.aggregate_size(1))
        assert _lib.lib().sonic_prover_aggregate_core(p._h, bytes(32), 1, aref.fr(5) + R.to_bytes(32, "little"), out) == BAD_ENCODING
        assert _lib.lib().sonic_prover_aggregate_core(p._h, bytes(32), 0, bytes(64), out) == INVALID_ARG
        assert _lib.lib().sonic_prover_aggregate_core(p._h, None, 1, bytes(64), out) == INVALID_ARG
        # a proof in flight: refused, and the flight is intact
        p.set_assignment(sonic.Assignment(*asg))
        tr = [random.Random(62).randrange(1, R) for _ in range(6)]
        want = p.prove_core_bytes(tr)
        agg = p.aggregate_core(yzs)
        p.submit_core(tr)
        assert refused(INVALID_ARG, lambda: p.aggregate_core(yzs))
        assert p.collect_core() == want
        assert p.aggregate_core(yzs) == agg                          # and the refusals left the handle as it was
        # a handle in share mode proves pieces of a proof, not signatures
        p.set_share(0, 2)
        assert refused(INVALID_ARG, lambda: p.aggregate_core(yzs))
    finally:
        p.close()


# ---- the helped verifier ----
def seed_of(tag) -> bytes:
    import hashlib
    return hashlib.sha256(b"helped-%s" % str(tag).encode()).digest()


def forge(sonic, srs, n, cs, y, z, pyr):
    """the forged head of tests/test_gpu_core_proofs.py: any r(X) and t'(X) committed and opened honestly, s SOLVED from
    t'(z) = a (b + s) - k(y) -- the three equations of the head hold for a statement nobody has a witness of"""
    r = {e: pyr.randrange(1, R) for e in range(-2 * n - 4, n + 1) if e != 0}
    t = {e: pyr.randrange(1, R) for e in range(-4 * n - 8, 3 * n + 1) if e != 0}
    cR, cT = sonic.commit_poly(srs, n, r), sonic.commit_poly(srs, srs.srsD, t)
    a, wa = sonic.open_poly(srs, z, r)
    b, wb = sonic.open_poly(srs, y * z % R, r)
    tz, wt = sonic.open_poly(srs, z, t)
    ky = sum(c * pow(y, n + 1 + q, R) for q, c in enumerate(cs)) % R
    return sonic.CoreProof(cR, cT, a, wa, b, wb, wt, ((tz + ky) * pow(a, -1, R) - b) % R)


def lying_aggregate(sonic, srs, circuit, n, Q, yzs, agg, k, s_forged: bytes) -> bytes:
    """the aggregate of a helper that states s_forged as s_k and is honest otherwise: S_j, W_j as they are, u from the transcript over the
    lie, C, W'_j, Q_j honestly at that u, v from the transcript, Q_v honestly at that v -- assembled from sonic_prover_hsc_prove, whose
    parts do not depend on the draws that follow them.  Every equation holds but `S_k opens to s_k at z_k`."""
    K = len(yzs)
    wd, sid = sonic.fs_weights_digest(circuit), sonic.fs_srs_id(srs)
    hscS = bytearray(aref.parts(K, agg)["hscS"])
    hscS[224 * k + 96:224 * k + 128] = s_forged
    p = sonic.Prover(srs, circuit)
    try:
        draft = bytes(hscS) + agg[224 * K:]
        u, _ = aref.aggregate_challenges(n, Q, srs.srsD, wd, sid, yzs, draft)
        second = hsc_bytes(sonic, p, yzs, u, 1)                                   # C and the second list at u
        draft = bytes(hscS) + second[224 * K:]
        u2, v = aref.aggregate_challenges(n, Q, srs.srsD, wd, sid, yzs, draft)
        assert u2 == u
        last = hsc_bytes(sonic, p, yzs, u, v)                                     # Q_v at v
    finally:
        p.close()
    assert last[224 * K:448 * K] == second[224 * K:448 * K]
    return bytes(hscS) + last[224 * K:]


@pytest.fixture(scope="module")
def batch17(sonic, ref, small_srs):
    """17 core proofs of 17 statements of one circuit (n = 5, Q = 2) at drawn (y_k, z_k), and the aggregates over the first 1, 3 and 17"""
    n, Q, K = 5, 2, 17
    circuit, _asg, _circ = circuit_of(sonic, ref, n, Q)
    pyr = random.Random(71)
    A, B = sonic.Prover(small_srs, circuit), sonic.Prover(small_srs, sonic.SparseCircuit.from_circuit(circuit), prepare=False)
    try:
        asgs = []
        for _ in range(K):
            aL, aR = [pyr.randrange(R) for _ in range(n)], [pyr.randrange(R) for _ in range(n)]
            asgs.append(sonic.Assignment(aL, aR, [a * b % R for a, b in zip(aL, aR)]))
        cs, gates = A.eval_constraints(asgs)
        assert all(g == (0, -1) for g in gates)
        trs = [[pyr.randrange(1, R) for _ in range(6)] for _ in range(K)]
        proofs = sonic.prove_core_batch([A, B], trs, assignments=asgs, constants=cs)
        yzs = [(t[4], t[5]) for t in trs]
        aggs = {k: (A if k != 3 else B).aggregate_core(yzs[:k]) for k in (1, 3, 17)}
    finally:
        A.close(); B.close()
    return dict(n=n, Q=Q, circuit=circuit, proofs=proofs, yzs=yzs, cs=cs, aggs=aggs)


def slow_composition(sonic, srs, circuit, n, proofs, yzs, cs, agg):
    """the helped verdicts from calls that existed before: the transcript, hsc_verify, s equality, pcV on each head"""
    from sonic_amd.protocol import _hsc_from_bytes
    K = len(proofs)
    u, v = sonic.fs_aggregate_challenges(srs, circuit, yzs, agg)
    if aref.fr(u) + aref.fr(v) != agg[-64:] or not sonic.hsc_verify(srs, circuit, yzs, _hsc_from_bytes(agg, K)):
        return [False] * K
    out = []
    for k, (raw, (y, z)) in enumerate(zip(proofs, yzs)):
        p = sonic.CoreProof.from_bytes(raw)
        t = (p.prA * (p.prB + p.prS) - sum(int(c) * pow(y, n + 1 + q, R) for q, c in enumerate(cs[k]))) % R
        out.append(raw[544:576] == aref.s_of(K, agg, k) and sonic.pc_v(srs, n, p.prR, z, (p.prA, p.prWa))
                   and sonic.pc_v(srs, n, p.prR, y * z % R, (p.prB, p.prWb)) and sonic.pc_v(srs, srs.srsD, p.prT, z, (t, p.prWt)))
    return out


@pytest.mark.parametrize("K", [1, 3, 17])
def test_helped_batch_agrees_with_the_unhelped_one_and_the_slow_composition(sonic, small_srs, batch17, K):
    b = batch17
    proofs, yzs, cs, agg = b["proofs"][:K], b["yzs"][:K], b["cs"][:K], b["aggs"][K]
    zs = [sonic.CoreProof.from_bytes(p).to_bytes(compressed=True) for p in proofs]
    v = sonic.Verifier(small_srs, b["circuit"])
    try:
        assert slow_composition(sonic, small_srs, b["circuit"], b["n"], proofs, yzs, cs, agg) == [True] * K
        for form in (proofs, zs):
            assert v.verify_core_batch_helped(form, yzs, agg, constants=cs) is True
            got = v.verify_core_batch_helped(form, yzs, agg, constants=cs, each=True, seed=seed_of(K))
            assert got == (True, [True] * K) == v.verify_core_batch(form, yzs, constants=cs, each=True, seed=seed_of(K))
        # against the handle's own constants every proof is one of another statement: both verifiers reject each, and the aggregate,
        # which does not depend on the constants, is not to blame
        own = v.verify_core_batch(proofs, yzs, each=True)
        assert own == (False, [False] * K) == v.verify_core_batch_helped(proofs, yzs, agg, each=True)
        assert v.verify_core_batch_helped(proofs, yzs, agg) is False
        # one proof of another statement among the rest: that one only, in either encoding, under a fixed seed and a drawn one
        if K > 1:
            mixed = [list(c) for c in cs]
            mixed[1] = [int(mixed[1][0]) + 1, int(mixed[1][1])]
            want = (False, [k != 1 for k in range(K)])
            assert slow_composition(sonic, small_srs, b["circuit"], b["n"], proofs, yzs, mixed, agg) == want[1]
            for form in (proofs, zs):
                first = v.verify_core_batch_helped(form, yzs, agg, constants=mixed, each=True, seed=seed_of("mixed"))
                assert first == want == v.verify_core_batch(form, yzs, constants=mixed, each=True)
                assert v.verify_core_batch_helped(form, yzs, agg, constants=mixed, each=True, seed=seed_of("mixed")) == first
                assert v.verify_core_batch_helped(form, yzs, agg, constants=mixed, each=True) == first
    finally:
        v.close()


def test_helped_fiat_shamir_form(sonic, ref, small_srs):
    n, Q, K = 5, 2, 3
    circuit, asg, _circ = circuit_of(sonic, ref, n, Q)
    digest = sonic.fs_circuit_digest(circuit)
    p = sonic.Prover(small_srs, circuit)
    try:
        p.set_assignment(sonic.Assignment(*asg))
        made = [p.prove_core_fs(digest, seed_of("blind%d" % k)) for k in range(K)]
        proofs = [m[0] if isinstance(m[0], (bytes, bytearray)) else m[0].to_bytes() for m in made]
        yzs = [sonic.fs_core_challenges(small_srs, circuit, pf) for pf in proofs]
        agg = p.aggregate_core(yzs)
    finally:
        p.close()
    v = sonic.Verifier(small_srs, circuit)
    try:
        assert v.verify_core_fs_batch(proofs, each=True) == (True, [True] * K)
        assert v.verify_core_fs_batch_helped(proofs, agg, each=True, seed=seed_of("fs")) == (True, [True] * K)
        assert v.verify_core_fs_batch_helped([sonic.CoreProof.from_bytes(pf).to_bytes(compressed=True) for pf in proofs], agg) is True
        assert v.verify_core_batch_helped(proofs, yzs, agg, each=True) == (True, [True] * K)
        # an aggregate over other pairs than the proofs' own transcripts give: every proof rejected
        other = sonic.Prover(small_srs, circuit)
        try:
            agg2 = other.aggregate_core([yzs[1], yzs[0], yzs[2]])
        finally:
            other.close()
        assert v.verify_core_fs_batch_helped(proofs, agg2, each=True) == (False, [False] * K)
    finally:
        v.close()


def test_the_digest_the_randomizers_bind(sonic, small_srs, batch17):
    """the library's D for this batch is the restated one, its randomizers are sonic_verify_batch_randomizers over it, and a fixed seed
    fixes the verdicts (what the randomizers are cannot be seen from a verdict: D covers every byte an error could be put into)"""
    import ctypes as C
    import hashlib
    from sonic_amd import _lib
    b, K = batch17, 3
    proofs, yzs, cs, agg = b["proofs"][:K], b["yzs"][:K], b["cs"][:K], b["aggs"][K]
    wd, sid = sonic.fs_weights_digest(b["circuit"]), sonic.fs_srs_id(small_srs)
    csb = [b"".join(aref.fr(int(c)) for c in k) for k in cs]
    D = C.create_string_buffer(32)
    assert _lib.lib().sonic_verify_core_helped_digest(b["n"], b["Q"], small_srs.srsD, wd, sid, K, b"".join(proofs), b"".join(aref.fr(y) + aref.fr(z) for y, z in yzs),
                                                      b"".join(csb), agg, D) == 0
    assert D.raw == aref.helped_digest(b["n"], b["Q"], small_srs.srsD, aref.weights_digest(sonic.fs_circuit_midstate(b["circuit"])), sid, proofs, yzs, csb, agg)
    rho = C.create_string_buffer(16 * (6 * K + 1))
    assert _lib.lib().sonic_verify_batch_randomizers(seed_of("rho"), D.raw, 6 * K + 1, rho) == 0
    want = [hashlib.sha256(b"sonic-hip/batch/v1" + seed_of("rho") + D.raw + i.to_bytes(8, "little")).digest()[:16] for i in range(6 * K + 1)]
    assert [rho.raw[16 * i:16 * i + 16] for i in range(6 * K + 1)] == want and len(set(want)) == 6 * K + 1


# ---- rejections: each case asserts the exact `each` vector ----
def test_rejections(sonic, ref, small_srs, batch17):
    from sonic_amd import _lib
    b, K = batch17, 3
    n, circuit = b["n"], b["circuit"]
    proofs, yzs, cs, agg = list(b["proofs"][:K]), b["yzs"][:K], [list(c) for c in b["cs"][:K]], b["aggs"][K]
    at = 448 * K
    v = sonic.Verifier(small_srs, circuit)

    def helped(proofs=proofs, yzs=yzs, agg=agg, cs=cs, **kw):
        return v.verify_core_batch_helped(proofs, yzs, agg, constants=cs, each=True, **kw)

    def flip(blob, where, bit=1):
        return blob[:where] + bytes([blob[where] ^ bit]) + blob[where + 1:]
    try:
        assert helped() == (True, [True] * K)
        # the forged core proof (a statement without a witness, s solved) next to two honest ones, under the honest aggregate: only it, by
        # the s linkage
        forged = forge(sonic, small_srs, n, cs[1], *yzs[1], random.Random(81))
        assert forged.to_bytes()[544:576] != aref.s_of(K, agg, 1)
        bad = [proofs[0], forged.to_bytes(), proofs[2]]
        assert helped(proofs=bad) == (False, [True, False, True])
        assert "s of proof 1" in _lib.last_error()
        assert helped(proofs=[sonic.CoreProof.from_bytes(p).to_bytes(compressed=True) for p in bad]) == (False, [True, False, True])
        # the same with s_1 of the aggregate overwritten by the forged s (u, v recomputed, as a cheating helper would): the linkage holds
        # now, and W_1 no longer opens S_1 to s_1 at z_1 -- only it
        agg_f = lying_aggregate(sonic, small_srs, circuit, n, b["Q"], yzs, agg, 1, forged.to_bytes()[544:576])
        assert agg_f[224 + 96:224 + 128] == forged.to_bytes()[544:576] and agg_f[:224 + 96] == agg[:224 + 96]
        assert helped(proofs=bad, agg=agg_f, seed=seed_of("forged")) == (False, [True, False, True])
        assert helped(proofs=bad, agg=agg_f) == (False, [True, False, True])
        # (and the honest proof 1 does not link to the lying aggregate)
        assert helped(agg=agg_f) == (False, [True, False, True])
        # a flipped bit in C or Q_v: a point off the curve -- all rejected, and the call itself succeeds
        for where in (at + 96, at):
            assert helped(agg=flip(agg, where)) == (False, [False] * K)
            assert "aggregate" in _lib.last_error()
        # Q_v and C replaced by other VALID points: the transcript moves with C; with Q_v alone only the global check fails -- all rejected
        gen2 = ref.g1_to_bytes(ref.g1_mul(ref.G1_GEN, 2))
        assert helped(agg=agg[:at] + gen2 + agg[at + 96:]) == (False, [False] * K)
        assert "s(u, v)" in _lib.last_error()
        assert helped(agg=agg[:at + 96] + gen2 + agg[at + 192:]) == (False, [False] * K)
        # u or v altered
        for where in (at + 192, at + 224):
            assert helped(agg=flip(agg, where)) == (False, [False] * K)
            assert "transcript" in _lib.last_error()
        # two pairs swapped in yz: the transcript is another one
        assert helped(yzs=[yzs[1], yzs[0], yzs[2]]) == (False, [False] * K)
        # a non-canonical s'_j, an off-curve W'_j: the aggregate is malformed -- all rejected, with SONIC_OK
        sp1 = 224 * K + 224
        assert helped(agg=agg[:sp1] + R.to_bytes(32, "little") + agg[sp1 + 32:]) == (False, [False] * K)
        assert helped(agg=agg[:sp1 + 32] + (1).to_bytes(48, "little") + (1).to_bytes(48, "little") + agg[sp1 + 128:]) == (False, [False] * K)
        assert "malformed" in _lib.last_error()
        # a non-canonical cs_k: that proof only
        cs_bad = [list(c) for c in cs]
        cs_bad[2] = R.to_bytes(32, "little") + int(cs[2][1]).to_bytes(32, "little")
        assert helped(cs=cs_bad) == (False, [True, True, False])
        # a malformed proof: that proof only; a zero y_k changes the pairs the aggregate is over -- all rejected
        assert helped(proofs=[proofs[0][:96] + (1).to_bytes(48, "little") + (1).to_bytes(48, "little") + proofs[0][192:]] + proofs[1:]) == (False, [False, True, True])
        assert helped(yzs=[(0, yzs[0][1])] + list(yzs[1:])) == (False, [False] * K)
    finally:
        v.close()
