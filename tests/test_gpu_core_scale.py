"""Core proofs free of Q on the GPU (include/sonic_hip.h, "Circuits with Q ~ n"): a fresh prover handle holds a core proof's prefixes and
no MSM slot per constraint; the first full proof adds the signature state and changes no byte; every core form runs on a handle that has
never made a full proof, with no byte of memory more; the refusals stay; k(y) over many blocks gives the bytes of the one-block form;
and a compiled R1CS runs end to end on core proofs without growth.  Every comparison is byte equality, an inequality the issue of this
change states, or a status.

Shapes: n <= 16 throughout; one SRS of d = 7 * 256.  Q = 1024 for the core forms, Q = 65 793 (257 blocks of 256 and one term) once for k(y).
"""
import ctypes as C
import json
import os
import random

import numpy as np
import pytest

import r1cs_ref as rref
from util import R

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
SLOT_BYTES = 12304            # sizeof(MsmSlot), sonic_amd/csrc/msm_slot.hpp: four ints and 64 window sums of 192 bytes
INVALID_ARG, SRS_INDEX, INEXACT_DIVISION = 7, 2, 4


@pytest.fixture(scope="module")
def srs(sonic):
    rng = random.Random(2301)
    s = sonic.SRS.new(7 * 256, rng.randrange(2, R), rng.randrange(2, R))
    yield s
    s.close()


def random_rows(rng, n, Q, max_len):
    rows = [{j: rng.randrange(1, R) for j in rng.sample(range(n), rng.randrange(1, max_len + 1))} for _ in range(3 * Q)]
    return rows[:Q], rows[Q:2 * Q], rows[2 * Q:]


def statement(rng, n, rows):
    """a random assignment with aO = aL aR and the constants it satisfies under the rows"""
    aL, aR = [rng.randrange(R) for _ in range(n)], [rng.randrange(R) for _ in range(n)]
    aO = [a * b % R for a, b in zip(aL, aR)]
    wL, wR, wO = rows
    cs = [(sum(v * aL[j] for j, v in wL[q].items()) + sum(v * aR[j] for j, v in wR[q].items()) + sum(v * aO[j] for j, v in wO[q].items())) % R for q in range(len(wL))]
    return (aL, aR, aO), cs


def refused(code, fn):
    from sonic_amd import _lib
    with pytest.raises(_lib.SonicError) as e:
        fn()
    assert e.value.code == code, e.value
    return str(e.value)


def sizes(p):
    return p.device_bytes, p.host_bytes


@pytest.fixture(scope="module")
def shapes(sonic):
    """n = 16: a circuit and two satisfied statements for Q = 64 and Q = 1024, rows of at most 4 entries"""
    rng = random.Random(2302)
    out = {}
    for Q in (64, 1024):
        rows = random_rows(rng, 16, Q, 4)
        stm = [statement(rng, 16, rows) for _ in range(2)]
        out[Q] = dict(rows=rows, sp=sonic.SparseCircuit.from_rows(16, *rows, stm[0][1]), asg=[sonic.Assignment(*s[0]) for s in stm], cs=[s[1] for s in stm])
    out["tr"] = [[rng.randrange(1, R) for _ in range(8 + 2 * 64)] for _ in range(3)]
    return out


# ---- 1. fresh handles do not grow with Q ----
def test_fresh_handles_do_not_grow_with_q(sonic, srs, shapes):
    """The O(Q) buffers that remain on a fresh handle are cs, su, pw, kpow, the CSR / CSC arrays, the row chunk tables and one Fr per chunk:
    roughly 700 bytes per Q at this density, so the bound is 4096 per Q; five MSM slots per Q would be 61 520.  Pinned memory: nothing
    per Q is left, the bound is 64 per Q."""
    fresh, after = {}, {}
    for Q in (64, 1024):
        p = sonic.Prover(srs, shapes[Q]["sp"], prepare=False)
        fresh[Q] = sizes(p)
        p.set_assignment(shapes[Q]["asg"][0])
        core = p.prove_core_bytes(shapes["tr"][0][:6])
        assert sonic.verify_core(srs, shapes[Q]["sp"], core, shapes["tr"][0][4], shapes["tr"][0][5])
        after[Q] = sizes(p)
        p.close()
    for got in (fresh, after):
        assert 0 < got[64][0] <= got[1024][0] and got[64][1] > 0, got
        assert got[1024][0] - got[64][0] < 4096 * 960, got
        assert got[1024][1] - got[64][1] <= 64 * 960, got


# ---- 2. the first full proof adds the state and changes no byte ----
@pytest.mark.parametrize("form", ["csr", "dense", "prepared"])
def test_the_first_full_proof_adds_the_signature_state_and_changes_no_byte(sonic, srs, shapes, form):
    n, Q = 16, 64
    sp, asg, tr = shapes[Q]["sp"], shapes[Q]["asg"][0], shapes["tr"]
    circuit = sp.to_dense() if form == "dense" else sp

    def handle():
        p = sonic.Prover(srs, circuit, prepare=(form == "prepared"))
        p.set_assignment(asg)
        return p

    a = handle()
    core0 = a.prove_core_bytes(tr[0][:6])
    before = sizes(a)
    assert a.prove_core_bytes(tr[0][:6]) == core0 and sizes(a) == before
    full0 = a.prove_bytes(tr[0])
    grown = sizes(a)
    assert grown[0] - before[0] >= 5 * Q * SLOT_BYTES + 32 * Q * (3 * n + 1), (before, grown)
    assert grown[1] - before[1] >= 5 * Q * SLOT_BYTES, (before, grown)
    # core, core, full, core, full on one handle
    assert core0 == full0[:576]
    assert a.prove_core_bytes(tr[0][:6]) == core0
    assert a.prove_bytes(tr[0]) == full0
    others = [a.prove_core_bytes(tr[k][:6]) for k in (1, 0, 1)]
    assert others[1] == core0 and others[0] == others[2] != core0
    assert a.prove_bytes(tr[0]) == full0
    assert sizes(a) == grown                                   # three more core proofs and one more full proof: nothing added
    a.close()
    b = handle()                                               # a second handle that starts with the full proof
    assert b.prove_bytes(tr[0]) == full0
    assert b.prove_core_bytes(tr[0][:6]) == core0
    b.close()


# ---- 3. every core form on a handle that has never made a full proof ----
CORE_FORMS_Q = 1024           # (the handle it is compared with makes ONE full proof of 7 + 4Q = 4103 MSMs first)


def core_forms(sonic, srs, shape, provers, tr):
    """every core form once, over `provers` (two handles of one circuit); returns everything they gave, for comparison"""
    p, q = provers
    sp, (asg0, asg1), (cs0, cs1) = shape["sp"], shape["asg"], shape["cs"]
    wd = sonic.fs_weights_digest_v2(sp)
    d0, d1 = sonic.fs_circuit_digest_v2(wd, cs0), sonic.fs_circuit_digest_v2(wd, cs1)
    out = {}
    for h in provers:
        h.set_assignment(asg0)
        h.set_constants(cs0)
    out["blocking"] = [p.prove_core_bytes(t[:6]) for t in tr[:2]]
    p.submit_core(tr[0][:6]); q.submit_core(tr[1][:6])
    out["flight"] = [q.collect_core(), p.collect_core()][::-1]
    assert out["flight"] == out["blocking"]
    out["fs"] = p.prove_core_fs(d0, b"\x31" * 32)
    out["batch"] = sonic.prove_core_batch(provers, [t[:6] for t in tr], assignments=[asg0, asg1, asg0], constants=[cs0, cs1, cs0])
    out["batch_fs"] = sonic.prove_core_batch_fs(provers, [d0, d1, d0], [bytes([k + 1]) * 32 for k in range(3)], assignments=[asg0, asg1, asg0], constants=[cs0, cs1, cs0])
    # set_constants in place: statement 1 on the first handle, then back
    p.set_assignment(asg1); p.set_constants(cs1)
    out["stmt1"] = p.prove_core_bytes(tr[2][:6])
    p.set_assignment(asg0); p.set_constants(cs0)
    yzs = [(y, z) for _, y, z in out["batch_fs"]]
    out["agg"] = p.aggregate_core(yzs, weights_digest=wd)
    return out


def test_every_core_form_runs_without_the_signature_state(sonic, srs, shapes):
    Q = CORE_FORMS_Q
    shape, tr = shapes[Q], shapes["tr"]
    sp, (cs0, cs1) = shape["sp"], shape["cs"]
    lean = [sonic.Prover(srs, sp, prepare=False) for _ in range(2)]
    lean[0].set_assignment(shape["asg"][0]); lean[1].set_assignment(shape["asg"][0])
    first = lean[0].prove_core_bytes(tr[0][:6]), lean[1].prove_core_bytes(tr[0][:6])      # (lane scratch and workspaces grow here)
    assert first[0] == first[1]
    before = [sizes(h) for h in lean]
    got = core_forms(sonic, srs, shape, lean, tr)
    aggregate_grew = [sizes(h) for h in lean]
    assert [s[1] for s in aggregate_grew] == [s[1] for s in before]            # pinned memory: unchanged across all of it
    # device memory: nothing of the order of the signature state (61 520 bytes per constraint in slots alone) -- what may still
    # grow is the scratch of a lane that a later form uses first, independent of Q
    assert all(a[0] - b[0] < Q * SLOT_BYTES for a, b in zip(aggregate_grew, before)), (before, aggregate_grew)
    again = core_forms(sonic, srs, shape, lean, tr)
    assert again == got and [sizes(h) for h in lean] == aggregate_grew         # the same calls again: not one byte more
    # accepted by the verifiers
    stmt = lambda cs: sonic.SparseCircuit(sp.n, sp.Q, sp.row_ptr, sp.col, sp.val, cs)      # noqa: E731
    assert got["blocking"][0] == first[0]
    for k, pf in enumerate(got["blocking"]):
        assert sonic.verify_core(srs, sp, pf, tr[k][4], tr[k][5])
    assert sonic.verify_core(srs, stmt(cs1), got["stmt1"], tr[2][4], tr[2][5])
    assert sonic.verify_core(srs, sp, got["stmt1"], tr[2][4], tr[2][5]) is False
    for k, pf in enumerate(got["batch"]):
        assert sonic.verify_core(srs, stmt([cs0, cs1, cs0][k]), pf, tr[k][4], tr[k][5])
    v = sonic.Verifier(srs, sp, digest=2)
    assert v.verify_core_fs_batch([got["fs"][0]], seed=b"\x41" * 32, each=True) == (True, [True])
    raws, yzs = [pf for pf, _, _ in got["batch_fs"]], [(y, z) for _, y, z in got["batch_fs"]]
    assert v.verify_core_fs_batch(raws, seed=b"\x41" * 32, each=True, constants=[cs0, cs1, cs0]) == (True, [True, True, True])
    assert v.verify_core_batch_helped(raws, yzs, got["agg"], seed=b"\x42" * 32, each=True, constants=[cs0, cs1, cs0]) == (True, [True, True, True])
    v.close()
    for h in lean:
        h.close()
    # the same calls on handles whose signature state was made first, by one full proof each
    full = [sonic.Prover(srs, sp, prepare=False) for _ in range(2)]
    tr_full = tr[0][:6] + [random.Random(2303).randrange(1, R) for _ in range(2 + 2 * Q)]
    for h in full:
        h.set_assignment(shape["asg"][0])
        lean_bytes = sizes(h)
        assert h.prove_bytes(tr_full)[:576] == first[0]
        assert sizes(h)[1] - lean_bytes[1] >= 5 * Q * SLOT_BYTES
    assert core_forms(sonic, srs, shape, full, tr) == got
    for h in full:
        h.close()


# ---- 4. refusals stay ----
def test_refusals_stay(sonic, srs, shapes):
    Q = 64
    shape, tr = shapes[Q], shapes["tr"]
    p = sonic.Prover(srs, shape["sp"], prepare=False)
    p.set_assignment(shape["asg"][0])
    core = p.prove_core_bytes(tr[0][:6])
    before = sizes(p)
    assert "transcript element 4 is zero" in refused(INEXACT_DIVISION, lambda: p.prove_core_bytes(tr[0][:4] + [0, tr[0][5]]))
    assert "transcript element 5 is zero" in refused(INEXACT_DIVISION, lambda: p.prove_core_bytes(tr[0][:5] + [0]))
    refused(INVALID_ARG, p.collect_core)                                           # nothing in flight
    p.submit_core(tr[0][:6])
    for other in (p.collect, p.collect_share, p.collect_fs):
        refused(INVALID_ARG, other)
    refused(INVALID_ARG, lambda: p.submit_core(tr[0][:6]))
    refused(INVALID_ARG, lambda: p.prove_core_bytes(tr[0][:6]))
    refused(INVALID_ARG, lambda: p.prove_bytes(tr[0]))
    assert p.collect_core() == core                                                # the flight survived all of it
    # an unsatisfied statement: one constant off by one
    bad = list(shape["cs"][0]); bad[5] = (bad[5] + 1) % R
    p.set_constants(bad)
    msg = refused(SRS_INDEX, lambda: p.prove_core_bytes(tr[0][:6]))
    assert "a non-zero coefficient needs an SRS element outside [-d, d] or the omitted g^alpha (index -1)" in msg and msg.split(": ", 1)[1].startswith("prove: ")
    p.set_constants(shape["cs"][0])
    assert p.prove_core_bytes(tr[0][:6]) == core
    assert sizes(p) == before                                                      # none of it made the signature state
    p.close()


# ---- 5. k(y) over many blocks ----
K_N = 8
K_SIZES = [1, 255, 256, 257, 512, 513, 65793]


def k_case(sonic, Q):
    """n = 8, one entry per row of wL (none in wR, wO), so that cs[q] = w_q aL[q mod n] is a non-zero random element for every q"""
    rng = random.Random(2310 + Q)
    n = K_N
    aL, aR = [rng.randrange(1, R) for _ in range(n)], [rng.randrange(1, R) for _ in range(n)]
    aO = [a * b % R for a, b in zip(aL, aR)]
    w = [rng.randrange(1, R) for _ in range(Q)]
    cs = [w[q] * aL[q % n] % R for q in range(Q)]
    assert all(cs)
    row_ptr = list(range(Q + 1)) + [Q] * (2 * Q)
    sp = sonic.SparseCircuit(n, Q, row_ptr, [q % n for q in range(Q)], w, cs)
    return dict(sp=sp, asg=(aL, aR, aO), w=w, cs=cs, tr=[rng.randrange(1, R) for _ in range(6)])


def oracle_head(ref, orc, osrs, n, case):
    """the head of the reference's proof (Protocol.hs:58-83) from the restatement's polynomials and the C oracle's commitPoly / openPoly:
    t(X, y) = r(X, 1) (r(X, y) + s(X, y)) - k(y), with s(X, Y) evaluated at y before the product"""
    aL, aR, aO = case["asg"]
    Q = len(case["cs"])
    cns, y, z = case["tr"][:4], case["tr"][4], case["tr"][5]
    wL = [[case["w"][q] if j == q % n else 0 for j in range(n)] for q in range(Q)]
    zero = [[0] * n for _ in range(Q)]
    blind = ref.biv_norm({-(2 * n + i): {-(2 * n + i): c} for i, c in enumerate(cns, start=1)})
    rXY = ref.biv_add(ref.r_poly(aL, aR, aO), blind)
    rX1, rXy = ref.eval_y(1, rXY), ref.eval_y(y, rXY)
    sXy = ref.eval_y(y, ref.s_poly(wL, zero, zero))
    ky = ref.lp_eval(ref.k_poly(case["cs"], n), y)
    tXy = ref.lp_norm(ref.lp_add(ref.lp_mul(rX1, ref.lp_add(rXy, sXy)), {0: (-ky) % R}))
    arr = lambda p: ([e for e, _ in ref.lp_items(p)], orc.fr_array([v for _, v in ref.lp_items(p)]))      # noqa: E731
    fr = lambda v: (v % R).to_bytes(32, "little")      # noqa: E731
    a, wa = orc.open_poly(osrs, z, *arr(rX1))
    b, wb = orc.open_poly(osrs, y * z % R, *arr(rX1))
    _, wt = orc.open_poly(osrs, z, *arr(tXy))
    return orc.commit_poly(osrs, n, *arr(rX1)) + orc.commit_poly(osrs, osrs.d, *arr(tXy)) + fr(a) + wa + fr(b) + wb + wt + fr(ref.lp_eval(sXy, z))


@pytest.fixture(scope="module")
def osrs(orc):
    rng = random.Random(2301)                                  # (the draws of `srs` above)
    return orc.SRS(7 * 256, rng.randrange(2, R), rng.randrange(2, R), threads=min(os.cpu_count() or 1, 16))


@pytest.mark.parametrize("Q", K_SIZES)
def test_k_of_y_over_many_blocks(sonic, srs, orc, ref, osrs, monkeypatch, Q):
    from sonic_amd import _lib
    L = _lib.lib()
    case = k_case(sonic, Q)
    sp, tr = case["sp"], case["tr"]
    monkeypatch.setenv("SONIC_K_OF_Y_SPAN", "256")
    monkeypatch.setenv("SONIC_K_OF_Y_SPLIT", "1")
    p = sonic.Prover(srs, sp, prepare=False)
    p.set_assignment(sonic.Assignment(*case["asg"]))
    assert L.sonic_profile_reset() == 0 and L.sonic_profile_enable(1) == 0
    try:
        split = p.prove_core_bytes(tr)
        ms, n1, n2, n0 = C.c_double(0), C.c_int64(0), C.c_int64(0), C.c_int64(0)
        assert L.sonic_profile_get(b"k_k_of_y_partials", C.byref(ms), C.byref(n1)) == 0 and L.sonic_profile_get(b"k_k_of_y_finish", C.byref(ms), C.byref(n2)) == 0
        L.sonic_profile_get(b"k_sub_k_of_y", C.byref(ms), C.byref(n0))
    finally:
        L.sonic_profile_enable(0)
    assert (n1.value, n2.value, n0.value) == (1, 1, 0)                      # the split form ran, and only it
    assert sonic.verify_core(srs, sp, split, tr[4], tr[5])                  # (the host verifier computes k(y) on its own)
    if Q <= 513:
        monkeypatch.setenv("SONIC_K_OF_Y_SPLIT", "0")
        assert p.prove_core_bytes(tr) == split
        monkeypatch.setenv("SONIC_K_OF_Y_SPLIT", "1")
        assert split == oracle_head(ref, orc, osrs, K_N, case)
    # one constant off by one: the first, the last, and the first and last term of a middle block (block 1 of three at Q = 513, block 128
    # of 258 at Q = 65 793)
    mid = 1 if Q == 513 else 128
    where = {0, Q - 1} | ({256 * mid, 256 * mid + 255} if Q > 256 * (mid + 1) else set())
    for q in sorted(where):
        bad = list(case["cs"]); bad[q] = (bad[q] + 1) % R
        p.set_constants(bad)
        refused(SRS_INDEX, lambda: p.prove_core_bytes(tr))
    p.set_constants(case["cs"])
    assert p.prove_core_bytes(tr) == split
    p.close()


def test_small_circuits_launch_the_one_block_kernel_and_keep_the_golden_bytes(sonic, monkeypatch):
    from sonic_amd import _lib
    L = _lib.lib()
    monkeypatch.delenv("SONIC_K_OF_Y_SPLIT", raising=False)
    monkeypatch.delenv("SONIC_K_OF_Y_SPAN", raising=False)
    c = next(k for k in json.load(open(os.path.join(HERE, "golden", "prove_small.json")))["cases"] if k["name"] == "rnd_n2")
    iv = lambda v: int(v, 16)      # noqa: E731
    m = lambda w: [[iv(v) for v in r] for r in w]      # noqa: E731
    assert c["Q"] == 2
    g = sonic.SRS.new(c["d"], iv(c["x"]), iv(c["alpha"]))
    p = sonic.Prover(g, sonic.ArithCircuit(sonic.GateWeights(m(c["wL"]), m(c["wR"]), m(c["wO"])), [iv(v) for v in c["cs"]]), prepare=False)
    p.set_assignment(sonic.Assignment([iv(v) for v in c["aL"]], [iv(v) for v in c["aR"]], [iv(v) for v in c["aO"]]))
    tr = [iv(v) for v in c["transcript"]]
    assert L.sonic_profile_reset() == 0 and L.sonic_profile_enable(1) == 0
    try:
        core, full = p.prove_core_bytes(tr[:6]), p.prove_bytes(tr)
        ms, n0, n1 = C.c_double(0), C.c_int64(0), C.c_int64(0)
        assert L.sonic_profile_get(b"k_sub_k_of_y", C.byref(ms), C.byref(n0)) == 0
        L.sonic_profile_get(b"k_k_of_y_partials", C.byref(ms), C.byref(n1))
    finally:
        L.sonic_profile_enable(0)
    assert (n0.value, n1.value) == (2, 0)
    assert full.hex() == c["proof"] and core == full[:576]
    p.close(); g.close()


# ---- 6. a compiled R1CS end to end on core proofs ----
def always_satisfiable(rng, n_in, m, N):
    """z = (1, n_in inputs, N - 1 - n_in products): row i < P multiplies two combinations of earlier columns into column 1 + n_in + i; the
    rows behind are <a, z> * 1 = <a, z>.  Every choice of inputs has its witness.  (tests/test_gpu_large_q.py)"""
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


def test_a_compiled_r1cs_end_to_end_on_core_proofs_without_growth(sonic, srs):
    import torch
    rng = random.Random(2320)
    m, N, n_in, n_pub, K = 64, 40, 9, 2, 3
    A, B, Cm, solve = always_satisfiable(rng, n_in, m, N)
    r = sonic.R1CS.from_rows(N, n_pub, [dict(x) for x in A], [dict(x) for x in B], [dict(x) for x in Cm])
    assert (r.n, r.Q) == (84, 194)
    inputs = [rng.randrange(R) for _ in range(n_in)]
    zs = [solve(inputs), solve([(inputs[0] + 1) % R] + inputs[1:]), solve(inputs[:5] + [(inputs[5] + 1) % R] + inputs[6:])]
    za = np.frombuffer(b"".join(v.to_bytes(32, "little") for z in zs for v in z), np.uint8).reshape(K, N, 32)
    wb, cs, bad = r.assign(torch.from_numpy(za.copy()).to(f"cuda:{r.device}"))
    assert bad == [(0, -1)] * K
    circuit = r.circuit(public=zs[0][1:3])
    p = sonic.Prover(srs, circuit, prepare=False)
    fresh = sizes(p)
    assert fresh[1] < 8 * SLOT_BYTES + 4096                   # a core proof's eight slots and a few hundred bytes, whatever Q is
    wd2 = p.weights_digest_v2()
    digests = [sonic.fs_circuit_digest_v2(wd2, c) for c in cs]
    seeds = [bytes([k + 21]) * 32 for k in range(K)]
    proofs = sonic.prove_core_batch_fs([p], digests, seeds, wb, constants=cs)
    warm = sizes(p)
    assert warm[1] == fresh[1] and warm[0] - fresh[0] < r.Q * SLOT_BYTES      # (lane workspaces and scratch; five slots per Q would be 5 Q SLOT_BYTES)
    assert sonic.prove_core_batch_fs([p], digests, seeds, wb, constants=cs) == proofs
    agg = p.aggregate_core([(y, z) for _, y, z in proofs], weights_digest=wd2)
    settled = sizes(p)
    assert sonic.prove_core_batch_fs([p], digests, seeds, wb, constants=cs) == proofs
    assert p.aggregate_core([(y, z) for _, y, z in proofs], weights_digest=wd2) == agg
    assert sizes(p) == settled and settled[1] == fresh[1]      # no growth
    v = sonic.Verifier(srs, circuit, digest=2)
    raws = [pf for pf, _, _ in proofs]
    assert v.verify_core_fs_batch(raws, seed=b"\x07" * 32, each=True, constants=cs) == (True, [True, True, True])
    assert v.verify_core_fs_batch_helped(raws, agg, seed=b"\x08" * 32, each=True, constants=cs) == (True, [True, True, True])
    assert v.verify_core_fs_batch(raws, seed=b"\x07" * 32, each=True, constants=[cs[0]] * K) == (False, [True, False, True])
    for h in (v, p, r):
        h.close()
