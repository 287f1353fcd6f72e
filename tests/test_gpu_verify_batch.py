"""The batched verifier on the GPU (include/sonic_hip.h, "the batched verifier"; sonic_amd/csrc/verify_batch.hip): K proofs folded into
one pairing product, with k_g1_validate, k_s_of_uv_batch and the variable-base MSM on the device.

THE YARDSTICK for every verdict is sonic_verify / sonic_verify_csr on the same proof (the per-equation host verifier, untouched by the
batched one), with SONIC_ERR_BAD_ENCODING -- and SONIC_ERR_INEXACT_DIVISION for u = 0 -- read as "rejected"; never the code under test.
For the kernels on their own it is Python: [r]P with oracle/sonic_ref.py, and s(u, v) from the reference's polynomial or from
tests/batch_ref.s_of_uv (which tests/test_verify_batch_host.py pins to that polynomial).

Reference: Sonic.Protocol.verify (src/Sonic/Protocol.hs:111-130), hscVerify (src/Sonic/Signature.hs:74-90)."""
import ctypes as C
import hashlib
import random
import threading

import numpy as np
import pytest

import batch_ref
from util import R, big_circuit, circuit_arrays, fr_bytes

pytestmark = pytest.mark.gpu

QMOD = 0x1a0111ea397fe69a4b1ba7b6434bacd764774b84f38512bf6730d2a0f6b0f6241eabfffeb153ffffb9feffffffffaaab
SEED = bytes(range(32))
SHAPES = [(16, 1), (256, 2), (1024, 5)]
KMAX = 33


# ---- proofs, made once per module -------------------------------------------------------------------------------------------------
class World:
    def __init__(self, sonic, ref, n, Q, K, fs=False):
        pyr = random.Random(1000 * n + Q)
        self.n, self.Q, self.d = n, Q, 7 * n + 12 + pyr.randrange(20)
        self.srs = sonic.SRS.new(self.d, pyr.randrange(2, R), pyr.randrange(2, R))
        if n <= 1024:
            circ, asg, enc = circuit_arrays(ref, pyr, n, Q)
            self.lists = circ
            self.dense = sonic.ArithCircuit(sonic.GateWeights(enc["wL"], enc["wR"], enc["wO"]), enc["cs"])
            asg = sonic.Assignment(enc["aL"], enc["aR"], enc["aO"])
        else:
            b = big_circuit(n + Q, n, Q)
            self.dense = sonic.ArithCircuit(sonic.GateWeights(b["wL"], b["wR"], b["wO"]), b["cs"])
            asg = sonic.Assignment(b["aL"], b["aR"], b["aO"])
        self.sparse = sonic.SparseCircuit.from_circuit(self.dense)
        p = sonic.Prover(self.srs, self.dense)
        p.set_assignment(asg)
        self.proofs, self.trs = [], []
        digest = sonic.fs_circuit_digest(self.dense) if fs else None
        for k in range(K):
            if fs:
                raw, tr = p.prove_fs(digest, hashlib.sha256(b"blind%d" % k).digest())
            else:
                tr = [pyr.randrange(1, R) for _ in range(8 + 2 * Q)]
                raw = p.prove_bytes(tr)
            self.proofs.append(raw)
            self.trs.append((tr[4], tr[5], list(zip(tr[6:6 + Q], tr[6 + Q:6 + 2 * Q]))))
        p.close()
        self._ver = {}

    def verifier(self, sonic, form):
        if form not in self._ver:
            self._ver[form] = sonic.Verifier(self.srs, self.dense if form == "dense" else self.sparse)
        return self._ver[form]

    def yard(self, sonic, raw, tr, form="dense"):
        """sonic_verify[_csr] on one proof's bytes: True / False, with a refused encoding (or u = 0) read as rejected"""
        from sonic_amd import _lib
        from sonic_amd.protocol import _circuit_args
        n, Q, suffix, args, _keep = _circuit_args(self.dense if form == "dense" else self.sparse)
        y, z, yzs = tr
        fr = lambda v: int(v).to_bytes(32, "little")      # noqa: E731
        flat = b"".join(fr(a) + fr(b) for a, b in yzs)
        ok = C.c_int(0)
        rc = getattr(_lib.lib(), "sonic_verify" + suffix)(self.srs._h, n, Q, *args, bytes(raw), fr(y), fr(z), flat, C.byref(ok))
        assert rc in (0, 3, 4), (rc, _lib.last_error())
        return rc == 0 and bool(ok.value)

    def close(self):
        for v in self._ver.values():
            v.close()
        self.srs.close()


@pytest.fixture(scope="module")
def worlds(sonic, ref):
    made = {}

    def get(n, Q, K=KMAX, fs=False):
        key = (n, Q, K, fs)
        if key not in made:
            made[key] = World(sonic, ref, n, Q, K, fs)
        return made[key]
    yield get
    for w in made.values():
        w.close()


# ---- the layout of a proof (include/sonic_hip.h): offsets of its G1 and Fr fields -----------------------------------------------------
def layout(Q):
    g1, fr, o = [], [], 0
    for kind in "GGFGFGGF" + "GFG" * Q + "FGG" * Q + "GGFF":
        (g1 if kind == "G" else fr).append(o)
        o += 96 if kind == "G" else 32
    return g1, fr, o


def put(raw, off, b):
    return raw[:off] + b + raw[off + len(b):]


def g1_shift(ref, raw, off, point):
    return put(raw, off, ref.g1_to_bytes(ref.g1_add(ref.g1_from_bytes(raw[off:off + 96]), point)))


def non_subgroup_point(ref, start=1):
    """a curve point outside the order-r subgroup: x = start, start + 1, ... with no cofactor clearing (q = 3 mod 4: one square root)"""
    x = start
    while True:
        rhs = (x * x * x + 4) % QMOD
        y = pow(rhs, (QMOD + 1) // 4, QMOD)
        if y * y % QMOD == rhs and subgroup_verdict(ref, (x, y)) is False:
            return (x, y)
        x += 1


def subgroup_verdict(ref, p):
    """[r]P == O by the reference's double-and-add (g1_mul reduces its scalar mod r, so r = (r - 1) + 1)"""
    return ref.g1_add(ref.g1_mul(p, R - 1), p) is ref.INF


# ---- 1. accepts what sonic_verify accepts ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", ["dense", "csr"])
@pytest.mark.parametrize("K", [1, 2, 33])
@pytest.mark.parametrize("n,Q", SHAPES)
def test_accepts_what_sonic_verify_accepts(sonic, worlds, n, Q, K, form):
    w = worlds(n, Q)
    proofs, trs = w.proofs[:K], w.trs[:K]
    assert all(w.yard(sonic, p, t, form) for p, t in zip(proofs, trs))
    assert w.verifier(sonic, form).verify_batch(proofs, trs, seed=SEED, each=True) == (True, [True] * K)
    assert w.verifier(sonic, form).verify_batch(proofs, trs, seed=SEED) is True


@pytest.mark.parametrize("K", [1, 2, 33])
def test_accepts_fiat_shamir_proofs(sonic, worlds, K):
    w = worlds(64, 2, KMAX, True)
    proofs = w.proofs[:K]
    assert all(sonic.verify_fs(w.srs, w.dense, sonic.Proof.from_bytes(p, 2)) for p in proofs[:3])
    for form in ("dense", "csr"):
        assert w.verifier(sonic, form).verify_fs_batch(proofs, seed=SEED, each=True) == (True, [True] * K)
    # a proof whose u is not its transcript's: rejected, as sonic_verify_fs rejects it
    _g1, fr, size = layout(2)
    bad = put(proofs[-1], fr[-2], ((int.from_bytes(proofs[-1][fr[-2]:fr[-2] + 32], "little") + 1) % R).to_bytes(32, "little"))
    assert not sonic.verify_fs(w.srs, w.dense, sonic.Proof.from_bytes(bad, 2))
    ok, each = w.verifier(sonic, "dense").verify_fs_batch(proofs[:-1] + [bad], seed=SEED, each=True)
    assert not ok and each == [True] * (K - 1) + [False]
    assert w.verifier(sonic, "dense").verify_fs_batch(proofs[:-1] + [bad], seed=SEED) is False


# ---- 2. rejects what it rejects, and names it ------------------------------------------------------------------------------------------
def _damages(ref, raw, tr, Q):
    g1, fr, _size = layout(Q)
    allg = raw
    for off in g1:
        allg = g1_shift(ref, allg, off, ref.G1_GEN)
    yield "every G1 + g", allg, tr
    allf = raw
    for off in fr:
        allf = put(allf, off, ((int.from_bytes(raw[off:off + 32], "little") + 1) % R).to_bytes(32, "little"))
    yield "every Fr + 1", allf, tr
    y, z, yzs = tr
    yield "y", raw, ((y + 1) % R, z, yzs)
    yield "z", raw, (y, (z + 1) % R, yzs)
    for j in range(Q):
        yield "y_%d" % j, raw, (y, z, yzs[:j] + [((yzs[j][0] + 1) % R, yzs[j][1])] + yzs[j + 1:])
        yield "z_%d" % j, raw, (y, z, yzs[:j] + [(yzs[j][0], (yzs[j][1] + 1) % R)] + yzs[j + 1:])


@pytest.mark.parametrize("n,Q", [(16, 1), (256, 2)])
def test_rejects_what_sonic_verify_rejects_and_names_it(sonic, ref, worlds, n, Q):
    w = worlds(n, Q)
    K, at = 4, 2
    for form in ("dense", "csr"):
        for what, raw, tr in _damages(ref, w.proofs[at], w.trs[at], Q):
            proofs, trs = list(w.proofs[:K]), list(w.trs[:K])
            proofs[at], trs[at] = raw, tr
            want = [w.yard(sonic, p, t, form) for p, t in zip(proofs, trs)]
            assert want == [k != at for k in range(K)], what
            assert w.verifier(sonic, form).verify_batch(proofs, trs, seed=SEED, each=True) == (False, want), (what, form)
            assert w.verifier(sonic, form).verify_batch(proofs, trs, seed=SEED) is False, (what, form)


# ---- 3. errors that cancel in an unweighted sum ----------------------------------------------------------------------------------------
def test_errors_that_cancel_without_randomizers_are_caught(sonic, ref, worlds):
    n, Q = 256, 2
    w = worlds(n, Q)
    g1, _fr, _size = layout(Q)
    Wa, Wt = g1[2], g1[4]
    D = ref.g1_mul(ref.G1_GEN, 12345)
    raw, tr = w.proofs[0], w.trs[0]
    seeds = [hashlib.sha256(b"s%d" % i).digest() for i in range(8)] + [None]
    v = w.verifier(sonic, "dense")
    # two copies of one proof under one transcript: W_a + D in the first, W_a - D in the second (sum W and sum z W unchanged)
    a, b = g1_shift(ref, raw, Wa, D), g1_shift(ref, raw, Wa, ref.g1_neg(D))
    assert not w.yard(sonic, a, tr) and not w.yard(sonic, b, tr) and w.yard(sonic, w.proofs[1], w.trs[1])
    for seed in seeds:
        assert v.verify_batch([a, b, w.proofs[1]], [tr, tr, w.trs[1]], seed=seed, each=True) == (False, [False, False, True]), seed
    # inside a single proof: W_a + D and W_t - D, both opened at z
    c = g1_shift(ref, g1_shift(ref, raw, Wa, D), Wt, ref.g1_neg(D))
    assert not w.yard(sonic, c, tr)
    for seed in seeds:
        assert v.verify_batch([c], [tr], seed=seed, each=True) == (False, [False]), seed


# ---- 4. malformed proofs: rejected proofs, not failed calls ----------------------------------------------------------------------------
def test_malformed_proofs_are_rejected_proofs(sonic, ref, worlds):
    from sonic_amd import _lib
    n, Q = 16, 1
    w = worlds(n, Q)
    g1, fr, _size = layout(Q)
    R_off, Wj_off = g1[0], g1[6]                       # R; W_0 of the first hsc list (R T Wa Wb Wt S_0 W_0)
    q48 = lambda v: int(v).to_bytes(48, "little")      # noqa: E731
    ns = non_subgroup_point(ref)
    points = {"order 3": q48(0) + q48(2), "outside the subgroup": q48(ns[0]) + q48(ns[1]), "off the curve": q48(1) + q48(1),
              "x >= q": q48(QMOD) + q48(2), "y >= q": q48(1) + q48(QMOD + 5)}
    cases = [(name, off, enc) for name, enc in points.items() for off in (R_off, Wj_off)]
    cases.append(("Fr >= r", fr[0], R.to_bytes(32, "little")))
    cases.append(("Fr >= r (u)", fr[-2], (R + 1).to_bytes(32, "little")))
    for form in ("dense", "csr"):
        v = w.verifier(sonic, form)
        for name, off, enc in cases:
            bad = put(w.proofs[1], off, enc)
            assert not w.yard(sonic, bad, w.trs[1], form), name
            proofs = [w.proofs[0], bad, w.proofs[2]]
            assert v.verify_batch(proofs, w.trs[:3], seed=SEED, each=True) == (False, [True, False, True]), (name, off, form)    # no exception: SONIC_OK
            assert "proof 1" in _lib.last_error(), name
        # a non-canonical challenge rejects its proof alone
        y, z, yzs = w.trs[1]
        assert v.verify_batch(w.proofs[:3], [w.trs[0], (R, z, yzs), w.trs[2]], seed=SEED, each=True) == (False, [True, False, True])
        # the encoding of infinity as a proof point: whatever sonic_verify says
        for off in (R_off, Wj_off):
            bad = put(w.proofs[1], off, bytes(96))
            want = w.yard(sonic, bad, w.trs[1], form)
            assert v.verify_batch([w.proofs[0], bad, w.proofs[2]], w.trs[:3], seed=SEED, each=True) == (want, [True, want, True])
        # u = 0: refused per proof
        bad = put(w.proofs[1], fr[-2], bytes(32))
        assert not w.yard(sonic, bad, w.trs[1], form)
        assert v.verify_batch([w.proofs[0], bad, w.proofs[2]], w.trs[:3], seed=SEED, each=True) == (False, [True, False, True])
        # the handle survives all of it
        assert v.verify_batch(w.proofs[:3], w.trs[:3], seed=SEED, each=True) == (True, [True] * 3)


def test_call_errors(sonic, worlds):
    from sonic_amd import _lib
    w = worlds(16, 1)
    v = w.verifier(sonic, "dense")
    ok = C.c_int(1)
    assert _lib.lib().sonic_verifier_verify_batch(v._h, 0, w.proofs[0], bytes(128), SEED, C.byref(ok), None) == 7 and ok.value == 0
    assert _lib.lib().sonic_verifier_verify_batch(v._h, (1 << 26) // 11 + 1, w.proofs[0], bytes(128), SEED, C.byref(ok), None) == 7
    assert _lib.lib().sonic_verifier_verify_batch(None, 1, w.proofs[0], bytes(128), SEED, C.byref(ok), None) == 7
    assert _lib.lib().sonic_verifier_device(v._h) == _lib.lib().sonic_srs_device(w.srs._h)
    with pytest.raises(sonic.SonicError) as e:                     # an SRS too short for h^{x^{n-d}} / the commitments: sonic_verify's status
        small = sonic.SRS.new(4, 5, 7)
        try:
            sonic.Verifier(small, w.dense)
        finally:
            small.close()
    assert e.value.code == 2
    with pytest.raises(sonic.SonicError) as e:                     # a non-canonical gate weight
        wL = np.array(w.dense.weights.wL, np.uint8).copy().reshape(-1, 32)
        wL[3] = np.frombuffer(R.to_bytes(32, "little"), np.uint8)
        sonic.Verifier(w.srs, sonic.ArithCircuit(sonic.GateWeights(wL, w.dense.weights.wR, w.dense.weights.wO), w.dense.cs))
    assert e.value.code == 3


# ---- 5. sonic_g1_validate alone ----------------------------------------------------------------------------------------------------------
def test_g1_validate_equals_r_times_p(sonic, ref, worlds):
    """flags == canonical and (infinity or (on the curve and [r]P = O)), [r]P by oracle/sonic_ref.py, on a few thousand points"""
    from sonic_amd import _lib
    w = worlds(256, 2)
    m = 2001
    buf = C.create_string_buffer(96 * m)
    _lib.check(_lib.lib().sonic_srs_get_points(w.srs._h, 0, -1000, m, buf))
    encs = [buf.raw[96 * i:96 * i + 96] for i in range(m)]               # multiples of the generator
    pyr = random.Random(7)
    q48 = lambda v: int(v).to_bytes(48, "little")      # noqa: E731
    x = 0
    for _ in range(150):                                                  # curve points by x = 1, 2, ...: no cofactor clearing
        x += 1
        rhs = (x * x * x + 4) % QMOD
        y = pow(rhs, (QMOD + 1) // 4, QMOD)
        if y * y % QMOD == rhs:
            encs += [q48(x) + q48(y), q48(x) + q48(QMOD - y)]
        else:
            encs.append(q48(x) + q48(y))                                  # off the curve
    encs += [q48(0) + q48(2), q48(0) + q48(QMOD - 2), bytes(96), q48(QMOD) + q48(0), q48(0) + q48(QMOD), q48(QMOD) + q48(QMOD)]
    for e in pyr.sample(encs[:m], 40):                                    # subgroup points with one coordinate damaged or lifted by q
        encs += [e[:48] + q48((int.from_bytes(e[48:], "little") + 1) % QMOD), q48(int.from_bytes(e[:48], "little") + QMOD) + e[48:]]
    pyr.shuffle(encs)

    def verdict(e):
        px, py = int.from_bytes(e[:48], "little"), int.from_bytes(e[48:], "little")
        if px == 0 and py == 0:
            return True
        if px >= QMOD or py >= QMOD or (py * py - px * px * px - 4) % QMOD:
            return False
        return subgroup_verdict(ref, (px, py))
    want = [verdict(e) for e in encs]
    assert 2000 < sum(want) < len(want) - 150
    flags = C.create_string_buffer(len(encs))
    _lib.check(_lib.lib().sonic_g1_validate(b"".join(encs), len(encs), flags))
    assert [bool(b) for b in flags.raw] == want
    # and the host verifier's load_g1, through sonic_pc_v's status, on one point of each class
    for e, ok in list(zip(encs, want))[:60]:
        acc = C.c_int(0)
        rc = _lib.lib().sonic_pc_v(w.srs._h, 16, e, bytes(32), bytes(32), bytes(96), C.byref(acc))
        assert (rc == 0) == ok and rc in (0, 3)


# ---- 6. sonic_verifier_eval_s alone ------------------------------------------------------------------------------------------------------
def _special_pairs(pyr):
    u = pyr.randrange(2, R)
    return [(pyr.randrange(1, R), pyr.randrange(1, R)), (1, pyr.randrange(2, R)), (u, u), (u, pow(u, -1, R)), (1, 1), (R - 1, R - 1)]


@pytest.mark.parametrize("n,Q", [(1, 1), (5, 2), (16, 3), (40, 2)])
def test_eval_s_equals_the_reference_polynomial(sonic, ref, n, Q):
    """byte-equal to eval_y(v, eval_x(u, s_poly(...))) of oracle/sonic_ref.py; dense and CSR handles; rnd_circuit's full rows; K = 1 and 257"""
    pyr = random.Random(31 * n + Q)
    circ, _asg, enc = circuit_arrays(ref, pyr, n, Q)
    srs = sonic.SRS.new(7 * n + 20, 11, 13)
    dense = sonic.ArithCircuit(sonic.GateWeights(enc["wL"], enc["wR"], enc["wO"]), enc["cs"])
    sXY = ref.s_poly(circ[0], circ[1], circ[2])
    pairs = _special_pairs(pyr)
    pairs += [(pyr.randrange(1, R), pyr.randrange(1, R)) for _ in range(257 - len(pairs))]
    want = [ref.lp_eval(ref.eval_y(v, sXY), u) for u, v in pairs]
    for circuit in (dense, sonic.SparseCircuit.from_circuit(dense)):
        ver = sonic.Verifier(srs, circuit)
        assert ver.eval_s(pairs) == want
        assert ver.eval_s(pairs[:1]) == want[:1]
        # u = 0 or v = 0: that pair is refused (INEXACT_DIVISION, 32 bytes of 0xff), the others still get their values
        from sonic_amd import _lib
        uv = fr_bytes([x for pr in [pairs[0], (0, 5), pairs[2], (5, 0)] for x in pr])
        out = C.create_string_buffer(32 * 4)
        assert _lib.lib().sonic_verifier_eval_s(ver._h, 4, uv.ctypes.data, out) == 4
        assert out.raw[32:64] == b"\xff" * 32 and out.raw[96:] == b"\xff" * 32
        assert [int.from_bytes(out.raw[o:o + 32], "little") for o in (0, 64)] == [want[0], want[2]]
        assert ver.eval_s(pairs[:3]) == want[:3]                       # usable afterwards
        ver.close()
    srs.close()


@pytest.mark.parametrize("kind,n,Q", [("rnd", 1 << 16, 2), ("sparse", 1 << 16, 64), ("sparse", 5000, 3)])
def test_eval_s_equals_the_python_restatement_at_size(sonic, kind, n, Q):
    """n up to 2^16 against tests/batch_ref.s_of_uv (numpy-free): rndCircuit's full rows, and sparse rows some of which are empty"""
    from sonic_amd import workload
    if kind == "rnd":
        b = big_circuit(3, n, Q)
        dense = sonic.ArithCircuit(sonic.GateWeights(b["wL"], b["wR"], b["wO"]), b["cs"])
        sp = sonic.SparseCircuit.from_circuit(dense)
        circuits = [dense, sp]
    else:
        s = workload.sparse_circuit(5, n, Q, 4)
        sp = sonic.SparseCircuit(n, Q, s["row_ptr"], s["col"], s["val"], s["cs"])
        assert any(sp.row_ptr[r] == sp.row_ptr[r + 1] for r in range(3 * Q))                 # rows with no entries
        circuits = [sp] + ([sp.to_dense()] if n <= 5000 else [])
    vals = [int.from_bytes(sp.val[i].tobytes(), "little") for i in range(sp.nnz)]
    rows = [[(int(sp.col[k]), vals[k]) for k in range(int(sp.row_ptr[r]), int(sp.row_ptr[r + 1]))] for r in range(3 * Q)]
    pyr = random.Random(n + Q)
    pairs = _special_pairs(pyr)[:4]
    want = [batch_ref.s_of_uv(n, Q, rows, u, v) for u, v in pairs]
    srs = sonic.SRS.new(n, 11, 13)                     # (the handle fetches h^{x^{n-d}} and h^{x^0}: d = n serves)
    for circuit in circuits:
        ver = sonic.Verifier(srs, circuit)
        assert ver.eval_s(pairs) == want
        ver.close()
    srs.close()


# ---- 7. seeds ----------------------------------------------------------------------------------------------------------------------------
def test_seeds(sonic, worlds):
    w = worlds(256, 2)
    v = w.verifier(sonic, "dense")
    proofs, trs = list(w.proofs[:5]), list(w.trs[:5])
    assert v.verify_batch(proofs, trs, seed=None, each=True) == (True, [True] * 5)           # the library draws the seed
    y, z, yzs = trs[3]
    trs[3] = (y, (z + 1) % R, yzs)
    first = v.verify_batch(proofs, trs, seed=SEED, each=True)
    assert first == (False, [True, True, True, False, True])
    for _ in range(3):
        assert v.verify_batch(proofs, trs, seed=SEED, each=True) == first
    assert v.verify_batch(proofs, trs, seed=None, each=True) == first
    assert sonic.verify_batch(w.srs, w.sparse, proofs, trs, each=True) == first              # the one-line convenience
    with pytest.raises(ValueError):
        v.verify_batch(proofs, trs, seed=b"short")


def test_two_handles_on_one_srs_from_two_threads(sonic, worlds):
    w = worlds(256, 2)
    proofs, trs = list(w.proofs[:8]), list(w.trs[:8])
    y, z, yzs = trs[5]
    trs[5] = ((y + 1) % R, z, yzs)
    want = (False, [k != 5 for k in range(8)])
    out = {}

    def run(i):
        try:
            v = sonic.Verifier(w.srs, w.dense if i else w.sparse)
            out[i] = [v.verify_batch(proofs, trs, seed=SEED, each=True) for _ in range(2)]
            v.close()
        except Exception as e:      # noqa: BLE001
            out[i] = e
    th = [threading.Thread(target=run, args=(i,)) for i in range(2)]
    for t in th:
        t.start()
    for t in th:
        t.join(600)
    assert out == {0: [want, want], 1: [want, want]}


# ---- 8. one larger batch -----------------------------------------------------------------------------------------------------------------
def test_larger_batch_256_at_2_12(sonic, ref, worlds):
    """K = 256 at n = 2^12, Q = 2: the MSM's multi-window path and more than one block per proof in the s-kernel"""
    n, Q, K = 1 << 12, 2, 256
    w = worlds(n, Q, K)
    assert w.yard(sonic, w.proofs[0], w.trs[0]) and w.yard(sonic, w.proofs[K - 1], w.trs[K - 1])
    v = w.verifier(sonic, "csr")
    assert v.verify_batch(w.proofs, w.trs, seed=SEED, each=True) == (True, [True] * K)
    g1, _fr, _size = layout(Q)
    proofs = list(w.proofs)
    proofs[K - 1] = g1_shift(ref, proofs[K - 1], g1[4], ref.G1_GEN)          # W_t + g in proof 255 alone
    assert not w.yard(sonic, proofs[K - 1], w.trs[K - 1])
    assert v.verify_batch(proofs, w.trs, seed=SEED, each=True) == (False, [True] * (K - 1) + [False])
    assert v.verify_batch(w.proofs, w.trs, seed=SEED) is True                # and the handle is usable afterwards
