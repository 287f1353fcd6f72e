"""The circuit kernels at their chunk, item, stage and finish-loop edges (sonic_amd/csrc: k_s_of_y_csc, k_s_of_u_csr, k_s_of_u_csr_finish,
k_csr_row_terms, k_t_operands in poly.hip; k_cs_csr, k_cs_dense, k_cs_finish in statement.hip; k_s_of_uv_batch, k_s_of_uv_finish in
verify_batch.hip; k_agg_s_of_y_csc in aggregate.hip).  Each picks its path by a threshold on row length, n or Q; the shapes here sit on
those thresholds and one past them, derived from the constants mirrored in tests/circuit_edges_ref.py, which the first test holds against
the sources.

Yardsticks: Python integers (the constants, s(u, v)), the CPU oracle (proof bytes) and the host verifiers (sonic_hsc_verify,
sonic_verify_core).  "CSR handle = dense handle" is asserted beside one of those, never alone.  Everything is byte or integer equality.
Where a path can be seen it is asserted through the kernel profiler's launch counts; the LDS `stage` argument cannot be seen, and the
pinned constants stand for it.

  0  the thresholds, pinned (no GPU)
  1  the t(X, y) product at exact fill of its transform: 7n + 9 = 2^10, 2^13, 2^16, and n + 1
  2  one circuit of n = 1025 whose rows have every length in {0, 1, 31, 32, 33, 63, 64, 65, 511, 512, 513, 1024, 1025} and three
     constraints of 255 / 256 / 257 terms: eval_constraints, eval_s, prove, hsc_prove
  3  finish loops on their second trip: 258 blocks of s(u, v) partials; rows of 131073 and 131072 entries (257 and 256 chunks), n = 131073
     (513 dense block partials)
  4  LDS staging switches: Q = 1024 / 1025 in s(X, y); (J, Q) = (8, 192) / (8, 193) / (1, 1536) / (1, 1537) in the aggregate's
"""
import ctypes as C
import random
from collections import Counter

import numpy as np
import pytest

import aggregate_ref as aref
import batch_ref
import circuit_edges_ref as ce
from util import NCPU, R, big_circuit, fr_bytes, rand_fr_array

gpu = pytest.mark.gpu
THREADS = min(NCPU, 16)
SRS_INDEX, INEXACT_DIVISION = 2, 4


# ---- 0. the thresholds, pinned ----------------------------------------------------------------------------------------------------------
def test_the_thresholds_the_shapes_rest_on():
    got = ce.source_thresholds()
    moved = {k: (got[k], ce.MIRRORED[k]) for k in ce.MIRRORED if got[k] != ce.MIRRORED[k]}
    assert not moved and set(got) == set(ce.MIRRORED), "; ".join(
        "%s is %r in the source, %r in tests/circuit_edges_ref.py: move it there, and with it %s" % (k, a, b, ce.MOVES[k]) for k, (a, b) in moved.items())
    # the shapes, as the sections below state them
    assert ce.exact_fill_ns() == [(145, True), (146, False), (1169, True), (1170, False), (9361, True)]
    for n, exact in ce.exact_fill_ns():
        check_fill(n, exact)
    assert [ce.transform_size(n) for n, _ in ce.exact_fill_ns()] == [1 << 10, 1 << 11, 1 << 13, 1 << 14, 1 << 16]
    assert ce.edge_lengths() == [0, 1, 31, 32, 33, 63, 64, 65, 511, 512, 513, 1024, 1025]
    assert [sum(t) for t in ce.term_triples()] == [255, 256, 257]
    assert ce.DIAGONAL_NS == [31, 32, 33] and ce.CSC_STAGE_QS == [1024, 1025]
    assert ce.agg_stage_cases() == [(192, 9), (193, 9), (1536, 1), (1537, 1)]
    assert [ce.agg_stages(Q, K) for Q, K in ce.agg_stage_cases()] == [[(8, True), (1, True)], [(8, False), (1, True)], [(1, True)], [(1, False)]]
    assert ce.CSC_STAGE_MAX_Q * ce.FR_BYTES == 32 * 1024                       # the largest dynamic-LDS launch of k_s_of_y_csc
    assert ce.uv_finish_shape() == (64, 22000) and ce.long_rows_shape() == (131073, (131073, 131072, 513))


def test_the_edge_circuit_is_what_it_claims():
    n, Q, rows = ce.edge_circuit(2)
    assert (n, Q, len(rows)) == (1025, 16, 48)
    lens = ce.row_lengths(rows)
    assert Counter(lens) == ce.expected_length_multiset()
    for m in range(3):                                                         # every length in each of wL, wR, wO
        assert set(ce.edge_lengths()) <= set(lens[m * Q:(m + 1) * Q])
    per_q = [(lens[q], lens[Q + q], lens[2 * Q + q]) for q in range(Q)]
    assert all(len(set(t)) == 3 for t in per_q[:13])                           # no constraint with three equal lengths
    assert [sum(t) for t in per_q[13:]] == [ce.ROW_TERMS_BLOCK - 1, ce.ROW_TERMS_BLOCK, ce.ROW_TERMS_BLOCK + 1]
    assert all(cols == sorted(set(cols)) and 0 <= cols[0] and cols[-1] < n for cols in ([c for c, _ in r] for r in rows if r))
    zeros = sum(1 for r in rows for _, v in r if v == 0)
    assert 3 <= zeros <= 10
    assert all(v for r in rows for k, (_, v) in enumerate(r) if k != 1)        # the explicit zeros are second entries only
    row_ptr, col, val = ce.csr_arrays(rows)
    assert row_ptr[-1] == len(col) == val.shape[0] == sum(lens) and ce.ints_of(val) == [v for r in rows for _, v in r]


# ---- helpers ----------------------------------------------------------------------------------------------------------------------------
def launches(names, fn):
    """fn() under the kernel profiler: (its result, {kernel name: launches})"""
    from sonic_amd import _lib
    L = _lib.lib()
    assert L.sonic_profile_reset() == 0 and L.sonic_profile_enable(1) == 0
    try:
        out = fn()
        counts = {}
        for name in names:
            ms, k = C.c_double(0), C.c_int64(0)
            assert L.sonic_profile_get(name.encode(), C.byref(ms), C.byref(k)) == 0
            counts[name] = k.value
    finally:
        L.sonic_profile_enable(0)
    return out, counts


def transcript(pyr, Q):
    return [pyr.randrange(1, R) for _ in range(8 + 2 * Q)]


def sparse_of(sonic, n, Q, rows, cs):
    row_ptr, col, val = ce.csr_arrays(rows)
    return sonic.SparseCircuit(n, Q, row_ptr, col, val, fr_bytes(cs))


def dense_args(dense):
    w = dense.weights
    return [np.ascontiguousarray(x).reshape(-1, 32) for x in (w.wL, w.wR, w.wO)] + [np.ascontiguousarray(dense.cs)]


def hsc_bytes(proof):
    from sonic_amd.protocol import _hsc_to_bytes
    return _hsc_to_bytes(proof)


def special_pairs(pyr):
    u = pyr.randrange(2, R)
    return [(pyr.randrange(1, R), pyr.randrange(1, R)), (pyr.randrange(1, R), pyr.randrange(1, R)), (1, pyr.randrange(2, R)), (u, u), (u, pow(u, -1, R)), (R - 1, R - 1)]


def refused(code, fn):
    from sonic_amd import _lib
    with pytest.raises(_lib.SonicError) as e:
        fn()
    assert e.value.code == code, e.value


# ---- 1. the t-product at exact fill -----------------------------------------------------------------------------------------------------
def check_fill(n, exact):
    """exact: 7n + 9 is a power of two and the transform has exactly that many points.  Otherwise n is the first size past one: n - 1
    fills its transform, 7n + 9 is that power of two and 7 more, and the transform is twice as large"""
    if exact:
        assert ce.is_pow2(ce.tlen(n)) and ce.transform_size(n) == ce.tlen(n)
    else:
        assert ce.is_pow2(ce.tlen(n - 1)) and ce.tlen(n) == ce.tlen(n - 1) + ce.T_LEN[0] and ce.transform_size(n) == 2 * ce.tlen(n - 1)


@gpu
@pytest.mark.parametrize("n,exact", ce.exact_fill_ns())
def test_t_product_at_exact_fill(sonic, orc, n, exact):
    """7n + 9 coefficients in a transform of exactly 7n + 9 points (no padding: a cyclic wrap lands on a live coefficient), and at n + 1
    the transform of twice the size; dense handle, with and without prepare, against the oracle"""
    check_fill(n, exact)
    Q = 2
    pyr = random.Random(7000 + n)
    d = 7 * n + 1 + pyr.randrange(1, 8)
    x, alpha = pyr.randrange(2, R), pyr.randrange(2, R)
    c = big_circuit(n, n, Q)
    tr = transcript(pyr, Q)
    g, o = sonic.SRS.new(d, x, alpha), orc.SRS(d, x, alpha, threads=THREADS)
    orc.set_mode(1, THREADS)
    want = orc.prove(o, n, Q, c["wL"], c["wR"], c["wO"], c["cs"], c["aL"], c["aR"], c["aO"], fr_bytes(tr), True)
    circuit = sonic.ArithCircuit(sonic.GateWeights(c["wL"], c["wR"], c["wO"]), c["cs"])
    try:
        for prepare in (False, True):
            p = sonic.Prover(g, circuit, prepare=prepare)
            try:
                p.set_assignment(sonic.Assignment(c["aL"], c["aR"], c["aO"]))
                got, ran = launches(["k_t_operands"], lambda: p.prove_bytes(tr))
                assert got == want, prepare
                assert ran == {"k_t_operands": 1}
            finally:
                p.close()
    finally:
        g.close()


# ---- 2. row lengths at every chunk, wave and item edge ----------------------------------------------------------------------------------
class EdgeWorld:
    """the circuit of section 2 in both forms, three satisfied assignments (the first one's constants are the circuit's) and its strings"""

    def __init__(self, sonic, orc):
        self.n, self.Q, self.rows = ce.edge_circuit(2)
        pyr = random.Random(1025)
        self.asgs = [ce.rand_assignment(pyr, self.n) for _ in range(3)]
        self.cs = [ce.cs_of(self.rows, self.Q, a) for a in self.asgs]
        self.sp = sparse_of(sonic, self.n, self.Q, self.rows, self.cs[0])
        self.dense = self.sp.to_dense()
        self.d = 7 * self.n + 9 + pyr.randrange(1, 8)
        x, alpha = pyr.randrange(2, R), pyr.randrange(2, R)
        self.srs, self.osrs = sonic.SRS.new(self.d, x, alpha), orc.SRS(self.d, x, alpha, threads=THREADS)
        self.tr = transcript(pyr, self.Q)
        self.nchunks = sum(ce.chunks(k) for k in ce.row_lengths(self.rows))

    def prover(self, sonic, form, prepare=False):
        p = sonic.Prover(self.srs, self.sp if form == "csr" else self.dense, prepare=prepare)
        p.set_assignment(sonic.Assignment(*self.asgs[0]))
        return p


@pytest.fixture(scope="module")
def edge(sonic, orc):
    w = EdgeWorld(sonic, orc)
    yield w
    w.srs.close()


CS_KERNELS = ["k_cs_csr", "k_cs_dense", "k_cs_finish"]


@gpu
@pytest.mark.parametrize("form", ["csr", "dense"])
def test_eval_constraints_at_the_row_length_edges(sonic, edge, form):
    w = edge
    assert Counter(ce.row_lengths(w.rows)) == ce.expected_length_multiset() and w.nchunks == 57
    p = w.prover(sonic, form)
    try:
        A = [sonic.Assignment(*a) for a in w.asgs]
        for B in (1, 3):
            (cs, gates), ran = launches(CS_KERNELS, lambda: p.eval_constraints(A[:B]))
            assert cs == w.cs[:B], B
            assert gates == [(0, -1)] * B
            assert ran == (dict(k_cs_csr=1, k_cs_dense=0, k_cs_finish=1) if form == "csr" else dict(k_cs_csr=0, k_cs_dense=1, k_cs_finish=1))
        aL, aR, aO = w.asgs[2]
        at = ce.CSR_CHUNK                                                       # gate 512: the 513th
        bad = (aL, aR, aO[:at] + [(aO[at] + 1) % R] + aO[at + 1:])
        cs, gates = p.eval_constraints([A[1], sonic.Assignment(*bad)])
        assert gates == [(0, -1), (1, at)]
        assert cs == [w.cs[1], ce.cs_of(w.rows, w.Q, bad)] and cs[1] != w.cs[2]
        assert p.eval_constraints() == ([w.cs[0]], [(0, -1)])                   # the resident assignment
    finally:
        p.close()


@gpu
@pytest.mark.parametrize("form", ["csr", "dense"])
def test_eval_s_at_the_row_length_edges(sonic, edge, form):
    w = edge
    pairs = special_pairs(random.Random(33))
    want = [batch_ref.s_of_uv(w.n, w.Q, w.rows, u, v) for u, v in pairs]
    assert len(set(want)) == len(want)
    ver = sonic.Verifier(w.srs, w.sp if form == "csr" else w.dense)
    try:
        got, ran = launches(["k_s_of_uv_batch", "k_s_of_uv_finish"], lambda: ver.eval_s(pairs))
        assert got == want
        assert ran == dict(k_s_of_uv_batch=1, k_s_of_uv_finish=1)
        assert ver.eval_s(pairs[3:4]) == want[3:4]
    finally:
        ver.close()


@gpu
@pytest.mark.parametrize("n", ce.DIAGONAL_NS)
def test_eval_s_diagonal_items_last_item(sonic, n):
    """n = 31, 32, 33 with full rows: the last diagonal item holds 31, 32 and 1 gates, the rows' last items as many entries"""
    Q = 1
    rows = ce.full_rows_circuit(300 + n, n, Q)
    assert ce.uv_blocks(n, ce.row_lengths(rows)) == ((3, 1, 1) if n <= ce.S_ITEM else (6, 2, 1))
    pairs = special_pairs(random.Random(n))
    want = [batch_ref.s_of_uv(n, Q, rows, u, v) for u, v in pairs]
    srs = sonic.SRS.new(7 * n, 11, 13)
    sp = sparse_of(sonic, n, Q, rows, [0] * Q)
    try:
        for circuit in (sp, sp.to_dense()):
            ver = sonic.Verifier(srs, circuit)
            try:
                assert ver.eval_s(pairs) == want
            finally:
                ver.close()
    finally:
        srs.close()


@gpu
@pytest.mark.parametrize("prepare", [False, True], ids=["unprepared", "prepared"])
def test_prove_at_the_row_length_edges(sonic, orc, edge, prepare):
    """the CSR handle's proof is the oracle's on the densified circuit; its s(u, Y) came from the chunked kernels, and a prepared handle
    gathered one MSM's terms per constraint (of 255, 256 and 257 terms among them)"""
    w = edge
    orc.set_mode(1, THREADS)
    a = w.asgs[0]
    want = orc.prove(w.osrs, w.n, w.Q, *dense_args(w.dense), fr_bytes(a[0]), fr_bytes(a[1]), fr_bytes(a[2]), fr_bytes(w.tr), True)
    p, made = launches(["k_csr_row_terms"], lambda: w.prover(sonic, "csr", prepare=prepare))
    try:
        assert made == dict(k_csr_row_terms=w.Q if prepare else 0)              # (no constraint of this circuit is empty)
        got, ran = launches(["k_s_of_u_csr", "k_s_of_u_csr_finish", "k_s_of_u_rows", "k_s_of_y_csc", "k_s_of_y"], lambda: p.prove_bytes(w.tr))
        assert got == want
        assert ran["k_s_of_u_csr"] == 1 and ran["k_s_of_u_csr_finish"] == 1 and ran["k_s_of_u_rows"] == 0 and ran["k_s_of_y"] == 0
        assert ran["k_s_of_y_csc"] == 1 + w.Q if not prepare else ran["k_s_of_y_csc"] >= 1      # s(X, y), and s(X, y_j) where S_j needs it
    finally:
        p.close()


@gpu
def test_hsc_prove_at_the_row_length_edges(sonic, edge):
    w = edge
    pyr = random.Random(65)
    yzs = [(pyr.randrange(1, R), pyr.randrange(1, R)) for _ in range(2)]
    u, v = pyr.randrange(1, R), pyr.randrange(1, R)
    pc, pd = w.prover(sonic, "csr"), w.prover(sonic, "dense")
    try:
        got, ran = launches(["k_s_of_u_csr", "k_s_of_u_csr_finish", "k_s_of_u_rows"], lambda: pc.hsc_prove(yzs, u, v))
        assert ran == dict(k_s_of_u_csr=1, k_s_of_u_csr_finish=1, k_s_of_u_rows=0)
        ref_proof, ran = launches(["k_s_of_u_csr", "k_s_of_u_rows"], lambda: pd.hsc_prove(yzs, u, v))
        assert ran == dict(k_s_of_u_csr=0, k_s_of_u_rows=1)
        assert hsc_bytes(got) == hsc_bytes(ref_proof)
        assert sonic.hsc_verify(w.srs, w.dense, yzs, got)                        # (the host evaluates s(u, v) on its own)
    finally:
        pc.close(); pd.close()


# ---- 3a. k_s_of_uv_finish on its second trip --------------------------------------------------------------------------------------------
@gpu
def test_s_of_uv_finish_over_more_than_one_trip(sonic):
    from sonic_amd import _lib
    n, Q = ce.uv_finish_shape()
    row_items, diag, blocks = ce.uv_blocks(n, [1] * (3 * Q))
    assert (row_items, diag, blocks) == (66000, 2, 258) and blocks > ce.S_BLOCK
    rng = np.random.default_rng(3)
    col, val = rng.integers(0, n, size=3 * Q), rand_fr_array(rng, 3 * Q)
    sp = sonic.SparseCircuit(n, Q, np.arange(3 * Q + 1), col, val, np.zeros((Q, 32), np.uint8))
    rows = [[(int(c), w)] for c, w in zip(col, ce.ints_of(val))]
    pyr = random.Random(66000)
    u = pyr.randrange(2, R)
    pairs = [(pyr.randrange(1, R), pyr.randrange(1, R)), (u, pow(u, -1, R)), (R - 1, pyr.randrange(1, R))]
    want = [batch_ref.s_of_uv(n, Q, rows, a, b) for a, b in pairs]
    srs = sonic.SRS.new(n, 11, 13)
    ver = sonic.Verifier(srs, sp, digest=2)
    try:
        got, ran = launches(["k_s_of_uv_batch", "k_s_of_uv_finish"], lambda: ver.eval_s(pairs))
        assert got == want
        assert ran == dict(k_s_of_uv_batch=1, k_s_of_uv_finish=1)
        # (0, v) in the middle of the batch: that pair is refused, its neighbours keep their values
        uv = fr_bytes([x for pr in [pairs[0], (0, 5), pairs[2]] for x in pr])
        out = C.create_string_buffer(32 * 3)
        assert _lib.lib().sonic_verifier_eval_s(ver._h, 3, uv.ctypes.data, out) == INEXACT_DIVISION
        assert out.raw[32:64] == b"\xff" * 32
        assert [int.from_bytes(out.raw[o:o + 32], "little") for o in (0, 64)] == [want[0], want[2]]
        assert ver.eval_s(pairs[1:2]) == want[1:2]
    finally:
        ver.close()
        srs.close()


# ---- 3b. rows of more than 256 chunks, n of more than 256 blocks ------------------------------------------------------------------------
class LongRows:
    """n = 131073, Q = 2: wL[0] full (256 chunks and one of one entry), wR[0] with all gates but one (exactly 256 chunks), wO[1] of 513
    entries; a CSR handle and the densified dense handle, neither prepared"""

    def __init__(self, sonic):
        n, (full, most, few) = ce.long_rows_shape()
        self.n, self.Q = n, 2
        rng = np.random.default_rng(131073)
        lens = [full, 0, most, 0, 0, few]                                         # wL[0], wL[1], wR[0], wR[1], wO[0], wO[1]
        self.lens = lens
        row_ptr = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
        col = np.concatenate([np.arange(n), np.delete(np.arange(n), 77), np.sort(rng.choice(n, size=few, replace=False))]).astype(np.int64)
        val = rand_fr_array(rng, int(row_ptr[-1]))
        vals = ce.ints_of(val)
        self.rows = [[(int(col[k]), vals[k]) for k in range(int(row_ptr[r]), int(row_ptr[r + 1]))] for r in range(6)]
        self.A = [(rand_fr_array(rng, n), rand_fr_array(rng, n)) for _ in range(2)]
        self.asgs = []
        for aL, aR in self.A:
            la, lb = ce.ints_of(aL), ce.ints_of(aR)
            self.asgs.append((la, lb, [a * b % R for a, b in zip(la, lb)]))
        self.cs = [ce.cs_of(self.rows, self.Q, a) for a in self.asgs]
        self.sp = sonic.SparseCircuit(n, self.Q, row_ptr, col, val, fr_bytes(self.cs[0]))
        self.dense = self.sp.to_dense()
        self.srs = sonic.SRS.new(7 * n + 9, 0x1234567891, 0x987654321)
        self.assignments = [sonic.Assignment(aL, aR, fr_bytes(a[2])) for (aL, aR), a in zip(self.A, self.asgs)]
        self.pc, self.pd = sonic.Prover(self.srs, self.sp, prepare=False), sonic.Prover(self.srs, self.dense, prepare=False)
        for p in (self.pc, self.pd):
            p.set_assignment(self.assignments[0])

    def close(self):
        self.pc.close(); self.pd.close(); self.srs.close()


@pytest.fixture(scope="module")
def long_rows(sonic):
    w = LongRows(sonic)
    yield w
    w.close()


@gpu
def test_long_rows_shape_facts(long_rows):
    w = long_rows
    assert [ce.chunks(k) for k in w.lens] == [ce.CSR_FINISH_BLOCK + 1, 0, ce.CSR_FINISH_BLOCK, 0, 0, 2] == [257, 0, 256, 0, 0, 2]
    assert w.lens[0] % ce.CSR_CHUNK == 1 and w.lens[2] % ce.CSR_CHUNK == 0
    assert -(-w.n // ce.CS_BLOCK) == 2 * ce.CS_BLOCK + 1 == 513                 # block partials per row of the dense form
    assert ce.row_lengths(w.rows) == w.lens


@gpu
@pytest.mark.parametrize("form", ["csr", "dense"])
def test_cs_finish_over_more_than_one_trip(sonic, long_rows, form):
    """k_cs_finish adds 257 + 256 chunk partials for q = 0 (CSR form) and 513 block partials per row (dense form)"""
    w = long_rows
    p = w.pc if form == "csr" else w.pd
    (cs, gates), ran = launches(CS_KERNELS, lambda: p.eval_constraints(w.assignments))
    assert cs == w.cs
    assert gates == [(0, -1)] * 2
    assert ran == (dict(k_cs_csr=1, k_cs_dense=0, k_cs_finish=1) if form == "csr" else dict(k_cs_csr=0, k_cs_dense=1, k_cs_finish=1))


@gpu
def test_s_of_u_csr_finish_over_more_than_one_trip(sonic, long_rows):
    """hsc_prove over a row of 257 chunks: the CSR handle's bytes are the dense handle's (k_s_of_u_rows), and the host verifier, which
    evaluates s(u, v) itself, accepts them"""
    w = long_rows
    pyr = random.Random(257)
    yzs = [(pyr.randrange(1, R), pyr.randrange(1, R))]
    u, v = pyr.randrange(1, R), pyr.randrange(1, R)
    got, ran = launches(["k_s_of_u_csr", "k_s_of_u_csr_finish", "k_s_of_u_rows"], lambda: w.pc.hsc_prove(yzs, u, v))
    assert ran == dict(k_s_of_u_csr=1, k_s_of_u_csr_finish=1, k_s_of_u_rows=0)
    ref_proof, ran = launches(["k_s_of_u_csr", "k_s_of_u_rows"], lambda: w.pd.hsc_prove(yzs, u, v))
    assert ran == dict(k_s_of_u_csr=0, k_s_of_u_rows=1)
    assert hsc_bytes(got) == hsc_bytes(ref_proof)
    assert sonic.hsc_verify(w.srs, w.dense, yzs, got)


@gpu
def test_eval_s_over_long_rows(sonic, long_rows):
    w = long_rows
    pyr = random.Random(513)
    u = pyr.randrange(2, R)
    pairs = [(pyr.randrange(1, R), pyr.randrange(1, R)), (u, pow(u, -1, R))]
    want = [batch_ref.s_of_uv(w.n, w.Q, w.rows, a, b) for a, b in pairs]
    ver = sonic.Verifier(w.srs, w.sp, digest=2)
    try:
        assert ver.eval_s(pairs) == want
    finally:
        ver.close()


# ---- 4. LDS staging switches ------------------------------------------------------------------------------------------------------------
STAGE_N, STAGE_D = 8, 2048


@pytest.fixture(scope="module")
def stage_srs(sonic):
    pyr = random.Random(48)
    g = sonic.SRS.new(STAGE_D, pyr.randrange(2, R), pyr.randrange(2, R))
    yield g
    g.close()


def stage_world(sonic, Q):
    """n = 8, rows of 1 to 4 entries, one satisfied statement, in both forms"""
    n = STAGE_N
    rows = ce.short_rows_circuit(4000 + Q, n, Q)
    asg = ce.rand_assignment(random.Random(4100 + Q), n)
    cs = ce.cs_of(rows, Q, asg)
    sp = sparse_of(sonic, n, Q, rows, cs)
    return rows, asg, cs, sp, sp.to_dense()


@gpu
@pytest.mark.parametrize("Q", ce.CSC_STAGE_QS)
def test_s_of_y_csc_at_the_staging_switch(sonic, stage_srs, Q):
    """Q = 1024: the largest staged launch (32 KB of LDS); Q = 1025: the first through L2.  The host verifier computes s(z, y) itself"""
    rows, asg, cs, sp, dense = stage_world(sonic, Q)
    tr = [random.Random(Q).randrange(1, R) for _ in range(6)]
    pc, pd = sonic.Prover(stage_srs, sp, prepare=False), sonic.Prover(stage_srs, dense, prepare=False)
    try:
        for p in (pc, pd):
            p.set_assignment(sonic.Assignment(*asg))
        core, ran = launches(["k_s_of_y_csc", "k_s_of_y"], lambda: pc.prove_core_bytes(tr))
        assert ran == dict(k_s_of_y_csc=1, k_s_of_y=0)
        want, ran = launches(["k_s_of_y_csc", "k_s_of_y"], lambda: pd.prove_core_bytes(tr))
        assert ran == dict(k_s_of_y_csc=0, k_s_of_y=1)
        assert core == want
        assert sonic.verify_core(stage_srs, sp, core, tr[4], tr[5])
        s_zy = batch_ref.s_of_uv(STAGE_N, Q, rows, tr[5], tr[4])
        assert core[544:576] == s_zy.to_bytes(32, "little")                     # the proof's s is s(z, y), in Python integers
        for q in (0, Q - 1):                                                    # one constant moved by one: t(X, y) keeps a constant term
            bad = list(cs); bad[q] = (bad[q] + 1) % R
            pc.set_constants(bad)
            refused(SRS_INDEX, lambda: pc.prove_core_bytes(tr))
        pc.set_constants(cs)
        assert pc.prove_core_bytes(tr) == core
    finally:
        pc.close(); pd.close()


@gpu
@pytest.mark.parametrize("Q,K", ce.agg_stage_cases())
def test_aggregate_at_the_staging_switch(sonic, stage_srs, Q, K):
    """(J, Q) = (8, 192): 48 KB exactly, staged; (8, 193): not staged, beside a last tile of J = 1 that is; (1, 1536) and (1, 1537) alike"""
    from sonic_amd.protocol import _hsc_from_bytes
    stages = ce.agg_stages(Q, K)
    assert [j for j, _ in stages] == ([ce.AGG_TILE, 1] if K > 1 else [1])
    rows, asg, cs, sp, dense = stage_world(sonic, Q)
    pyr = random.Random(100 * Q + K)
    trs = [[pyr.randrange(1, R) for _ in range(6)] for _ in range(K)]
    yzs = [(t[4], t[5]) for t in trs]
    wd = sonic.fs_weights_digest_v2(sp)
    # the same circuit with one weight moved by one
    r0, (c0, v0) = next((r, row[0]) for r, row in enumerate(rows) if row)
    rows2 = [list(row) for row in rows]
    rows2[r0][0] = (c0, (v0 + 1) % R or 1)
    sp2 = sparse_of(sonic, STAGE_N, Q, rows2, cs)
    pc, pd, p2 = (sonic.Prover(stage_srs, c, prepare=False) for c in (sp, dense, sp2))
    ver = sonic.Verifier(stage_srs, sp, digest=2)
    try:
        pc.set_assignment(sonic.Assignment(*asg))
        proofs = [pc.prove_core_bytes(t) for t in trs]
        agg, ran = launches(["k_agg_s_of_y_csc", "k_agg_s_of_y"], lambda: pc.aggregate_core(yzs, weights_digest=wd))
        assert ran["k_agg_s_of_y_csc"] >= len(stages) and ran["k_agg_s_of_y"] == 0
        want, ran = launches(["k_agg_s_of_y_csc", "k_agg_s_of_y"], lambda: pd.aggregate_core(yzs, weights_digest=wd))
        assert ran["k_agg_s_of_y_csc"] == 0 and ran["k_agg_s_of_y"] >= len(stages)
        assert agg == want
        # s_k of the aggregate is s(z_k, y_k) in Python integers, and the host verifier accepts the signature
        assert [aref.s_of(K, agg, k) for k in range(K)] == [batch_ref.s_of_uv(STAGE_N, Q, rows, z, y).to_bytes(32, "little") for y, z in yzs]
        assert sonic.hsc_verify(stage_srs, dense, yzs, _hsc_from_bytes(agg, K))
        assert ver.verify_core_batch_helped(proofs, yzs, agg, seed=b"\x51" * 32, each=True) == (True, [True] * K)
        # the changed circuit's aggregate, made under the honest circuit's digest: rejected
        other = p2.aggregate_core(yzs, weights_digest=wd)
        assert other != agg
        assert ver.verify_core_batch_helped(proofs, yzs, other, seed=b"\x51" * 32, each=True) == (False, [False] * K)
        assert not sonic.hsc_verify(stage_srs, dense, yzs, _hsc_from_bytes(other, K))
    finally:
        ver.close()
        for p in (pc, pd, p2):
            p.close()
