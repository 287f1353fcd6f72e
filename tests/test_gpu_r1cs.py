"""R1CS front end on the GPU (include/sonic_hip.h, "R1CS front end"): sonic_r1cs_assign against the Python-integer model of the mapping
(tests/r1cs_ref.py), every byte of aL, aR, aO, cs and bad, with no tolerance -- at row lengths on both sides of the row chunk, every
witness kind and memory, strides, and the seam between staging chunks; the refusals, which leave the outputs untouched; a compiled circuit
through the prover's core proofs and the verifier; and the cubic example as a full proof against the CPU oracle.

Shapes are the smallest that reach every path: N = 2T + 2 or 2T + 3 around the row chunk T, m up to 300 (two blocks of gates), K up to 17.
On an MI355X the whole file takes 3.7 s; the slowest cases are 0.39 s (the cubic full proof), 0.27 s (m = 300, K = 17) and 0.23 s (end to end)."""
import os
import random
import sys

import numpy as np
import pytest

import r1cs_ref as ref
from util import NCPU, R, fr_bytes

pytestmark = pytest.mark.gpu

INVALID_ARG, BAD_ENCODING = 7, 3
I64_MIN, I64_MAX = -(1 << 63), (1 << 63) - 1
FILL = 0xAB


@pytest.fixture(scope="module")
def torch():
    import torch as t
    return t


@pytest.fixture(scope="module")
def T(sonic):
    from sonic_amd import _lib
    t = _lib.lib().sonic_r1cs_row_chunk()
    assert t >= 2
    return t


def coeff(rng):
    return lambda: rng.choice([0, 1, R - 1, rng.randrange(R)])


def row_lengths(m, N, T):
    """rows of 0, 1, T - 1, T, T + 1 and 2T + 1 entries in each of A, B, C (shifted against each other), as far as m and N allow"""
    want = [0, 1, T - 1, T, T + 1, 2 * T + 1]
    if m < 6:
        want = [2 * T + 1, T, T + 1, 1, 0, T - 1]
    clip = lambda v: min(v, N)      # noqa: E731
    # (B and C of a row are equally long: an empty C row stays empty only beside a product that is zero)
    return [(clip(want[i % 6]), clip(want[(i + 2) % 6]), clip(want[(i + 2) % 6])) for i in range(m)]


def witnesses(rng, N, K, kind, first=None):
    """K witnesses as python integers in (-2^63, 2^63) for int64 or [0, r) for Fr; witness 0 is `first` when given"""
    out = []
    for k in range(K):
        if kind == "i64":
            z = [1] + [rng.choice([I64_MIN, I64_MAX, -1, 0, rng.randrange(I64_MIN, I64_MAX + 1)]) for _ in range(N - 1)]
        else:
            z = [1] + [rng.choice([0, R - 1, rng.randrange(R)]) for _ in range(N - 1)]
        out.append(z)
    if first is not None:
        out[0] = list(first)
    return out


def z_array(zs, N, kind, pad=0):
    """[K, N + pad, ...] numpy array whose [:, :N] holds the witnesses (pad > 0: a leading stride above one witness)"""
    K = len(zs)
    if kind == "i64":
        a = np.full((K, N + pad), 77, np.int64)
        a[:, :N] = np.array(zs, dtype=np.int64)
    else:
        a = np.full((K, N + pad, 32), 0, np.uint8)
        a[:, :N] = np.frombuffer(b"".join((v % R).to_bytes(32, "little") for z in zs for v in z), np.uint8).reshape(K, N, 32)
    return a


def model(m, N, n_pub, A, B, C, zs):
    n, Q, _ = ref.shape(m, N, n_pub)
    planes = [bytearray(), bytearray(), bytearray()]
    cs_all, bad_all = [], []
    for z in zs:
        aL, aR, aO, cs, bad = ref.assign(m, N, n_pub, A, B, C, z)
        for p, v in zip(planes, (aL, aR, aO)):
            p += b"".join(x.to_bytes(32, "little") for x in v)
        cs_all.append(cs)
        bad_all.append(bad)
    return [bytes(p) for p in planes], cs_all, bad_all


def handle(sonic, m, N, n_pub, A, B, C):
    return sonic.R1CS.from_rows(N, n_pub, [dict(r) for r in A], [dict(r) for r in B], [dict(r) for r in C])


def raw_assign(torch, r, K, z, kind, on_device, z_stride, out_pad=0, outs=None, z_ptr=None, stream=None):
    """sonic_r1cs_assign through the C ABI -> (status, [aL, aR, aO] as torch uint8 [K, n + out_pad, 32], cs, bad)"""
    from sonic_amd import _lib
    dev = r.device
    planes = outs if outs is not None else [torch.full((K, r.n + out_pad, 32), FILL, dtype=torch.uint8, device=f"cuda:{dev}") for _ in range(3)]
    torch.cuda.synchronize(dev)
    cs = np.full((K, r.Q, 32), FILL, np.uint8)
    bad = np.full((K, 2), -7, np.int64)
    ptrs = [p if isinstance(p, int) else p.data_ptr() for p in planes]
    if z_ptr is None:
        z_ptr = z.data_ptr() if on_device else z.ctypes.data
    rc = _lib.lib().sonic_r1cs_assign(r._h, K, z_ptr, 1 if kind == "i64" else 0, int(on_device), z_stride, stream, ptrs[0], ptrs[1], ptrs[2],
                                      32 * (r.n + out_pad) if out_pad else 0, cs.ctypes.data, bad.ctypes.data)
    return rc, planes, cs, bad


def check_against_model(torch, r, want, K, rc, planes, cs, bad, out_pad):
    from sonic_amd import _lib
    assert rc == 0, _lib.last_error()
    want_planes, want_cs, want_bad = want
    for name, p, w in zip(("aL", "aR", "aO"), planes, want_planes):
        host = p.cpu().numpy()
        assert host[:, :r.n].tobytes() == w, name
        assert (host[:, r.n:] == FILL).all(), name + ": bytes between the witnesses' planes were written"
    assert cs.tobytes() == b"".join(v.to_bytes(32, "little") for c in want_cs for v in c)
    assert [tuple(int(x) for x in b) for b in bad] == want_bad


# (m, N as a function of T, n_pub: 0, 1 or "all", K, kind, z on the device, strided z and outputs)
CASES = [
    (1, lambda T: 1, 0, 1, "fr", False, False),
    (1, lambda T: 2 * T + 2, 0, 1, "fr", False, False),
    (2, lambda T: 2 * T + 3, 1, 3, "i64", True, True),
    (63, lambda T: 2 * T + 2, "all", 17, "fr", True, True),
    (64, lambda T: 2 * T + 3, 0, 3, "i64", False, True),
    (65, lambda T: 2 * T + 2, 1, 1, "fr", True, False),
    (300, lambda T: 2 * T + 3, "all", 17, "i64", True, False),
    (300, lambda T: 2 * T + 2, 1, 3, "fr", False, False),
    (7, lambda T: 6, "all", 3, "i64", False, False),
]


@pytest.mark.parametrize("case", range(len(CASES)))
def test_assign_equals_the_model_in_every_byte(sonic, torch, T, case):
    m, Nf, pub, K, kind, on_device, strided = CASES[case]
    N = Nf(T)
    n_pub = N - 1 if pub == "all" else min(pub, N - 1)
    rng = random.Random(1000 + case)
    first = witnesses(rng, N, 1, kind)[0]
    A, B, C, _ = ref.random_r1cs(rng, m, N, n_pub, row_lengths(m, N, T), z=[v % R for v in first], coeffs=coeff(rng))
    zs = witnesses(rng, N, K, kind, first)
    want = model(m, N, n_pub, A, B, C, zs)
    assert want[2][0] == (0, -1)                      # the system was made for witness 0
    if m >= 6 and N > 2 * T:
        for M in (A, B, C):
            assert {len(r) for r in M} >= {0, 1, T - 1, T, T + 1, 2 * T + 1}
    r = handle(sonic, m, N, n_pub, A, B, C)
    assert (r.n, r.Q, r.g, r.nnz) == (*ref.shape(m, N, n_pub)[:2], N // 2, ref.nnz_formula(m, n_pub, A, B, C))
    pad = 3 if strided else 0
    za = z_array(zs, N, kind, pad)
    elem = 8 if kind == "i64" else 32
    z = torch.from_numpy(za).to(f"cuda:{r.device}") if on_device else za
    rc, planes, cs, bad = raw_assign(torch, r, K, z, kind, on_device, elem * (N + pad) if strided else 0, out_pad=2 if strided else 0)
    check_against_model(torch, r, want, K, rc, planes, cs, bad, 2 if strided else 0)
    # the compiled circuit is the model's, and its constants are the ones assign returned
    rows, cs_fixed = ref.compile_r1cs(m, N, n_pub, A, B, C)
    rp, col, val = ref.csr_of(rows)
    sp = r.circuit()
    assert sp.row_ptr.tolist() == rp and sp.col.tolist() == col and sp.val.tobytes() == b"".join(v.to_bytes(32, "little") for v in val)
    assert sp.cs.tobytes() == b"".join(v.to_bytes(32, "little") for v in cs_fixed)
    r.close()


@pytest.mark.parametrize("kind,on_device", [("fr", True), ("i64", False)])
def test_python_assign_and_the_seam_between_staging_chunks(sonic, torch, T, monkeypatch, kind, on_device):
    m, N, n_pub, K = 65, 2 * T + 3, 2, 5
    rng = random.Random(52)
    first = witnesses(rng, N, 1, kind)[0]
    A, B, C, _ = ref.random_r1cs(rng, m, N, n_pub, row_lengths(m, N, T), z=[v % R for v in first], coeffs=coeff(rng))
    zs = witnesses(rng, N, K, kind, first)
    want = model(m, N, n_pub, A, B, C, zs)
    r = handle(sonic, m, N, n_pub, A, B, C)
    za = z_array(zs, N, kind)
    z = torch.from_numpy(za).to(f"cuda:{r.device}") if on_device else za
    for stage in (None, "2", "1"):                    # one chunk; three chunks of 2, 2, 1; five of one
        if stage is None:
            monkeypatch.delenv("SONIC_R1CS_STAGE", raising=False)
        else:
            monkeypatch.setenv("SONIC_R1CS_STAGE", stage)
        rc, planes, cs, bad = raw_assign(torch, r, K, z, kind, on_device, 0)
        check_against_model(torch, r, want, K, rc, planes, cs, bad, 0)
    # the Python call: the same bytes, as a WitnessBatch of tensors on the handle's GPU; lists of ints are a third form of z
    for zz in (z, [[v % R for v in w] for w in zs]):
        wb, cs, bad = r.assign(zz)
        assert len(wb) == K and wb.aL.device.type == "cuda" and tuple(wb.aL.shape) == (K, r.n, 32) and wb.aL.dtype == torch.uint8
        assert [t.cpu().numpy().tobytes() for t in (wb.aL, wb.aR, wb.aO)] == want[0]
        assert cs == want[1] and bad == want[2]
    with pytest.raises(ValueError):
        r.assign(za[:, :N - 1])
    with pytest.raises(ValueError):
        r.assign(za.astype(np.int32))
    r.close()


def chain_system(rng, n_in, m):
    """a system every choice of inputs satisfies: z = (1, n_in inputs, m products); row i: <a, z> <b, z> = z[1 + n_in + i] over earlier columns"""
    N = 1 + n_in + m
    A, B, C = [], [], []
    for i in range(m):
        top = 1 + n_in + i
        A.append(ref.random_row(rng, top, rng.randrange(1, 4)))
        B.append(ref.random_row(rng, top, rng.randrange(1, 4)))
        C.append([(top, 1)])

    def solve(inputs):
        z = [1] + [v % R for v in inputs]
        for i in range(m):
            z.append(ref.dot(A[i], z) * ref.dot(B[i], z) % R)
        return z
    return N, A, B, C, solve


def test_an_unsatisfied_witness_is_named_and_the_others_are_not(sonic, torch):
    rng = random.Random(3)
    N, A, B, C, solve = chain_system(rng, 10, 70)
    zs = [solve([rng.randrange(R) for _ in range(10)]) for _ in range(3)]
    j = 1 + 10 + 20                                   # the product of row 20: changing it breaks row 20 and whatever reads it later
    zs[1][j] = (zs[1][j] + 1) % R
    want = model(70, N, 2, A, B, C, zs)
    assert want[2][0] == (0, -1) and want[2][2] == (0, -1) and want[2][1][0] >= 1 and want[2][1][1] == 20
    r = handle(sonic, 70, N, 2, A, B, C)
    rc, planes, cs, bad = raw_assign(torch, r, 3, z_array(zs, N, "fr"), "fr", False, 0)
    check_against_model(torch, r, want, 3, rc, planes, cs, bad, 0)
    r.close()


def test_refusals_leave_the_outputs_untouched(sonic, torch, monkeypatch):
    from sonic_amd import _lib
    rng = random.Random(4)
    N, A, B, C, solve = chain_system(rng, 6, 9)
    r = handle(sonic, 9, N, 2, A, B, C)
    dev = f"cuda:{r.device}"
    K = 3
    good = [solve([rng.randrange(R) for _ in range(6)]) for _ in range(K)]

    def untouched(rc, status, word, planes, cs, bad):
        assert rc == status, (rc, _lib.last_error())
        assert word in _lib.last_error(), _lib.last_error()
        for p in planes:
            if not isinstance(p, int) and p.device.type == "cuda":
                assert bool((p == FILL).all())
        assert (cs == FILL).all() and (bad == -7).all()

    for stage in (None, "1"):                         # in one chunk, and with the offending witness in a later chunk than the first
        if stage:
            monkeypatch.setenv("SONIC_R1CS_STAGE", stage)
        zs = [list(z) for z in good]
        zs[1][0] = 2
        rc, planes, cs, bad = raw_assign(torch, r, K, z_array(zs, N, "fr"), "fr", False, 0)
        untouched(rc, INVALID_ARG, "witness 1", planes, cs, bad)
        zs[2][0] = 3                                  # the first such witness is the one named
        rc, planes, cs, bad = raw_assign(torch, r, K, torch.from_numpy(z_array(zs, N, "fr")).to(dev), "fr", True, 0)
        untouched(rc, INVALID_ARG, "witness 1", planes, cs, bad)
        za = z_array(good, N, "fr")
        za[2, N - 1] = np.frombuffer(R.to_bytes(32, "little"), np.uint8)          # r itself: the smallest non-canonical value
        rc, planes, cs, bad = raw_assign(torch, r, K, za, "fr", False, 0)
        untouched(rc, BAD_ENCODING, "non-canonical", planes, cs, bad)
    monkeypatch.delenv("SONIC_R1CS_STAGE", raising=False)
    za = z_array(good, N, "fr")
    zd = torch.from_numpy(za).to(dev)
    # misaligned device pointers: an output plane, then z
    big = [torch.full((K * r.n * 32 + 64,), FILL, dtype=torch.uint8, device=dev) for _ in range(3)]
    rc, planes, cs, bad = raw_assign(torch, r, K, zd, "fr", True, 0, outs=[big[0].data_ptr(), big[1].data_ptr() + 16, big[2].data_ptr()])
    untouched(rc, INVALID_ARG, "d_aR is not 32-byte aligned", big, cs, bad)
    zbig = torch.zeros(K * N * 32 + 64, dtype=torch.uint8, device=dev)
    rc, planes, cs, bad = raw_assign(torch, r, K, zd, "fr", True, 0, z_ptr=zbig.data_ptr() + 8)
    untouched(rc, INVALID_ARG, "z is not 32-byte aligned", planes, cs, bad)
    # an output pointer that is host memory; a z that is host memory given as a device pointer
    hostbuf = np.full(K * r.n * 32 + 32, FILL, np.uint8)
    base = hostbuf.ctypes.data + (-hostbuf.ctypes.data) % 32
    rc, planes, cs, bad = raw_assign(torch, r, K, zd, "fr", True, 0, outs=[big[0].data_ptr(), big[1].data_ptr(), base])
    untouched(rc, INVALID_ARG, "d_aO is a host pointer", big, cs, bad)
    assert (hostbuf == FILL).all()
    zhost = np.zeros(K * N * 32 + 32, np.uint8)
    rc, planes, cs, bad = raw_assign(torch, r, K, zd, "fr", True, 0, z_ptr=zhost.ctypes.data + (-zhost.ctypes.data) % 32)
    untouched(rc, INVALID_ARG, "z is a host pointer", planes, cs, bad)
    # strides that break the rules, no witness, an unknown kind
    L = _lib.lib()
    for z_stride, out_stride, word in ((32 * N - 32, 0, "z_stride"), (0, 32 * r.n - 32, "out_stride"), (0, 32 * r.n + 8, "out_stride")):
        assert L.sonic_r1cs_assign(r._h, K, zd.data_ptr(), 0, 1, z_stride, None, big[0].data_ptr(), big[1].data_ptr(), big[2].data_ptr(), out_stride, None, None) == INVALID_ARG
        assert word in _lib.last_error()
    assert L.sonic_r1cs_assign(r._h, 0, zd.data_ptr(), 0, 1, 0, None, big[0].data_ptr(), big[1].data_ptr(), big[2].data_ptr(), 0, None, None) == INVALID_ARG
    assert L.sonic_r1cs_assign(r._h, K, zd.data_ptr(), 2, 1, 0, None, big[0].data_ptr(), big[1].data_ptr(), big[2].data_ptr(), 0, None, None) == INVALID_ARG
    torch.cuda.synchronize()
    assert all(bool((b == FILL).all()) for b in big)
    # and the handle still works, with out_cs and out_bad left out
    assert L.sonic_r1cs_assign(r._h, K, zd.data_ptr(), 0, 1, 0, None, big[0].data_ptr(), big[1].data_ptr(), big[2].data_ptr(), 0, None, None) == 0
    want = model(9, N, 2, A, B, C, good)
    assert [b[:K * r.n * 32].cpu().numpy().tobytes() for b in big] == want[0]
    # a system that does not validate makes no handle
    with pytest.raises(sonic.SonicError) as e:
        sonic.R1CS(1, 3, 0, ([0, 2], [1, 1], [1, 1]), ([0, 0], [], []), ([0, 0], [], []))
    assert e.value.code == INVALID_ARG and "A: row 0" in str(e.value)
    with pytest.raises(sonic.SonicError) as e:
        sonic.R1CS(1, 3, 0, ([0, 0], [], []), ([0, 1], [2], np.frombuffer(R.to_bytes(32, "little"), np.uint8).reshape(1, 32)), ([0, 0], [], []))
    assert e.value.code == BAD_ENCODING and "B: row 0" in str(e.value)
    r.close()


def test_end_to_end_core_proofs_of_a_compiled_circuit(sonic, torch):
    rng = random.Random(5)
    n_in, m, n_pub, K = 20, 40, 2, 3
    N, A, B, C, solve = chain_system(rng, n_in, m)
    assert N == 61
    r = handle(sonic, m, N, n_pub, A, B, C)
    assert (r.n, r.Q) == (70, 122)
    zs = [solve([rng.randrange(R) for _ in range(n_in)]) for _ in range(K)]
    srs = sonic.SRS.new(512, rng.randrange(2, R), rng.randrange(2, R))
    circuit = r.circuit(public=zs[0][1:3])
    wb, cs, bad = r.assign(torch.from_numpy(z_array(zs, N, "fr")).to(f"cuda:{r.device}"))
    assert bad == [(0, -1)] * K and [c[3 * m:] for c in cs] == [z[1:3] for z in zs]
    p = sonic.Prover(srs, circuit, prepare=False)
    trs = [[rng.randrange(1, R) for _ in range(6)] for _ in range(K)]
    singles = []
    for k in range(K):
        p.set_witness(wb.aL[k], wb.aR[k], wb.aO[k])
        p.set_constants(cs[k])
        singles.append(p.prove_core_bytes(trs[k]))
    y, zpt = trs[0][4], trs[0][5]
    assert sonic.verify_core(srs, circuit, singles[0], y, zpt)
    moved = [zs[0][1], (zs[0][2] + 1) % R]
    assert sonic.verify_core(srs, r.circuit(public=moved), singles[0], y, zpt) is False
    assert sonic.verify_core(srs, r.circuit(public=zs[1][1:3]), singles[1], trs[1][4], trs[1][5])
    got_cs, got_gates = p.eval_constraints(wb)
    assert got_cs == cs and got_gates == [(0, -1)] * K
    assert sonic.prove_core_batch([p], trs, wb, constants=cs) == singles
    p.close()
    srs.close()
    r.close()


def test_the_cubic_example_as_a_full_proof_against_the_oracle(sonic, orc, torch):
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "examples"))
    try:
        import r1cs_cubic
    finally:
        sys.path.pop(0)
    N, n_pub, A, B, C, z = r1cs_cubic.cubic(3)
    assert z[1] == 35
    r = sonic.R1CS.from_rows(N, n_pub, A, B, C)
    n, Q = r.n, r.Q
    assert (n, Q) == (5, 10)
    rng = random.Random(6)
    d, x, alpha = 64, rng.randrange(2, R), rng.randrange(2, R)
    srs = sonic.SRS.new(d, x, alpha)
    o = orc.SRS(d, x, alpha, threads=NCPU)
    circuit = r.circuit(public=[35])
    wb, cs, bad = r.assign(np.array([z], dtype=np.int64))
    assert bad == [(0, -1)] and cs[0] == [0, 0, 5, 0, 0, 1, 0, 0, 0, 35]      # A_20 = 5, B_20 = 1, the public input
    aL, aR, aO, want_cs, _ = ref.assign(3, N, n_pub, [sorted(a.items()) for a in A], [sorted(b.items()) for b in B], [sorted(c.items()) for c in C], z)
    assert cs[0] == want_cs
    p = sonic.Prover(srs, circuit, prepare=False)
    p.set_witness(wb.aL[0], wb.aR[0], wb.aO[0])
    p.set_constants(cs[0])
    tr = [rng.randrange(1, R) for _ in range(8 + 2 * Q)]
    raw = p.prove_bytes(tr)
    dense = circuit.to_dense()
    w = dense.weights
    wL, wR, wO = (np.ascontiguousarray(v).reshape(-1, 32) for v in (w.wL, w.wR, w.wO))
    orc.set_mode(1, NCPU)
    want = orc.prove(o, n, Q, wL, wR, wO, fr_bytes(cs[0]), fr_bytes(aL), fr_bytes(aR), fr_bytes(aO), fr_bytes(tr), False)
    assert raw == want
    assert sonic.verify(srs, circuit, sonic.Proof.from_bytes(raw, Q), tr[4], tr[5], list(zip(tr[6:6 + Q], tr[6 + Q:6 + 2 * Q])))
    p.close()
    srs.close()
    r.close()
