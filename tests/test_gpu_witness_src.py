"""Witness sources on the GPU (include/sonic_hip.h, "Witness sources"; sonic_amd/csrc/witness_src.hip): sonic_prover_set_witness,
sonic_prover_eval_constraints_src, sonic_prove_batch_src, sonic_prove_batch_fs_src and their Python forms.

Every result is exact, so every comparison is on bytes.  The yardstick is always the existing path -- sonic_prover_set_assignment,
sonic_prove_batch_statements, sonic_prove_batch_fs over three host buffers of canonical bytes -- on an assignment written out with Python
integers mod r; never the code under test.  Circuits are sonic_amd.workload's (big_circuit: the reference's rndCircuit,
test/Test/Reference.hs:125-169), d = 8 n rounded up to a power of two (d_for), Q = 2."""
import ctypes as C
import hashlib
import os
import random
import subprocess
import threading

import numpy as np
import pytest

from util import R, big_circuit, fr_bytes

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
Q = 2
I64_MAX, I64_MIN = (1 << 63) - 1, -(1 << 63)
R_BYTES = np.frombuffer(R.to_bytes(32, "little"), np.uint8)


def d_for(n):
    """8 n rounded up to a power of two -- and at least 4 n + 8, the lowest exponent of t(X, y) (Protocol.hs:81), which 8 n is not at
    n = 1: the existing path itself refuses n = 1 over d = 8 with SONIC_ERR_SRS_INDEX, so that one case runs over d = 16"""
    return 1 << (max(8 * n, 4 * n + 8) - 1).bit_length()


_srs, _circuits = {}, {}


@pytest.fixture(scope="module")
def srs_of(sonic):
    def get(n):
        d = d_for(n)
        if d not in _srs:
            pyr = random.Random(d)
            _srs[d] = sonic.SRS.new(d, pyr.randrange(2, R), pyr.randrange(2, R))
        return _srs[d]
    yield get
    for s in _srs.values():
        s.close()
    _srs.clear()


def circuit(n):
    """big_circuit(n), made once: weights, a satisfied assignment (bytes and ints), its constants"""
    if n not in _circuits:
        _circuits[n] = big_circuit(1000 + n, n, Q)
    return _circuits[n]


def arith(sonic, c, cs=None):
    return sonic.ArithCircuit(sonic.GateWeights(c["wL"], c["wR"], c["wO"]), c["cs"] if cs is None else fr_bytes(cs))


def cs_of(c, la, lb, lo):
    """the constants of an assignment (ints mod r) under big_circuit's weights: one all-ones row per matrix"""
    cs = [0] * Q
    for k, row in enumerate(c["rows"]):
        cs[row] = (cs[row] + sum((la, lb, lo)[k])) % R
    return cs


def transcript(seed):
    pyr = random.Random(seed)
    return [pyr.randrange(1, R) for _ in range(8 + 2 * Q)]


def dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def zero_assignment(sonic, n):
    z = np.zeros((n, 32), np.uint8)
    return sonic.Assignment(z, z, z)


def i64_values(pyr, n):
    """n values from {0, 1, -1, 2^63 - 1, -2^63, small random}, every special value present when n allows"""
    special = [0, 1, -1, I64_MAX, I64_MIN]
    vals = [pyr.choice(special) if pyr.random() < 0.5 else pyr.randrange(-1000, 1000) for _ in range(n)]
    for k, v in enumerate(special):                                  # (index 0 is the caller's)
        if 1 + k < n:
            vals[1 + k] = v
    return vals


def src_struct(_lib, aL, aR, aO, kind, on_device, stride=0, stream=None):
    return _lib.WitnessSrc(aL, aR, aO, kind, on_device, stride, stream)


# ---- 1. equality with the existing path ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 31, 33, 257, 4097])
def test_fr32_sources_equal_set_assignment(sonic, srs_of, n):
    c = circuit(n)
    tr = transcript(n)
    p = sonic.Prover(srs_of(n), arith(sonic, c), prepare=False)
    try:
        p.set_assignment(sonic.Assignment(c["aL"], c["aR"], c["aO"]))
        want = (p.prove_bytes(tr), p.witness_digest(), p.eval_constraints())
        assert want[2] == ([c["cs_ints"]], [(0, -1)])
        sources = {"host": (c["aL"], c["aR"], c["aO"]), "device": tuple(dev(c[k]) for k in ("aL", "aR", "aO"))}
        for name, (aL, aR, aO) in sources.items():
            p.set_assignment(zero_assignment(sonic, n))              # so that a set_witness that did nothing would show
            assert p.witness_digest() != want[1]
            p.set_witness(aL, aR, aO)
            got = (p.prove_bytes(tr), p.witness_digest(), p.eval_constraints())
            print(n, name, "proof", got[0][:8].hex(), "digest", got[1][:8].hex())
            assert got[1] == want[1], name
            assert got[2] == want[2], name
            assert got[0] == want[0], name
    finally:
        p.close()


# ---- 2. int64 -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [33, 257])
def test_i64_sources_with_aO_derived(sonic, srs_of, n):
    c = circuit(n)
    pyr = random.Random(64 + n)
    vL, vR = i64_values(pyr, n), i64_values(pyr, n)
    vL[0], vR[0] = I64_MIN, I64_MIN                                  # the largest product: 2^126
    la, lb = [v % R for v in vL], [v % R for v in vR]
    lo = [a * b % R for a, b in zip(la, lb)]
    assert {0, 1, R - 1, I64_MAX, R - (1 << 63)} <= set(la) and {0, 1, R - 1, I64_MAX, R - (1 << 63)} <= set(lb)
    cs = cs_of(c, la, lb, lo)
    tr = transcript(2 * n)
    p = sonic.Prover(srs_of(n), arith(sonic, c, cs), prepare=False)
    try:
        p.set_assignment(sonic.Assignment(la, lb, lo))
        want = (p.prove_bytes(tr), p.witness_digest())
        hL, hR = np.array(vL, np.int64), np.array(vR, np.int64)
        for name, (aL, aR) in {"host": (hL, hR), "device": (dev(hL), dev(hR))}.items():
            p.set_assignment(zero_assignment(sonic, n))
            p.set_witness(aL, aR)
            assert p.eval_constraints() == ([cs], [(0, -1)]), name
            assert (p.prove_bytes(tr), p.witness_digest()) == want, name
            assert p.eval_constraints(sonic.WitnessBatch(aL.reshape(1, n), aR.reshape(1, n))) == ([cs], [(0, -1)]), name
    finally:
        p.close()


def test_i64_with_aO_given_satisfied_and_off_by_one(sonic, srs_of):
    from sonic_amd import _lib
    n = 257
    c = circuit(n)
    pyr = random.Random(6464)
    vL = [pyr.randrange(-(1 << 31), 1 << 31) for _ in range(n)]
    vR = [pyr.randrange(-(1 << 31), 1 << 31) for _ in range(n)]
    vO = [a * b for a, b in zip(vL, vR)]                             # fits: |aO| <= 2^62
    assert all(I64_MIN <= v <= I64_MAX for v in vO) and min(vO) < 0 < max(vO)
    la, lb, lo = ([v % R for v in vs] for vs in (vL, vR, vO))
    cs = cs_of(c, la, lb, lo)
    tr = transcript(77)
    bad_at = 200
    vBad = list(vO)
    vBad[bad_at] += 1
    p = sonic.Prover(srs_of(n), arith(sonic, c, cs), prepare=False)
    try:
        p.set_assignment(sonic.Assignment(la, lb, lo))
        want = p.prove_bytes(tr)
        # what an unsatisfied set_assignment does: the yardstick of the failure
        lbad = [v % R for v in vBad]
        p.set_assignment(sonic.Assignment(la, lb, lbad))
        with pytest.raises(_lib.SonicError) as e:
            p.prove_bytes(tr)
        assert e.value.code == 2
        for name, put in {"host": lambda a: np.array(a, np.int64), "device": lambda a: dev(np.array(a, np.int64))}.items():
            aL, aR, aO, aBad = put(vL), put(vR), put(vO), put(vBad)
            p.set_witness(aL, aR, aO)
            assert p.prove_bytes(tr) == want, name
            batch = sonic.WitnessBatch(aL.reshape(1, n), aR.reshape(1, n), aBad.reshape(1, n))
            got_cs, gates = p.eval_constraints(batch)
            print(name, "gates of the off-by-one aO:", gates)
            assert gates == [(1, bad_at)], name
            assert got_cs == [cs_of(c, la, lb, lbad)], name
            p.set_witness(aL, aR, aBad)
            assert p.eval_constraints()[1] == [(1, bad_at)], name
            with pytest.raises(_lib.SonicError) as e:
                p.prove_bytes(tr)
            assert e.value.code == 2, name
    finally:
        p.close()


# ---- 3. aO derived for 32-byte elements -------------------------------------------------------------------------------------------------
def test_fr32_device_source_with_aO_derived(sonic, srs_of):
    n = 257
    c = circuit(n)                                                    # aL, aR uniform over Fr, aO = aL aR mod r in Python integers
    assert max(c["ints"][0]) >> 250 and c["ints"][2] == [a * b % R for a, b in zip(*c["ints"][:2])]
    tr = transcript(3)
    p = sonic.Prover(srs_of(n), arith(sonic, c), prepare=False)
    try:
        p.set_assignment(sonic.Assignment(c["aL"], c["aR"], c["aO"]))
        want = (p.prove_bytes(tr), p.witness_digest())
        p.set_assignment(zero_assignment(sonic, n))
        p.set_witness(dev(c["aL"]), dev(c["aR"]))
        assert (p.prove_bytes(tr), p.witness_digest()) == want
        assert p.eval_constraints(sonic.WitnessBatch(dev(c["aL"]).reshape(1, n, 32), dev(c["aR"]).reshape(1, n, 32))) == ([c["cs_ints"]], [(0, -1)])
    finally:
        p.close()


# ---- 4. refusals -----------------------------------------------------------------------------------------------------------------------
def test_refusals(sonic, srs_of):
    """argument checks are made before any launch; none of these may fault"""
    import torch
    from sonic_amd import _lib
    L = _lib.lib()
    n = 257
    c = circuit(n)
    tr = transcript(4)
    p = sonic.Prover(srs_of(n), arith(sonic, c), prepare=False)

    def refused(call, code, word):
        rc = call()
        msg = _lib.last_error()
        print(code, rc, msg)
        assert rc == code and word in msg, (rc, msg)

    try:
        # a non-canonical element (r itself) at index 0 and at index n - 1, in each vector in turn
        for at, k in ((0, "aL"), (n - 1, "aO"), (n - 1, "aR")):
            p.set_assignment(sonic.Assignment(c["aL"], c["aR"], c["aO"]))
            arrs = {m: c[m].copy() for m in ("aL", "aR", "aO")}
            arrs[k][at] = R_BYTES
            with pytest.raises(_lib.SonicError) as e:
                p.set_witness(dev(arrs["aL"]), dev(arrs["aR"]), dev(arrs["aO"]))
            assert e.value.code == 3, (at, k)
            with pytest.raises(_lib.SonicError) as e:
                p.prove_bytes(tr)
            assert e.value.code == 7 and "no assignment set" in e.value.message, (at, k)
        p.set_assignment(sonic.Assignment(c["aL"], c["aR"], c["aO"]))
        want = p.prove_bytes(tr)
        dL, dR, dO = (dev(c[k]) for k in ("aL", "aR", "aO"))
        FR32, I64 = _lib.WIT_FR32, _lib.WIT_I64
        out = np.zeros((2, Q, 32), np.uint8)
        # a device pointer misaligned by 8
        raw = torch.zeros(32 * n + 64, dtype=torch.uint8, device="cuda")
        off = (-raw.data_ptr()) % 32 + 8
        mis = raw[off:off + 32 * n].view(n, 32)
        assert mis.data_ptr() % 32 == 8
        with pytest.raises(_lib.SonicError) as e:
            p.set_witness(mis, dR, dO)
        assert e.value.code == 7 and "aligned" in e.value.message
        # a stride that is not a multiple of the alignment (two assignments)
        two = torch.zeros(2 * 32 * n + 64, dtype=torch.uint8, device="cuda")
        base = two.data_ptr() + (-two.data_ptr()) % 32
        s = src_struct(_lib, base, base, base, FR32, 1, 32 * n + 8)
        refused(lambda: L.sonic_prover_eval_constraints_src(p._h, 2, C.byref(s), out.ctypes.data, None), 7, "multiple of 32")
        s = src_struct(_lib, base, base, None, I64, 1, 8 * n + 4)
        refused(lambda: L.sonic_prover_eval_constraints_src(p._h, 2, C.byref(s), out.ctypes.data, None), 7, "multiple of 8")
        # a host pointer passed as device memory
        # (32-byte aligned, so that it is the memory's kind that is refused and not the alignment, which numpy does not promise)
        room = np.zeros(32 * n + 32, np.uint8)
        host = room[(-room.ctypes.data) % 32:][:32 * n]
        host[:] = c["aL"].reshape(-1)
        assert host.ctypes.data % 32 == 0
        s = src_struct(_lib, host.ctypes.data, host.ctypes.data, host.ctypes.data, FR32, 1)
        refused(lambda: L.sonic_prover_set_witness(p._h, C.byref(s)), 7, "host pointer")
        # an unknown kind
        s = src_struct(_lib, dL.data_ptr(), dR.data_ptr(), dO.data_ptr(), 2, 1)
        refused(lambda: L.sonic_prover_set_witness(p._h, C.byref(s)), 7, "kind")
        refused(lambda: L.sonic_prover_set_witness(p._h, None), 7, "NULL")
        # B n beyond 2^26
        s = src_struct(_lib, dL.data_ptr(), dR.data_ptr(), dO.data_ptr(), FR32, 1)
        refused(lambda: L.sonic_prover_eval_constraints_src(p._h, (1 << 26) // n + 1, C.byref(s), out.ctypes.data, None), 7, "2^26")
        # none of them touched the resident assignment
        assert p.prove_bytes(tr) == want
        # a proof in flight
        p.submit(tr)
        try:
            refused(lambda: L.sonic_prover_set_witness(p._h, C.byref(s)), 7, "submitted proof")
            refused(lambda: L.sonic_prover_eval_constraints_src(p._h, 1, C.byref(s), out.ctypes.data, None), 7, "submitted proof")
        finally:
            assert p.collect() == want
        arr = (C.c_void_p * 1)(p._h)
        st = (C.c_int * 2)()
        refused(lambda: L.sonic_prove_batch_src(arr, 1, 2, None, None, fr_bytes(tr + tr).ctypes.data, np.zeros(2 * len(want), np.uint8).ctypes.data, st), 7, "NULL")
    finally:
        p.close()


# ---- 5. batches ------------------------------------------------------------------------------------------------------------------------
def test_batches_from_a_strided_int64_device_tensor(sonic, srs_of):
    import torch
    from sonic_amd import _lib
    L = _lib.lib()
    n, K = 257, 5
    c = circuit(n)
    pyr = random.Random(55)
    vL = [i64_values(pyr, n) for _ in range(K)]
    vR = [i64_values(pyr, n) for _ in range(K)]
    ints = [([a % R for a in vL[k]], [b % R for b in vR[k]]) for k in range(K)]
    ints = [(la, lb, [a * b % R for a, b in zip(la, lb)]) for la, lb in ints]
    want_cs = [cs_of(c, *t) for t in ints]
    assert len({tuple(x) for x in want_cs}) == K
    wide = n + 7                                                     # the leading stride exceeds n
    tL, tR = (torch.full((K, wide), 12345, dtype=torch.int64, device="cuda") for _ in range(2))
    tL[:, :n] = dev(np.array(vL, np.int64))
    tR[:, :n] = dev(np.array(vR, np.int64))
    batch = sonic.WitnessBatch(tL[:, :n], tR[:, :n])
    assert tL[:, :n].stride(0) == wide and len(batch) == K
    trs = [transcript(500 + k) for k in range(K)]
    provers = [sonic.Prover(srs_of(n), arith(sonic, c)) for _ in range(2)]
    try:
        css, gates = provers[0].eval_constraints(batch)              # sonic_prover_eval_constraints_src
        assert css == want_cs and gates == [(0, -1)] * K
        A = [sonic.Assignment(*t) for t in ints]
        want = sonic.prove_batch(provers, trs, A, constants=css)     # sonic_prove_batch_statements on the canonical host arrays
        got = sonic.prove_batch(provers, trs, batch, constants=css)
        print("batch proofs", [g[:6].hex() for g in got])
        assert got == want
        # each handle holds the assignment of the last proof it ran: proofs 4 and 3
        assert provers[0].prove_bytes(trs[4]) == want[4] and provers[1].prove_bytes(trs[3]) == want[3]
        # Fiat-Shamir: proofs and transcripts both
        mid = sonic.fs_circuit_midstate(arith(sonic, c))
        digests = [sonic.fs_circuit_digest_resume(mid, cs) for cs in css]
        seeds = [hashlib.sha256(b"seed%d" % k).digest() for k in range(K)]
        want_fs = sonic.prove_batch_fs(provers, digests, seeds, A, constants=css)
        got_fs = sonic.prove_batch_fs(provers, digests, seeds, batch, constants=css)
        assert [g[0] for g in got_fs] == [w[0] for w in want_fs]
        assert [g[1] for g in got_fs] == [w[1] for w in want_fs]
        # the same batch from host memory, strided as well
        host = sonic.WitnessBatch(tL.cpu().numpy()[:, :n], tR.cpu().numpy()[:, :n])
        assert sonic.prove_batch(provers, trs, host, constants=css) == want
        # one proof of a batch of 32-byte elements carries a non-canonical element: its own status, the others' bytes
        enc = [np.ascontiguousarray(np.stack([fr_bytes(t[m]) for t in ints])) for m in range(3)]
        enc[1][2, n - 1] = R_BYTES
        d3 = [dev(a) for a in enc]
        s = src_struct(_lib, d3[0].data_ptr(), d3[1].data_ptr(), d3[2].data_ptr(), _lib.WIT_FR32, 1, 0, torch.cuda.current_stream().cuda_stream or None)
        torch.cuda.current_stream().synchronize()
        tr = np.ascontiguousarray(np.stack([fr_bytes(t) for t in trs]))
        cs = np.ascontiguousarray(np.stack([fr_bytes(x) for x in css]))
        psz = L.sonic_proof_size(Q)
        out = np.zeros((K, psz), np.uint8)
        status = (C.c_int * K)()
        arr = (C.c_void_p * 2)(*[p._h for p in provers])
        rc = L.sonic_prove_batch_src(arr, 2, K, C.byref(s), cs.ctypes.data, tr.ctypes.data, out.ctypes.data, status)
        assert rc == 3 and list(status) == [0, 0, 3, 0, 0], (rc, list(status), _lib.last_error())
        assert [out[k].tobytes() for k in (0, 1, 3, 4)] == [want[k] for k in (0, 1, 3, 4)]
        tro = np.zeros((K, 8 + 2 * Q, 32), np.uint8)
        rc = L.sonic_prove_batch_fs_src(arr, 2, K, C.byref(s), cs.ctypes.data, b"".join(digests), b"".join(seeds), out.ctypes.data, tro.ctypes.data, status)
        assert rc == 3 and list(status) == [0, 0, 3, 0, 0], (rc, list(status), _lib.last_error())
        assert [out[k].tobytes() for k in (0, 1, 3, 4)] == [want_fs[k][0] for k in (0, 1, 3, 4)]
        # handle 0 ran proof 2 last but one, then proof 4: it holds a good assignment again; a handle whose LAST proof was refused has none
        rc = L.sonic_prove_batch_src(arr, 2, 3, C.byref(s), cs.ctypes.data, tr.ctypes.data, out.ctypes.data, status)
        assert rc == 3 and list(status)[:3] == [0, 0, 3]
        with pytest.raises(_lib.SonicError) as e:
            provers[0].prove_bytes(trs[0])
        assert e.value.code == 7 and "no assignment set" in e.value.message
    finally:
        for p in provers:
            p.close()


# ---- 6. ordering -----------------------------------------------------------------------------------------------------------------------
def test_the_handle_waits_for_the_stream_that_fills_the_source(sonic, srs_of):
    """The source is filled on a side stream behind a few milliseconds of sleep, and set_witness is called with that stream from a thread
    whose current stream is another one: the proof must be the proof of the FINAL contents.  A wrong implementation (no wait) can pass
    this by luck -- the sleep may be over before the handle reads; a right one never fails it."""
    import torch
    n = 4097
    c = circuit(n)
    tr = transcript(6)
    p = sonic.Prover(srs_of(n), arith(sonic, c), prepare=False)
    try:
        p.set_assignment(sonic.Assignment(c["aL"], c["aR"], c["aO"]))
        want = p.prove_bytes(tr)
        final = [dev(c[k]) for k in ("aL", "aR", "aO")]
        target = [torch.zeros_like(t) for t in final]
        torch.cuda.synchronize()
        side = torch.cuda.Stream()
        with torch.cuda.stream(side):
            torch.cuda._sleep(4_000_000)
            for t, f in zip(target, final):
                t.copy_(f, non_blocking=True)
        err = []

        def call():
            try:
                assert torch.cuda.current_stream().cuda_stream != side.cuda_stream
                p.set_witness(*target, stream=side)
            except BaseException as e:      # noqa: BLE001
                err.append(e)
        th = threading.Thread(target=call)
        th.start()
        th.join()
        assert not err, err
        assert p.prove_bytes(tr) == want
        side.synchronize()
    finally:
        p.close()


# ---- 7. Python -------------------------------------------------------------------------------------------------------------------------
def test_python_forms_agree_and_type_errors(sonic, srs_of):
    import torch
    n = 33
    c = circuit(n)
    tr = transcript(7)
    p = sonic.Prover(srs_of(n), arith(sonic, c), prepare=False)
    try:
        p.set_assignment(sonic.Assignment(c["aL"], c["aR"], c["aO"]))
        want = (p.prove_bytes(tr), p.witness_digest())
        la, lb, lo = c["ints"]
        forms = {
            "numpy": (c["aL"], c["aR"], c["aO"]),
            "torch cpu": tuple(torch.from_numpy(c[k]) for k in ("aL", "aR", "aO")),
            "torch cuda": tuple(dev(c[k]) for k in ("aL", "aR", "aO")),
            "torch cuda, explicit stream": tuple(dev(c[k]) for k in ("aL", "aR", "aO")),
            "lists": (la, lb, lo),
            "lists, aO derived": (la, lb, None),
        }
        for name, (aL, aR, aO) in forms.items():
            p.set_assignment(zero_assignment(sonic, n))
            if "explicit" in name:
                side = torch.cuda.Stream()
                side.wait_stream(torch.cuda.current_stream())
                p.set_witness(aL, aR, aO, stream=side.cuda_stream)
            else:
                p.set_witness(aL, aR, aO)
            assert (p.prove_bytes(tr), p.witness_digest()) == want, name
        dL, dR = dev(c["aL"]), dev(c["aR"])
        i64 = torch.zeros(n, dtype=torch.int64, device="cuda")
        for name, call in {
            "mixed kinds": lambda: p.set_witness(dL, i64),
            "mixed devices": lambda: p.set_witness(dL, c["aR"]),
            "wrong shape": lambda: p.set_witness(dL[:n - 1], dR[:n - 1]),
            "flat bytes": lambda: p.set_witness(dL.reshape(-1), dR.reshape(-1)),
            "wrong dtype": lambda: p.set_witness(dL.to(torch.int32), dR.to(torch.int32)),
            "not contiguous": lambda: p.set_witness(torch.zeros((n, 64), dtype=torch.uint8, device="cuda")[:, :32], dR),
            "a stream with host memory": lambda: p.set_witness(c["aL"], c["aR"], stream=5),
            "a batch for one handle": lambda: p.set_witness(dL.reshape(1, n, 32), dR.reshape(1, n, 32)),
            "batch of another n": lambda: p.eval_constraints(sonic.WitnessBatch(dL[:n - 1].reshape(1, n - 1, 32), dR[:n - 1].reshape(1, n - 1, 32))),
            "lists as a batch": lambda: p.eval_constraints(sonic.WitnessBatch([la], [lb])),
            "batch length": lambda: sonic.prove_batch([p], [tr, tr], sonic.WitnessBatch(dL.reshape(1, n, 32), dR.reshape(1, n, 32))),
        }.items():
            with pytest.raises(ValueError):
                call()
                pytest.fail(name + " was accepted")
        p.set_assignment(sonic.Assignment(c["aL"], c["aR"], c["aO"]))
        assert p.prove_bytes(tr) == want[0]
    finally:
        p.close()


def test_c99_harness(sonic, tmp_path):
    """witness sources from plain C99 (tests/host/witness_src_harness.c): a host int64 source with aO derived, then sonic_prover_prove"""
    exe = str(tmp_path / "witness_src_harness")
    subprocess.check_call(["gcc", "-std=c99", "-pedantic", "-Wall", "-Wextra", "-Werror", "-I" + os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "host", "witness_src_harness.c"), "-L" + os.path.join(ROOT, "sonic_amd", "csrc"), "-lsonic_hip",
                           "-Wl,-rpath," + os.path.join(ROOT, "sonic_amd", "csrc"), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and "witness_src_harness: OK" in out.stdout, out.stdout + out.stderr
