"""Gate weights as CSR (include/sonic_hip.h, "gate weights as CSR") without a GPU: the new symbols are declared, exported and bound at
ABI version 7; sonic_fs_circuit_digest_csr hashes the rows as the dense bytes they stand for; the one validator refuses every broken
form with the stated status; SparseCircuit round-trips through the dense form; workload.sparse_circuit is satisfied; without a device
the sparse prover entry points refuse like the dense ones."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from util import R, fr_bytes, rand_fr_array

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("sonic_prover_new_csr", "sonic_prove_csr", "sonic_fs_circuit_digest_csr", "sonic_verify_csr", "sonic_verify_fs_csr")


@pytest.fixture(scope="module")
def L():
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "sonic_amd", "csrc"), "-s", "-j8"])
    from sonic_amd import _lib
    return _lib


def test_symbols_declared_exported_bound_at_abi_7(L):
    hdr = open(os.path.join(ROOT, "include", "sonic_hip.h")).read()
    assert int(re.search(r"#define SONIC_ABI_VERSION (\d+)", hdr).group(1)) == 7 == L.ABI_VERSION == L.lib().sonic_abi_version()
    for s in NEW:
        assert re.search(r"\b%s\s*\(" % s, hdr), s
        assert s in L.EXPORTED
        assert getattr(L.lib(), s).argtypes, s
    hs = open(os.path.join(ROOT, "haskell", "Sonic", "HIP.hs")).read()
    assert int(re.search(r"abiExpected = (\d+)", hs).group(1)) == 7
    for s in NEW:
        assert '"%s"' % s in hs, s


def _digest(L, n, Q, row_ptr, col, val, cs):
    out = C.create_string_buffer(32)
    row_ptr = np.ascontiguousarray(row_ptr, np.int64)
    col = np.ascontiguousarray(col, np.int64)
    val = np.ascontiguousarray(val, np.uint8).reshape(-1, 32)
    cs = np.ascontiguousarray(cs, np.uint8).reshape(-1, 32)
    rc = L.lib().sonic_fs_circuit_digest_csr(n, Q, row_ptr.ctypes.data, col.ctypes.data if col.size else None,
                                             val.ctypes.data if val.size else None, cs.ctypes.data, out)
    return rc, out.raw


def _dense_digest(L, n, Q, W, cs):
    """W: uint8 [3Q, n, 32]"""
    W = np.ascontiguousarray(W)
    out = C.create_string_buffer(32)
    wL, wR, wO = (np.ascontiguousarray(W[m * Q:(m + 1) * Q]) for m in range(3))
    assert L.lib().sonic_fs_circuit_digest(n, Q, wL.ctypes.data, wR.ctypes.data, wO.ctypes.data, np.ascontiguousarray(cs).ctypes.data, out) == 0
    return out.raw


def _densify(n, Q, row_ptr, col, val):
    W = np.zeros((3 * Q, n, 32), np.uint8)
    for r in range(3 * Q):
        for k in range(row_ptr[r], row_ptr[r + 1]):
            W[r, col[k]] = val[k]
    return W


def _cases():
    rng = np.random.default_rng(7)
    out = []
    # random sparse circuits (a few entries per row, some rows empty)
    for n, Q in ((1, 1), (7, 3), (257, 16), (5000, 2)):
        counts = rng.integers(0, min(4, n) + 1, size=3 * Q)
        rp = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
        col = np.concatenate([np.sort(rng.choice(n, size=c, replace=False)) for c in counts] or [np.zeros(0, np.int64)]).astype(np.int64)
        out.append(("random", n, Q, rp, col, rand_fr_array(rng, int(rp[-1]))))
    n, Q = 9, 3
    out.append(("empty matrix", n, Q, np.zeros(3 * Q + 1, np.int64), np.zeros(0, np.int64), np.zeros((0, 32), np.uint8)))
    # empty rows around one dense row of wR
    rp = np.zeros(3 * Q + 1, np.int64); rp[Q + 2:] = n
    out.append(("one fully dense row", n, Q, rp, np.arange(n, dtype=np.int64), rand_fr_array(rng, n)))
    # one gate (column 4) with an entry in every row
    out.append(("one gate in every row", n, Q, np.arange(3 * Q + 1, dtype=np.int64), np.full(3 * Q, 4, np.int64), rand_fr_array(rng, 3 * Q)))
    # explicit zeros among the values
    v = rand_fr_array(rng, 3 * Q); v[::2] = 0
    out.append(("explicit zeros", n, Q, np.arange(3 * Q + 1, dtype=np.int64), np.arange(3 * Q, dtype=np.int64) % n, v))
    out.append(("n = 1, Q = 1", 1, 1, np.array([0, 1, 1, 2], np.int64), np.array([0, 0], np.int64), fr_bytes([5, R - 1])))
    return out


@pytest.mark.parametrize("case", _cases(), ids=lambda c: f"{c[0]}-{c[1]}x{c[2]}")
def test_digest_equals_the_dense_digest(L, case):
    name, n, Q, rp, col, val = case
    cs = rand_fr_array(np.random.default_rng(n * 31 + Q), Q)
    rc, got = _digest(L, n, Q, rp, col, val, cs)
    assert rc == 0, L.last_error()
    assert got == _dense_digest(L, n, Q, _densify(n, Q, rp, col, val), cs)


def test_python_digest_dispatches_on_the_circuit_type(L):
    import sonic_amd
    from sonic_amd import workload
    c = workload.sparse_circuit(3, 300, 5, 4)
    sp = sonic_amd.SparseCircuit(c["n"], c["Q"], c["row_ptr"], c["col"], c["val"], c["cs"])
    assert sonic_amd.fs_circuit_digest(sp) == sonic_amd.fs_circuit_digest(sp.to_dense())


def test_validator_refuses_each_broken_form(L):
    n, Q = 6, 2
    rp = np.array([0, 2, 2, 3, 3, 4, 5], np.int64)
    col = np.array([1, 4, 0, 5, 2], np.int64)
    val = fr_bytes([3, 4, 5, 6, 7])
    cs = fr_bytes([1, 2])
    assert _digest(L, n, Q, rp, col, val, cs)[0] == 0

    def bad(rp_=rp, col_=col, val_=val, status=7, row=None):
        rc, _ = _digest(L, n, Q, rp_, col_, val_, cs)
        assert rc == status, (rc, L.last_error())
        if row is not None:
            assert f"row {row}" in L.last_error(), L.last_error()

    r0 = rp.copy(); r0[0] = 1
    bad(rp_=r0, row=0)                                              # row_ptr[0] != 0
    dec = rp.copy(); dec[3] = 1
    bad(rp_=dec, row=2)                                             # a decreasing row_ptr
    hi = col.copy(); hi[2] = n
    bad(col_=hi, row=2)                                             # a column >= n
    neg = col.copy(); neg[3] = -1
    bad(col_=neg, row=4)                                            # a column < 0
    uns = col.copy(); uns[0], uns[1] = 4, 1
    bad(col_=uns, row=0)                                            # unsorted
    dup = col.copy(); dup[1] = 1
    bad(col_=dup, row=0)                                            # duplicate
    nc = val.copy(); nc[4] = np.frombuffer(R.to_bytes(32, "little"), np.uint8)
    bad(val_=nc, status=3, row=5)                                   # a non-canonical value
    big = rp.copy(); big[-1] = 1 << 31
    bad(rp_=big)                                                    # nnz > 2^31 - 1


def test_sparse_circuit_round_trips_through_dense(L):
    import sonic_amd
    from sonic_amd import workload
    c = workload.sparse_circuit(11, 64, 6, 4)
    sp = sonic_amd.SparseCircuit(c["n"], c["Q"], c["row_ptr"], c["col"], c["val"], c["cs"])
    back = sonic_amd.SparseCircuit.from_circuit(sp.to_dense())
    nonzero = sp.val.any(axis=1)
    assert back.nnz == int(nonzero.sum())                          # from_circuit drops (explicit) zeros; there are none here
    assert np.array_equal(back.row_ptr, sp.row_ptr) and np.array_equal(back.col, sp.col) and np.array_equal(back.val, sp.val)
    assert np.array_equal(back.cs, sp.cs)
    # from_rows with {gate: value} mappings, and zeros dropped by from_circuit
    rows = [{0: 5, 3: 0}, {}, {2: 7}, {1: 1}, {}, {}]
    s2 = sonic_amd.SparseCircuit.from_rows(4, rows[0:2], rows[2:4], rows[4:6], [1, 2])
    assert list(s2.row_ptr) == [0, 2, 2, 3, 4, 4, 4] and list(s2.col) == [0, 3, 2, 1]
    d = s2.to_dense()
    s3 = sonic_amd.SparseCircuit.from_circuit(d)
    assert list(s3.row_ptr) == [0, 1, 1, 2, 3, 3, 3] and list(s3.col) == [0, 2, 1]
    assert [int.from_bytes(v.tobytes(), "little") for v in s3.val] == [5, 7, 1]
    # csr_from_dense on big_circuit's arrays: one all-ones row per matrix
    b = workload.big_circuit(5, 40, 3)
    rp, col, val = workload.csr_from_dense(b["wL"], b["wR"], b["wO"], 40, 3)
    assert rp[-1] == 3 * 40 and all(rp[m * 3 + b["rows"][m] + 1] - rp[m * 3 + b["rows"][m]] == 40 for m in range(3))


@pytest.mark.parametrize("n,Q,k", [(1, 1, 4), (50, 7, 4), (300, 16, 2)])
def test_sparse_circuit_is_satisfied(n, Q, k):
    """every constraint q: sum wL_q aL + wR_q aR + wO_q aO = cs_q, and aL * aR = aO gate by gate (Python integers)"""
    from sonic_amd import workload
    c = workload.sparse_circuit(n * 100 + Q, n, Q, k)
    iv = lambda a, i: int.from_bytes(a[i].tobytes(), "little")      # noqa: E731
    a = [[iv(c[nm], i) for i in range(n)] for nm in ("aL", "aR", "aO")]
    assert all(a[0][i] * a[1][i] % R == a[2][i] for i in range(n))
    rp, col, val = c["row_ptr"], c["col"], c["val"]
    assert np.all(np.diff(rp) <= k) and np.all(np.diff(rp) >= 0)
    for q in range(Q):
        acc = 0
        for m in range(3):
            r = m * Q + q
            cols = col[rp[r]:rp[r + 1]]
            assert np.all(np.diff(cols) > 0) and np.all((cols >= 0) & (cols < n))
            acc += sum(iv(val, kk) * a[m][int(col[kk])] for kk in range(rp[r], rp[r + 1]))
        assert acc % R == iv(c["cs"], q)


def _have_gpu():
    return os.path.exists("/dev/kfd")


@pytest.mark.skipif(_have_gpu(), reason="this box has a GPU; the refusal path needs none")
def test_no_device_refuses_the_sparse_prover(L):
    lib = L.lib()
    rp = np.zeros(4, np.int64)
    cs = fr_bytes([0])
    h = C.c_void_p()
    assert lib.sonic_prover_new_csr(None, 1, 1, rp.ctypes.data, None, None, cs.ctypes.data, C.byref(h)) == 6
    a = fr_bytes([0])
    tr = fr_bytes([1] * 10)
    out = C.create_string_buffer(lib.sonic_proof_size(1))
    assert lib.sonic_prove_csr(None, 1, 1, rp.ctypes.data, None, None, cs.ctypes.data, a.ctypes.data, a.ctypes.data, a.ctypes.data,
                               tr.ctypes.data, out) == 6
