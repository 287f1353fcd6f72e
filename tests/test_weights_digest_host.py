"""Weights digest v2 and circuit digest v2, the parts that need no GPU (include/sonic_hip.h, "Circuits with Q ~ n"): the SHA-256 tree of
sonic_amd/csrc/weights_tree.hpp -- the text the kernels of weights_digest.hip compile -- driven on the host by a stand-alone program built
plain and under ASan / UBSan (tests/host/weights_digest_host.cpp) and by the library's host calls through ctypes, against a hashlib
restatement (tests/weights_digest_ref.py); and the header / exports / bindings.  Every comparison is byte equality."""
import ctypes as C
import copy
import os
import re
import subprocess

import numpy as np
import pytest

import weights_digest_ref as wref
from weights_digest_ref import CASES, TREES, R

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
HOST = os.path.join(HERE, "host")
ENV = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
NEW_SYMBOLS = ["sonic_fs_weights_digest_v2_csr", "sonic_fs_circuit_digest_v2", "sonic_prover_weights_digest_v2", "sonic_verifier_weights_digest_v2",
               "sonic_verifier_new_digest", "sonic_verifier_digest_kind", "sonic_prover_device_bytes"]
OK, BAD_ENCODING, NO_DEVICE, INVALID_ARG = 0, 3, 6, 7


def test_restatement_has_the_shapes_the_cases_are_named_for():
    assert [c.name for c in CASES] == list(TREES)
    for c in CASES:
        assert c.name == "nnz%d" % c.nnz and c.leaves_and_nodes() == TREES[c.name], c.name
    by = {c.name: c for c in CASES}
    # first row empty / last row empty / a run of empty rows inside a leaf / Q = 1 / a column n - 1
    assert by["nnz1"].Q == 1 and by["nnz1"].row_ptr == [0, 0, 1, 1] and by["nnz1"].col == [7] and by["nnz1"].n == 8
    assert by["nnz16"].row_ptr == [0, 0, 7, 7, 7, 16, 16] and by["nnz16"].col[-1] == 15
    # a row boundary at a leaf boundary
    assert by["nnz17"].row_ptr[1] == 16
    # one row that spans three leaves: entries 16 .. 55 are leaves 1, 2, 3
    rp = by["nnz512"].row_ptr
    assert (rp[1], rp[2]) == (16, 56) and {k // 16 for k in range(rp[1], rp[2])} == {1, 2, 3}
    # the values 0 (explicit), 1 and r - 1
    for c in CASES:
        if c.nnz >= 3:
            assert {0, 1, R - 1} <= set(c.val), c.name
    assert len(wref.leaf_header(5)) == 64 and len(wref.node_header(2, 7)) == 64
    assert wref.leaf_header(5)[56:] == (5).to_bytes(8, "little") and wref.node_header(2, 7)[48:] == (2).to_bytes(8, "little") + (7).to_bytes(8, "little")
    assert len(b"sonic-hip/weights-leaf/v2") == len(b"sonic-hip/weights-node/v2") == len(b"sonic-hip/witness-leaf/v2") == 25


@pytest.fixture(scope="module")
def drivers():
    subprocess.check_call(["make", "-C", HOST, "-s", "-f", "weights_digest.mk", "weights_digest_host", "weights_digest_host_san"])
    return {"plain": os.path.join(HOST, "weights_digest_host"), "san": os.path.join(HOST, "weights_digest_host_san")}


@pytest.fixture(scope="module")
def want():
    """the restatement's answers, once: name -> (root, weights digest v2, circuit digest v2)"""
    out = {}
    for c in CASES:
        wd = c.digest()
        out[c.name] = (wref.weights_levels(c.row_ptr, c.col, c.val)[-1][0], wd, wref.circuit_digest_v2(wd, c.cs))
    return out


def run_driver(path, lines):
    out = subprocess.run([path], input="\n".join(lines) + "\n", capture_output=True, text=True, timeout=600, env=ENV)
    assert out.returncode == 0 and out.stdout.endswith("weights_digest_host ok\n"), out.stdout[-2000:] + out.stderr[-3000:]
    return out.stdout.splitlines()[:-1]


def case_line(c):
    ints = lambda v: ",".join(str(x) for x in v) or "-"      # noqa: E731
    return "csr %d %d %s %s %s %s" % (c.n, c.Q, ints(c.row_ptr), ints(c.col), b"".join(wref.fr(v) for v in c.val).hex() or "-",
                                      b"".join(wref.fr(v) for v in c.cs).hex())


@pytest.mark.parametrize("build", ["plain", "san"])
def test_host_program_matches_the_restatement(drivers, want, build):
    got = run_driver(drivers[build], [case_line(c) for c in CASES])
    assert len(got) == len(CASES)
    for c, g in zip(CASES, got):
        root, wd, cd = want[c.name]
        # (the ABI's form, and the form the kernels read: int32 indices, Montgomery values)
        assert g == "%s %s %s %s" % (root.hex(), wd.hex(), wd.hex(), cd.hex()), c.name
    assert len({want[c.name][1] for c in CASES}) == len(CASES)


# ---- the library's host calls through ctypes ----
def lib_wd2(c, n=None, Q=None):
    from sonic_amd import _lib
    rp, col = np.array(c.row_ptr, np.int64), np.array(c.col, np.int64)
    val = np.frombuffer(b"".join(wref.fr(v) for v in c.val), np.uint8)
    out = C.create_string_buffer(32)
    rc = _lib.lib().sonic_fs_weights_digest_v2_csr(c.n if n is None else n, c.Q if Q is None else Q, rp.ctypes.data, col.ctypes.data if c.nnz else None,
                                                   val.ctypes.data if c.nnz else None, out)
    return rc, out.raw


def lib_cd2(wd, cs_bytes, Q):
    from sonic_amd import _lib
    out = C.create_string_buffer(32)
    return _lib.lib().sonic_fs_circuit_digest_v2(wd, Q, cs_bytes, out), out.raw


def test_library_host_calls_match_the_restatement(want):
    import sonic_amd
    for c in CASES:
        rc, wd = lib_wd2(c)
        assert rc == OK and wd == want[c.name][1], c.name
        rc, cd = lib_cd2(wd, b"".join(wref.fr(v) for v in c.cs), c.Q)
        assert rc == OK and cd == want[c.name][2], c.name
        # the Python layer: a SparseCircuit is hashed as given
        sp = sonic_amd.SparseCircuit(c.n, c.Q, c.row_ptr, c.col, c.val, c.cs)
        assert sonic_amd.fs_weights_digest_v2(sp) == wd and sonic_amd.fs_circuit_digest_v2(wd, c.cs) == cd, c.name


def test_a_dense_circuit_goes_through_its_non_zero_entries():
    import sonic_amd
    c = next(k for k in CASES if k.name == "nnz513")
    sp = sonic_amd.SparseCircuit(c.n, c.Q, c.row_ptr, c.col, c.val, c.cs)
    dense = sp.to_dense()
    kept = [(r, cc, v) for r, cc, v in wref.entries_of(c.row_ptr, c.col, c.val) if v != 0]
    assert len(kept) < c.nnz                                   # (the case holds explicit zeros: from_circuit drops them)
    rp = [0] * (3 * c.Q + 1)
    for r, _, _ in kept:
        rp[r + 1] += 1
    for r in range(3 * c.Q):
        rp[r + 1] += rp[r]
    assert sonic_amd.fs_weights_digest_v2(dense) == wref.weights_digest_v2(c.n, c.Q, rp, [k[1] for k in kept], [k[2] for k in kept]) != c.digest()


def changed(c, **kw):
    d = copy.deepcopy(c)
    for k, v in kw.items():
        setattr(d, k, v)
    return d


def test_digest_moves_with_every_part_of_the_input(want):
    c = next(k for k in CASES if k.name == "nnz17")
    base = want[c.name][1]
    seen = {base}

    def differs(d, what):
        rc, wd = lib_wd2(d)
        assert rc == OK and wd == d.digest(), what
        assert wd not in seen, what
        seen.add(wd)

    val = list(c.val); val[5] = (val[5] + 1) % R
    differs(changed(c, val=val), "one value")
    col = list(c.col); col[16] = (col[16] + 1) % c.n
    differs(changed(c, col=col), "one column")
    # entry 16, alone in row 1, moves to row 2: the same (col, val) sequence, only r changes
    differs(changed(c, row_ptr=[0, 16, 16, 17, 17, 17, 17]), "an entry moved to the next row")
    # an explicit zero added behind it in row 1 (a column the row does not hold yet)
    zc = c.col[16] + 1 if c.col[16] + 1 < c.n else c.col[16] - 1
    order = sorted([(c.col[16], c.val[16]), (zc, 0)])
    differs(changed(c, row_ptr=[0, 16, 18, 18, 18, 18, 18], col=c.col[:16] + [o[0] for o in order], val=c.val[:16] + [o[1] for o in order]), "an explicit zero")
    differs(changed(c, n=c.n + 1), "n")
    # Q changed, nnz and the entries (their stacked rows included) the same: three more empty rows at the end
    differs(changed(c, Q=c.Q + 1, row_ptr=c.row_ptr + [17, 17, 17]), "Q")
    # circuit digest v2 moves with one constant
    cs = list(c.cs); cs[1] = (cs[1] + 1) % R
    assert wref.circuit_digest_v2(base, cs) != want[c.name][2]
    rc, cd = lib_cd2(base, b"".join(wref.fr(v) for v in cs), c.Q)
    assert rc == OK and cd == wref.circuit_digest_v2(base, cs)


def test_refusals_are_those_of_the_midstate_call():
    from sonic_amd import _lib
    L = _lib.lib()
    c = next(k for k in CASES if k.name == "nnz17")

    def both(d, n=None, Q=None):
        """(status, message) of the v2 call and of sonic_fs_circuit_midstate_csr over the same arguments"""
        rc2, _ = lib_wd2(d, n, Q)
        m2 = _lib.last_error()
        rp, col = np.array(d.row_ptr, np.int64), np.array(d.col, np.int64)
        val = np.frombuffer(b"".join(wref.fr(v) for v in d.val), np.uint8)
        rc1 = L.sonic_fs_circuit_midstate_csr(d.n if n is None else n, d.Q if Q is None else Q, rp.ctypes.data, col.ctypes.data, val.ctypes.data, C.create_string_buffer(112))
        m1 = _lib.last_error()
        return rc2, m2, rc1, m1.replace("sonic_fs_circuit_midstate_csr", "sonic_fs_weights_digest_v2_csr")

    # a value >= r
    rc2, m2, rc1, m1 = both(changed(c, val=c.val[:3] + [R] + c.val[4:]))
    assert rc2 == rc1 == BAD_ENCODING and m2 == m1 and "non-canonical" in m2
    # broken structure: row_ptr[0] != 0, a decreasing row_ptr, a column out of range, columns not increasing, n < 1
    broken = [changed(c, row_ptr=[1] + c.row_ptr[1:]), changed(c, row_ptr=[0, 16, 15, 17, 17, 17, 17]), changed(c, col=c.col[:16] + [c.n]),
              changed(c, col=[c.col[1], c.col[0]] + c.col[2:])]
    for d in broken:
        rc2, m2, rc1, m1 = both(d)
        assert rc2 == rc1 == INVALID_ARG and m2 == m1 and m2.startswith("sonic_fs_weights_digest_v2_csr: "), m2
    rc2, m2, rc1, m1 = both(c, n=0)
    assert rc2 == rc1 == INVALID_ARG and m2 == m1
    assert L.sonic_fs_weights_digest_v2_csr(c.n, c.Q, np.array(c.row_ptr, np.int64).ctypes.data, None, None, C.create_string_buffer(32)) == INVALID_ARG      # entries and no col
    assert L.sonic_fs_weights_digest_v2_csr(c.n, c.Q, None, None, None, C.create_string_buffer(32)) == INVALID_ARG
    # circuit digest v2: a constant >= r names its q; missing arguments
    wd = c.digest()
    cs = [wref.fr(v) for v in c.cs]
    rc, _ = lib_cd2(wd, cs[0] + (R).to_bytes(32, "little"), c.Q)
    assert rc == BAD_ENCODING and "cs[1]" in _lib.last_error()
    assert lib_cd2(wd, b"".join(cs), 0)[0] == INVALID_ARG and lib_cd2(None, b"".join(cs), c.Q)[0] == INVALID_ARG
    assert L.sonic_fs_circuit_digest_v2(wd, c.Q, None, C.create_string_buffer(32)) == INVALID_ARG


# ---- header, exports, bindings, and no device ----
def test_header_declares_library_exports_python_and_haskell_bind():
    from sonic_amd import _lib as L
    import sonic_amd
    hdr = open(os.path.join(ROOT, "include", "sonic_hip.h")).read()
    lib = L.lib()
    for name in NEW_SYMBOLS:
        assert re.search(r"\bint\s+%s\s*\(" % name, hdr), name
        assert name in L.EXPORTED and hasattr(lib, name), name
        assert getattr(lib, name).argtypes is not None, name
    assert "#define SONIC_ABI_VERSION 7" in hdr and lib.sonic_abi_version() == 7 and L.ABI_VERSION == 7
    assert all(hasattr(sonic_amd.Prover, m) for m in ("weights_digest_v2", "device_bytes"))
    assert all(hasattr(sonic_amd.Verifier, m) for m in ("weights_digest_v2", "digest_kind"))
    assert callable(sonic_amd.fs_weights_digest_v2) and callable(sonic_amd.fs_circuit_digest_v2)
    hs = open(os.path.join(ROOT, "haskell", "Sonic", "HIP.hs")).read()
    for name in NEW_SYMBOLS:
        assert re.search(r'foreign import ccall\s+safe\s+"%s"' % name, hs), name
    for name in ("fsWeightsDigestV2", "fsCircuitDigestV2", "proverWeightsDigestV2", "verifierWeightsDigestV2", "newVerifierDigest", "verifierDigestKind",
                 "proverDeviceBytes"):
        assert re.search(r"^%s\s*::" % name, hs, re.M), name
    # the normative text stands in fs.hpp and is repeated in the header
    fs = open(os.path.join(ROOT, "sonic_amd", "csrc", "fs.hpp")).read()
    for text in ("sonic-hip/weights-leaf/v2", "sonic-hip/weights-node/v2", "sonic-hip/weights/v2", "sonic-hip/circuit/v2"):
        assert text in fs and text in hdr, text


def test_device_calls_report_no_device_without_one():
    """(on a box with a GPU the same calls report the NULL handle instead)"""
    from sonic_amd import _lib
    L = _lib.lib()
    n = C.c_int(0)
    want = NO_DEVICE if L.sonic_device_count(C.byref(n)) == NO_DEVICE else INVALID_ARG
    buf = C.create_string_buffer(64)
    out = C.c_int64(0)
    h = C.c_void_p()
    assert L.sonic_prover_weights_digest_v2(None, buf) == want
    assert L.sonic_verifier_weights_digest_v2(None, buf) == want
    assert L.sonic_prover_device_bytes(None, C.byref(out)) == want
    assert L.sonic_verifier_new_digest(None, 1, 1, None, None, None, None, 2, C.byref(h)) == want
    assert L.sonic_verifier_digest_kind(None) == -1
