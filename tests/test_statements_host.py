"""One circuit, many statements, the parts that need no GPU (include/sonic_hip.h, "One circuit, many statements"): the circuit digest in two
halves (midstate + resume) against the whole digest, the batch digest v2 and its randomizers against a hashlib restatement
(tests/statements_ref.py), the same functions in a stand-alone host program built under ASan / UBSan (tests/host/statements_host.cpp), and
the header / exports / bindings.  Every comparison is byte equality."""
import ctypes as C
import hashlib
import json
import os
import random
import re
import subprocess

import numpy as np
import pytest

import statements_ref as sref
from util import R

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
HOST = os.path.join(HERE, "host")
ENV = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
# 3 Q n is odd and even across the set, so the weights end both at and off a 64-byte SHA block boundary ((36 + 96 Q n) % 64 = 4 or 36)
SHAPES = [(1, 1), (2, 1), (3, 1), (5, 3), (64, 2)]
NEW_SYMBOLS = ["sonic_prover_eval_constraints", "sonic_prover_set_constants", "sonic_prove_batch_statements", "sonic_fs_circuit_midstate",
               "sonic_fs_circuit_midstate_csr", "sonic_fs_circuit_digest_resume", "sonic_verifier_verify_batch_cs", "sonic_verifier_verify_fs_batch_cs",
               "sonic_verify_batch_digest_v2"]


def _L():
    from sonic_amd import _lib
    return _lib


def shape_case(n, Q):
    """random weights with zeros among them (so that the sparse form has gaps, empty rows included) and two sets of constants"""
    pyr = random.Random(100 * n + Q)
    mats = [[[pyr.randrange(R) if pyr.randrange(3) else 0 for _ in range(n)] for _ in range(Q)] for _ in range(3)]
    if Q > 1:
        mats[1][0] = [0] * n
    return mats, [[pyr.randrange(R) for _ in range(Q)] for _ in range(2)]


def circuits(n, Q, mats, cs):
    import sonic_amd
    dense = sonic_amd.ArithCircuit(sonic_amd.GateWeights(*mats), cs)
    return dense, sonic_amd.SparseCircuit.from_circuit(dense)


@pytest.mark.parametrize("n,Q", SHAPES)
def test_resume_of_the_midstate_is_the_whole_digest(n, Q):
    import sonic_amd
    mats, css = shape_case(n, Q)
    assert sref.weights_length(n, Q) % 64 in (4, 36)
    dense, sparse = circuits(n, Q, mats, css[0])
    mid = sonic_amd.fs_circuit_midstate(dense)
    assert len(mid) == 112 and mid == sonic_amd.fs_circuit_midstate(sparse)
    assert int.from_bytes(mid[96:104], "little") == sref.weights_length(n, Q) and int.from_bytes(mid[104:112], "little") == Q
    assert mid[32 + sref.weights_length(n, Q) % 64:96] == bytes(64 - sref.weights_length(n, Q) % 64)
    for cs in css + [[0] * Q, [R - 1] * Q]:
        d, s = circuits(n, Q, mats, cs)
        want = sref.circuit_digest(n, Q, *mats, cs)
        assert sonic_amd.fs_circuit_digest(d) == want and sonic_amd.fs_circuit_digest(s) == want      # the existing calls: one code path now
        assert sonic_amd.fs_circuit_digest_resume(mid, cs) == want
        assert sonic_amd.fs_circuit_digest_resume(mid, b"".join(sref.fr(c) for c in cs)) == want


def test_shapes_end_at_and_off_a_block_boundary():
    tails = {sref.weights_length(n, Q) % 64 for n, Q in SHAPES}
    assert tails == {4, 36}                                          # 3 Q n even: the weights end at a block boundary (+ the 36-byte head); odd: 32 off it
    assert {(3 * Q * n) % 2 for n, Q in SHAPES} == {0, 1}


def test_resume_matches_the_oracle_on_the_golden_circuit(ref):
    import sonic_amd
    c = json.load(open(os.path.join(HERE, "golden", "fs_small.json")))["cases"][0]
    b = next(x for x in json.load(open(os.path.join(HERE, "golden", "prove_small.json")))["cases"] if x["name"] == c["name"])
    iv = lambda v: int(v, 16)    # noqa: E731
    circ = tuple([[iv(v) for v in r] for r in b[k]] for k in ("wL", "wR", "wO")) + ([iv(v) for v in b["cs"]],)
    dense = sonic_amd.ArithCircuit(sonic_amd.GateWeights(*circ[:3]), circ[3])
    mid = sonic_amd.fs_circuit_midstate(dense)
    assert sonic_amd.fs_circuit_digest_resume(mid, circ[3]) == ref.fs_circuit_digest(circ) == bytes.fromhex(c["circuit_digest"])
    other = [(v + 1) % R for v in circ[3]]
    assert sonic_amd.fs_circuit_digest_resume(mid, other) == ref.fs_circuit_digest(circ[:3] + (other,))


def test_resume_refusals():
    import sonic_amd
    L = _L()
    n, Q = 5, 3
    mats, css = shape_case(n, Q)
    mid = sonic_amd.fs_circuit_midstate(circuits(n, Q, mats, css[0])[0])
    cs = b"".join(sref.fr(c) for c in css[0])
    out = C.create_string_buffer(32)
    put = lambda off, v: mid[:off] + v + mid[off + len(v):]      # noqa: E731
    bad = [put(96, sref.le64(sref.weights_length(n, Q) + 32)),       # a length that is not 36 + 96 Q n
           put(96, sref.le64(36)),                                   # n = 0
           put(104, sref.le64(Q + 1)), put(104, sref.le64(0)), put(104, sref.le64(1 << 63)),
           put(95, b"\x01")]                                         # a byte behind the pending ones
    for m in bad:
        assert L.lib().sonic_fs_circuit_digest_resume(m, cs, out) == 7, m.hex()
    assert L.lib().sonic_fs_circuit_digest_resume(mid, cs[:32] + R.to_bytes(32, "little") + cs[64:], out) == 3      # a non-canonical constant
    assert L.lib().sonic_fs_circuit_digest_resume(None, cs, out) == 7 and L.lib().sonic_fs_circuit_digest_resume(mid, None, out) == 7
    # n = 2, Q = 3 hashes as many bytes as n = 3, Q = 2, and the midstate keeps them apart by its Q
    assert L.lib().sonic_fs_circuit_digest_resume(mid, cs, out) == 0


# ---- batch digest v2 ----
def batch_case(n, Q, K, seed):
    pyr = random.Random(seed)
    psz = (7 + 4 * Q) * 96 + (5 + 2 * Q) * 32
    proofs = [pyr.randbytes(psz) for _ in range(K)]
    chal = [pyr.randbytes(32 * (2 + 2 * Q)) for _ in range(K)]
    cs = [b"".join(sref.fr(pyr.randrange(R)) for _ in range(Q)) for _ in range(K)]
    return pyr.randrange(7 * n, 9 * n + 9), pyr.randbytes(32), pyr.randbytes(32), proofs, chal, cs


@pytest.mark.parametrize("n,Q", SHAPES)
def test_batch_digest_v2_and_randomizers_match_the_hashlib_restatement(n, Q):
    import batch_ref
    L = _L().lib()
    for K in (1, 3):
        d, dg, sid, proofs, chal, cs = batch_case(n, Q, K, 7 * n + Q + K)
        out = C.create_string_buffer(32)
        assert L.sonic_verify_batch_digest_v2(n, Q, d, dg, sid, K, b"".join(proofs), b"".join(chal), b"".join(cs), out) == 0
        D = sref.batch_digest_v2(n, Q, d, dg, sid, proofs, chal, cs)
        assert out.raw == D
        assert D != batch_ref.batch_digest(n, Q, d, dg, sid, proofs, chal)                       # v1 does not bind the constants; v2 is another hash
        other = list(cs)
        other[K - 1] = cs[K - 1][:-32] + sref.fr(int.from_bytes(cs[K - 1][-32:], "little") + 1)
        assert sref.batch_digest_v2(n, Q, d, dg, sid, proofs, chal, other) != D                  # ... and v2 moves with one constant
        assert L.sonic_verify_batch_digest_v2(n, Q, d, dg, sid, K, b"".join(proofs), b"".join(chal), b"".join(other), out) == 0 and out.raw != D
        count = K * (3 * Q + 4)
        rho = C.create_string_buffer(16 * count)
        seed = hashlib.sha256(b"seed%d" % K).digest()
        assert L.sonic_verify_batch_randomizers(seed, D, count, rho) == 0
        assert [int.from_bytes(rho.raw[16 * i:16 * i + 16], "little") for i in range(count)] == sref.randomizers(seed, D, count)
    assert L.sonic_verify_batch_digest_v2(n, Q, 8 * n, None, bytes(32), 0, None, None, None, C.create_string_buffer(32)) == 7


# ---- the same functions in a stand-alone program, plain and under ASan / UBSan ----
@pytest.fixture(scope="module")
def drivers():
    subprocess.check_call(["make", "-C", HOST, "-s", "-f", "statements.mk", "statements_host", "statements_host_san"])
    return {"plain": os.path.join(HOST, "statements_host"), "san": os.path.join(HOST, "statements_host_san")}


def run_driver(path, lines):
    out = subprocess.run([path], input="\n".join(lines) + "\n", capture_output=True, text=True, timeout=600, env=ENV)
    assert out.returncode == 0 and out.stdout.endswith("statements_host ok\n"), out.stdout[-2000:] + out.stderr[-3000:]
    return out.stdout.splitlines()[:-1]


def ints(a):
    return ",".join(str(int(v)) for v in a) if len(a) else "-"


@pytest.mark.parametrize("build", ["plain", "san"])
def test_host_program(drivers, build):
    import sonic_amd
    lines, want = [], []
    for n, Q in SHAPES:
        mats, css = shape_case(n, Q)
        dense, sparse = circuits(n, Q, mats, css[0])
        W = b"".join(sref.fr(v) for m in mats for row in m for v in row)
        cs = b"".join(sref.fr(c) for c in css[1])
        mid, dg = sonic_amd.fs_circuit_midstate(dense), sref.circuit_digest(n, Q, *mats, css[1])
        lines.append("dense %d %d %s %s" % (n, Q, W.hex(), cs.hex()))
        want.append("%s %s %s" % (mid.hex(), dg.hex(), dg.hex()))
        lines.append("csr %d %d %s %s %s %s" % (n, Q, ints(sparse.row_ptr), ints(sparse.col), sparse.val.tobytes().hex() or "-", cs.hex()))
        want.append("%s %s" % (mid.hex(), dg.hex()))
        lines.append("resume %s %s" % (mid.hex(), cs.hex()))
        want.append("0 " + dg.hex())
        lines.append("resume %s %s" % (mid.hex(), (R.to_bytes(32, "little") + cs[32:]).hex()))
        want.append("2 " + bytes(32).hex())
        lines.append("resume %s %s" % ((mid[:96] + sref.le64(sref.weights_length(n, Q) + 1) + mid[104:]).hex(), cs.hex()))
        want.append("1 " + bytes(32).hex())
        for K in (1, 3):
            d, cd, sid, proofs, chal, kcs = batch_case(n, Q, K, 7 * n + Q + K)
            lines.append("d2 %d %d %d %d %s %s %s %s %s" % (n, Q, d, K, cd.hex(), sid.hex(), b"".join(proofs).hex(), b"".join(chal).hex(), b"".join(kcs).hex()))
            want.append(sref.batch_digest_v2(n, Q, d, cd, sid, proofs, chal, kcs).hex())
    # an all-empty sparse circuit: no entries at all
    n, Q = 3, 1
    zero = [[[0] * n] * Q] * 3
    lines.append("csr %d %d %s - - %s" % (n, Q, ints([0] * (3 * Q + 1)), sref.fr(5).hex()))
    dg = sref.circuit_digest(n, Q, *zero, [5])
    want.append(None)
    got = run_driver(drivers[build], lines)
    assert len(got) == len(want)
    for g, w, l in zip(got[:-1], want[:-1], lines):
        assert g == w, l[:60]
    assert got[-1].split()[1] == dg.hex()


# ---- header, exports, bindings, and no device ----
def test_header_declares_library_exports_python_binds():
    hdr = open(os.path.join(ROOT, "include", "sonic_hip.h")).read()
    L = _L()
    lib = L.lib()
    for name in NEW_SYMBOLS:
        assert re.search(r"\bint\s+%s\s*\(" % name, hdr), name
        assert name in L.EXPORTED and hasattr(lib, name), name
        assert getattr(lib, name).argtypes is not None, name
    assert "#define SONIC_FS_MIDSTATE_SIZE 112" in hdr and L.FS_MIDSTATE_SIZE == 112
    assert "#define SONIC_ABI_VERSION 7" in hdr and lib.sonic_abi_version() == 7 and L.ABI_VERSION == 7
    import inspect
    import sonic_amd
    assert callable(sonic_amd.fs_circuit_midstate) and callable(sonic_amd.fs_circuit_digest_resume)
    assert all(hasattr(sonic_amd.Prover, m) for m in ("set_constants", "eval_constraints"))
    assert inspect.signature(sonic_amd.prove_batch).parameters["constants"].default is None
    assert inspect.signature(sonic_amd.Prover.eval_constraints).parameters["assignments"].default is None
    for m in (sonic_amd.Verifier.verify_batch, sonic_amd.Verifier.verify_fs_batch):
        assert inspect.signature(m).parameters["constants"].default is None


def test_device_calls_report_no_device_without_one():
    """(on a box with a GPU the same calls report the NULL handle instead)"""
    L = _L().lib()
    n = C.c_int(0)
    want = 6 if L.sonic_device_count(C.byref(n)) == 6 else 7
    ok = C.c_int(0)
    buf = np.zeros(64, np.uint8).ctypes.data
    assert L.sonic_prover_eval_constraints(None, 1, None, None, None, buf, None) == want
    assert L.sonic_prover_set_constants(None, buf) == want
    assert L.sonic_prove_batch_statements(None, 1, 1, None, None, None, buf, buf, buf, None) == want
    assert L.sonic_verifier_verify_batch_cs(None, 1, buf, 0, buf, buf, bytes(32), C.byref(ok), None) == want
    assert L.sonic_verifier_verify_fs_batch_cs(None, 1, buf, 1, buf, bytes(32), C.byref(ok), None) == want
