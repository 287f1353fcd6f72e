"""Helped verification, the parts that need no GPU (include/sonic_hip.h, "Helped verification"): the weights digest, the transcript of an
aggregate and the digest of a helped batch -- the host-only library calls against the hashlib restatement in tests/aggregate_ref.py, on
random bytes (the transcript reads points and field elements as bytes) -- and the header / exports / bindings.  Every comparison is byte
equality."""
import ctypes as C
import os
import random
import re

import pytest

import aggregate_ref as aref
from util import R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ["sonic_fs_weights_digest", "sonic_fs_aggregate_challenges", "sonic_prover_aggregate_core", "sonic_verify_core_helped_digest",
               "sonic_verifier_verify_core_batch_helped", "sonic_verifier_verify_core_fs_batch_helped"]
KS, QS = [1, 2, 17], [1, 5]


def case(pyr, Q, K):
    n, d = pyr.randrange(1, 1 << 20), pyr.randrange(1, 1 << 24)
    yzs = [(pyr.randrange(R), pyr.randrange(R)) for _ in range(K)]
    return dict(n=n, d=d, wd=pyr.randbytes(32), sid=pyr.randbytes(32), yzs=yzs, yz=b"".join(aref.fr(y) + aref.fr(z) for y, z in yzs),
                agg=pyr.randbytes(aref.aggregate_size(K)), proofs=[pyr.randbytes(aref.CORE_SIZE) for _ in range(K)],
                cs=[b"".join(aref.fr(pyr.randrange(R)) for _ in range(Q)) for _ in range(K)])


def test_weights_digest_matches_hashlib():
    from sonic_amd import _lib
    L = _lib.lib()
    pyr = random.Random(41)
    seen = set()
    for _ in range(4):
        mid = pyr.randbytes(aref.MIDSTATE_SIZE)
        out = C.create_string_buffer(32)
        assert L.sonic_fs_weights_digest(mid, out) == 0
        assert out.raw == aref.weights_digest(mid)
        seen.add(out.raw)
    assert len(seen) == 4
    assert L.sonic_fs_weights_digest(None, C.create_string_buffer(32)) == 7 and L.sonic_fs_weights_digest(bytes(112), None) == 7


def test_weights_digest_of_a_circuit_ignores_the_constants():
    """the digest is of the midstate, which ends before cs: two statements of one circuit share it, another circuit does not"""
    import sonic_amd as sonic
    pyr = random.Random(42)
    n, Q = 5, 2
    w = [[[pyr.randrange(R) for _ in range(n)] for _ in range(Q)] for _ in range(3)]
    a = sonic.ArithCircuit(sonic.GateWeights(*w), [pyr.randrange(R) for _ in range(Q)])
    b = sonic.ArithCircuit(sonic.GateWeights(*w), [pyr.randrange(R) for _ in range(Q)])
    w2 = [[list(row) for row in m] for m in w]
    w2[2][1][3] = (w2[2][1][3] + 1) % R
    c = sonic.ArithCircuit(sonic.GateWeights(*w2), a.cs)
    assert sonic.fs_weights_digest(a) == sonic.fs_weights_digest(b) == aref.weights_digest(sonic.fs_circuit_midstate(a))
    assert sonic.fs_weights_digest(sonic.SparseCircuit.from_circuit(a)) == sonic.fs_weights_digest(a)
    assert sonic.fs_weights_digest(c) != sonic.fs_weights_digest(a)
    assert sonic.fs_weights_digest(sonic.fs_circuit_midstate(a)) == sonic.fs_weights_digest(a)


@pytest.mark.parametrize("Q", QS)
@pytest.mark.parametrize("K", KS)
def test_aggregate_challenges_match_hashlib(K, Q):
    from sonic_amd import _lib
    L = _lib.lib()
    c = case(random.Random(100 * K + Q), Q, K)
    out = C.create_string_buffer(64)
    assert L.sonic_fs_aggregate_challenges(c["n"], Q, c["d"], c["wd"], c["sid"], K, c["yz"], c["agg"], out) == 0
    u, v = aref.aggregate_challenges(c["n"], Q, c["d"], c["wd"], c["sid"], c["yzs"], c["agg"])
    assert out.raw == aref.fr(u) + aref.fr(v) and 0 < u < R and 0 < v < R
    at = 448 * K
    # what each challenge binds: u everything up to the W_j, v also C and the second list; neither the aggregate's own Q_v, u, v
    for name, lo, moves_u in (("n", None, True), ("wd", None, True), ("sid", None, True), ("yz", None, True), ("hscS", 0, True), ("hscW", 224 * K, False),
                              ("C", at + 96, False), ("Qv", at, None), ("u", at + 192, None), ("v", at + 224, None)):
        args = dict(c)
        if lo is None and name == "n":
            args["n"] = c["n"] + 1
        elif lo is None:
            args[name] = bytes([c[name][0] ^ 1]) + c[name][1:]
        else:
            args["agg"] = c["agg"][:lo] + bytes([c["agg"][lo] ^ 1]) + c["agg"][lo + 1:]
        o2 = C.create_string_buffer(64)
        assert L.sonic_fs_aggregate_challenges(args["n"], Q, c["d"], args["wd"], args["sid"], K, args["yz"], args["agg"], o2) == 0
        if moves_u is None:
            assert o2.raw == out.raw, name
        else:
            assert (o2.raw[:32] != out.raw[:32]) == moves_u and o2.raw[32:] != out.raw[32:], name
    # K is bound as well: the same bytes read as K - 1 pairs give other challenges
    if K > 1:
        o2 = C.create_string_buffer(64)
        assert L.sonic_fs_aggregate_challenges(c["n"], Q, c["d"], c["wd"], c["sid"], K - 1, c["yz"], c["agg"], o2) == 0 and o2.raw[:32] != out.raw[:32]
    assert L.sonic_fs_aggregate_challenges(c["n"], Q, c["d"], c["wd"], c["sid"], 0, c["yz"], c["agg"], out) == 7
    assert L.sonic_fs_aggregate_challenges(0, Q, c["d"], c["wd"], c["sid"], K, c["yz"], c["agg"], out) == 7
    assert L.sonic_fs_aggregate_challenges(c["n"], Q, c["d"], c["wd"], c["sid"], K, None, c["agg"], out) == 7


@pytest.mark.parametrize("Q", QS)
@pytest.mark.parametrize("K", KS)
def test_helped_batch_digest_matches_hashlib(K, Q):
    from sonic_amd import _lib
    L = _lib.lib()
    c = case(random.Random(200 * K + Q), Q, K)
    D = C.create_string_buffer(32)
    call = lambda proofs, yz, cs, agg, out: L.sonic_verify_core_helped_digest(c["n"], Q, c["d"], c["wd"], c["sid"], K, proofs, yz, cs, agg, out)  # noqa: E731
    blobs = [b"".join(c["proofs"]), c["yz"], b"".join(c["cs"]), c["agg"]]
    assert call(*blobs, D) == 0
    assert D.raw == aref.helped_digest(c["n"], Q, c["d"], c["wd"], c["sid"], c["proofs"], c["yzs"], c["cs"], c["agg"])
    # every part is bound: the first and the last bit of the proofs, the challenges, the constants and the aggregate
    for i, blob in enumerate(blobs):
        for flipped in (bytes([blob[0] ^ 1]) + blob[1:], blob[:-1] + bytes([blob[-1] ^ 0x80])):
            D2 = C.create_string_buffer(32)
            assert call(*(blobs[:i] + [flipped] + blobs[i + 1:]), D2) == 0 and D2.raw != D.raw
    # not the digest of the unhelped batch over the same proofs
    D3 = C.create_string_buffer(32)
    assert L.sonic_verify_core_batch_digest(c["n"], Q, c["d"], c["wd"], c["sid"], K, blobs[0], blobs[1], blobs[2], D3) == 0 and D3.raw != D.raw
    assert call(None, blobs[1], blobs[2], blobs[3], D) == 7 and call(*blobs, None) == 7


def test_header_declares_library_exports_python_and_haskell_bind():
    from sonic_amd import _lib as L
    import sonic_amd
    hdr = open(os.path.join(ROOT, "include", "sonic_hip.h")).read()
    lib = L.lib()
    for name in NEW_SYMBOLS:
        assert re.search(r"\bint\s+%s\s*\(" % name, hdr), name
        assert name in L.EXPORTED and hasattr(lib, name), name
        assert getattr(lib, name).argtypes is not None, name
    assert "#define SONIC_ABI_VERSION 7" in hdr and lib.sonic_abi_version() == 7
    assert hasattr(sonic_amd.Prover, "aggregate_core")
    assert all(hasattr(sonic_amd.Verifier, m) for m in ("verify_core_batch_helped", "verify_core_fs_batch_helped"))
    assert all(callable(getattr(sonic_amd, f)) for f in ("aggregate_core", "fs_weights_digest", "fs_aggregate_challenges"))
    hs = open(os.path.join(ROOT, "haskell", "Sonic", "HIP.hs")).read()
    for name in ("aggregateCore", "fsWeightsDigest", "verifyCoreBatchHelped"):
        assert re.search(r"^%s\s*::" % name, hs, re.M), name
    # the calls that launch kernels and wait for them must not block the runtime's capability
    for name in ("sonic_prover_aggregate_core", "sonic_verifier_verify_core_batch_helped"):
        assert re.search(r'foreign import ccall\s+safe\s+"%s"' % name, hs), name
    for knob in ("SONIC_AGG_KEEP",):
        assert knob in open(os.path.join(ROOT, "README.md")).read(), knob


def test_the_helper_checks_its_arguments_before_it_needs_a_device():
    from sonic_amd import _lib
    L = _lib.lib()
    n = C.c_int(0)
    want = 6 if L.sonic_device_count(C.byref(n)) == 6 else 7
    assert L.sonic_prover_aggregate_core(None, bytes(32), 1, bytes(64), C.create_string_buffer(aref.aggregate_size(1))) == want
    ok = C.c_int(1)
    buf = bytes(576)
    assert L.sonic_verifier_verify_core_batch_helped(None, 1, buf, 0, bytes(64), None, bytes(aref.aggregate_size(1)), None, C.byref(ok), None) == want and ok.value == 0
    ok.value = 1
    assert L.sonic_verifier_verify_core_fs_batch_helped(None, 1, buf, 0, None, bytes(aref.aggregate_size(1)), None, C.byref(ok), None) == want and ok.value == 0
