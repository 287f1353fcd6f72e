"""The batched verifier, the parts that need no GPU (include/sonic_hip.h, "the batched verifier"): the randomizer derivation against a
hashlib restatement, the fold as mathematics over oracle/pairing.py on the golden proofs, and the header / bindings.

Reference: Sonic.Protocol.verify (src/Sonic/Protocol.hs:111-130), hscVerify (src/Sonic/Signature.hs:74-90), pcV
(src/Sonic/CommitmentScheme.hs:51-68)."""
import ctypes as C
import hashlib
import json
import os
import re

import pytest

import batch_ref
from util import R

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CASES = json.load(open(os.path.join(HERE, "golden", "prove_small.json")))["cases"]

NEW_SYMBOLS = ["sonic_verifier_new", "sonic_verifier_new_csr", "sonic_verifier_free", "sonic_verifier_device", "sonic_verifier_verify_batch",
               "sonic_verifier_verify_fs_batch", "sonic_verifier_eval_s", "sonic_g1_validate", "sonic_verify_batch_randomizers"]


def _lib():
    from sonic_amd import _lib as L
    return L


@pytest.mark.parametrize("count", [0, 1, 2, 33, 1000])
def test_randomizers_match_the_hashlib_restatement(count):
    """rho_i = 128 bits of SHA-256("sonic-hip/batch/v1" || seed || D || le64 i), 0 replaced by 1: several seeds, digests and counts"""
    lib = _lib().lib()
    for s in range(3):
        seed = hashlib.sha256(b"seed%d" % s).digest() if s else bytes(32)
        D = hashlib.sha256(b"digest%d" % (s * 7 + count)).digest()
        out = C.create_string_buffer(max(16 * count, 1))
        assert lib.sonic_verify_batch_randomizers(seed, D, count, out) == 0
        got = [int.from_bytes(out.raw[16 * i:16 * i + 16], "little") for i in range(count)]
        assert got == batch_ref.randomizers(seed, D, count)
        assert all(0 < r < 1 << 128 for r in got)
        assert len(set(got)) == count
    assert lib.sonic_verify_batch_randomizers(None, bytes(32), 1, C.create_string_buffer(16)) == 7      # SONIC_ERR_INVALID_ARG


def _case(name):
    from oracle import pairing as pg
    c = next(x for x in CASES if x["name"] == name)
    Q = c["Q"]
    ints = lambda rows: [[int(v, 16) for v in row] for row in rows]      # noqa: E731
    circuit = (ints(c["wL"]), ints(c["wR"]), ints(c["wO"]), [int(v, 16) for v in c["cs"]])
    tr = [int(v, 16) for v in c["transcript"]]
    y, z, yzs = tr[4], tr[5], list(zip(tr[6:6 + Q], tr[6 + Q:6 + 2 * Q]))
    srs = pg.SRS(c["d"], int(c["x"], 16), int(c["alpha"], 16))
    return c, srs, circuit, pg.proof_from_bytes(bytes.fromhex(c["proof"]), Q), y, z, yzs


def test_the_fold_accepts_the_golden_proof_and_rejects_a_changed_value():
    """the fold restated in Python (tests/batch_ref.py over oracle/pairing.py): four Miller loops per case.  It accepts a golden proof
    under derived randomizers, and rejects it with one opened value changed and with one opening moved by the generator."""
    from oracle import sonic_ref as ref
    c, srs, circuit, proof, y, z, yzs = _case(CASES[0]["name"])
    checks = batch_ref.checks_of(circuit, c["d"], proof, y, z, yzs)
    assert len(checks) == 4 + 3 * c["Q"]
    assert sorted({m for m, *_ in checks}) == sorted({c["n"], c["d"]})
    rhos = batch_ref.randomizers(bytes(32), hashlib.sha256(bytes.fromhex(c["proof"])).digest(), len(checks))
    assert batch_ref.fold_accepts(srs, checks, rhos)
    bad = dict(proof, prA=(proof["prA"] + 1) % R)
    assert not batch_ref.fold_accepts(srs, batch_ref.checks_of(circuit, c["d"], bad, y, z, yzs), rhos)
    bad = dict(proof, prWt=ref.g1_add(proof["prWt"], ref.G1_GEN))
    assert not batch_ref.fold_accepts(srs, batch_ref.checks_of(circuit, c["d"], bad, y, z, yzs), rhos)


def test_unit_randomizers_miss_errors_that_cancel():
    """why the randomizers must be real: W_a + D and W_t - D inside one proof (both opened at z) pass an UNWEIGHTED sum and fail the fold"""
    from oracle import sonic_ref as ref
    c, srs, circuit, proof, y, z, yzs = _case(CASES[0]["name"])
    D = ref.g1_mul(ref.G1_GEN, 5)
    bad = dict(proof, prWa=ref.g1_add(proof["prWa"], D), prWt=ref.g1_add(proof["prWt"], ref.g1_neg(D)))
    checks = batch_ref.checks_of(circuit, c["d"], bad, y, z, yzs)
    assert batch_ref.fold_accepts(srs, checks, [1] * len(checks))
    assert not batch_ref.fold_accepts(srs, checks, batch_ref.randomizers(bytes(32), bytes(32), len(checks)))


def test_header_and_bindings():
    hdr = open(os.path.join(ROOT, "include", "sonic_hip.h")).read()
    L = _lib()
    lib = L.lib()
    for name in NEW_SYMBOLS:
        assert re.search(r"\b(int|void)\s+%s\s*\(" % name, hdr), name
        assert name in L.EXPORTED and hasattr(lib, name), name
        assert getattr(lib, name).argtypes is not None, name
    assert "typedef struct sonic_verifier sonic_verifier_t;" in hdr
    assert "#define SONIC_ABI_VERSION 7" in hdr and lib.sonic_abi_version() == 7 and L.ABI_VERSION == 7
    import sonic_amd
    assert callable(sonic_amd.verify_batch) and all(hasattr(sonic_amd.Verifier, m) for m in ("verify_batch", "verify_fs_batch", "eval_s", "close"))


def test_python_restatement_of_s_of_uv_matches_the_polynomial():
    """tests/batch_ref.s_of_uv (the yardstick of the GPU test at larger n) against eval_y(v, eval_x(u, s_poly)) of the reference"""
    import random
    from oracle import sonic_ref as ref
    pyr = random.Random(5)
    for n, Q in ((1, 1), (5, 2), (16, 3)):
        (wL, wR, wO, cs), _ = ref.rnd_circuit(pyr, n, Q)
        sXY = ref.s_poly(wL, wR, wO)
        for u, v in ((pyr.randrange(1, R), pyr.randrange(1, R)), (1, 7), (9, 9), (3, pow(3, -1, R))):
            want = ref.lp_eval(ref.eval_y(v, sXY), u)
            assert batch_ref.s_of_uv(n, Q, batch_ref.dense_rows(wL, wR, wO), u, v) == want
