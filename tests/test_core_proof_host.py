"""Core proofs, the parts that need no GPU (include/sonic_hip.h, "Core proofs"): the layout, record order and repack of
sonic_amd/csrc/proof_layout.hpp, the core transcript and the batch digest of fs.hpp -- driven on the host by a stand-alone program built plain
and under ASan / UBSan (tests/host/core_proof_host.cpp) against the hashlib restatement in tests/core_proof_ref.py -- the host-only library
calls against the same restatement, and the header / exports / bindings / no-device statuses.  Every comparison is byte equality."""
import ctypes as C
import os
import random
import re
import subprocess

import pytest

import core_proof_ref as cref
from util import R

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
HOST = os.path.join(HERE, "host")
ENV = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
NEW_SYMBOLS = ["sonic_prover_prove_core", "sonic_prover_submit_core", "sonic_prover_collect_core", "sonic_prover_prove_core_fs", "sonic_fs_core_challenges",
               "sonic_prove_batch_core_src", "sonic_prove_batch_core_fs_src", "sonic_verify_core", "sonic_verify_core_csr", "sonic_verify_core_fs",
               "sonic_verify_core_fs_csr", "sonic_verifier_verify_core_batch", "sonic_verifier_verify_core_fs_batch", "sonic_verify_core_batch_digest",
               "sonic_core_proof_compress", "sonic_core_proof_decompress"]
# (n, Q, d, K) of the transcript and digest cases: the smallest circuit, Q > 1, a K that is no power of two
SHAPES = [(1, 1, 8, 1), (5, 2, 64, 3), (257, 5, 4096, 17)]


@pytest.fixture(scope="module")
def drivers():
    subprocess.check_call(["make", "-C", HOST, "-s", "-f", "core_proof.mk", "core_proof_host", "core_proof_host_san"])
    return {"plain": os.path.join(HOST, "core_proof_host"), "san": os.path.join(HOST, "core_proof_host_san")}


def run_driver(path, lines):
    out = subprocess.run([path], input="\n".join(lines) + "\n", capture_output=True, text=True, timeout=600, env=ENV)
    assert out.returncode == 0 and out.stdout.endswith("core_proof_host ok\n"), out.stdout[-2000:] + out.stderr[-3000:]
    return out.stdout.splitlines()[:-1]


def cases(seed):
    """per shape: digest, srs id, K proofs (random bytes: the transcript reads them as bytes), K (y, z), K constants"""
    pyr = random.Random(seed)
    out = []
    for n, Q, d, K in SHAPES:
        proofs = [pyr.randbytes(cref.CORE_SIZE) for _ in range(K)]
        yzs = [(pyr.randrange(R), pyr.randrange(R)) for _ in range(K)]
        cs = [b"".join(cref.fr(pyr.randrange(R)) for _ in range(Q)) for _ in range(K)]
        out.append((n, Q, d, K, pyr.randbytes(32), pyr.randbytes(32), proofs, yzs, cs))
    return out


@pytest.mark.parametrize("build", ["plain", "san"])
def test_layout_record_order_and_repack(drivers, build):
    for Q in (1, 2, 5, 64):
        got = run_driver(drivers[build], ["layout %d" % Q])
        counts = {ln.split()[1]: int(ln.split()[2]) for ln in got if ln.startswith("count ")}
        assert counts == {"core_K": 5, "core_F": 3, "core_transcript_len": 6, "core_proof_bytes": cref.CORE_SIZE, "core_proof_bytes_compressed": cref.CORE_SIZE_Z}

        def fields(tag):
            return [(int(a), k, int(i)) for t, a, k, i in (ln.split() for ln in got if ln.startswith(tag + " "))]
        assert fields("field") == cref.field_offsets(96)
        # a core proof IS the first 576 bytes of the full record, whatever Q is
        assert fields("head") == cref.field_offsets(96)
        assert fields("z") == cref.field_offsets(48)
        # 96 -> 48 accepted; 48 -> 96 with the second point refused: false, all five points still visited, s carried over
        assert [ln for ln in got if ln.startswith("repack ")] == ["repack 1 0 5 1"]
    assert cref.field_offsets(96)[-1][0] + 32 == cref.CORE_SIZE and cref.field_offsets(48)[-1][0] + 32 == cref.CORE_SIZE_Z
    assert [cref.OFFSETS[k] for k in ("R", "T", "a", "Wa", "b", "Wb", "Wt", "s")] == [a for a, _, _ in cref.field_offsets(96)]


@pytest.mark.parametrize("build", ["plain", "san"])
def test_transcript_and_batch_digest_match_hashlib(drivers, build):
    lines, want = [], []
    for n, Q, d, K, dg, sid, proofs, yzs, cs in cases(11):
        for p in proofs[:2]:
            lines.append("chal %d %d %d %s %s %s" % (n, Q, d, dg.hex(), sid.hex(), p.hex()))
            y, z = cref.core_challenges(n, Q, d, dg, sid, p)
            assert (y, z) != cref.full_challenges_yz(n, Q, d, dg, sid, p)          # its own label: never a full proof's challenges
            want.append((cref.fr(y) + cref.fr(z)).hex())
        lines.append("bdigest %d %d %d %s %s %d %s %s %s" % (n, Q, d, dg.hex(), sid.hex(), K, b"".join(proofs).hex(),
                                                             b"".join(cref.fr(y) + cref.fr(z) for y, z in yzs).hex(), b"".join(cs).hex()))
        want.append(cref.core_batch_digest(n, Q, d, dg, sid, proofs, yzs, cs).hex())
    assert run_driver(drivers[build], lines) == want
    assert len(set(want)) == len(want)


def test_library_host_calls_match_hashlib():
    """sonic_fs_core_challenges and sonic_verify_core_batch_digest need no device"""
    from sonic_amd import _lib
    L = _lib.lib()
    for n, Q, d, K, dg, sid, proofs, yzs, cs in cases(12):
        out = C.create_string_buffer(64)
        assert L.sonic_fs_core_challenges(n, Q, d, dg, sid, proofs[0], out) == 0
        y, z = cref.core_challenges(n, Q, d, dg, sid, proofs[0])
        assert out.raw == cref.fr(y) + cref.fr(z)
        D = C.create_string_buffer(32)
        yz = b"".join(cref.fr(a) + cref.fr(b) for a, b in yzs)
        assert L.sonic_verify_core_batch_digest(n, Q, d, dg, sid, K, b"".join(proofs), yz, b"".join(cs), D) == 0
        assert D.raw == cref.core_batch_digest(n, Q, d, dg, sid, proofs, yzs, cs)
        # every part is bound: one bit of a proof, of a challenge, of a constant, and K
        for i, blob in enumerate((b"".join(proofs), yz, b"".join(cs))):
            parts = [b"".join(proofs), yz, b"".join(cs)]
            parts[i] = bytes([blob[0] ^ 1]) + blob[1:]
            D2 = C.create_string_buffer(32)
            assert L.sonic_verify_core_batch_digest(n, Q, d, dg, sid, K, *parts, D2) == 0 and D2.raw != D.raw
    assert L.sonic_fs_core_challenges(0, 1, 8, bytes(32), bytes(32), bytes(576), C.create_string_buffer(64)) == 7
    assert L.sonic_verify_core_batch_digest(1, 1, 8, bytes(32), bytes(32), 1, None, bytes(64), bytes(32), C.create_string_buffer(32)) == 7


def test_compress_roundtrip_and_refusals_on_the_host():
    """sonic_core_proof_compress / _decompress are host code: a record of points at infinity round-trips, a point off the curve and a
    non-canonical field element are refused (real points: tests/test_gpu_core_proofs.py)"""
    from sonic_amd import _lib, CoreProof
    L = _lib.lib()
    inf = bytes(96)
    fr = cref.fr
    raw = inf + inf + fr(1) + inf + fr(R - 1) + inf + inf + fr(7)
    z = C.create_string_buffer(cref.CORE_SIZE_Z)
    assert L.sonic_core_proof_compress(raw, z) == 0
    assert [z.raw[a:a + 48] for a, k, _ in cref.field_offsets(48) if k == "G"] == [b"\xc0" + bytes(47)] * 5
    back = C.create_string_buffer(cref.CORE_SIZE)
    assert L.sonic_core_proof_decompress(z.raw, back) == 0 and back.raw == raw
    assert CoreProof.from_bytes(z.raw).to_bytes() == raw and CoreProof.from_bytes(raw).to_bytes(compressed=True) == z.raw
    # (1, 1) is not on y^2 = x^3 + 4
    bad = (1).to_bytes(48, "little") + (1).to_bytes(48, "little")
    assert L.sonic_core_proof_compress(bad + raw[96:], z) == 3
    # a non-canonical s is refused by decompress as the verifiers refuse it
    zs = bytearray(z.raw)
    zs[304:336] = fr(R)
    assert L.sonic_core_proof_decompress(bytes(zs), back) == 3
    assert L.sonic_core_proof_compress(None, z) == 7 and L.sonic_core_proof_decompress(z.raw, None) == 7


# ---- header, exports, bindings, and no device ----
def test_header_declares_library_exports_python_binds():
    from sonic_amd import _lib as L
    import sonic_amd
    hdr = open(os.path.join(ROOT, "include", "sonic_hip.h")).read()
    lib = L.lib()
    for name in NEW_SYMBOLS:
        assert re.search(r"\bint\s+%s\s*\(" % name, hdr), name
        assert name in L.EXPORTED and hasattr(lib, name), name
        assert getattr(lib, name).argtypes is not None, name
    assert "#define SONIC_ABI_VERSION 7" in hdr and lib.sonic_abi_version() == 7 and L.ABI_VERSION == 7
    assert "#define SONIC_CORE_PROOF_SIZE 576" in hdr and "#define SONIC_CORE_PROOF_SIZE_COMPRESSED 336" in hdr
    assert (L.CORE_PROOF_SIZE, L.CORE_PROOF_SIZE_COMPRESSED) == (cref.CORE_SIZE, cref.CORE_SIZE_Z)
    assert all(hasattr(sonic_amd.Prover, m) for m in ("prove_core_bytes", "submit_core", "collect_core", "prove_core_fs"))
    assert all(hasattr(sonic_amd.Verifier, m) for m in ("verify_core_batch", "verify_core_fs_batch"))
    assert all(callable(getattr(sonic_amd, f)) for f in ("prove_core_batch", "prove_core_batch_fs", "verify_core", "verify_core_fs", "fs_core_challenges"))
    assert hasattr(sonic_amd.Proof, "core") and hasattr(sonic_amd.CoreProof, "from_bytes")
    hs = open(os.path.join(ROOT, "haskell", "Sonic", "HIP.hs")).read()
    for name in ("proveCore", "submitCore", "collectCore", "proveCoreFs", "verifyCore", "verifyCoreBatch"):
        assert re.search(r"^%s\s*::" % name, hs, re.M), name


def test_device_calls_report_no_device_without_one():
    """(on a box with a GPU the same calls report the NULL handle instead)"""
    from sonic_amd import _lib
    L = _lib.lib()
    n = C.c_int(0)
    want = 6 if L.sonic_device_count(C.byref(n)) == 6 else 7
    buf = C.create_string_buffer(cref.CORE_SIZE)
    ok = C.c_int(1)
    assert L.sonic_prove_batch_core_src(None, 1, 1, None, None, buf, buf, None) == want
    assert L.sonic_prove_batch_core_fs_src(None, 1, 1, None, None, buf, buf, buf, None, None) == want
    assert L.sonic_verifier_verify_core_batch(None, 1, buf, 0, buf, None, None, C.byref(ok), None) == want and ok.value == 0
    ok.value = 1
    assert L.sonic_verifier_verify_core_fs_batch(None, 1, buf, 0, None, None, C.byref(ok), None) == want and ok.value == 0
    # the calls on one handle check their arguments first, as sonic_prover_prove / submit / collect do
    assert L.sonic_prover_prove_core(None, buf, buf) == 7 and L.sonic_prover_submit_core(None, buf) == 7 and L.sonic_prover_collect_core(None, buf) == 7
    assert L.sonic_prover_prove_core_fs(None, bytes(32), bytes(32), buf, None) == 7
    assert L.sonic_verify_core(None, 1, 1, buf, buf, buf, buf, buf, bytes(32), bytes(32), C.byref(ok)) == 7


def test_c99_harness_compiles_against_the_header_alone(tmp_path):
    """tests/host/core_proof_harness.c under -std=c99 -pedantic -Werror; without a GPU it says so and exits 77 (with one: tests/test_gpu_core_proofs.py)"""
    exe = str(tmp_path / "core_proof_harness")
    subprocess.check_call(["gcc", "-std=c99", "-pedantic", "-Wall", "-Wextra", "-Werror", "-I" + os.path.join(ROOT, "include"),
                           os.path.join(HOST, "core_proof_harness.c"), "-L" + os.path.join(ROOT, "sonic_amd", "csrc"), "-lsonic_hip",
                           "-Wl,-rpath," + os.path.join(ROOT, "sonic_amd", "csrc"), "-o", exe])
    from sonic_amd import _lib
    n = C.c_int(0)
    if _lib.lib().sonic_device_count(C.byref(n)) == 6:
        out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
        assert out.returncode == 77 and "SONIC_ERR_NO_DEVICE" in out.stderr, out.stdout + out.stderr
