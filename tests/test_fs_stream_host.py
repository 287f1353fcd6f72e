"""Fiat-Shamir proofs in flight, the parts that need no GPU (include/sonic_hip.h, "Fiat-Shamir proofs in flight"): witness digest v2 -- the
SHA-256 tree of sonic_amd/csrc/witness_tree.hpp, the text the kernels of witness.hip compile -- driven on the host by a stand-alone program
built plain and under ASan / UBSan (tests/host/fs_stream_host.cpp) against a hashlib restatement (tests/fs_stream_ref.py), its compression
function against sha256.hpp, and the header / exports / bindings.  Every comparison is byte equality."""
import ctypes as C
import hashlib
import os
import random
import re
import subprocess

import pytest

import fs_stream_ref as fref
from util import R

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
HOST = os.path.join(HERE, "host")
ENV = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
# n -> (leaves, the node levels above them): one partial leaf; 30 elements; 33 elements, leaf 0 spans aL, aR and aO; three full leaves; 32
# leaves under exactly one node; 33 leaves: two nodes, then one; 1024 leaves: 32 nodes, then one; 1025 leaves: 33, 2, 1
TREE_SHAPES = {1: (1, []), 10: (1, []), 11: (2, [1]), 32: (3, [1]), 341: (32, [1]), 342: (33, [2, 1]), 10922: (1024, [32, 1]), 10923: (1025, [33, 2, 1])}
SHA_LENGTHS = [0, 55, 56, 63, 64, 119, 120, 1088]
NEW_SYMBOLS = ["sonic_prover_witness_digest_v2", "sonic_prover_submit_fs", "sonic_prover_collect_fs", "sonic_prove_batch_fs"]


def test_restatement_has_the_shapes_the_cases_are_named_for():
    for n, (leaves, nodes) in TREE_SHAPES.items():
        levels = fref.witness_levels(bytes(96 * n))
        assert [len(lv) for lv in levels] == [leaves] + nodes, n
    # leaf 0 of n = 11 holds all of aL, all of aR and ten elements of aO
    assert 2 * 11 < 32 < 3 * 11
    # a header is one SHA block, so every later block is two whole elements
    assert len(fref.leaf_header(5)) == 64 and len(fref.node_header(2, 7)) == 64
    assert fref.leaf_header(5)[56:] == (5).to_bytes(8, "little") and fref.node_header(2, 7)[48:] == (2).to_bytes(8, "little") + (7).to_bytes(8, "little")


@pytest.fixture(scope="module")
def drivers():
    subprocess.check_call(["make", "-C", HOST, "-s", "-f", "fs_stream.mk", "fs_stream_host", "fs_stream_host_san"])
    return {"plain": os.path.join(HOST, "fs_stream_host"), "san": os.path.join(HOST, "fs_stream_host_san")}


def run_driver(path, lines):
    out = subprocess.run([path], input="\n".join(lines) + "\n", capture_output=True, text=True, timeout=600, env=ENV)
    assert out.returncode == 0 and out.stdout.endswith("fs_stream_host ok\n"), out.stdout[-2000:] + out.stderr[-3000:]
    return out.stdout.splitlines()[:-1]


@pytest.mark.parametrize("build", ["plain", "san"])
def test_host_program_tree_matches_the_restatement(drivers, build):
    lines, want = [], []
    seed, cd, sid = b"\x07" * 32, b"\x01" * 32, b"\x02" * 32
    for n in TREE_SHAPES:
        aL, aR, aO = fref.assignment_values(n)
        assert 0 in aL + aR + aO and R - 1 in aL + aR + aO
        lines.append("tree %d %s" % (n, fref.witness_bytes(aL, aR, aO).hex()))
        dg = fref.witness_digest_v2(aL, aR, aO)
        want.append("%s %s %s" % (fref.witness_root(aL, aR, aO).hex(), dg.hex(), fref.fr(fref.blinders(seed, cd, sid, dg)[0]).hex()))
    got = run_driver(drivers[build], lines)
    assert len(got) == len(want)
    for n, g, w in zip(TREE_SHAPES, got, want):
        assert g == w, n
    assert len({w.split()[1] for w in want}) == len(want)


@pytest.mark.parametrize("build", ["plain", "san"])
def test_compression_function_matches_sha256_hpp_and_hashlib(drivers, build):
    pyr = random.Random(5)
    msgs = [pyr.randbytes(k) for k in SHA_LENGTHS]
    got = run_driver(drivers[build], ["sha %s" % (m.hex() or "-") for m in msgs])
    for m, g in zip(msgs, got):
        ours, theirs = g.split()
        assert ours == theirs == hashlib.sha256(m).hexdigest(), len(m)


def test_digest_moves_with_one_element_and_with_n():
    aL, aR, aO = fref.assignment_values(342)
    d0 = fref.witness_digest_v2(aL, aR, aO)
    bumped = list(aO)
    bumped[-1] = (bumped[-1] + 1) % R
    assert fref.witness_digest_v2(aL, aR, bumped) != d0
    # the tree sees one string of bytes; n is hashed on top of its root
    root = fref.witness_levels(b"".join(fref.fr(v) for v in aL + aR + aO))[-1][0]
    assert root == fref.witness_root(aL, aR, aO)
    assert d0 == hashlib.sha256(b"sonic-hip/witness/v2" + fref.le64(342) + root).digest() != hashlib.sha256(b"sonic-hip/witness/v2" + fref.le64(343) + root).digest()


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
    assert all(hasattr(sonic_amd.Prover, m) for m in ("submit_fs", "collect_fs", "witness_digest"))
    assert callable(sonic_amd.prove_batch_fs)
    hs = open(os.path.join(ROOT, "haskell", "Sonic", "HIP.hs")).read()
    for name in ("submitFs", "collectFs", "proveBatchFs", "witnessDigest"):
        assert re.search(r"^%s\s*::" % name, hs, re.M), name


def test_device_calls_report_no_device_without_one():
    """(on a box with a GPU the same calls report the NULL handle instead)"""
    from sonic_amd import _lib
    L = _lib.lib()
    n = C.c_int(0)
    want = 6 if L.sonic_device_count(C.byref(n)) == 6 else 7
    buf = C.create_string_buffer(64)
    assert L.sonic_prover_witness_digest_v2(None, buf) == want
    assert L.sonic_prover_submit_fs(None, bytes(32), bytes(32)) == want
    assert L.sonic_prover_collect_fs(None, buf, None) == want
    assert L.sonic_prove_batch_fs(None, 1, 1, None, None, None, None, buf, buf, buf, None, None) == want
