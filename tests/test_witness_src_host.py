"""Witness sources, the parts that need no GPU (include/sonic_hip.h, "Witness sources"): the int64 -> Fr conversion of
sonic_amd/csrc/witness_src.hpp -- the text the kernel of witness_src.hip compiles -- and the checks of a sonic_witness_src_t that are host
code, driven by a stand-alone program built plain and under ASan / UBSan (tests/host/witness_src_host.cpp); the expected bytes are Python
integers mod r.  Then the header / exports / bindings, the Python argument checks, and the refusal without a device.  Negating INT64_MIN in
signed arithmetic is undefined behaviour: the sanitized build is the one that would say so."""
import ctypes as C
import os
import random
import re
import subprocess

import numpy as np
import pytest

from util import R

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
HOST = os.path.join(HERE, "host")
ENV = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
NEW_SYMBOLS = ["sonic_prover_set_witness", "sonic_prover_eval_constraints_src", "sonic_prove_batch_src", "sonic_prove_batch_fs_src"]
I64_MAX, I64_MIN = (1 << 63) - 1, -(1 << 63)
I64_VALUES = [0, 1, -1, I64_MAX, -I64_MAX, I64_MIN, 2, -2, 1 << 32, -(1 << 32), (1 << 32) - 1, -((1 << 32) - 1)] + \
             [random.Random(64).randrange(I64_MIN, I64_MAX + 1) for _ in range(8)]


@pytest.fixture(scope="module")
def drivers():
    subprocess.check_call(["make", "-C", HOST, "-s", "-f", "witness_src.mk", "witness_src_host", "witness_src_host_san"])
    return {"plain": os.path.join(HOST, "witness_src_host"), "san": os.path.join(HOST, "witness_src_host_san")}


def run_driver(path, lines):
    out = subprocess.run([path], input="\n".join(lines) + "\n", capture_output=True, text=True, timeout=600, env=ENV)
    assert out.returncode == 0 and out.stdout.endswith("witness_src_host ok\n"), out.stdout[-2000:] + out.stderr[-3000:]
    return out.stdout.splitlines()[:-1]


@pytest.mark.parametrize("build", ["plain", "san"])
def test_i64_to_fr_matches_python_integers(drivers, build):
    got = run_driver(drivers[build], ["i64 %d" % v for v in I64_VALUES])
    assert len(got) == len(I64_VALUES)
    for v, g in zip(I64_VALUES, got):
        want = (v % R).to_bytes(32, "little").hex()
        assert g.split() == [want, want], v
    # what the header says in words
    assert (I64_MIN % R) == R - (1 << 63) and (-1 % R) == R - 1


# (kind, on_device, aL, aR, aO, stride, stream, n, B) -> the verdict: (resolved stride) or a word of the message
A = 1 << 20          # an address with every alignment
SRC_CASES = [
    ((0, 0, A + 1, A + 3, A + 5, 0, 0, 4, 1), 128),                    # host: any alignment, packed
    ((0, 0, A, A, 0, 0, 0, 4, 3), 128),                                # aO derived
    ((1, 0, A + 1, A + 2, 0, 0, 0, 4, 3), 32),
    ((0, 1, A, A + 32, A + 64, 160, 0, 4, 3), 160),                    # device: aligned, strided
    ((1, 1, A, A + 8, 0, 40, 77, 4, 3), 40),
    ((0, 1, A + 8, A, A, 0, 0, 4, 1), "aL is not 32-byte aligned"),    # misaligned by 8
    ((0, 1, A, A + 16, A, 0, 0, 4, 1), "aR is not 32-byte aligned"),
    ((0, 1, A, A, A + 24, 0, 0, 4, 1), "aO is not 32-byte aligned"),
    ((1, 1, A + 4, A, 0, 0, 0, 4, 1), "aL is not 8-byte aligned"),
    ((0, 1, A, A, A, 136, 0, 4, 2), "not a multiple of 32"),
    ((1, 1, A, A, 0, 36, 0, 4, 2), "not a multiple of 8"),
    ((0, 0, A, A, A, 96, 0, 4, 2), "below n * element size"),
    ((0, 0, A, A, A, -128, 0, 4, 2), "below n * element size"),
    ((2, 0, A, A, A, 0, 0, 4, 1), "unknown kind 2"),
    ((-1, 0, A, A, A, 0, 0, 4, 1), "unknown kind -1"),
    ((0, 2, A, A, A, 0, 0, 4, 1), "on_device = 2"),
    ((0, 0, 0, A, A, 0, 0, 4, 1), "aL and aR must be given"),
    ((0, 0, A, 0, 0, 0, 0, 4, 1), "aL and aR must be given"),
    ((0, 0, A, A, A, 0, 77, 4, 1), "hip_stream is for device sources"),
    ((0, 0, A, A, A, 0, 0, 4, 0), "at least one assignment"),
]


@pytest.mark.parametrize("build", ["plain", "san"])
def test_description_checks(drivers, build):
    got = run_driver(drivers[build], ["src " + " ".join(str(x) for x in case) for case, _ in SRC_CASES] + ["null"])
    assert len(got) == len(SRC_CASES) + 1
    for (case, want), g in zip(SRC_CASES, got):
        if isinstance(want, int):
            assert g == "0 %d %d %d" % (case[0], case[1], want), (case, g)
        else:
            assert g.startswith("7 ") and want in g, (case, g)
    assert got[-1].startswith("7 ") and "NULL" in got[-1]


# ---- header, exports, bindings ----
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
    assert "#define SONIC_WIT_FR32 0" in hdr and re.search(r"#define SONIC_WIT_I64\s+1", hdr) and (L.WIT_FR32, L.WIT_I64) == (0, 1)
    # the struct as the header lays it out: three pointers, two int32, an int64, a pointer
    assert C.sizeof(L.WitnessSrc) == 48 and [f[0] for f in L.WitnessSrc._fields_] == ["aL", "aR", "aO", "kind", "on_device", "stride", "hip_stream"]
    assert (L.WitnessSrc.kind.offset, L.WitnessSrc.on_device.offset, L.WitnessSrc.stride.offset, L.WitnessSrc.hip_stream.offset) == (24, 28, 32, 40)
    assert hasattr(sonic_amd.Prover, "set_witness") and callable(sonic_amd.WitnessBatch)
    hs = open(os.path.join(ROOT, "haskell", "Sonic", "HIP.hs")).read()
    for name in ("setWitnessI64", "proveBatchI64"):
        assert re.search(r"^%s\s*::" % name, hs, re.M), name
    assert "instance Storable WitnessSrc" in hs and "sizeOf _    = 48" in hs


def test_the_three_documents_state_the_rules_in_the_same_words():
    """the struct, the ordering rule and the lifetime rule: README, DESIGN.md and the header"""
    texts = [" ".join(re.sub(r"^\s*(\*|//|--)\s?", "", ln) for ln in open(os.path.join(ROOT, p)).read().splitlines())
             for p in ("include/sonic_hip.h", "README.md", "DESIGN.md")]
    texts = [re.sub(r"\s+", " ", t).replace("`", "") for t in texts]
    for sentence in ("The source is only read, and it must stay unchanged until the call returns; every call here is blocking.",
                     "With a non-NULL hip_stream the library records an event on that stream at entry, and the handle's stream (each handle's, in a batch) waits on that event before it reads the source.",
                     "With NULL the caller states that the data is complete.",
                     "The library never makes the caller's stream wait.",
                     "A device source must lie on the GPU of every handle that reads it"):
        for name, t in zip(("header", "README", "DESIGN"), texts):
            assert sentence in t, (name, sentence)
    for name, t in zip(("header", "README", "DESIGN"), texts):
        for field in ("const void *aL, *aR, *aO;", "int32_t kind;", "int32_t on_device;", "int64_t stride;", "hip_stream;"):
            assert field in t, (name, field)


# ---- the Python argument checks: ValueError before any C call (no device is needed to get there) ----
def _src(*a, **k):
    from sonic_amd.protocol import _witness_src
    return _witness_src(*a, **k)


def test_python_forms_and_value_errors():
    from sonic_amd import _lib as L
    n = 5
    fr = np.zeros((n, 32), np.uint8)
    i64 = np.arange(n, dtype=np.int64)
    s, _ = _src(fr, fr, fr, None, n, None, [0], "t")
    assert (s.kind, s.on_device, s.stride, s.hip_stream, s.aL) == (L.WIT_FR32, 0, 32 * n, None, fr.ctypes.data)
    s, _ = _src(i64, i64, None, None, n, None, [0], "t")
    assert (s.kind, s.on_device, s.stride, s.aO) == (L.WIT_I64, 0, 8 * n, None)
    s, keep = _src(list(range(n)), [R - 1] * n, None, None, n, None, [0], "t")          # lists: the existing conversion
    assert s.kind == L.WIT_FR32 and keep[1][0].tobytes() == (R - 1).to_bytes(32, "little")
    big = np.zeros((3, 2 * n), np.int64)
    s, _ = _src(big[:, :n], big[:, :n], None, None, n, 3, [0], "t")                     # a leading stride beyond n
    assert (s.kind, s.stride) == (L.WIT_I64, 16 * n)
    import torch
    t = torch.zeros((3, n, 32), dtype=torch.uint8)
    s, _ = _src(t, t, t, None, n, 3, [0], "t")
    assert (s.kind, s.on_device, s.stride, s.aL) == (L.WIT_FR32, 0, 32 * n, t.data_ptr())
    ti = torch.zeros((3, 2 * n), dtype=torch.int64)[:, :n]
    assert _src(ti, ti, None, None, n, 3, [0], "t")[0].stride == 16 * n
    bad = [
        lambda: _src(fr, i64, None, None, n, None, [0], "t"),                            # mixed kinds
        lambda: _src(fr, fr[:4], None, None, n, None, [0], "t"),                         # wrong shape
        lambda: _src(fr.astype(np.int32), fr.astype(np.int32), None, None, n, None, [0], "t"),      # wrong dtype
        lambda: _src(i64.astype(np.uint64), i64.astype(np.uint64), None, None, n, None, [0], "t"),
        lambda: _src(big[0, ::2], big[0, ::2], None, None, n, None, [0], "t"),           # inner dimension not contiguous
        lambda: _src(np.zeros((n, 64), np.uint8)[:, :32], fr, None, None, n, None, [0], "t"),
        lambda: _src(fr, fr, None, None, n, 3, [0], "t"),                                # a batch needs the leading dimension
        lambda: _src([1] * n, [1] * n, None, None, n, 3, [0], "t"),                      # lists are not batches
        lambda: _src(big[:, :n], np.zeros((3, n), np.int64), None, None, n, 3, [0], "t"),           # two leading strides
        lambda: _src(fr, fr, None, 5, n, None, [0], "t"),                                # a stream with host memory
        lambda: _src(torch.zeros((n, 32), dtype=torch.float32), fr, None, None, n, None, [0], "t"),
    ]
    for k, call in enumerate(bad):
        with pytest.raises(ValueError):
            call()
            pytest.fail("case %d was accepted" % k)


def test_device_calls_report_no_device_without_one():
    """(on a box with a GPU the same calls report the NULL handle instead)"""
    from sonic_amd import _lib
    L = _lib.lib()
    n = C.c_int(0)
    want = 6 if L.sonic_device_count(C.byref(n)) == 6 else 7
    buf = C.create_string_buffer(64)
    src = _lib.WitnessSrc()
    assert L.sonic_prover_set_witness(None, C.byref(src)) == want
    assert L.sonic_prover_eval_constraints_src(None, 1, C.byref(src), buf, None) == want
    assert L.sonic_prove_batch_src(None, 1, 1, C.byref(src), None, buf, buf, None) == want
    assert L.sonic_prove_batch_fs_src(None, 1, 1, C.byref(src), None, buf, buf, buf, None, None) == want
