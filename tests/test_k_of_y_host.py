"""k(y) over many blocks, the parts that need no GPU (include/sonic_hip.h, "Circuits with Q ~ n"): the span plan of
sonic_amd/csrc/k_of_y_plan.hpp -- the text the kernels of poly.hip compile -- and the two-stage sum over field.hpp's host arithmetic, driven
by a stand-alone program built plain and under ASan / UBSan (tests/host/k_of_y_host.cpp); and the header / exports / bindings of
sonic_prover_host_bytes.  Every comparison is equality."""
import ctypes as C
import os
import re
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
HOST = os.path.join(HERE, "host")
ENV = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
SPANS = (256, 2048)
NO_DEVICE, INVALID_ARG = 6, 7


def sizes(span):
    return [1, 255, 256, 257, span - 1, span, span + 1, 2 * span, 257 * span + 1]


@pytest.fixture(scope="module")
def drivers():
    subprocess.check_call(["make", "-C", HOST, "-s", "-f", "k_of_y.mk", "k_of_y_host", "k_of_y_host_san"])
    return {"plain": os.path.join(HOST, "k_of_y_host"), "san": os.path.join(HOST, "k_of_y_host_san")}


def run_driver(path, lines):
    out = subprocess.run([path], input="\n".join(lines) + "\n", capture_output=True, text=True, timeout=600, env=ENV)
    assert out.returncode == 0 and out.stdout.endswith("k_of_y_host ok\n"), out.stdout[-2000:] + out.stderr[-3000:]
    return out.stdout.splitlines()[:-1]


@pytest.mark.parametrize("build", ["plain", "san"])
def test_the_plan_covers_every_q_exactly_once_with_no_empty_block(drivers, build):
    cases = [(Q, span) for span in SPANS for Q in sizes(span)]
    got = run_driver(drivers[build], ["plan %d %d" % c for c in cases])
    assert len(got) == len(cases)
    for (Q, span), g in zip(cases, got):
        blocks, first_len, last_len, covered, mn, mx, empty = (int(x) for x in g.split())
        want_blocks = -(-Q // span)
        assert blocks == want_blocks and covered == Q and (mn, mx) == (1, 1) and empty == 0, (Q, span, g)
        assert first_len == min(Q, span) and last_len == Q - (want_blocks - 1) * span and 1 <= last_len <= span, (Q, span, g)
    # the last size is 257 blocks and one term: the second stage loops over more than 256 partials
    assert all(-(-(257 * span + 1) // span) == 258 for span in SPANS)


@pytest.mark.parametrize("build", ["plain", "san"])
def test_the_two_stage_sum_is_the_one_pass_sum(drivers, build):
    cases = [(Q, span, 1000 + 7 * k) for k, (Q, span) in enumerate((Q, span) for span in SPANS for Q in sizes(span))]
    got = run_driver(drivers[build], ["sum %d %d %d" % c for c in cases])
    assert len(got) == len(cases)
    seen = set()
    for c, g in zip(cases, got):
        one_pass, one_block, two_stage = g.split()
        assert len(one_pass) == 64 and one_pass == one_block == two_stage, c
        seen.add(one_pass)
    assert len(seen) == len(cases)                             # (the sums are not all one trivial value)


# ---- header, exports, bindings, and no device ----
def test_host_bytes_is_declared_exported_and_bound():
    from sonic_amd import _lib as L
    import sonic_amd
    hdr = open(os.path.join(ROOT, "include", "sonic_hip.h")).read()
    lib = L.lib()
    name = "sonic_prover_host_bytes"
    assert re.search(r"\bint\s+%s\s*\(\s*sonic_prover_t\s*\*\s*\w+\s*,\s*int64_t\s*\*\s*\w+\s*\)" % name, hdr)
    assert name in L.EXPORTED and hasattr(lib, name) and getattr(lib, name).argtypes is not None
    assert "#define SONIC_ABI_VERSION 7" in hdr and lib.sonic_abi_version() == 7
    assert isinstance(sonic_amd.Prover.host_bytes, property) and isinstance(sonic_amd.Prover.device_bytes, property)
    hs = open(os.path.join(ROOT, "haskell", "Sonic", "HIP.hs")).read()
    assert re.search(r'foreign import ccall\s+safe\s+"%s"' % name, hs)
    assert re.search(r"^proverHostBytes\s*::", hs, re.M) and re.search(r"^\s*, proverHostBytes\b", hs, re.M)
    for knob in ("SONIC_K_OF_Y_SPLIT", "SONIC_K_OF_Y_SPAN"):
        assert knob in hdr and knob in open(os.path.join(ROOT, "README.md")).read(), knob


def test_host_bytes_reports_no_device_without_one():
    """(on a box with a GPU the same call reports the NULL handle instead)"""
    from sonic_amd import _lib
    L = _lib.lib()
    n = C.c_int(0)
    want = NO_DEVICE if L.sonic_device_count(C.byref(n)) == NO_DEVICE else INVALID_ARG
    out = C.c_int64(0)
    assert L.sonic_prover_host_bytes(None, C.byref(out)) == want
    assert L.sonic_prover_device_bytes(None, C.byref(out)) == want
