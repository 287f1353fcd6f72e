"""The prover's stream pool, the part that needs no GPU (sonic_amd/csrc/stream_pool.hpp): the role -> stream mapping and its three rules
for every pool size 2..32, the parsing of GPU_MAX_HW_QUEUES and SONIC_STREAM_POOL, and a simulation of two proofs on in-order streams,
all checked inside a stand-alone program (tests/host/stream_pool_host.cpp) that is built plain and under ASan / UBSan.  The mapping it
prints is checked once more here at the sizes the GPU test runs (tests/test_gpu_stream_pool.py)."""
import os
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
HOST = os.path.join(HERE, "host")
ENV = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")


@pytest.fixture(scope="module")
def drivers():
    subprocess.check_call(["make", "-C", HOST, "-s", "-f", "stream_pool.mk", "stream_pool_host", "stream_pool_host_san"])
    return {"plain": os.path.join(HOST, "stream_pool_host"), "san": os.path.join(HOST, "stream_pool_host_san")}


def mapping_lines(path):
    out = subprocess.run([path], capture_output=True, text=True, timeout=120, env=ENV)
    assert out.returncode == 0 and out.stdout.endswith("stream_pool_host ok\n"), out.stdout[-3000:] + out.stderr[-3000:]
    rows = {}
    for line in out.stdout.splitlines()[:-1]:
        w = line.split()
        assert w[0] == "P" and w[2] == "head" and w[4] == "ntt" and w[6] == "groups" and w[13] == "t" and w[15] == "chains" and w[18] == "tail", line
        rows[int(w[1])] = dict(head=int(w[3]), ntt=int(w[5]), groups=[int(x) for x in w[7:13]], t=int(w[14]), chains=[int(w[16]), int(w[17])], tail=int(w[19]))
    return rows


@pytest.mark.parametrize("build", ["plain", "san"])
def test_host_program_rules_parsing_and_simulation(drivers, build):
    rows = mapping_lines(drivers[build])
    assert sorted(rows) == list(range(2, 33))
    for P, r in rows.items():
        every = [r["head"], r["ntt"], r["t"], r["tail"]] + r["groups"] + r["chains"]
        assert all(0 <= s < P for s in every), P
        assert r["tail"] not in (r["head"], r["ntt"]) and r["tail"] == r["t"], P
        assert r["head"] not in r["groups"] + r["chains"] + [r["t"]], P
        assert (r["head"] == r["ntt"]) == (P == 2), P
        if P > 2:
            assert r["tail"] not in r["groups"] and not set(r["groups"]) & set(r["chains"]), P
            assert all((c == r["tail"]) == (P < 6) for c in r["chains"]), P
    # the sizes the GPU test forces, written out: 2 streams; the runtime's default of 4 queues; the library's cap of 8
    assert rows[2] == dict(head=0, ntt=0, groups=[1] * 6, t=1, chains=[1, 1], tail=1)
    assert rows[4] == dict(head=0, ntt=1, groups=[2, 1, 2, 1, 2, 1], t=3, chains=[3, 3], tail=3)
    assert rows[8] == dict(head=0, ntt=1, groups=[2, 3, 4, 5, 2, 3], t=7, chains=[6, 6], tail=7)


def test_library_reads_the_queue_count_and_never_sets_it():
    """the native setenv is gone (it ran after the first HIP call of a process that had loaded torch, and never overwrote a value)"""
    csrc = os.path.join(ROOT, "sonic_amd", "csrc")
    for name in sorted(os.listdir(csrc)):
        if name.endswith((".hip", ".hpp")):
            text = open(os.path.join(csrc, name)).read()
            assert "setenv(" not in text, name
    assert 'getenv("GPU_MAX_HW_QUEUES")' in open(os.path.join(csrc, "device.hip")).read()
