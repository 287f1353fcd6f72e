"""The prover's stream pool on the GPU (sonic_amd/csrc/stream_pool.hpp; prover.hpp, `pooled`): handles that borrow the device's pooled
streams give the bytes of proofs made one at a time on a fresh handle with private streams -- two handles alternately, five in a ring, a
handle freed beside a proof in flight, sonic_prove_batch's thread per handle, a Fiat-Shamir proof beside a streamed one -- at pool sizes 2,
4 and 8 and with the pool off (0).  The pool's size is fixed when a process first makes a handle, so every case is one fresh child
process (tests/stream_pool_child.py); they run one at a time.  The reference is made once, by a child with SONIC_STREAM_POOL=0.  A hang
would be a failure of the ordering argument at the enqueue lock (internal.hpp): the child's time limit is there to report it, not to be
waited for."""
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
CHILD = os.path.join(HERE, "stream_pool_child.py")


def run_child(mode, path, pool):
    env = dict(os.environ, SONIC_STREAM_POOL=str(pool))
    for k in ("SONIC_PROVE_FUSED", "SONIC_PROVE_GRAPH", "SONIC_FUSED_LANES"):
        env.pop(k, None)
    out = subprocess.run([sys.executable, CHILD, mode, path], capture_output=True, text=True, timeout=300, env=env)
    assert out.returncode == 0 and out.stdout.endswith("stream_pool_child ok\n"), (pool, out.stdout[-2000:], out.stderr[-4000:])


@pytest.fixture(scope="module")
def reference(tmp_path_factory):
    path = str(tmp_path_factory.mktemp("stream_pool") / "ref.json")
    run_child("ref", path, 0)
    return path


@pytest.mark.parametrize("pool", [0, 2, 4, 8])
def test_pooled_handles_give_the_bytes_of_private_ones(reference, pool):
    run_child("check", reference, pool)
