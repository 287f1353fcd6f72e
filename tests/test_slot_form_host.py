"""msm_finish_host (sonic_amd/csrc/msm_slot.hpp) folds what the MSM kernels leave in a slot.  A stand-alone host program
(tests/host/slot_form_host.cpp, built with -fsanitize=address,undefined) fills slots in the form of the two-level running sums -- pad1 == 3:
the bit sums of 2^L segment runs, the sum of the segments' local totals, K in pad0 -- from small multiples of the generator, for
L in {2, 12, 13} and K in {8, 64}, and compares the fold with the directly weighted sum; all-infinity runs and a zero total included.
CPU only."""
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "tests", "host")


def test_slot_forms_fold_to_the_weighted_sum_under_sanitizers():
    subprocess.check_call(["make", "-C", HOST, "-s", "-f", "slot_form.mk", "slot_form_host_san"])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    out = subprocess.run([os.path.join(HOST, "slot_form_host_san")], capture_output=True, text=True, timeout=300, env=env)
    assert out.returncode == 0 and not out.stderr and out.stdout.endswith("slot_form_host ok\n"), out.stdout[-2000:] + out.stderr[-3000:]
    cases = set()
    for ln in out.stdout.splitlines()[:-1]:
        m = re.fullmatch(r"L=(\d+) K=(\d+) runs=(\d) zero_tot=([01]) mul=\d+ ok", ln)
        assert m, ln
        cases.add(tuple(int(v) for v in m.groups()))
    # every (L, K) the kernels produce at the sizes of the GPU tests, with random, all-infinity, all-equal and sparse runs (0 .. 3),
    # each with and without a total
    for L in (2, 12, 13):
        for K in (8, 64):
            for runs in range(4):
                for zero_tot in (0, 1):
                    assert (L, K, runs, zero_tot) in cases
