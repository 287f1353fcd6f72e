"""sonic_amd/csrc/srs_policy.hpp sizes an SRS handle: the window width of its tables by d, full versus endomorphism versus no tables by the
free device memory, and whether the running sums and the symmetric sums of the alpha basis are held.  A host program
(tests/host/srs_policy_host.cpp, plain g++ and once more under ASan / UBSan) prints its decisions; the expected values here are worked
out by hand from the rule as written, with SONIC_SRS_POINT_BYTES = 128, ENDO_BITS = 130 and per_table = 2 (2d + 1) 128.  CPU only."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "tests", "host")
MAX = "max"


def per_table(d):
    return 2 * (2 * d + 1) * 128


D20 = 1 << 20
PT = per_table(D20)
NONE = (0, 1, 0)

# (d, free_bytes, knobs) -> (c, W, endo)
WINDOWS = [
    # unlimited memory, no knobs: the width by d
    ((1 << 21, MAX, ""), (20, 13, 0)), ((1 << 20, MAX, ""), (20, 13, 0)),
    ((1 << 19, MAX, ""), (17, 15, 0)), ((3 << 18, MAX, ""), (17, 15, 0)), ((1 << 18, MAX, ""), (17, 15, 0)),
    ((1 << 17, MAX, ""), (16, 16, 0)), ((1 << 16, MAX, ""), (16, 16, 0)),
    ((1 << 15, MAX, ""), (15, 17, 0)), ((1 << 14, MAX, ""), (14, 19, 0)), ((1 << 10, MAX, ""), (10, 26, 0)),
    ((25, MAX, ""), (9, 29, 0)), ((1, MAX, ""), (9, 29, 0)),
    # SONIC_MSM_TABLE_C: 9 .. 22 is taken, anything else ignored
    ((1 << 12, MAX, "SONIC_MSM_TABLE_C=9"), (9, 29, 0)), ((1 << 12, MAX, "SONIC_MSM_TABLE_C=22"), (22, 12, 0)),
    ((1 << 12, MAX, "SONIC_MSM_TABLE_C=8"), (12, 22, 0)), ((1 << 12, MAX, "SONIC_MSM_TABLE_C=23"), (12, 22, 0)),
    ((1 << 20, MAX, "SONIC_MSM_TABLE_C=8"), (20, 13, 0)), ((1 << 20, MAX, "SONIC_MSM_TABLE_C=23"), (20, 13, 0)),
    ((1 << 20, MAX, "SONIC_MSM_TABLES=0"), NONE), ((1 << 20, MAX, "SONIC_MSM_TABLES=0 SONIC_MSM_ENDO=1"), NONE),
    # SONIC_MSM_ENDO=1: windows over 130 bits
    ((1 << 20, MAX, "SONIC_MSM_ENDO=1"), (19, 7, 1)), ((1 << 18, MAX, "SONIC_MSM_ENDO=1"), (17, 8, 1)), ((1 << 16, MAX, "SONIC_MSM_ENDO=1"), (15, 9, 1)),
    # memory, d = 2^20: the full tables (13) must fit half of what is free, else the endomorphism tables (7), else none
    ((D20, 2 * 13 * PT, ""), (20, 13, 0)),
    ((D20, 2 * 13 * PT - 1, ""), (19, 7, 1)),
    ((D20, 2 * 13 * PT - 1, "SONIC_MSM_ENDO=0"), NONE),
    ((D20, 2 * 7 * PT, ""), (19, 7, 1)),
    ((D20, 2 * 7 * PT - 1, ""), NONE),
    ((D20, 2 * 7 * PT - 1, "SONIC_MSM_ENDO=1"), NONE),
    ((D20, 2 * 13 * PT, "SONIC_MSM_ENDO=1"), (19, 7, 1)),
]

# (d, free before the second question, free before the third, knobs) -> (prefix held, sym held): prefix iff 128 (2d + 1) <= free / 4 and
# SONIC_SRS_PREFIX != 0; sym iff W > 1, not endo, 128 (d + 1) W <= free / 4 and SONIC_SRS_SYM != 0.  The windows are chosen with unlimited
# memory: d = 1024 has W = 26.
D = 1024
PREFIX_B, SYM_B = 128 * (2 * D + 1), 128 * (D + 1) * 26
HELD = [
    ((D, MAX, MAX, ""), (1, 1)),
    ((D, MAX, MAX, "SONIC_SRS_PREFIX=0"), (0, 1)), ((D, MAX, MAX, "SONIC_SRS_SYM=0"), (1, 0)), ((D, MAX, MAX, "SONIC_SRS_PREFIX=1 SONIC_SRS_SYM=1"), (1, 1)),
    ((D, MAX, MAX, "SONIC_MSM_ENDO=1"), (1, 0)), ((D, MAX, MAX, "SONIC_MSM_TABLES=0"), (1, 0)),
    ((D, 4 * PREFIX_B, 4 * SYM_B, ""), (1, 1)), ((D, 4 * PREFIX_B + 3, 4 * SYM_B + 3, ""), (1, 1)),
    ((D, 4 * PREFIX_B - 1, 4 * SYM_B - 1, ""), (0, 0)),
    ((D, 0, MAX, ""), (0, 1)), ((D, MAX, 0, ""), (1, 0)),
]


@pytest.fixture(scope="module", params=["srs_policy_host", "srs_policy_host_san"])
def decisions(request):
    """{case: (c, W, endo, prefix, sym)} as the program built plain / under the sanitizers prints them"""
    subprocess.check_call(["make", "-C", HOST, "-s", request.param])
    lines = {c: f"{c[0]} {c[1]} {c[1]} {c[1]} {c[2]}\n" for c, _ in WINDOWS}
    lines.update({c: f"{c[0]} {MAX} {c[1]} {c[2]} {c[3]}\n" for c, _ in HELD})
    cases = list(lines)
    text = "".join(lines.values())
    env = {k: v for k, v in os.environ.items() if not k.startswith("SONIC_")}
    out = subprocess.run([os.path.join(HOST, request.param)], input=text, capture_output=True, text=True, timeout=60, env=env)
    assert out.returncode == 0 and not out.stderr, out.stdout[-2000:] + out.stderr[-3000:]
    rows = [tuple(int(w) for w in ln.split()) for ln in out.stdout.splitlines()]
    assert len(rows) == len(cases)
    return dict(zip(cases, rows))


@pytest.mark.parametrize("case,want", WINDOWS, ids=[f"d={c[0]}-free={c[1]}-{c[2] or 'default'}" for c, _ in WINDOWS])
def test_window_policy(decisions, case, want):
    assert decisions[case][:3] == want


@pytest.mark.parametrize("case,want", HELD, ids=[f"free={c[1]},{c[2]}-{c[3] or 'default'}" for c, _ in HELD])
def test_prefix_and_sym_are_held(decisions, case, want):
    assert decisions[case][3:] == want
