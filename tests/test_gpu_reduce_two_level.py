"""The two-level bucket reduction of shared bucket sets (sonic_amd/csrc/msm.hip: k_bucket_segments<true> writes a run and a local total
per K-bucket segment, the bit-sum butterfly reduces the runs with weights from 0, k_group_sum / k_window_sum add the totals, and
msm_finish_host folds slot form 3) against the CPU oracle, byte for byte.

prove() takes that path for the batched groups of a proof whose bucket sets hold more than 2^17 buckets and whose jobs have at most
2^21 terms, except the group that finishes last.  The tests force the table width on a small SRS (SONIC_MSM_TABLE_C, read when the SRS is made) and leave the workload small:
n = 2^11, d = 2^14.  c = 19 gives 2^18 buckets per set, c = 20 gives 2^19.  With prove()'s segments of K = 32 buckets that is nseg = 8192
and 16384 segments per set, whose totals go through the 256-way k_group_sum first.  SONIC_PROVE_SEGMENT=64 gives nseg = 4096 at c = 19,
where k_window_sum adds the totals directly, and 8192 at c = 20.  The runs of such a group (at most 4 x 16384 points) take the
butterfly's all-quad form; SONIC_PROVE_SEGMENT=8 at c = 20 makes them 65536 per job, more than 2^17 per group, for its three-launch
form (what a batch of more than eight jobs reaches at K = 32).  Such a handle is not a small-proof handle (more than 2^17 buckets), so it does not fall
into the fused one-chain form and d need not grow.  At this size nearly every bucket is empty, so infinity meets every operand position
of both levels; with the degenerate SRS x = 1 (the reference benchmark's) all points coincide and P + P, P - P turn up inside
run += B[j], tot += run and the butterfly.  Q = 1, 2, 3 put two, three and four jobs into one batch.  Every case checks through the
library's launch table that k_bucket_segments really ran."""
import ctypes as C
import random

import numpy as np
import pytest

from util import NCPU, R, big_circuit, fr_bytes, rand_fr_array

pytestmark = pytest.mark.gpu
T = min(NCPU, 16)
N, D = 1 << 11, 1 << 14
ALPHA = 0x5EED5EED5EED5EED
X_RANDOM = random.Random(2 ** 19).randrange(2, R)


def _launches(L):
    """{kernel name: launches} of the library's launch table"""
    names = C.create_string_buffer(16384)
    L.sonic_profile_names(names, 16384)
    out = {}
    for nm in names.value.decode().split():
        ms, cnt = C.c_double(), C.c_int64()
        L.sonic_profile_get(nm.encode(), C.byref(ms), C.byref(cnt))
        out[nm] = cnt.value
    return out


def _x1_oracle_srs(orc):
    """the oracle's SRS for x = 1 from its two distinct points"""
    g, ga = orc.g1_mul(orc.g1_gen(), 1), orc.g1_mul(orc.g1_gen(), ALPHA)
    b0 = np.tile(np.frombuffer(g, np.uint8), (2 * D + 1, 1))
    b1 = np.tile(np.frombuffer(ga, np.uint8), (2 * D + 1, 1))
    b1[D] = 0                                                    # the empty slot e = 0 of the alpha basis
    return orc.SRS.from_points(D, np.ascontiguousarray(b0), np.ascontiguousarray(b1), threads=T)


@pytest.fixture(scope="module")
def oracle_srs(orc):
    return {"random": orc.SRS(D, X_RANDOM, ALPHA, threads=T), "x1": _x1_oracle_srs(orc)}


@pytest.fixture(scope="module")
def gpu_srs(sonic):
    """SRS handles by (table width, trapdoor), made on demand under SONIC_MSM_TABLE_C and closed with the module"""
    made = {}

    def get(c, x):
        if (c, x) not in made:
            mp = pytest.MonkeyPatch()
            mp.setenv("SONIC_MSM_TABLE_C", str(c))
            try:
                made[(c, x)] = sonic.SRS.new(D, 1 if x == "x1" else X_RANDOM, ALPHA)
            finally:
                mp.undo()
        return made[(c, x)]

    yield get
    for s in made.values():
        s.close()


@pytest.fixture(scope="module")
def circuits():
    return {Q: big_circuit(1000 + Q, N, Q) for Q in (1, 2, 3)}


# (table width, trapdoor, Q, SONIC_PROVE_SEGMENT or None for prove()'s own K = 32)
CASES = [(19, "random", 2, 64), (20, "random", 2, 64), (19, "x1", 2, 64), (20, "x1", 2, 64),
         (19, "random", 2, None), (20, "random", 2, None), (19, "x1", 2, None), (20, "x1", 2, None),
         (19, "random", 1, 64), (20, "random", 1, None), (19, "random", 3, 64), (20, "random", 3, None), (19, "random", 3, None),
         (20, "random", 2, 8), (20, "x1", 2, 8)]


@pytest.mark.parametrize("c,x,Q,seg", CASES, ids=[f"c{c}-nseg{(1 << (c - 1)) // (seg or 32)}-{x}-Q{Q}" for c, x, Q, seg in CASES])
def test_prove_two_level_reduction(sonic, orc, monkeypatch, gpu_srs, oracle_srs, circuits, c, x, Q, seg):
    from sonic_amd import _lib
    L = _lib.lib()
    monkeypatch.delenv("SONIC_PROVE_TWO_LEVEL", raising=False)
    if seg:
        monkeypatch.setenv("SONIC_PROVE_SEGMENT", str(seg))
    else:
        monkeypatch.delenv("SONIC_PROVE_SEGMENT", raising=False)
    nseg = (1 << (c - 1)) // (seg or 32)
    srs = gpu_srs(c, x)
    pc, pw, sets = C.c_int(), C.c_int(), C.c_int()
    _lib.check(L.sonic_msm_plan(srs._h, N, C.byref(pc), C.byref(pw), C.byref(sets)))
    assert (pc.value, sets.value) == (c, 1)                      # one shared set of 2^(c-1) > 2^17 buckets
    circ = circuits[Q]
    tr = fr_bytes([random.Random(c * 10 + Q).randrange(2, R) for _ in range(8 + 2 * Q)])
    orc.set_mode(1, T)
    want = orc.prove(oracle_srs[x], N, Q, circ["wL"], circ["wR"], circ["wO"], circ["cs"], circ["aL"], circ["aR"], circ["aO"], tr, True)
    p = sonic.Prover(srs, sonic.ArithCircuit(sonic.GateWeights(circ["wL"], circ["wR"], circ["wO"]), circ["cs"]))
    try:
        p.set_assignment(sonic.Assignment(circ["aL"], circ["aR"], circ["aO"]))
        L.sonic_profile_reset()
        L.sonic_profile_enable(1)
        try:
            got = p.prove_bytes(tr)
        finally:
            L.sonic_profile_enable(0)
        ran = _launches(L)
        L.sonic_profile_reset()
    finally:
        p.close()
    segments = {k: v for k, v in ran.items() if k.startswith("k_bucket_segments") and v}
    print(f"c={c} x={x} Q={Q} nseg={nseg}: " + ", ".join(f"{k} x{v}" for k, v in sorted(ran.items()) if k.startswith(("k_bucket_", "k_group_sum", "k_window_sum")) and v))
    assert segments, f"no group of this proof took the running sums: {sorted(k for k, v in ran.items() if v)}"
    assert set(segments) == {"k_bucket_segments<true>"}          # shared bucket sets: the form without the multiple
    # the totals: 256-way groups first above 4096 segments per set, else straight into k_window_sum
    assert ran.get("k_group_sum", 0) == (segments["k_bucket_segments<true>"] if nseg > 4096 else 0)
    assert got == want


@pytest.mark.parametrize("x", ["random", "x1"])
def test_prove_groups_with_the_multiple(sonic, orc, monkeypatch, gpu_srs, oracle_srs, circuits, x):
    """SONIC_PROVE_TWO_LEVEL=0: the form that groups of more than 2^21 terms per job keep (a size no test of a few seconds reaches) --
    every segment multiplies its run, K = 64 -- on the same proof: k_bucket_segments<false> over shared bucket sets, the same bytes"""
    from sonic_amd import _lib
    L = _lib.lib()
    monkeypatch.setenv("SONIC_PROVE_TWO_LEVEL", "0")
    monkeypatch.delenv("SONIC_PROVE_SEGMENT", raising=False)
    srs, circ, Q = gpu_srs(20, x), circuits[2], 2
    tr = fr_bytes([random.Random(77).randrange(2, R) for _ in range(8 + 2 * Q)])
    orc.set_mode(1, T)
    want = orc.prove(oracle_srs[x], N, Q, circ["wL"], circ["wR"], circ["wO"], circ["cs"], circ["aL"], circ["aR"], circ["aO"], tr, True)
    p = sonic.Prover(srs, sonic.ArithCircuit(sonic.GateWeights(circ["wL"], circ["wR"], circ["wO"]), circ["cs"]))
    try:
        p.set_assignment(sonic.Assignment(circ["aL"], circ["aR"], circ["aO"]))
        L.sonic_profile_reset()
        L.sonic_profile_enable(1)
        try:
            got = p.prove_bytes(tr)
        finally:
            L.sonic_profile_enable(0)
        ran = _launches(L)
        L.sonic_profile_reset()
    finally:
        p.close()
    assert ran.get("k_bucket_segments<false>", 0) > 0 and ran.get("k_bucket_segments<true>", 0) == 0
    assert ran.get("k_group_sum", 0) == ran["k_bucket_segments<false>"]          # nseg = 2^19 / 64 = 8192 > 4096
    assert got == want


def test_per_window_sets_keep_the_multiple(sonic, orc):
    """a stand-alone MSM over caller-supplied points (no tables: a bucket set per window, Wb > 1) still multiplies inside the segments
    kernel -- its W window sums fill the slot -- and gives the oracle's point"""
    from sonic_amd import _lib
    L = _lib.lib()
    n = 5000
    pyr = random.Random(5000)
    srs = sonic.SRS.new(n, pyr.randrange(2, R), pyr.randrange(2, R))
    pts = srs.points(0, -n // 2, n)
    srs.close()
    sc = rand_fr_array(np.random.default_rng(5000), n)
    L.sonic_msm_set_window(8)
    L.sonic_profile_reset()
    L.sonic_profile_enable(1)
    try:
        got = sonic.msm_g1(pts, sc)
    finally:
        L.sonic_profile_enable(0)
        L.sonic_msm_set_window(0)
    ran = _launches(L)
    L.sonic_profile_reset()
    assert ran.get("k_bucket_segments<false>", 0) == 1 and ran.get("k_bucket_segments<true>", 0) == 0
    assert got == orc.msm(pts, sc, 1, T)
