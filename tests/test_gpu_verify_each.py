"""`each` after a failed fold, on the device (verify_batch.hip, fold_each_device): with SONIC_PAIRING_GPU=1 every
well-formed proof is folded on its own by k_each_terms, k_each_sums and the kernels of pairing.hip, with =0 by the host's MSM calls and
Miller loops.  Both must give the same (ok, each) pairs, and those are the expected lists.  The workload is the small one of
tests/test_gpu_verify_batch.py, built by its helpers; dense and CSR handles, two classes of max degree (n and d)."""
import ctypes as C
import os

import pytest

from test_gpu_verify_batch import SEED, World, _damages, g1_shift, layout, put
from util import R

pytestmark = pytest.mark.gpu

KNOB = "SONIC_PAIRING_GPU"
N, Q = 16, 2


@pytest.fixture(scope="module")
def world(sonic, ref):
    w = World(sonic, ref, N, Q, 3)
    yield w
    w.close()


@pytest.fixture(scope="module")
def fs_world(sonic, ref):
    w = World(sonic, ref, N, Q, 3, True)
    yield w
    w.close()


def both(call):
    """the call under SONIC_PAIRING_GPU=1 and =0: equal results, returned once"""
    got = {}
    old = os.environ.get(KNOB)
    try:
        for knob in ("1", "0"):
            os.environ[KNOB] = knob
            got[knob] = call()
    finally:
        if old is None:
            os.environ.pop(KNOB, None)
        else:
            os.environ[KNOB] = old
    assert got["1"] == got["0"], got
    return got["1"]


def false_proof(ref, raw):
    """well-formed and rejected: W_a + g"""
    g1, _fr, _size = layout(Q)
    return g1_shift(ref, raw, g1[2], ref.G1_GEN)


def malformed_proof(raw):
    g1, _fr, _size = layout(Q)
    return put(raw, g1[0], (1).to_bytes(48, "little") + (1).to_bytes(48, "little"))       # R off the curve


@pytest.mark.parametrize("form", ["dense", "csr"])
def test_three_proofs_with_the_bad_one_at_each_position(sonic, ref, world, form):
    v = world.verifier(sonic, form)
    for at in range(3):
        proofs = list(world.proofs)
        proofs[at] = false_proof(ref, proofs[at])
        assert not world.yard(sonic, proofs[at], world.trs[at], form)
        assert both(lambda: v.verify_batch(proofs, world.trs, seed=SEED, each=True)) == (False, [k != at for k in range(3)]), at


def test_sixty_six_proofs_with_bad_ones_at_the_block_edges(sonic, ref, world):
    K, bad = 66, (0, 63, 64, 65)
    proofs = [world.proofs[k % 3] for k in range(K)]
    trs = [world.trs[k % 3] for k in range(K)]
    for k in bad:
        proofs[k] = false_proof(ref, proofs[k])
    v = world.verifier(sonic, "dense")
    assert both(lambda: v.verify_batch(proofs, trs, seed=SEED, each=True)) == (False, [k not in bad for k in range(K)])


def test_every_proof_bad_and_malformed_beside_false(sonic, ref, world):
    v = world.verifier(sonic, "csr")
    allbad = [false_proof(ref, p) for p in world.proofs]
    assert both(lambda: v.verify_batch(allbad, world.trs, seed=SEED, each=True)) == (False, [False] * 3)
    mixed = [malformed_proof(world.proofs[0]), world.proofs[1], false_proof(ref, world.proofs[2])]
    assert both(lambda: v.verify_batch(mixed, world.trs, seed=SEED, each=True)) == (False, [False, True, False])
    mixed = [world.proofs[0], false_proof(ref, world.proofs[1]), malformed_proof(world.proofs[2])]
    assert both(lambda: v.verify_batch(mixed, world.trs, seed=None, each=True)) == (False, [True, False, False])


def test_the_other_batched_forms(sonic, ref, world, fs_world):
    v = world.verifier(sonic, "dense")
    bad = [world.proofs[0], false_proof(ref, world.proofs[1]), world.proofs[2]]
    want = (False, [True, False, True])
    # one statement per proof (`_cs`), plain and compressed
    cs = [world.lists[3]] * 3
    assert both(lambda: v.verify_batch(bad, world.trs, seed=SEED, each=True, constants=cs)) == want
    zs = [sonic.Proof.from_bytes(p, Q).to_bytes(compressed=True) for p in bad]
    assert both(lambda: v.verify_batch(zs, world.trs, seed=SEED, each=True)) == want
    assert both(lambda: v.verify_batch(zs, world.trs, seed=SEED, each=True, constants=cs)) == want
    # core proofs: the head of the record, checked at (y, z)
    cores = [p[:576] for p in bad]
    yzs = [(y, z) for y, z, _ in world.trs]
    assert both(lambda: v.verify_core_batch([p[:576] for p in world.proofs], yzs, seed=SEED, each=True)) == (True, [True] * 3)
    assert both(lambda: v.verify_core_batch(cores, yzs, seed=SEED, each=True)) == want
    assert both(lambda: v.verify_core_batch([sonic.CoreProof.from_bytes(p).to_bytes(compressed=True) for p in cores], yzs, seed=SEED, each=True)) == want
    # Fiat-Shamir
    fv = fs_world.verifier(sonic, "dense")
    assert both(lambda: fv.verify_fs_batch(fs_world.proofs, seed=SEED, each=True)) == (True, [True] * 3)
    fbad = [fs_world.proofs[0], false_proof(ref, fs_world.proofs[1]), fs_world.proofs[2]]
    assert both(lambda: fv.verify_fs_batch(fbad, seed=SEED, each=True)) == want


def profiled(call):
    from sonic_amd import _lib
    L = _lib.lib()
    L.sonic_profile_enable(1)
    try:
        L.sonic_profile_reset()
        result = call()
        buf = C.create_string_buffer(1 << 16)
        L.sonic_profile_names(buf, len(buf))
        names, cnt = set(), C.c_int64(0)
        for name in buf.value.decode().split("\n"):          # (the table keeps the names of earlier calls with no launches)
            L.sonic_profile_get(name.encode(), None, C.byref(cnt))
            if name and cnt.value:
                names.add(name)
        L.sonic_profile_get(b"k_miller_loops", None, C.byref(cnt))
        return result, names, cnt.value
    finally:
        L.sonic_profile_reset()
        L.sonic_profile_enable(0)


def test_the_profiler_shows_which_form_ran(sonic, ref, world, monkeypatch):
    v = world.verifier(sonic, "dense")
    bad = [world.proofs[0], false_proof(ref, world.proofs[1]), world.proofs[2]]
    monkeypatch.setenv(KNOB, "1")
    got, names, loops = profiled(lambda: v.verify_batch(bad, world.trs, seed=SEED, each=True))
    assert got == (False, [True, False, True])
    assert "verify_batch:each_gpu" in names and "k_miller_loops" in names and loops == 1
    assert {"k_each_terms", "k_each_sums", "k_gt_group_product", "k_final_exp"} <= names and "verify_batch:each" not in names
    monkeypatch.setenv(KNOB, "0")
    got, names, loops = profiled(lambda: v.verify_batch(bad, world.trs, seed=SEED, each=True))
    assert got == (False, [True, False, True])
    assert "verify_batch:each_gpu" not in names and "k_miller_loops" not in names and loops == 0 and "verify_batch:each" in names
    # a batch whose fold holds enters neither form
    for knob in ("1", "0"):
        monkeypatch.setenv(KNOB, knob)
        got, names, loops = profiled(lambda: v.verify_batch(world.proofs, world.trs, seed=SEED, each=True))
        assert got == (True, [True] * 3)
        assert not ({"verify_batch:each_gpu", "verify_batch:each", "k_miller_loops", "k_each_terms"} & names) and loops == 0


def test_the_unset_knob_takes_the_measured_rule(sonic, ref, world, monkeypatch):
    """EACH_GPU_MIN_PROOFS = 64 (pairing_device.hpp): K = 66 folds on the device, K = 63 and K = 3 on the host"""
    monkeypatch.delenv(KNOB, raising=False)
    v = world.verifier(sonic, "dense")
    for K, device in ((66, True), (63, False), (3, False)):
        proofs = [world.proofs[k % 3] for k in range(K)]
        trs = [world.trs[k % 3] for k in range(K)]
        proofs[K - 1] = false_proof(ref, proofs[K - 1])
        got, names, loops = profiled(lambda: v.verify_batch(proofs, trs, seed=SEED, each=True))
        assert got == (False, [True] * (K - 1) + [False]), K
        assert ("verify_batch:each_gpu" in names) == device and ("verify_batch:each" in names) == (not device) and loops == int(device), K


def test_the_device_fold_in_several_slices(sonic, ref, world, monkeypatch):
    """SONIC_EACH_SLICE: 66 proofs in slices of 4 (the last one of 2) and of 1 give what one slice gives"""
    K, bad = 66, (0, 3, 4, 63, 64, 65)
    proofs = [world.proofs[k % 3] for k in range(K)]
    trs = [world.trs[k % 3] for k in range(K)]
    for k in bad:
        proofs[k] = false_proof(ref, proofs[k])
    proofs[5] = malformed_proof(proofs[5])
    want = (False, [k not in bad and k != 5 for k in range(K)])
    v = world.verifier(sonic, "dense")
    monkeypatch.setenv(KNOB, "1")
    assert v.verify_batch(proofs, trs, seed=SEED, each=True) == want
    monkeypatch.setenv("SONIC_EACH_SLICE", "4")
    got, names, loops = profiled(lambda: v.verify_batch(proofs, trs, seed=SEED, each=True))
    assert got == want and loops == 17          # 65 well-formed proofs
    monkeypatch.setenv("SONIC_EACH_SLICE", "64")
    got, names, loops = profiled(lambda: v.verify_batch(proofs, trs, seed=SEED, each=True))
    assert got == want and loops == 2


# ---- the device form field by field: k_each_terms reads scalars[s * N + k * NP + j] over S arrays and NP + 1 slots, k_each_sums negates by s ----
def cycle(world, K):
    return [world.proofs[k % 3] for k in range(K)], [world.trs[k % 3] for k in range(K)]


@pytest.mark.parametrize("form", ["dense", "csr"])
def test_one_damaged_field_per_proof_in_one_batch(sonic, ref, world, form):
    """one proof per field of the record: proof k has its k-th G1 field + g, then its Fr fields + 1 in turn, the last proof is intact.
    each[k] is what sonic_verify says of proof k alone, under both forms: a slot or an array indexed wrongly moves a rejection to
    another proof or loses it"""
    g1, fr, _size = layout(Q)
    K = len(g1) + len(fr) + 1
    assert (len(g1), len(fr)) == (4 * Q + 7, 2 * Q + 5)
    proofs, trs = cycle(world, K)
    for k, off in enumerate(g1):
        proofs[k] = g1_shift(ref, proofs[k], off, ref.G1_GEN)
    for k, off in enumerate(fr, len(g1)):
        proofs[k] = put(proofs[k], off, ((int.from_bytes(proofs[k][off:off + 32], "little") + 1) % R).to_bytes(32, "little"))
    want = [world.yard(sonic, p, t, form) for p, t in zip(proofs, trs)]
    assert not all(want[:len(g1)]) and not all(want[len(g1):K - 1]) and want[K - 1]
    v = world.verifier(sonic, form)
    assert both(lambda: v.verify_batch(proofs, trs, seed=SEED, each=True)) == (False, want)


def test_damaged_challenges_under_both_forms(sonic, ref, world):
    """y, z, y_j and z_j of one proof of four off by one: the scalars of that proof's slots alone change"""
    K, at = 4, 2
    v = world.verifier(sonic, "dense")
    seen = []
    for what, raw, tr in _damages(ref, world.proofs[at], world.trs[at], Q):
        if what.startswith("every"):
            continue
        proofs, trs = cycle(world, K)
        proofs[at], trs[at] = raw, tr
        want = [world.yard(sonic, p, t) for p, t in zip(proofs, trs)]
        assert want == [k != at for k in range(K)], what
        assert both(lambda: v.verify_batch(proofs, trs, seed=SEED, each=True)) == (False, want), what
        seen.append(what)
    assert seen == ["y", "z", "y_0", "z_0", "y_1", "z_1"]


def test_infinity_as_a_proof_point_under_both_forms(sonic, ref, world):
    """R, then W_0, as the encoding of infinity in one proof of three: whatever sonic_verify says of it; once more beside a false proof,
    so that the per-proof fold runs whatever that verdict is and k_each_terms / k_each_sums meet the point"""
    g1, _fr, _size = layout(Q)
    v = world.verifier(sonic, "dense")
    for off in (g1[0], g1[6]):                       # R; W_0 of the first hsc list (R T Wa Wb Wt S_0 W_0)
        bad = put(world.proofs[1], off, bytes(96))
        want = world.yard(sonic, bad, world.trs[1])
        proofs = [world.proofs[0], bad, world.proofs[2]]
        assert both(lambda: v.verify_batch(proofs, world.trs, seed=SEED, each=True)) == (want, [True, want, True]), off
        proofs = [false_proof(ref, world.proofs[0]), bad, world.proofs[2]]
        assert both(lambda: v.verify_batch(proofs, world.trs, seed=SEED, each=True)) == (False, [False, want, True]), off


def test_258_proofs_are_one_slice_of_258_groups(sonic, ref, world, monkeypatch):
    """one group per proof gives k_gt_plan more groups than it has threads (per = 2, trailing empty slices); false proofs at 0 and at
    255, 256, 257"""
    K, bad = 258, (0, 255, 256, 257)
    proofs, trs = cycle(world, K)
    for k in bad:
        proofs[k] = false_proof(ref, proofs[k])
    want = (False, [k not in bad for k in range(K)])
    v = world.verifier(sonic, "dense")
    monkeypatch.delenv("SONIC_EACH_SLICE", raising=False)
    assert both(lambda: v.verify_batch(proofs, trs, seed=SEED, each=True)) == want
    monkeypatch.setenv(KNOB, "1")
    got, names, loops = profiled(lambda: v.verify_batch(proofs, trs, seed=SEED, each=True))
    assert got == want and "verify_batch:each_gpu" in names and loops == 1
