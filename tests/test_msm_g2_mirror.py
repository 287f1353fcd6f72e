"""util.g2_msm_mirror, the G2 MSM replayed on integers, against what it must add up to: sum_i s_i k_i, modulo r or over the integers.  No
GPU: the mirror is what tests/test_gpu_msm_g2_paths.py takes its claims from, so its totals, its counts on hand-worked inputs and the
number of additions it replays per stage are checked here."""
import random

import pytest

from util import HALF_R, R, g2_msm_mirror, root_of_unity

WIDTHS = (4, 5, 7, 9, 12, 13, 16)
KINDS = ("both_inf", "p_inf", "q_inf", "dbl", "neg", "add")


def additions(m, stage):
    return sum(m[stage][k] for k in KINDS)


@pytest.mark.parametrize("c", WIDTHS)
@pytest.mark.parametrize("bits,fold", [(255, True), (256, False), (129, True)])
def test_totals_are_the_weighted_sum(c, bits, fold):
    pyr = random.Random(100 * c + bits)
    n = 40
    ks = [pyr.randrange(R) for _ in range(n)]
    top = 1 << 128 if bits == 129 else R
    sc = [pyr.randrange(top) for _ in range(n - 4)] + [0, 1, top - 1, HALF_R if bits != 129 else 1 << 127]
    for walk_max in (3, 256):
        m = g2_msm_mirror(ks, sc, c, bits, fold, walk_max)
        assert m.total == sum(s * k for s, k in zip(sc, ks)) % R
        assert m.plan["W"] == -(-bits // c) and m.plan["NB"] == 1 << (c - 1) and m.plan["nseg"] == max(1, (1 << (c - 1)) // 8)


@pytest.mark.parametrize("x", (1, R - 1, root_of_unity(2), root_of_unity(8)))
def test_totals_over_degenerate_bases(x):
    pyr = random.Random(x % 1000)
    n = 600
    ks = [pow(x, e, R) for e in range(-300, 300)]
    for sc in ([pyr.randrange(R)] * n, [pyr.choice((3, R - 3, 4, R - 4)) for _ in range(n)]):
        for c, fold, bits in ((4, True, 255), (7, False, 256)):
            m = g2_msm_mirror(ks, sc, c, bits, fold, 256)
            assert m.total == sum(s * k for s, k in zip(sc, ks)) % R


def test_totals_over_plain_integers():
    pyr = random.Random(9)
    ks = [pyr.choice((1, -1)) for _ in range(50)]
    sc = [pyr.choice((1, R - 1, (R + 1) // 2, pyr.randrange(R))) for _ in range(50)]
    m = g2_msm_mirror(ks, sc, 5, 256, False, 16, mod=None)
    assert m.total == sum(s * k for s, k in zip(sc, ks))


def test_counts_on_hand_worked_inputs():
    # two equal points under scalar 1: bucket 0 of window 0 walks inf + P, P + P
    m = g2_msm_mirror([5, 5], [1, 1], 4, 256, False, 256)
    assert m.order_free and dict(m["accum"]) == {"p_inf": 1, "dbl": 1} and dict(m["combine"]) == {"p_inf": 1} and m.total == 10
    # P and -P: the walk ends at infinity
    m = g2_msm_mirror([5, R - 5], [1, 1], 4, 256, False, 256)
    assert dict(m["accum"]) == {"p_inf": 1, "neg": 1} and m.total == 0
    # the fold puts s and r - s into one bucket with opposite signs
    m = g2_msm_mirror([5, 5], [3, R - 3], 4, 255, True, 256)
    assert dict(m["accum"]) == {"p_inf": 1, "neg": 1} and m.total == 0
    # five equal entries under a walk bound of two: chunks 2P, 2P, P; the combine doubles and then adds
    m = g2_msm_mirror([1] * 5, [1] * 5, 4, 256, False, 2)
    assert m.order_free and dict(m["combine"]) == {"p_inf": 1, "dbl": 1, "add": 1} and m["accum"]["dbl"] == 2 and m.total == 5
    # three distinct entries in one bucket: the counts would depend on their order
    assert not g2_msm_mirror([1, 2, 3], [1, 1, 1], 4, 256, False, 256).order_free
    # buckets 1 and 2 hold h and -h: run passes through infinity below a finite acc
    m = g2_msm_mirror([1, 1], [1, R - 2], 4, 255, True, 256)
    assert m["seg_run"]["neg"] == 1 and m["seg_acc"]["q_inf"] == 1 and m.total == R - 1
    # the top bucket holds h and the one below it -2h: acc = h meets run = -h
    m = g2_msm_mirror([1, 1, 1], [8, R - 7, R - 7], 4, 255, True, 256)
    assert m["seg_acc"]["neg"] == 1 and m.total == (8 - 14) % R
    # Horner: P in window 1 and 2^c P in window 0
    m = g2_msm_mirror([3, 48, R - 48], [(1 << 4) + (1 << 12), 1, 1 << 8], 4, 256, False, 256)
    assert m["fold"]["dbl"] == 1 and m["fold"]["neg"] == 1 and m.total == (3 * ((1 << 4) + (1 << 12)) + 48 - 48 * 256) % R


@pytest.mark.parametrize("c", WIDTHS)
def test_every_stage_replays_the_additions_of_its_kernel(c):
    bits = 255
    W, NB = -(-bits // c), 1 << (c - 1)
    K = min(NB, 8)
    nseg = NB // K
    pyr = random.Random(c)
    n = 30
    m = g2_msm_mirror([pyr.randrange(1, R) for _ in range(n)], [pyr.randrange(R) for _ in range(n)], c, bits, True, 256)
    assert additions(m, "seg_run") == additions(m, "seg_acc") == W * nseg * K
    assert additions(m, "seg_join") == W * (nseg - 1)
    assert m["seg_mul"]["dbl_op"] + m["seg_mul"]["dbl_of_inf"] == W * (nseg - 1) * (c - 1)
    assert additions(m, "seg_mul") == W * sum(bin(s * K).count("1") for s in range(nseg))
    blocks = min(-(-nseg // 64), 64)
    assert additions(m, "range") == W * nseg and additions(m, "range_tree") == W * blocks * 63
    assert additions(m, "range2") == (W * blocks if blocks > 1 else 0) and additions(m, "range2_tree") == (W * 63 if blocks > 1 else 0)
    assert additions(m, "fold") == W and m["fold"]["dbl_op"] + m["fold"]["dbl_of_inf"] == (W - 1) * c
