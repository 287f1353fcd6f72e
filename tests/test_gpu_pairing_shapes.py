"""The segmented product of the device pairing (pairing.hip: k_gt_plan, k_gt_group_product; pairing_groups.hpp) walked on the GPU at every
pass count, chunk edge and group count at which it changes behaviour.  Three references, none of them the code under test:

  * where = "host", which multiplies each group in a straight loop: every group's 576 bytes;
  * plain integers: pair i is (a_i G1_GEN, b_i G2_GEN), so a group is one exactly when sum a_i b_i = 0 mod r: every group's verdict;
  * oracle/pairing.py: a group's value is E^(sum a_i b_i) for E the oracle's value of (G1_GEN, G2_GEN) (tests/pairing_ref.py): the bytes of
    the first and last group, of every group of more than GT_CHUNK = 16 pairs, of the groups 255 .. 257, and of others up to 48 a case.

Groups that are not one have pairwise distinct exponents (asserted), so a value that lands in another group's slot changes bytes.  Every
case holds a group closed to one by its last pair, and such a group with that pair's scalar changed (asserted on the integers)."""
import numpy as np
import pytest

import pairing_ref as pref

pytestmark = pytest.mark.gpu

GT_CHUNK, PLAN_BLOCK, ORACLE_MAX = 16, 256, 48
CYCLE = (0, 1, 2, 17, 16, 3)


def passes(n):
    """gt_passes of pairing_groups.hpp, restated"""
    chunks = lambda m: 1 if m <= GT_CHUNK else -(-m // GT_CHUNK)      # noqa: E731
    p, m = 1, chunks(n)
    while m > 1:
        p, m = p + 1, chunks(m)
    return p


def group(g, m, close=None):
    """m pairs for group g: its first scalar is offset by the index -- ((g + 1) G1_GEN, b G2_GEN) -- and the rest cycle through the pools
    from index g.  close = 0: the last of the m pairs closes the group to one; close = c: that pair's scalar is off by c"""
    if m == 0:
        return []
    body = m if close is None else m - 1
    pairs = ([(g + 1, pref.G2_POOL[g % len(pref.G2_POOL)])] + pref.pool_pairs(body - 1, g))[:body]
    return pairs if close is None else pref.closed(pairs, close)


def oracle_picks(sizes):
    G = len(sizes)
    must = {0, G - 1} | {g for g in range(G) if sizes[g] > GT_CHUNK} | {g for g in (255, 256, 257) if g < G}
    rest = [g for g in range(G) if g not in must]
    room = max(0, ORACLE_MAX - len(must))
    step = max(1, -(-len(rest) // room)) if room else 0
    return sorted(must | set(rest[::step][:room] if room else ()))


def check(sonic, groups, want_passes):
    sizes = [len(grp) for grp in groups]
    G, n = len(sizes), sum(sizes)
    assert passes(n) == want_passes
    g1, g2, ends, exps = pref.build(groups)
    nonzero = [e for e in exps if e]
    assert len(set(nonzero)) == len(nonzero)
    vg, tg = sonic.pairing_check(g1, g2, ends, where="gpu", gt=True)
    vh, th = sonic.pairing_check(g1, g2, ends, where="host", gt=True)
    want = [int(e != 0) for e in exps]
    assert vg.tolist() == want
    assert vh.tolist() == want
    differ = np.nonzero((tg != th).any(axis=1))[0]
    assert differ.size == 0, differ[:20].tolist()
    for g in range(G):
        if exps[g] == 0:
            assert tg[g].tobytes() == pref.GT_ONE, g
    for g in oracle_picks(sizes):
        assert tg[g].tobytes() == pref.expected(exps[g]), (g, sizes[g])
    # without the values: the same verdicts
    assert sonic.pairing_check(g1, g2, ends, where="gpu").tolist() == want
    return tg


def test_chunk_edges(sonic):
    """sizes 15, 16, 17, 31, 32, 33, 255, 256, 257 -- where gt_chunks_of, the `s + GT_CHUNK < ge` clamp and gt_group_of's search change
    behaviour -- with empty groups first, in the middle and last; three passes.  The groups of 33 and 257 are closed to one by their last
    pair, those of 17 and 256 are closed with that pair's scalar changed"""
    sizes = [0, 1, 15, 16, 17, 31, 32, 33, 0, 255, 256, 257, 0]
    close = {4: 5, 7: 0, 10: 9, 11: 0}
    groups = [group(g, m, close.get(g)) for g, m in enumerate(sizes)]
    assert [len(grp) for grp in groups] == sizes and [pref.exponent(groups[g]) for g in (4, 7, 10, 11)] == [5, 0, 9, 0]
    check(sonic, groups, 3)


def test_cancellation_across_a_chunk_boundary(sonic):
    """32 pairs whose first 16 are (a_j G1_GEN, Q) and whose next 16 are (-a_j G1_GEN, Q): one only if both chunks are combined; the same
    with one scalar of the second chunk changed; 17 pairs whose 17th alone closes the sum, and the same with that scalar off by one"""
    b = pref.G2_POOL[5]
    a = [pref.G1_POOL[j % len(pref.G1_POOL)] + 100 * j for j in range(16)]
    cancel = [(x, b) for x in a] + [(pref.R - x, b) for x in a]
    changed = list(cancel)
    changed[21] = (changed[21][0] + 1, b)
    groups = [group(0, 3), [], cancel, changed, group(4, 17, 0), group(4, 17, 1), group(6, 5)]
    assert [len(grp) for grp in groups] == [3, 0, 32, 32, 17, 17, 5] and [pref.exponent(grp) for grp in groups[2:6]] == [0, b, 0, 1]
    check(sonic, groups, 2)


@pytest.mark.parametrize("sizes,close", [((3, 0, 4097, 1, 2), {0: 0, 2: 0, 4: 7}), ((4096, 1), {0: 7})])
def test_four_passes(sonic, sizes, close):
    """n >= 4097 takes four passes, and the passes come from n: 4096 pairs and a singleton take four as well.  The small groups before and
    after the large one are down to one value after the first pass, are copied through three more and must stay in order.  The group of
    4097 is closed to one, which it is only if every one of its pairs enters the product, as is the group of 3; the group of 2 and the
    group of 4096 are closed with the last scalar off by 7, so their value is E^7"""
    groups = [group(g, m, close.get(g)) for g, m in enumerate(sizes)]
    assert [len(grp) for grp in groups] == list(sizes) and [pref.exponent(groups[g]) for g in sorted(close)] == [close[g] for g in sorted(close)]
    check(sonic, groups, 4)


@pytest.mark.parametrize("G", [255, 256, 257, 513])
def test_more_groups_than_the_plan_block(sonic, G):
    """k_gt_plan's 256 threads take per = ceil(G / 256) groups each: per = 1 with an idle last thread (255), exactly one each (256), per = 2
    with trailing empty slices (257), per = 3 (513); sizes cycle through (0, 1, 2, 17, 16, 3), so the slices' counts are uneven.  Of the
    groups of 17, those at g = 3 mod 24 are closed to one, those at g = 9 mod 24 are closed with the last scalar off by g + 1, and the
    others are left open, with exponents of full size"""
    groups = [group(g, CYCLE[g % 6], {3: 0, 9: g + 1}.get(g % 24)) for g in range(G)]
    assert [len(grp) for grp in groups] == [CYCLE[g % 6] for g in range(G)]
    assert pref.exponent(groups[3]) == 0 and pref.exponent(groups[9]) == 10
    assert -(-G // PLAN_BLOCK) == {255: 1, 256: 1, 257: 2, 513: 3}[G]
    check(sonic, groups, 3)


@pytest.mark.parametrize("close", [0, 12345])
def test_launch_bound_beyond_the_buffers(sonic, close):
    """G = 1000 with 257 pairs in group 0 and 39 singletons: the passes launch 1018, 1063 and 1066 threads over buffers of 1018 values, and
    gt_chunk_product must refuse every thread beyond the pass's true count.  All 1000 results are checked: group 0 (closed to one, and
    with its last scalar changed), the singletons, and the empty groups, which read exactly GT_ONE with verdict 0"""
    G = 1000
    single = {1, 255, 256, 257, 999} | set(range(27, 1000, 29))
    groups = [group(0, 257, close)] + [group(g, 1) if g in single else [] for g in range(1, G)]
    n = sum(len(grp) for grp in groups)
    assert n == 257 + 39 and sum(1 for grp in groups if grp) == 40 and pref.exponent(groups[0]) == close
    b1 = n // GT_CHUNK + G
    b2 = b1 // GT_CHUNK + G
    b3 = b2 // GT_CHUNK + G
    assert (b1, b2, b3) == (1018, 1063, 1066)
    tg = check(sonic, groups, 3)
    empty = [g for g in range(G) if not groups[g]]
    assert len(empty) == G - 40 and all(tg[g].tobytes() == pref.GT_ONE for g in empty)
