"""Shared helpers for the parity tests: synthetic circuits in the encodings both sides take."""
import os
import random

import numpy as np

R = 0x73EDA753299D7D483339D80809A1D80553BDA402FFFE5BFEFFFFFFFF00000001
NCPU = os.cpu_count() or 1


from sonic_amd.workload import big_circuit, fr_bytes, rand_fr_array  # noqa: E402,F401  (the generators live with the product: bench.py and the tools use them too)


def circuit_arrays(ref, pyrng: random.Random, n: int, Q: int):
    """rndCircuit (test/Test/Reference.hs:125-169) as (python lists, encoded arrays)."""
    circ, asg = ref.rnd_circuit(pyrng, n, Q)
    wL, wR, wO, cs = circ
    aL, aR, aO = asg
    enc = dict(wL=fr_bytes([v for r_ in wL for v in r_]), wR=fr_bytes([v for r_ in wR for v in r_]),
               wO=fr_bytes([v for r_ in wO for v in r_]), cs=fr_bytes(cs), aL=fr_bytes(aL), aR=fr_bytes(aR), aO=fr_bytes(aO))
    return circ, asg, enc


# ---- MSM path and digit references (tests/test_msm_digits.py, tests/test_gpu_msm_paths.py) --------------------------------------------
HALF_R = (R - 1) // 2
LAM = 0xd201000000010000 ** 2 - 1          # the endomorphism's eigenvalue (sonic_amd/csrc/endo.hpp ENDO_LAMBDA)
ENDO_BITS = 130


def root_of_unity(k: int) -> int:
    """a primitive 2^k-th root of unity in Fr (7 generates Fr^*)"""
    w = pow(7, (R - 1) >> k, R)
    assert pow(w, 1 << (k - 1), R) == R - 1
    return w


def msm_even_width(W: int, w: int, bits: int = 255) -> int:          # msm.hpp:14
    return bits // W + (1 if w < bits % W else 0)


def msm_even_shift(W: int, w: int, bits: int = 255) -> int:          # msm.hpp:15
    base, extra = divmod(bits, W)
    return w * base + min(w, extra)


def table_widths(W: int, bits: int = 255):
    """window widths of a plan over window tables (even widths, k_part_hist / k_part_scatter with keystride 0)"""
    return [msm_even_width(W, w, bits) for w in range(W)]


def msm_plan_points(n: int, fold: bool = False):
    """msm_plan (msm.hip:109-127): (c, W) of an MSM without tables; sonic_msm_g1 plans with fold = false"""
    lg = max(n, 1).bit_length() - 1
    c = min(max(lg - 4, 4), 16)
    return c, ((255 if fold else 256) + c - 1) // c


def heavy_threshold(n: int, W: int, Wb: int, NB: int) -> int:        # plan_finish, msm.hip:91-99
    return max(256, 8 * (n * (W // Wb) // NB))


def msm_path(sets: int, NB: int, shared: bool, K: int = 8) -> dict:
    """Which kernels one MSM chain runs (msm_enqueue_batch).  sets = bucket sets of the launch (jobs x Wb), NB buckets each.
    lanes: msm.hip:1240 (k_bucket_accum_split<4> up to 65536 buckets, <2> up to 131072, k_bucket_accum above).
    reduction: a shared bucket set (window tables, or an endomorphism plan) takes the bit-sum tree (msm.hip:1256), in its latency form
    while sets x NB <= 2^17 (msm.hip:1027) and its level form above; per-window sets take k_bucket_segments with K-bucket segments,
    whose segment multiple is none (nseg = 1), g1_mul_small (nseg not a multiple of 64) or the wave-uniform double-and-add
    (msm.hip:858-876)."""
    M = sets * NB
    lanes = 4 if M <= 65536 else (2 if M <= 131072 else 1)
    if shared:
        red = "tree_latency" if M <= 1 << 17 else "tree_level"
    else:
        nseg = NB // min(K, NB)
        red = "seg_none" if nseg == 1 else ("seg_wave" if nseg % 64 == 0 else "seg_mul_small")
    return dict(M=M, lanes=lanes, reduction=red)


def digit_stream(s: int, widths, fold: bool):
    """DigitStream (msm.hip:222-244): the fold s -> r - s on the negated point when s > (r-1)/2, then signed digits window by window.
    Returns ([(magnitude, sign)], negated, carry and bits left over the top window)."""
    neg = fold and s > HALF_R
    if neg:
        s = R - s
    carry, out = 0, []
    for c in widths:
        half = 1 << (c - 1)
        d = (s & ((1 << c) - 1)) + carry
        s >>= c
        sign = 1 if neg else 0
        if d > half:
            d, carry, sign = (1 << c) - d, 1, sign ^ 1
        else:
            carry = 0
        out.append((d, sign))
    return out, neg, (carry, s)


def digits_value(digs, widths) -> int:
    """sum sign * digit * 2^shift over the windows"""
    acc, sh = 0, 0
    for (d, sg), c in zip(digs, widths):
        acc += (-d if sg else d) << sh
        sh += c
    return acc


def _from_signed(D, widths) -> int:
    acc, sh = 0, 0
    for d, c in zip(D, widths):
        acc += d << sh
        sh += c
    return acc


def digit_families(widths, limit: int, v: int = 3):
    """Scalars aimed at the digit edges of a window layout, each with the signed digits the recoding must produce (the signed digits are
    in [-(half - 1), half] per window, so they are unique).  Every pattern covers the k lowest windows, k as large as keeps the value
    <= limit.  Families:
      half      every digit = half (the largest positive digit, no carry)
      half+1    every raw digit = half + 1: negative digit and a carry into each next window, +1 past the last
      all-ones  every raw digit = 2^cw - 1: a carry chain of zero digits, +1 past the last
      top-max   all-ones below a top window at the largest digit that keeps the value <= limit (the carry lands there)
      repeat    one digit value v in every window
    Returns {name: (scalar, signed digits)}."""
    W = len(widths)
    half = [1 << (c - 1) for c in widths]

    def fit(make):
        for k in range(W, 0, -1):
            D = make(k)
            s = _from_signed(D, widths)
            if 0 < s <= limit:
                return s, D
        raise AssertionError("no window of the pattern fits")

    fam = {}
    fam["half"] = fit(lambda k: [half[w] if w < k else 0 for w in range(W)])
    fam["half+1"] = fit(lambda k: [-(half[0] - 1) if w == 0 else -(half[w] - 2) if w < k else 1 if w == k else 0 for w in range(W)]
                        if k < W else [0] * W)
    fam["all-ones"] = fit(lambda k: [-1 if w == 0 else 1 if w == k else 0 for w in range(W)] if k < W else [0] * W)
    # (the top window the value reaches: with sonic_msm_g1's W = ceil(256 / c) the last window may hold nothing but the carry)
    t = max(w for w in range(1, W) if (limit + 1) >> sum(widths[:w]))
    top = min((limit + 1) >> sum(widths[:t]), half[t])
    fam["top-max"] = (top << sum(widths[:t])) - 1, [-1] + [0] * (t - 1) + [top] + [0] * (W - t - 1)
    fam["repeat"] = fit(lambda k: [v if w < k else 0 for w in range(W)])
    return fam


def endo_split(s: int):
    """endo_split (endo.hpp): s = s1 + lambda s2"""
    return s % LAM, s // LAM


def srs_exponent(x: int, alpha: int, basis: int, e0: int, scalars) -> int:
    """discrete log of msm_g1_srs(srs, basis, e0, scalars) over an SRS with trapdoor (x, alpha), independent of any MSM algorithm:
    sum_i s_i a_b x^(e0 + i) with a_0 = 1, a_1 = alpha, and the empty slot e = 0 of basis 1 contributing nothing (SRS.hs:27-43)"""
    acc, p = 0, pow(x, e0, R)
    for i, s in enumerate(scalars):
        if s and not (basis == 1 and e0 + i == 0):
            acc += s * p
        p = p * x % R
    return acc % R * (alpha if basis else 1) % R


def fr_ints(arr) -> list:
    """uint8 [n, 32] canonical Fr -> python integers"""
    b = np.ascontiguousarray(arr, np.uint8).tobytes()
    return [int.from_bytes(b[i:i + 32], "little") for i in range(0, len(b), 32)]


def valued_scalars(rng: np.random.Generator, pyr: random.Random, n: int, pairs: int = 8):
    """n scalars drawn from 2 pairs + 2 <= 64 values: `pairs` pairs v, r - v (the fold puts both in one bucket with opposite signs) and
    1, r - 1.  Few distinct values: heavy buckets whose partial sums coincide or cancel.  Returns (uint8 [n, 32], values, value index)."""
    vals = [1, R - 1]
    for _ in range(pairs):
        v = pyr.randrange(2, R)
        vals += [v, R - v]
    idx = rng.integers(0, len(vals), size=n)
    table = fr_bytes(vals)
    return table[idx], vals, idx


# ---- the G2 MSM replayed on integers (tests/test_msm_g2_mirror.py, tests/test_gpu_msm_g2_paths.py) -------------------------------------
G2_MIRROR_STAGES = ("accum", "combine", "seg_run", "seg_acc", "seg_mul", "seg_join", "range", "range_tree", "range2", "range2_tree", "fold")
G2_SUM_BLOCK = 64                          # srs_g2.hip: threads of a k_g2_sum block, and the most blocks per range of g2_sum_ranges_enqueue


class G2Mirror:
    """what g2_msm_mirror returns: the total, per stage a Counter of addition kinds, whether the accumulate / combine counts hold for
    every order of a bucket's entries, and the window sums"""

    def __init__(self, total, events, order_free, windows, plan):
        self.total, self.events, self.order_free, self.windows, self.plan = total, events, order_free, windows, plan

    def __getitem__(self, stage):
        return self.events[stage]


def g2_msm_mirror(ks, scalars, c: int, bits: int, fold: bool, walk_max: int, mod=R) -> G2Mirror:
    """One chain of g2_msm_blocking (sonic_amd/csrc/msm_g2.hip) over points that are known multiples ks[i] of one point, replayed on
    integers: modulo `mod` (r, for multiples of h), or over plain integers with mod = None (a point whose order is not known to divide
    anything: equal integers are equal points, and the replay claims no more).  ks[i] = 0 is the point at infinity.

    Digits: util.digit_stream with widths [c] * W, W = ceil(bits / c); digit d of window w goes to bucket d - 1 of that window's NB =
    2^(c-1) (msm.hip, key = w NB + d - 1), zero digits make no entry.  Buckets are cut into chunks of walk_max entries
    (k_g2_bucket_accum, mixed additions from infinity), a bucket's partial sums are added from infinity (k_g2_bucket_combine), segments of
    K = min(NB, 8) buckets run `run += B_j; acc += run` from the top and add (s K) run by double-and-add over c - 1 bits
    (k_g2_bucket_segments), the nseg segment results of a window are summed by k_g2_sum (thread-stride sums, a 64-leaf LDS tree, and a
    second launch over the block totals once nseg > 64: g2_sum_ranges_enqueue), and the host folds the window sums by Horner.

    Every addition p + q is counted once under its stage as one of
      both_inf, p_inf, q_inf   an operand at infinity (the branch the code returns from first)
      dbl                      equal operands: the doubling branch
      neg                      opposite operands: the result is infinity
      add                      the generic formula
    and the doublings of seg_mul and fold as dbl_of_inf or dbl_op.

    The sort of msm.hip does not keep the order of a bucket's entries (its placement is by atomic counters), so the accum and combine
    counts are those of the entries in index order and hold for the device only where order_free is true: every bucket has at most two
    entries or holds one value throughout.  The counts from seg_run on depend on the buckets' sums alone."""
    from collections import Counter
    W = -(-bits // c)
    NB = 1 << (c - 1)
    K = min(NB, 8)
    nseg = NB // K
    widths = [c] * W
    assert len(ks) == len(scalars) and 0 < len(ks) <= 1 << 19, "one slab"
    norm = (lambda v: v % mod) if mod else (lambda v: v)
    ev = {st: Counter() for st in G2_MIRROR_STAGES}

    def add(st, p, q):
        if q == 0 or p == 0:
            ev[st]["both_inf" if p == 0 and q == 0 else ("p_inf" if p == 0 else "q_inf")] += 1
            return p if q == 0 else q
        if p == q:
            ev[st]["dbl"] += 1
        elif norm(p + q) == 0:
            ev[st]["neg"] += 1
        else:
            ev[st]["add"] += 1
        return norm(p + q)

    def dbl(st, p):
        ev[st]["dbl_op" if p else "dbl_of_inf"] += 1
        return norm(2 * p)

    entries = {}
    for k, s in zip(ks, scalars):
        digs, _, (carry, rest) = digit_stream(s, widths, fold)
        assert carry == 0 and rest == 0, "the recoding stays inside the W windows"
        for w, (dg, sg) in enumerate(digs):
            if dg:
                entries.setdefault((w, dg - 1), []).append(norm(-k if sg else k))
    order_free = all(len(v) <= 2 or len(set(v)) == 1 for v in entries.values())

    buckets = {}
    for key, vals in entries.items():
        partial = []
        for at in range(0, len(vals), walk_max):
            acc = 0
            for v in vals[at:at + walk_max]:
                acc = add("accum", acc, v)
            partial.append(acc)
        acc = 0
        for p in partial:
            acc = add("combine", acc, p)
        buckets[key] = acc

    live = {(w, b // K) for (w, b) in buckets}
    windows = []
    for w in range(W):
        seg = [0] * nseg
        idle = 0
        for s in range(nseg):
            if (w, s) not in live:
                idle += 1
                continue
            run = acc = 0
            for j in range(K - 1, -1, -1):
                run = add("seg_run", run, buckets.get((w, s * K + j), 0))
                acc = add("seg_acc", acc, run)
            m = s * K
            if m:
                up = 0
                for bit in range(c - 2, -1, -1):
                    up = dbl("seg_mul", up)
                    if m >> bit & 1:
                        up = add("seg_mul", up, run)
                acc = add("seg_join", acc, up)
            seg[s] = acc
        # segments without an entry: every operand at infinity
        ev["seg_run"]["both_inf"] += idle * K
        ev["seg_acc"]["both_inf"] += idle * K
        for s in range(nseg):
            if s and (w, s) not in live:
                ev["seg_mul"]["dbl_of_inf"] += c - 1
                ev["seg_mul"]["both_inf"] += bin(s * K).count("1")
                ev["seg_join"]["both_inf"] += 1

        def block_sum(st, vals, b, nblocks):
            sh = []
            for t in range(G2_SUM_BLOCK):
                acc = 0
                for i in range(b * G2_SUM_BLOCK + t, len(vals), nblocks * G2_SUM_BLOCK):
                    acc = add(st, acc, vals[i])
                sh.append(acc)
            h = G2_SUM_BLOCK // 2
            while h:
                for t in range(h):
                    sh[t] = add(st + "_tree", sh[t], sh[t + h])
                h //= 2
            return sh[0]

        blocks = min(-(-nseg // G2_SUM_BLOCK), G2_SUM_BLOCK)
        if blocks <= 1:
            windows.append(block_sum("range", seg, 0, 1))
        else:
            tmp = [block_sum("range", seg, b, blocks) for b in range(blocks)]
            windows.append(block_sum("range2", tmp, 0, 1))

    acc = 0
    for w in range(W - 1, -1, -1):
        if w + 1 < W:
            for _ in range(c):
                acc = dbl("fold", acc)
        acc = add("fold", acc, windows[w])
    return G2Mirror(acc, ev, order_free, windows, dict(c=c, W=W, NB=NB, K=K, nseg=nseg, blocks=blocks))
