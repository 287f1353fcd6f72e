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
