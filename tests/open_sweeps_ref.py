"""Python-integer model of the batched opening chain as built (sonic_amd/csrc/poly.hip, "Horner sweeps"): the two sides of X^0, the
padding in front of a side, the chunk values from a zero carry, the scan over a tile's chunks with one shared multiplier per level, the
scan of the tile values in blocks with the carry folded into a block's first tile, the second sweep from the true carries, and the f(z)
formula.  The chunk length L and the workgroup size (chunks per tile, and tiles per block of the tile scan) are parameters, so that every
edge can be met at a few dozen coefficients; BLOCK and sweep_chunk restate the library's own.

A dense Laurent polynomial is (lo, c) as in open_ref.py: c[i] is the coefficient of X^(lo + i), lo <= 0 <= lo + len(c) - 1."""
from open_ref import R

BLOCK = 256                 # SWEEP_BLOCK
CHUNK_MAX = 16              # SWEEP_CHUNK_MAX


def sweep_chunk(length: int) -> int:
    """open_sweep_chunk (poly.hpp): coefficients per thread that prove() takes at this length"""
    return max(2, min(CHUNK_MAX, length // (BLOCK * 64)))


def sweep_entries(length: int, L: int) -> int:
    """open_sweep_entries (poly.hpp): the size rule of OpenBatch::tiles"""
    return (length // (BLOCK * L) + 2) * (BLOCK + 1) + 2 * (BLOCK + 1)


def _scan(v, mu1, block):
    """inclusive scan of `block` affine maps x -> mu1 x + v[t], level by level as the kernels do it: at distance o the multiplier is
    mu1^o, squared from level to level"""
    v = list(v)
    mu, o = mu1, 1
    while o < block:
        v = [(v[t] + (v[t - o] * mu if t >= o else 0)) % R for t in range(block)]
        mu = mu * mu % R
        o *= 2
    return v


def _side(a, m, up, L, block):
    """one side: a[t], t = 0 .. M - 1, in sweep order; x_t = m (x_{t-1} - a_t) (up) or a_t + m x_{t-1} (down), x_{-1} = 0.  Returns
    (x_0 .. x_{M-1}, end value, tiles used) computed the chunked way."""
    M = len(a)
    tile = block * L
    nb = -(-M // tile)
    pad = nb * tile - M

    def step(x, v):
        return (x - v) * m % R if up else (v + m * x) % R

    def chunk(t0, x, out):
        for t in range(t0, t0 + L):
            if t >= 0:                                   # (t < 0: the padding in front, x stays 0)
                x = step(x, a[t])
                if out is not None:
                    out[t] = x
        return x

    mL = pow(m, L, R)
    # k_sweep_chunks_b: chunk values from 0, scan over the tile, exclusive carries and the tile's value
    carry_in, tile_val = [], []
    for j in range(nb):
        b = [chunk((j * block + t) * L - pad, 0, None) for t in range(block)]
        incl = _scan(b, mL, block)
        carry_in.append([0] + incl[:-1])
        tile_val.append(incl[-1])
    # the power table of the side's first workgroup: (m^L)^t as a product over the bits of t of m^(L 2^k)
    mu = [pow(mL, 1 << k, R) for k in range(block.bit_length())]
    power = []
    for t in range(block):
        p = 1
        for k in range(block.bit_length() - 1):
            if (t >> k) & 1:
                p = p * mu[k] % R
        power.append(p)
    muT = mu[block.bit_length() - 1]
    assert muT == pow(m, tile, R)
    # k_sweep_carries_b: the tile values scanned in blocks of `block` tiles, the carry of a block entering the next one's first tile
    tile_carry, end, carry = [0] * nb, 0, 0
    if nb == 1:
        end = tile_val[0]
    elif nb > 1:
        for bs in range(0, nb, block):
            v = [tile_val[bs + u] if bs + u < nb else 0 for u in range(block)]
            v[0] = (v[0] + carry * muT) % R
            incl = _scan(v, muT, block)
            for u in range(block):
                if bs + u < nb:
                    tile_carry[bs + u] = incl[u - 1] if u else carry
            if bs <= nb - 1 < bs + block:
                end = incl[nb - 1 - bs]
            carry = incl[-1]
    # k_sweep_quotient_b: the recurrence again from the true carry
    x = [None] * M
    for j in range(nb):
        for t in range(block):
            t0 = (j * block + t) * L - pad
            if t0 + L <= 0:
                continue
            c = carry_in[j][t]
            if j > 0:
                c = (c + power[t] * tile_carry[j]) % R
            chunk(t0, c, x)
    return x, end, nb


def open_chunked(lo: int, c, z: int, L: int, block: int = BLOCK):
    """(f(z), quotient coefficients over [lo, lo + len - 2]) the way open_batch_enqueue computes them"""
    n, i0 = len(c), -lo
    assert 0 <= i0 < n and z % R and block & (block - 1) == 0
    c = [v % R for v in c]
    zinv = pow(z, -1, R)
    below, end_b, _ = _side(c[:i0], zinv, True, L, block)                          # w_i, i < i0, upward
    above, end_a, _ = _side(c[:i0:-1], z, False, L, block)                          # a_t = c[n - 1 - t]; x_t = w_{n - 2 - t}
    q = below + above[::-1]
    fz = (c[i0] + z * end_a - end_b) % R
    assert len(q) == n - 1
    return fz, q
