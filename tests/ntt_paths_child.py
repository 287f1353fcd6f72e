"""The body of tests/test_gpu_ntt_paths.py's table-state cases: ONE fresh process, so that the twiddle tables the stand-alone transforms
share per device (poly_api.hip shared_ntt(), NttTables::ensure) are in the state the calls of this process alone leave them in.
  python ntt_paths_child.py ORDER SIZES IDENTITY
    ORDER     a label (down, up, mixed), repeated in every line
    SIZES     log2n of the transforms, comma separated, in the order they run; each size runs forward, then inverse
    IDENTITY  lg of the copy-identity products (identity_operands) that run last, comma separated ("-": none)
After the transforms come the schoolbook-sized products (PRODUCTS, EDGE_PRODUCTS), then the copy-identity products.  One line per call:
  ORDER ntt LOG2N INVERSE SHA256 / ORDER mul NA NB SHA256 / ORDER edge NA NB SHA256 / ORDER ident LG SHA256
and "ntt_paths_child ok" last.  No oracle call is made here: the parent holds the digests against the oracle's (and the copied
expectation's).  The inputs come from fixed seeds through the functions below, which the parent imports: both sides make the same bytes."""
import hashlib
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

R = 0x73EDA753299D7D483339D80809A1D80553BDA402FFFE5BFEFFFFFFFF00000001

ORDERS = {
    "down": list(range(18, -1, -1)),          # every size below 18 reads the 2^18 table: tw_shift = 18 - log2n
    "up": list(range(0, 19)),                 # every call regrows the tables: tw_shift = 0
    "mixed": [12, 18, 12, 5, 18, 11],         # the same size before and after a regrowth
}


def _split(rl, long_first):
    """(na, nb) with na + nb - 1 = rl, one operand about twice the other (halves below 8 terms: no operand of one term past rl = 2)"""
    na = (rl + 1) // 2 if rl < 8 else (rl + 1) // 3
    nb = rl + 1 - na
    return (nb, na) if long_first else (na, nb)


def _products():
    out = []
    for k in (1, 2, 4, 5, 6, 7, 9, 10, 12, 13):
        out.append(_split(1 << k, False))                  # na + nb - 1 = 2^k: no padding
        out.append(_split((1 << (k - 1)) + 1, True))       # just past 2^(k-1): the most padding (at k = 1 both are 2 terms: (1, 2) and (2, 1))
    return out


# (na, nb) of the dense random products whose transform size is each of 2^1, 2^2, 2^4 .. 2^7, 2^9, 2^10, 2^12, 2^13
PRODUCTS = _products()
# (na, nb) of the products with every coefficient r - 1, at 2^10 and 2^12
EDGE_PRODUCTS = [(400, 625), (1500, 2597)]


def transform_log2(na, nb):
    lg = 0
    while (1 << lg) < na + nb - 1:
        lg += 1
    return lg


def rand_fr(seed, n):
    from sonic_amd.workload import rand_fr_array
    return rand_fr_array(np.random.default_rng(seed), n)


def ntt_input(log2n):
    return rand_fr(1000 + log2n, 1 << log2n)


def product_operands(na, nb):
    return rand_fr(50000 + 31 * na + nb, na), rand_fr(90000 + 31 * nb + na, nb)


def edge_operands(na, nb):
    top = np.frombuffer((R - 1).to_bytes(32, "little"), np.uint8)
    return np.tile(top, (na, 1)), np.tile(top, (nb, 1))


def identity_operands(lg, padded=False):
    """a: 2^(lg-2) dense random coefficients; b = 1 + X^e with e = 2^lg - na (the product fills the transform) or, padded,
    e = 2^(lg-1) + 1 - na (na + nb - 1 is just past 2^(lg-1): the most zero padding).  a * b = a + X^e a needs no field arithmetic
    where the two copies do not overlap.  Returns (a, b, e)."""
    na = 1 << (lg - 2)
    e = ((1 << (lg - 1)) + 1 if padded else (1 << lg)) - na
    a = rand_fr(2000 + lg + (100 if padded else 0), na)
    b = np.zeros((e + 1, 32), np.uint8)
    b[0, 0] = 1
    b[e, 0] = 1
    return a, b, e


def identity_pieces(a, e):
    """a * (1 + X^e) as the consecutive pieces of its na + e coefficients: a, zeros, a -- or, where the copies overlap (e < na), a's head,
    the sums a[i] + a[i - e] mod r over the overlap (python integers), a's tail"""
    na = a.shape[0]
    if e >= na:
        return [a, np.zeros((e - na, 32), np.uint8), a]
    raw = a.tobytes()
    val = [int.from_bytes(raw[32 * i:32 * i + 32], "little") for i in range(na)]
    mid = b"".join(((val[i] + val[i - e]) % R).to_bytes(32, "little") for i in range(e, na))
    return [a[:e], np.frombuffer(mid, np.uint8).reshape(na - e, 32), a[na - e:]]


def digest_pieces(pieces):
    h = hashlib.sha256()
    for p in pieces:
        h.update(np.ascontiguousarray(p).data)
    return h.hexdigest()


def main():
    order, sizes, identity = sys.argv[1], sys.argv[2], sys.argv[3]
    sizes = [int(s) for s in sizes.split(",")]
    identity = [] if identity == "-" else [int(s) for s in identity.split(",")]
    from sonic_amd import _lib
    L = _lib.lib()
    _lib.check(L.sonic_init(0))

    def mul(a, b):
        na, nb = a.shape[0], b.shape[0]
        out = np.zeros((na + nb - 1, 32), np.uint8)
        _lib.check(L.sonic_poly_mul_fr(a.ctypes.data, na, b.ctypes.data, nb, out.ctypes.data))
        return digest_pieces([out])

    for log2n in sizes:
        a = ntt_input(log2n)
        for inverse in (0, 1):
            got = a.copy()
            _lib.check(L.sonic_ntt_fr(got.ctypes.data, log2n, inverse))
            print(order, "ntt", log2n, inverse, digest_pieces([got]), flush=True)
    for na, nb in PRODUCTS:
        print(order, "mul", na, nb, mul(*product_operands(na, nb)), flush=True)
    for na, nb in EDGE_PRODUCTS:
        print(order, "edge", na, nb, mul(*edge_operands(na, nb)), flush=True)
    for lg in identity:
        a, b, _ = identity_operands(lg)
        print(order, "ident", lg, mul(a, b), flush=True)
    print("ntt_paths_child ok")


if __name__ == "__main__":
    main()
