"""What tests/test_gpu_circuit_edges.py rests on, in Python integers and without the library: the thresholds of the circuit kernels as the
sources state them (read with plain regular expressions), the shapes that sit on those thresholds, and the sums the kernels compute.

The mirrored constants below are what the shapes are derived from; source_thresholds() reads the same values from sonic_amd/csrc, and the
first test of the file holds the two against each other -- so a moved threshold fails there, by name, before any shape misses its edge
unnoticed."""
import os
import random
import re
from collections import Counter

import numpy as np

R = 0x73EDA753299D7D483339D80809A1D80553BDA402FFFE5BFEFFFFFFFF00000001
CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "sonic_amd", "csrc")

# ---- the mirrored constants -------------------------------------------------------------------------------------------------------------
CSR_CHUNK = 512              # csr.hpp: entries of one row per wave in k_s_of_u_csr and k_cs_csr
WAVE = 64                    # poly.hip, statement.hip: `k += 64` in those two kernels' entry loops
S_ITEM = 32                  # verify_batch.hip: entries (or diagonal gates) per thread of k_s_of_uv_batch
S_BLOCK = 256                # verify_batch.hip: threads per block there, and partials per trip of k_s_of_uv_finish
CS_BLOCK = 256               # statement.hip: gates per block of k_cs_dense, and partials per trip of k_cs_finish
CSR_FINISH_BLOCK = 256       # poly.hip: partials per trip of k_s_of_u_csr_finish (`c += 256`)
ROW_TERMS_BLOCK = 256        # poly.hip: terms per block of k_csr_row_terms (`ceil_div(total, 256L)`)
CSC_STAGE_MAX_Q = 1024       # poly.hip, s_of_y_csc_enqueue: the Q powers are staged in LDS iff Q <= this
AGG_TILE = 8                 # aggregate.hip: pairs per polynomial launch
AGG_CSC_LDS = 48 * 1024      # aggregate.hip: k_agg_s_of_y_csc stages iff J * Q * 32 <= this
FR_BYTES = 32
T_LEN = (7, 9)               # prove.hip: tlen = 7 * n + 9, the coefficients of the t(X, y) product

MIRRORED = dict(CSR_CHUNK=CSR_CHUNK, WAVE_CSR_U=WAVE, WAVE_CSR_CS=WAVE, S_ITEM=S_ITEM, S_BLOCK=S_BLOCK, CS_BLOCK=CS_BLOCK,
                CSR_FINISH_BLOCK=CSR_FINISH_BLOCK, ROW_TERMS_BLOCK=ROW_TERMS_BLOCK, CSC_STAGE_MAX_Q=CSC_STAGE_MAX_Q, AGG_TILE=AGG_TILE,
                AGG_CSC_LDS=AGG_CSC_LDS, T_LEN=T_LEN)

# which shapes of tests/test_gpu_circuit_edges.py move with each constant
MOVES = dict(CSR_CHUNK="edge_lengths() (section 2) and long_rows_shape() (section 3b)", WAVE_CSR_U="edge_lengths() (section 2)",
             WAVE_CSR_CS="edge_lengths() (section 2)", S_ITEM="edge_lengths(), DIAGONAL_NS (section 2) and uv_finish_shape() (section 3a)",
             S_BLOCK="uv_finish_shape() (section 3a)", CS_BLOCK="long_rows_shape() (section 3b)", CSR_FINISH_BLOCK="long_rows_shape() (section 3b)",
             ROW_TERMS_BLOCK="term_triples() (section 2)", CSC_STAGE_MAX_Q="CSC_STAGE_QS (section 4a)", AGG_TILE="agg_stage_cases() (section 4b)",
             AGG_CSC_LDS="agg_stage_cases() (section 4b)", T_LEN="exact_fill_ns() (section 1)")


def _read(name):
    with open(os.path.join(CSRC, name)) as f:
        return f.read()


def _body(text, start, end):
    """the text between the first `start` and the next `end` after it"""
    a = text.index(start)
    return text[a:text.index(end, a + len(start))]


def _one(pattern, text, what):
    m = re.findall(pattern, text)
    assert len(m) == 1, "%s: %d matches of %r" % (what, len(m), pattern)
    return m[0]


def _product(expr):
    out = 1
    for f in expr.split("*"):
        out *= int(f.strip())
    return out


def source_thresholds():
    """the values of MIRRORED as sonic_amd/csrc states them"""
    csr, poly, stm, vb, agg, prove = (_read(f) for f in ("csr.hpp", "poly.hip", "statement.hip", "verify_batch.hip", "aggregate.hip", "prove.hip"))
    k_u = _body(poly, "void k_s_of_u_csr(", "\n}")
    k_cs = _body(stm, "void k_cs_csr(", "\n}")
    k_fin = _body(poly, "void k_s_of_u_csr_finish(", "\n}")
    enq_y = _body(poly, "void s_of_y_csc_enqueue(", "\n}")
    enq_t = _body(poly, "void csr_row_terms_enqueue(", "\n}")
    assert "CSR_CHUNK" in k_u and "CSR_CHUNK" in k_cs, "k_s_of_u_csr and k_cs_csr cut rows by CSR_CHUNK"
    a, b = _one(r"const long tlen = (\d+) \* n \+ (\d+);", prove, "prove.hip tlen")
    return dict(CSR_CHUNK=int(_one(r"constexpr int CSR_CHUNK = (\d+);", csr, "csr.hpp")),
                WAVE_CSR_U=int(_one(r"k < k1; k \+= (\d+)\)", k_u, "k_s_of_u_csr")),
                WAVE_CSR_CS=int(_one(r"k < k1; k \+= (\d+)\)", k_cs, "k_cs_csr")),
                S_ITEM=int(_one(r"constexpr int S_ITEM = (\d+);", vb, "verify_batch.hip")),
                S_BLOCK=int(_one(r"constexpr int S_BLOCK = (\d+);", vb, "verify_batch.hip")),
                CS_BLOCK=int(_one(r"constexpr int CS_BLOCK = (\d+);", stm, "statement.hip")),
                CSR_FINISH_BLOCK=int(_one(r"c < row_chunk\[r \+ 1\]; c \+= (\d+)\)", k_fin, "k_s_of_u_csr_finish")),
                ROW_TERMS_BLOCK=int(_one(r"ceil_div\(total, (\d+)L\), (?:\1),", enq_t, "csr_row_terms_enqueue")),
                CSC_STAGE_MAX_Q=int(_one(r"const int stage = Q <= (\d+) \? 1 : 0;", enq_y, "s_of_y_csc_enqueue")),
                AGG_TILE=int(_one(r"constexpr int AGG_TILE = (\d+);", agg, "aggregate.hip")),
                AGG_CSC_LDS=_product(_one(r"constexpr size_t AGG_CSC_LDS = ([\d *]+);", agg, "aggregate.hip")),
                T_LEN=(int(a), int(b)))


# ---- shapes on the thresholds -----------------------------------------------------------------------------------------------------------
def tlen(n):
    return T_LEN[0] * n + T_LEN[1]


def is_pow2(v):
    return v > 0 and v & (v - 1) == 0


def transform_size(n):
    """prover_new: the smallest M = 2^lg >= 7n + 9"""
    M = 1
    while M < tlen(n):
        M *= 2
    return M


def exact_fill_ns(lgs=(10, 13, 16)):
    """[(n, exact)]: n whose product fills 2^lg exactly, and (but for the largest) n + 1, whose transform doubles"""
    out = []
    for lg in lgs:
        n, rem = divmod((1 << lg) - T_LEN[1], T_LEN[0])
        assert rem == 0, "2^%d is not 7n + 9 for any n" % lg
        out.append((n, True))
        if lg != lgs[-1]:
            out.append((n + 1, False))
    return out


def edge_lengths():
    """row lengths at every item, wave and chunk edge; the longest is the circuit's n"""
    return [0, 1, S_ITEM - 1, S_ITEM, S_ITEM + 1, WAVE - 1, WAVE, WAVE + 1, CSR_CHUNK - 1, CSR_CHUNK, CSR_CHUNK + 1, 2 * CSR_CHUNK, 2 * CSR_CHUNK + 1]


def term_triples():
    """(wL, wR, wO) row lengths of three constraints with one term fewer than, exactly, and one term more than a block of k_csr_row_terms"""
    B, W = ROW_TERMS_BLOCK, WAVE
    return [(W, W, B - 1 - 2 * W), (W, W, B - 2 * W), (W + 1, W, B - 2 * W)]


DIAGONAL_NS = [S_ITEM - 1, S_ITEM, S_ITEM + 1]
CSC_STAGE_QS = [CSC_STAGE_MAX_Q, CSC_STAGE_MAX_Q + 1]


def agg_stage_cases():
    """[(Q, K)]: a full tile of AGG_TILE pairs whose powers just fit / just miss the LDS budget, beside a last tile of one pair (K = AGG_TILE
    + 1); and one pair alone at its own edge"""
    q8, q1 = AGG_CSC_LDS // (AGG_TILE * FR_BYTES), AGG_CSC_LDS // FR_BYTES
    return [(q8, AGG_TILE + 1), (q8 + 1, AGG_TILE + 1), (q1, 1), (q1 + 1, 1)]


def agg_stages(Q, K):
    """per tile of an aggregate over K pairs: (J, whether k_agg_s_of_y_csc stages the powers)"""
    return [(min(AGG_TILE, K - k0), min(AGG_TILE, K - k0) * Q * FR_BYTES <= AGG_CSC_LDS) for k0 in range(0, K, AGG_TILE)]


def chunks(length):
    return -(-length // CSR_CHUNK)


def uv_blocks(n, lengths):
    """(row items, diagonal items, blocks) of k_s_of_uv_batch over rows of these lengths"""
    row_items = sum(-(-k // S_ITEM) for k in lengths)
    diag = -(-n // S_ITEM)
    return row_items, diag, -(-(row_items + diag) // S_BLOCK)


def uv_finish_shape():
    """(n, Q) of section 3a: 3Q rows of one entry each, one block more than two trips of k_s_of_uv_finish would need at the least"""
    return 2 * S_ITEM, 22000


def long_rows_shape():
    """section 3b: n, and the lengths of wL[0], wR[0], wO[1] (every other row of the Q = 2 circuit is empty)"""
    n = CSR_FINISH_BLOCK * CSR_CHUNK + 1
    return n, (n, n - 1, CSR_CHUNK + 1)


# ---- circuits ---------------------------------------------------------------------------------------------------------------------------
def edge_circuit(seed):
    """Section 2's circuit: n = the longest edge length; constraint q < 13 has rows of lengths L[q], L[q + 4], L[q + 9] (indices mod 13:
    three different lengths, and every length once in each matrix); three more constraints hold term_triples().  Columns: a sorted
    random sample; values: random non-zero, but an explicit zero as the SECOND entry of every row of at least 3 entries whose stacked
    index is a multiple of 5 (never a row's first or last entry, nor a chunk's).
    Returns (n, Q, rows): rows[m * Q + q] = [(column, value)], m = 0, 1, 2 for wL, wR, wO."""
    pyr = random.Random(seed)
    L = edge_lengths()
    n, k = max(L), len(L)
    triples = term_triples()
    Q = k + len(triples)
    lens = [[L[(q + off) % k] for q in range(k)] + [t[m] for t in triples] for m, off in enumerate((0, 4, 9))]
    rows = []
    for m in range(3):
        for q in range(Q):
            cols = sorted(pyr.sample(range(n), lens[m][q]))
            row = [(c, pyr.randrange(1, R)) for c in cols]
            if len(row) >= 3 and (m * Q + q) % 5 == 0:
                row[1] = (row[1][0], 0)
            rows.append(row)
    return n, Q, rows


def row_lengths(rows):
    return [len(r) for r in rows]


def expected_length_multiset():
    want = Counter({k: 3 for k in edge_lengths()})
    for t in term_triples():
        want.update(t)
    return want


def csr_arrays(rows):
    """rows of (column, value) -> (row_ptr, col, val as uint8 [nnz, 32])"""
    row_ptr = np.zeros(len(rows) + 1, np.int64)
    np.cumsum([len(r) for r in rows], out=row_ptr[1:])
    col = np.array([c for r in rows for c, _ in r], np.int64)
    raw = b"".join(int(v).to_bytes(32, "little") for r in rows for _, v in r)
    return row_ptr, col, np.frombuffer(raw, np.uint8).reshape(-1, 32).copy()


def full_rows_circuit(seed, n, Q=1):
    """every row of wL, wR, wO full, random non-zero values"""
    pyr = random.Random(seed)
    return [[(i, pyr.randrange(1, R)) for i in range(n)] for _ in range(3 * Q)]


def short_rows_circuit(seed, n, Q, longest=4):
    """rows of 1 .. longest entries"""
    pyr = random.Random(seed)
    return [[(c, pyr.randrange(1, R)) for c in sorted(pyr.sample(range(n), pyr.randrange(1, longest + 1)))] for _ in range(3 * Q)]


# ---- the sums ---------------------------------------------------------------------------------------------------------------------------
def ints_of(arr):
    """uint8 [k, 32] -> python integers"""
    b = np.ascontiguousarray(arr, np.uint8).tobytes()
    return [int.from_bytes(b[i:i + 32], "little") for i in range(0, len(b), 32)]


def rand_assignment(pyr, n):
    aL = [pyr.randrange(R) for _ in range(n)]
    aR = [pyr.randrange(R) for _ in range(n)]
    return aL, aR, [a * b % R for a, b in zip(aL, aR)]


def cs_of(rows, Q, asg):
    """cs[q] = wL[q] . aL + wR[q] . aR + wO[q] . aO over rows of (column, value); asg = (aL, aR, aO) as integers"""
    return [sum(w * asg[m][i] for m in range(3) for i, w in rows[m * Q + q]) % R for q in range(Q)]
