"""Python restatement of weights digest v2 and circuit digest v2 (sonic_amd/csrc/fs.hpp), with hashlib and integers only, independent of
the library, and the CSR cases that the host and the GPU tests share.  Test infrastructure, like fs_stream_ref.py."""
import hashlib
import random

R = 0x73EDA753299D7D483339D80809A1D80553BDA402FFFE5BFEFFFFFFFF00000001
LEAF_ENTRIES = 16
FANOUT = 32


def le64(v: int) -> bytes:
    return int(v).to_bytes(8, "little")


def fr(v: int) -> bytes:
    return int(v).to_bytes(32, "little")


def leaf_header(i: int) -> bytes:
    return b"sonic-hip/weights-leaf/v2".ljust(56, b"\0") + le64(i)


def node_header(level: int, j: int) -> bytes:
    return b"sonic-hip/weights-node/v2".ljust(48, b"\0") + le64(level) + le64(j)


def entries_of(row_ptr, col, val):
    """[(stacked row, column, value)] in CSR order"""
    out = []
    for r in range(len(row_ptr) - 1):
        for k in range(row_ptr[r], row_ptr[r + 1]):
            out.append((r, col[k], val[k]))
    return out


def weights_levels(row_ptr, col, val):
    """every level of the tree, leaves first; the last level is [root]"""
    items = []
    for r, c, v in entries_of(row_ptr, col, val):
        items.append(le64(r) + le64(c) + bytes(16))
        items.append(fr(v))
    nleaves = max(1, -(-(len(items) // 2) // LEAF_ENTRIES))
    level = [hashlib.sha256(leaf_header(i) + b"".join(items[32 * i:32 * (i + 1)])).digest() for i in range(nleaves)]
    levels = [level]
    while len(level) > 1:
        level = [hashlib.sha256(node_header(len(levels), j) + b"".join(level[FANOUT * j:FANOUT * (j + 1)])).digest()
                 for j in range(-(-len(level) // FANOUT))]
        levels.append(level)
    return levels


def weights_digest_v2(n, Q, row_ptr, col, val) -> bytes:
    assert len(row_ptr) == 3 * Q + 1 and row_ptr[0] == 0 and row_ptr[-1] == len(col) == len(val)
    root = weights_levels(row_ptr, col, val)[-1][0]
    return hashlib.sha256(b"sonic-hip/weights/v2" + le64(n) + le64(Q) + le64(len(col)) + root).digest()


def circuit_digest_v2(wd: bytes, cs) -> bytes:
    return hashlib.sha256(b"sonic-hip/circuit/v2" + wd + le64(len(cs)) + b"".join(fr(c) for c in cs)).digest()


class Case:
    """one stacked CSR: counts[r] entries in row r, columns a sorted random sample (pins: {(row, position): column}), random values with an
    explicit 0, a 1 and an r - 1 among them where there is room"""

    def __init__(self, name, n, Q, counts, pins=None, seed=0):
        assert len(counts) == 3 * Q and all(0 <= c <= n for c in counts)
        pyr = random.Random(1000003 * n + 1009 * Q + 7 * sum(counts) + seed)
        self.name, self.n, self.Q = name, n, Q
        self.row_ptr, self.col, self.val = [0], [], []
        for r, c in enumerate(counts):
            cols = sorted(pyr.sample(range(n), c))
            for (pr, pos), pc in (pins or {}).items():
                if pr == r:
                    cols[pos] = pc
            assert cols == sorted(set(cols))
            self.col += cols
            self.val += [pyr.randrange(R) for _ in cols]
            self.row_ptr.append(len(self.col))
        nnz = len(self.col)
        for k, v in ((15, 0), (16, R - 1), (0, R - 1), (nnz // 2, 0), (nnz - 1, 1)):      # (both sides of the first leaf boundary, then the ends)
            if 0 <= k < nnz and nnz >= 3:
                self.val[k] = v
        self.cs = [pyr.randrange(R) for _ in range(Q)]

    @property
    def nnz(self):
        return len(self.col)

    def digest(self):
        return weights_digest_v2(self.n, self.Q, self.row_ptr, self.col, self.val)

    def leaves_and_nodes(self):
        return [len(lv) for lv in weights_levels(self.row_ptr, self.col, self.val)]


# nnz -> the tree: 0 and 1 and 16: one leaf; 17: two leaves, one node; 512: 32 leaves under exactly one node; 513: 33 -> 2 -> 1;
# 16385: 1025 -> 33 -> 2 -> 1.  Row shapes mixed in (the comments name them).
_M = [128] * 127 + [127, 2]
CASES = [
    Case("nnz0", 4, 1, [0, 0, 0]),
    # Q = 1; first row empty, last row empty; the one entry sits in column n - 1
    Case("nnz1", 8, 1, [0, 1, 0], pins={(1, 0): 7}),
    # first row empty, a run of empty rows inside the leaf, last row empty, column n - 1
    Case("nnz16", 16, 2, [0, 7, 0, 0, 9, 0], pins={(4, 8): 15}),
    # a row boundary at the leaf boundary: row 0 is exactly leaf 0, row 1 begins leaf 1; every later row empty
    Case("nnz17", 32, 2, [16, 1, 0, 0, 0, 0], pins={(0, 15): 31}),
    # row 0 fills leaf 0, row 1 (40 entries: 16 .. 55) spans the three leaves 1, 2, 3; rows 2 .. 4 and 12 empty inside / between leaves; last row empty
    Case("nnz512", 64, 5, [16, 40, 0, 0, 0, 64, 64, 64, 64, 64, 64, 8, 0, 64, 0]),
    Case("nnz513", 64, 5, [16, 40, 0, 0, 0, 64, 64, 64, 64, 64, 64, 8, 0, 64, 1]),
    Case("nnz16385", 128, 43, _M),
]
TREES = {"nnz0": [1], "nnz1": [1], "nnz16": [1], "nnz17": [2, 1], "nnz512": [32, 1], "nnz513": [33, 2, 1], "nnz16385": [1025, 33, 2, 1]}
