"""R1CS front end (include/sonic_hip.h, "R1CS front end"): a rank-1 constraint system -- three sparse matrices A, B, C with
<A_i, z> <B_i, z> = <C_i, z> -- compiled to a Sonic constraint system, and witness vectors turned into assignments and constants on the GPU.

    r = R1CS.from_rows(N, n_pub, A_rows, B_rows, C_rows)
    circuit = r.circuit(public=[35])
    wb, cs, bad = r.assign(z)

Column 0 of the matrices is the constant one (z[0] = 1), columns 1..n_pub are the public inputs.  A circuit made here has Q = 3m + n_pub
linear constraints, of the order of its n gates: prove it with core proofs (Prover(..., prepare=False), prove_core_bytes, prove_core_batch)
and verify with verify_core or helped verification; a full proof costs 7 + 4Q multi-scalar multiplications.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib
from .encoding import R_MODULUS, fr_array, witness_vector, _is_torch
from .protocol import SparseCircuit, WitnessBatch


def _csr_of_rows(rows, who: str):
    row_ptr = np.zeros(len(rows) + 1, np.int64)
    cols, vals = [], []
    for i, row in enumerate(rows):
        items = sorted((int(k), int(v) % R_MODULUS) for k, v in dict(row).items())
        cols.extend(k for k, _ in items)
        vals.extend(v for _, v in items)
        row_ptr[i + 1] = row_ptr[i] + len(items)
    return row_ptr, np.array(cols, np.int64), fr_array(vals)


class R1CS:
    """A, B, C of one rank-1 constraint system resident on one GPU (sonic_r1cs_t).  A, B, C: CSR triples (row_ptr int64 [m + 1], col
    int64 [nnz], val uint8 [nnz, 32] canonical Fr or ints), columns strictly increasing within a row, explicit zeros kept."""

    def __init__(self, m: int, N: int, n_pub: int, A, B, C_, device=None):
        self.m, self.N, self.n_pub = int(m), int(N), int(n_pub)
        self._h = C.c_void_p()
        mats, keep = [], []
        for name, M in (("A", A), ("B", B), ("C", C_)):
            row_ptr = np.ascontiguousarray(M[0], dtype=np.int64).reshape(-1)
            col = np.ascontiguousarray(M[1], dtype=np.int64).reshape(-1)
            val = fr_array(M[2])
            if row_ptr.shape[0] != self.m + 1:
                raise ValueError(f"R1CS: {name} needs m + 1 = {self.m + 1} row pointers, got {row_ptr.shape[0]}")
            if col.shape[0] != val.shape[0] or (row_ptr.shape[0] and int(row_ptr[-1]) != col.shape[0]):
                raise ValueError(f"R1CS: {name}: row_ptr[m], col and val disagree on the number of entries")
            keep.append((row_ptr, col, val))
            mats.append(_lib.R1csMatrix(row_ptr.ctypes.data, col.ctypes.data if col.shape[0] else None, val.ctypes.data if val.shape[0] else None))
        L = _lib.lib()
        if device is None:
            _lib.check(L.sonic_r1cs_new(self.m, self.N, self.n_pub, C.byref(mats[0]), C.byref(mats[1]), C.byref(mats[2]), C.byref(self._h)))
        else:
            _lib.check(L.sonic_r1cs_new_on(int(device), self.m, self.N, self.n_pub, C.byref(mats[0]), C.byref(mats[1]), C.byref(mats[2]), C.byref(self._h)))
        shape = (C.c_int64 * 4)()
        _lib.check(L.sonic_r1cs_shape(self._h, shape))
        self.n, self.Q, self.nnz, self.g = (int(v) for v in shape)
        self._compiled = None

    @classmethod
    def from_rows(cls, N: int, n_pub: int, A_rows, B_rows, C_rows, device=None) -> "R1CS":
        """from per-row {column: int} mappings, m of them per matrix; zero values are kept as explicit entries"""
        A_rows, B_rows, C_rows = list(A_rows), list(B_rows), list(C_rows)
        if not (len(A_rows) == len(B_rows) == len(C_rows)):
            raise ValueError("R1CS.from_rows: A, B, C need the same number of rows")
        return cls(len(A_rows), N, n_pub, *(_csr_of_rows(rows, "R1CS.from_rows") for rows in (A_rows, B_rows, C_rows)), device=device)

    @property
    def device(self) -> int:
        return _lib.lib().sonic_r1cs_device(self._h)

    def circuit(self, public=None) -> SparseCircuit:
        """the compiled Sonic constraint system (sonic_r1cs_circuit).  public: the n_pub public inputs (ints) that fill the last n_pub
        constants; None leaves those slots zero (the per-proof constants come from assign)."""
        if self._compiled is None:
            row_ptr = np.zeros(3 * self.Q + 1, np.int64)
            col = np.zeros(max(self.nnz, 1), np.int64)
            val = np.zeros((max(self.nnz, 1), 32), np.uint8)
            cs = np.zeros((self.Q, 32), np.uint8)
            _lib.check(_lib.lib().sonic_r1cs_circuit(self._h, row_ptr.ctypes.data, col.ctypes.data, val.ctypes.data, cs.ctypes.data))
            self._compiled = (row_ptr, col[:self.nnz], val[:self.nnz], cs)
        row_ptr, col, val, cs = self._compiled
        cs = cs.copy()
        if public is not None:
            public = list(public)
            if len(public) != self.n_pub:
                raise ValueError(f"R1CS.circuit: need n_pub = {self.n_pub} public inputs, got {len(public)}")
            if public:
                cs[3 * self.m:] = fr_array([int(v) % R_MODULUS for v in public])
        return SparseCircuit(self.n, self.Q, row_ptr, col, val, cs)

    def assign(self, z, stream=None):
        """K witnesses -> (WitnessBatch of torch uint8 [K, n, 32] tensors on this handle's GPU, [cs of witness k as Q ints],
        [(broken constraint gates, the first or -1)]) (sonic_r1cs_assign).  z: K lists of N ints, or a numpy array / torch tensor, uint8
        [K, N, 32] (canonical Fr) or int64 [K, N] (v < 0 stands for r - |v|), on the CPU or on this handle's GPU.  stream: for a tensor
        on the GPU, the stream whose work produces it (default: the current stream of its device)."""
        try:
            import torch
        except ImportError as e:
            raise RuntimeError("R1CS.assign returns its assignments as torch tensors on the GPU, and torch cannot be imported "
                               f"({e}); call sonic_r1cs_assign of the C ABI with device buffers of your own") from e
        who = "R1CS.assign"
        if not _is_torch(z) and not isinstance(z, np.ndarray):
            rows = [list(w) for w in z]
            if not rows or any(len(w) != self.N for w in rows):
                raise ValueError(f"{who}: need at least one witness, of N = {self.N} values each")
            z = fr_array([int(v) % R_MODULUS for w in rows for v in w]).reshape(len(rows), self.N, 32)
        if len(z.shape) < 2 or int(z.shape[0]) < 1:
            raise ValueError(f"{who}: z is [K, N, 32] uint8 or [K, N] int64 with K >= 1, got shape {tuple(z.shape)}")
        K = int(z.shape[0])
        kind, ptr, stride, zdev, _keep = witness_vector(z, self.N, K, f"{who}: z")
        dev = self.device
        if zdev is not None and zdev != dev:
            raise ValueError(f"{who}: z lies on GPU {zdev}, the handle on GPU {dev}")
        handle = None
        if zdev is not None:
            if stream is None:
                stream = torch.cuda.current_stream(zdev)
            if hasattr(stream, "cuda_stream"):
                if stream.cuda_stream == 0:
                    stream.synchronize()        # (the library takes NULL as "the data is complete")
                stream = stream.cuda_stream
            handle = int(stream) or None
        elif stream is not None:
            raise ValueError(f"{who}: stream is for a tensor on a GPU")
        planes = [torch.empty((K, self.n, 32), dtype=torch.uint8, device=f"cuda:{dev}") for _ in range(3)]
        torch.cuda.current_stream(dev).synchronize()      # the planes may reuse memory that work queued by torch still reads
        cs = np.zeros((K, self.Q, 32), np.uint8)
        bad = np.zeros((K, 2), np.int64)
        _lib.check(_lib.lib().sonic_r1cs_assign(self._h, K, ptr, kind, int(zdev is not None), stride, handle, planes[0].data_ptr(), planes[1].data_ptr(),
                                                planes[2].data_ptr(), 0, cs.ctypes.data, bad.ctypes.data))
        raw = cs.tobytes()
        Q = self.Q
        cs_ints = [[int.from_bytes(raw[32 * (k * Q + q):32 * (k * Q + q) + 32], "little") for q in range(Q)] for k in range(K)]
        return WitnessBatch(planes[0], planes[1], planes[2]), cs_ints, [(int(c), int(f)) for c, f in bad]

    def close(self):
        if getattr(self, "_h", None) is not None and self._h:
            _lib.lib().sonic_r1cs_free(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:       # noqa: BLE001
            pass
