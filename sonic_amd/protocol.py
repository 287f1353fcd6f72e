"""Sonic.Protocol.prove with Sonic.Signature.hscProve (src/Sonic/Protocol.hs:47-109,
src/Sonic/Signature.hs:38-72) over the C ABI."""
from __future__ import annotations

import ctypes as C
import secrets
from dataclasses import dataclass
from typing import List, Optional, Tuple

import numpy as np

from . import _lib
from .encoding import R_MODULUS, fr_array, fr_matrix, fr_to_bytes, g1_from_bytes, g1_to_bytes, witness_vector
from .srs import SRS
from .workload import csr_from_dense


@dataclass
class GateWeights:           # Bulletproofs.ArithmeticCircuit.GateWeights
    wL: list
    wR: list
    wO: list


@dataclass
class ArithCircuit:          # Bulletproofs.ArithmeticCircuit.ArithCircuit (commitmentWeights is never forced)
    weights: GateWeights
    cs: list
    commitmentWeights: object = None


class SparseCircuit:
    """ArithCircuit with its gate weights as ONE CSR of 3Q rows (include/sonic_hip.h, "gate weights as CSR"): rows 0..Q-1 are wL, Q..2Q-1
    wR, 2Q..3Q-1 wO; column i is gate i + 1 of the reference.  row_ptr int64 [3Q + 1], col int64 [nnz] (strictly increasing within a
    row), val uint8 [nnz, 32] canonical Fr, cs uint8 [Q, 32].  Every entry point that takes an ArithCircuit takes this too, with the same
    result bytes as for the densified circuit; the cost of the circuit's part of a proof follows nnz + n instead of Q n."""

    def __init__(self, n: int, Q: int, row_ptr, col, val, cs):
        self.n, self.Q = int(n), int(Q)
        self.row_ptr = np.ascontiguousarray(row_ptr, dtype=np.int64).reshape(-1)
        self.col = np.ascontiguousarray(col, dtype=np.int64).reshape(-1)
        self.val = fr_array(val)
        self.cs = fr_array(cs)
        if self.n < 1 or self.Q < 1 or self.row_ptr.shape[0] != 3 * self.Q + 1 or self.cs.shape[0] != self.Q:
            raise ValueError("SparseCircuit: need n >= 1, Q >= 1, 3Q + 1 row pointers and Q constants")
        if self.col.shape[0] != self.val.shape[0]:
            raise ValueError("SparseCircuit: col and val differ in length")

    @property
    def nnz(self) -> int:
        return int(self.col.shape[0])

    @classmethod
    def from_dense(cls, n: int, Q: int, wL, wR, wO, cs) -> "SparseCircuit":
        """from the dense encodings (uint8 [Q * n, 32] or [Q, n, 32] each): every non-zero entry, in row order"""
        row_ptr, col, val = csr_from_dense(fr_matrix(wL), fr_matrix(wR), fr_matrix(wO), n, Q)
        return cls(n, Q, row_ptr, col, val, fr_array(cs))

    @classmethod
    def from_circuit(cls, circuit: "ArithCircuit") -> "SparseCircuit":
        """the non-zero entries of an ArithCircuit's weights"""
        wL, wR, wO, cs, n, Q = _circuit_arrays(circuit)
        return cls.from_dense(n, Q, wL, wR, wO, cs)

    @classmethod
    def from_rows(cls, n: int, wL_rows, wR_rows, wO_rows, cs) -> "SparseCircuit":
        """from per-row {gate index (0-based): value} mappings, Q of them per matrix; zero values are kept as explicit entries"""
        rows = list(wL_rows) + list(wR_rows) + list(wO_rows)
        Q = len(rows) // 3
        if len(rows) != 3 * Q or len(list(wL_rows)) != Q:
            raise ValueError("SparseCircuit.from_rows: wL, wR, wO need the same number of rows")
        row_ptr = np.zeros(3 * Q + 1, np.int64)
        cols, vals = [], []
        for r, row in enumerate(rows):
            items = sorted((int(k), v) for k, v in dict(row).items())
            cols.extend(k for k, _ in items)
            vals.extend(v for _, v in items)
            row_ptr[r + 1] = row_ptr[r] + len(items)
        return cls(n, Q, row_ptr, np.array(cols, np.int64), fr_array(vals), fr_array(cs))

    def to_dense(self) -> "ArithCircuit":
        """the ArithCircuit the rows stand for (weights as uint8 [Q, n, 32] arrays, cs as uint8 [Q, 32])"""
        W = np.zeros((3 * self.Q, self.n, 32), np.uint8)
        rows = np.repeat(np.arange(3 * self.Q), np.diff(self.row_ptr))
        W[rows, self.col] = self.val
        return ArithCircuit(GateWeights(W[:self.Q], W[self.Q:2 * self.Q], W[2 * self.Q:]), self.cs.copy())

    def _args(self):
        """(row_ptr, col, val) pointers for the C ABI (NULL col / val when there are no entries)"""
        ptr = lambda a: a.ctypes.data if a.shape[0] else None      # noqa: E731
        return self.row_ptr.ctypes.data, ptr(self.col), ptr(self.val)


@dataclass
class Assignment:            # Bulletproofs.ArithmeticCircuit.Assignment
    aL: list
    aR: list
    aO: list


class WitnessBatch:
    """K assignments as a witness source (include/sonic_hip.h, "Witness sources"), accepted by Prover.eval_constraints, prove_batch and
    prove_batch_fs in place of a list of Assignment objects: aL, aR and optionally aO as torch tensors or numpy arrays, uint8 [K, n, 32]
    (canonical Fr) or int64 [K, n] (v < 0 stands for r - |v|), on the handles' GPU or on the CPU, inner dimensions contiguous, any
    leading stride.  aO = None: the GPU sets aO = aL * aR.  stream: for CUDA tensors, the stream whose work produces them (an int handle,
    or a torch stream); default: the current stream of their device.  Nothing is copied or converted on the host."""

    def __init__(self, aL, aR, aO=None, stream=None):
        self.aL, self.aR, self.aO, self.stream = aL, aR, aO, stream
        self.K = int(aL.shape[0]) if hasattr(aL, "shape") and len(aL.shape) else 0

    def __len__(self) -> int:
        return self.K


def _witness_src(aL, aR, aO, stream, n: int, batch, devices, who: str):
    """the sonic_witness_src_t of one source, and what keeps its memory alive; every mismatch is a ValueError, before any C call.
    devices: the GPUs of the handles that will read it"""
    vecs = [witness_vector(v, n, batch, f"{who}: {name}") for name, v in (("aL", aL), ("aR", aR), ("aO", aO)) if v is not None]
    if len({v[0] for v in vecs}) != 1:
        raise ValueError(f"{who}: aL, aR, aO must be of one kind (all uint8 [.., 32] or all int64)")
    if len({v[3] for v in vecs}) != 1:
        raise ValueError(f"{who}: aL, aR, aO must lie in one memory (one GPU, or the CPU)")
    if len({v[2] for v in vecs}) != 1:
        raise ValueError(f"{who}: aL, aR, aO must have the same leading stride")
    kind, _, stride, device, _ = vecs[0]
    if device is not None and any(d != device for d in devices):
        raise ValueError(f"{who}: the tensors lie on GPU {device}, the handle(s) on {sorted(set(devices))}")
    handle = None
    if device is not None:
        import torch
        if stream is None:
            stream = torch.cuda.current_stream(device)
        if hasattr(stream, "cuda_stream"):
            if stream.cuda_stream == 0:
                stream.synchronize()        # (the library takes NULL as "the data is complete": the default stream is waited for here)
            stream = stream.cuda_stream
        handle = int(stream) or None
    elif stream is not None:
        raise ValueError(f"{who}: stream is for tensors on a GPU")
    ptrs = [v[1] for v in vecs] + ([None] if aO is None else [])
    return _lib.WitnessSrc(ptrs[0], ptrs[1], ptrs[2], kind, int(device is not None), stride, handle), [v[4] for v in vecs]


@dataclass
class HscProof:              # Signature.hs:22-29
    hscS: List[Tuple[object, Tuple[int, object]]]
    hscW: List[Tuple[int, object, object]]
    hscQv: object
    hscC: object
    hscU: int
    hscV: int


def _hsc_to_bytes(h: "HscProof") -> bytes:
    if len(h.hscS) != len(h.hscW):
        raise ValueError("HscProof: hscS and hscW must have one entry per (y_j, z_j) pair")

    def fr(v):                   # as is: a non-canonical field element must reach the verifier (which rejects it) unreduced
        return int(v).to_bytes(32, "little")
    out = []
    for cm, (sj, wj) in h.hscS:
        out += [g1_to_bytes(cm), fr(sj), g1_to_bytes(wj)]
    for sjp, wjp, qj in h.hscW:
        out += [fr(sjp), g1_to_bytes(wjp), g1_to_bytes(qj)]
    out += [g1_to_bytes(h.hscQv), g1_to_bytes(h.hscC), fr(h.hscU), fr(h.hscV)]
    return b"".join(out)


def _hsc_from_bytes(b: bytes, m: int) -> "HscProof":
    if len(b) != (2 + 4 * m) * 96 + (2 + 2 * m) * 32:
        raise ValueError(f"HscProof for m = {m} is {(2 + 4 * m) * 96 + (2 + 2 * m) * 32} bytes, got {len(b)}")
    pos = 0

    def g():
        nonlocal pos
        v = g1_from_bytes(b[pos:pos + 96]); pos += 96
        return v

    def f():
        nonlocal pos
        v = int.from_bytes(b[pos:pos + 32], "little"); pos += 32
        return v
    hscS = []
    for _ in range(m):
        cm, sj, wj = g(), f(), g()
        hscS.append((cm, (sj, wj)))
    hscW = []
    for _ in range(m):
        sjp, wjp, qj = f(), g(), g()
        hscW.append((sjp, wjp, qj))
    qv, c, u, v = g(), g(), f(), f()
    return HscProof(hscS, hscW, qv, c, u, v)


@dataclass
class CoreProof:
    """A core proof (include/sonic_hip.h, "Core proofs"): the head of a Proof -- R, T, a, W_a, b, W_b, W_t, s -- and no signature; its
    verifier (verify_core, Verifier.verify_core_batch) evaluates s(z, y) itself.  576 bytes, 336 compressed, whatever Q is."""
    prR: object
    prT: object
    prA: int
    prWa: object
    prB: int
    prWb: object
    prWt: object
    prS: int

    def to_bytes(self, compressed: bool = False) -> bytes:
        """record order R T a Wa b Wb Wt s, serialised from the fields; compressed=True: every point as its 48 compressed bytes
        (sonic_core_proof_compress, which validates the points)"""
        fr = lambda v: int(v).to_bytes(32, "little")     # noqa: E731  (as is: a non-canonical element must reach the verifier unreduced)
        raw = b"".join([g1_to_bytes(self.prR), g1_to_bytes(self.prT), fr(self.prA), g1_to_bytes(self.prWa), fr(self.prB),
                        g1_to_bytes(self.prWb), g1_to_bytes(self.prWt), fr(self.prS)])
        if not compressed:
            return raw
        out = C.create_string_buffer(_lib.CORE_PROOF_SIZE_COMPRESSED)
        _lib.check(_lib.lib().sonic_core_proof_compress(raw, out))
        return out.raw

    @classmethod
    def from_bytes(cls, b: bytes) -> "CoreProof":
        b = bytes(b)
        if len(b) == _lib.CORE_PROOF_SIZE_COMPRESSED:
            out = C.create_string_buffer(_lib.CORE_PROOF_SIZE)
            _lib.check(_lib.lib().sonic_core_proof_decompress(b, out))
            b = out.raw
        if len(b) != _lib.CORE_PROOF_SIZE:
            raise ValueError(f"a core proof is {_lib.CORE_PROOF_SIZE} bytes ({_lib.CORE_PROOF_SIZE_COMPRESSED} compressed), got {len(b)}")
        g = lambda o: g1_from_bytes(b[o:o + 96])                  # noqa: E731
        f = lambda o: int.from_bytes(b[o:o + 32], "little")       # noqa: E731
        return cls(g(0), g(96), f(192), g(224), f(320), g(352), g(448), f(544))


@dataclass
class Proof:                 # Protocol.hs:28-38
    prR: object
    prT: object
    prA: int
    prWa: object
    prB: int
    prWb: object
    prWt: object
    prS: int
    prHscProof: HscProof

    def to_bytes(self, compressed: bool = False) -> bytes:
        """canonical proof bytes (include/sonic_hip.h): the record order of `Proof` then `HscProof`, serialised from the
        fields -- an edited or hand-built Proof is what gets verified, never a cached copy of the prover's output.
        compressed=True: the same record with every point as its 48 compressed bytes (sonic_proof_compress, which validates the points)"""
        if compressed:
            from .compressed import proof_compress
            return proof_compress(self.to_bytes(), len(self.prHscProof.hscS))
        def fr(v):               # as is: a non-canonical field element must reach the verifier (which rejects it) unreduced
            return int(v).to_bytes(32, "little")
        head = [g1_to_bytes(self.prR), g1_to_bytes(self.prT), fr(self.prA), g1_to_bytes(self.prWa), fr(self.prB),
                g1_to_bytes(self.prWb), g1_to_bytes(self.prWt), fr(self.prS)]
        return b"".join(head) + _hsc_to_bytes(self.prHscProof)

    def core(self) -> CoreProof:
        """the head of this proof as a core proof: what verify_core checks soundly, with this proof's own y, z"""
        return CoreProof(self.prR, self.prT, self.prA, self.prWa, self.prB, self.prWb, self.prWt, self.prS)

    @classmethod
    def from_bytes(cls, b: bytes, Q: int) -> "Proof":
        b = bytes(b)
        if len(b) == (7 + 4 * Q) * 48 + (5 + 2 * Q) * 32:         # the compressed form (the two lengths never coincide for one Q)
            from .compressed import proof_decompress
            b = proof_decompress(b, Q)
        if len(b) != (7 + 4 * Q) * 96 + (5 + 2 * Q) * 32:
            raise ValueError(f"proof for Q = {Q} is {(7 + 4 * Q) * 96 + (5 + 2 * Q) * 32} bytes ({(7 + 4 * Q) * 48 + (5 + 2 * Q) * 32} compressed), got {len(b)}")
        g = lambda o: g1_from_bytes(b[o:o + 96])                  # noqa: E731
        f = lambda o: int.from_bytes(b[o:o + 32], "little")       # noqa: E731
        # R T a Wa b Wb Wt s
        return cls(g(0), g(96), f(192), g(224), f(320), g(352), g(448), f(544), _hsc_from_bytes(b[576:], Q))


@dataclass
class RndOracle:             # Protocol.hs:40-45
    rndOracleY: int
    rndOracleZ: int
    rndOracleYZs: List[Tuple[int, int]]


def transcript_len(Q: int) -> int:
    return 8 + 2 * Q


def draw_transcript(Q: int, rng=None) -> List[int]:
    """The prover's `rnd` draws in draw order: c_{n+1..n+4}, y, z, ys, zs, then hscProve's u, v."""
    if rng is None:
        return [secrets.randbelow(R_MODULUS) for _ in range(transcript_len(Q))]
    return [rng.randrange(R_MODULUS) for _ in range(transcript_len(Q))]


class Prover:
    """Circuit (and assignment) resident in HBM across proofs: sonic_prover_* of the C ABI."""

    def __init__(self, srs: SRS, circuit: ArithCircuit, prepare: bool = True):
        self.n, self.Q, suffix, args, _keep = _circuit_args(circuit)
        self._srs = srs
        self._circuit = circuit          # (aggregate_core: the weights digest, made on first use)
        self._weights_digest = None
        self._h = C.c_void_p()
        _lib.check(getattr(_lib.lib(), "sonic_prover_new" + suffix)(srs._h, self.n, self.Q, *args, C.byref(self._h)))
        if prepare:     # a handle exists to prove repeatedly: commit the constraint rows once (sonic_prover_prepare)
            _lib.check(_lib.lib().sonic_prover_prepare(self._h))

    def set_assignment(self, assignment: Assignment):
        aL, aR, aO = fr_array(assignment.aL), fr_array(assignment.aR), fr_array(assignment.aO)
        assert aL.shape[0] == self.n and aR.shape[0] == self.n and aO.shape[0] == self.n
        _lib.check(_lib.lib().sonic_prover_set_assignment(self._h, aL.ctypes.data, aR.ctypes.data, aO.ctypes.data))

    def set_witness(self, aL, aR, aO=None, stream=None) -> None:
        """the assignment from a witness source (sonic_prover_set_witness): each vector a torch tensor or numpy array, uint8 [n, 32]
        (canonical Fr) or int64 [n] (v < 0 stands for r - |v|), on this handle's GPU or on the CPU, contiguous -- or a list of ints.
        aO = None: the GPU sets aO = aL * aR.  A tensor on the GPU is read where it lies, after the work queued on `stream` (default: the
        current stream of its device).  Same proofs and digests as set_assignment of the same values."""
        src, _keep = _witness_src(aL, aR, aO, stream, self.n, None, [self.device], "set_witness")
        _lib.check(_lib.lib().sonic_prover_set_witness(self._h, C.byref(src)))

    @property
    def device(self) -> int:
        return _lib.lib().sonic_prover_device(self._h)

    def set_constants(self, cs) -> None:
        """the constants of the next statement (sonic_prover_set_constants): the handle's cs overwritten in place -- the assignment, the
        prepared rows, the share mode and a captured proof graph stay.  cs: Q ints, or Q x 32 canonical bytes (passed as they are)"""
        raw = _constants_bytes(cs, self.Q, "set_constants")
        _lib.check(_lib.lib().sonic_prover_set_constants(self._h, raw))

    def eval_constraints(self, assignments=None):
        """the constants the assignments satisfy under this handle's weights, and the multiplication gates they break, on the GPU
        (sonic_prover_eval_constraints): ([cs of assignment b as Q ints], [(bad_count, first_bad or -1)]).  assignments: Assignment
        objects, a WitnessBatch (sonic_prover_eval_constraints_src), or None for the handle's resident assignment (one entry)."""
        n, Q = self.n, self.Q
        if isinstance(assignments, WitnessBatch):
            w, B = assignments, len(assignments)
            if B < 1:
                raise ValueError("eval_constraints: need at least one assignment")
            src, _keep = _witness_src(w.aL, w.aR, w.aO, w.stream, n, B, [self.device], "eval_constraints")
            out = np.zeros((B, Q, 32), np.uint8)
            gates = np.zeros((B, 2), np.int64)
            _lib.check(_lib.lib().sonic_prover_eval_constraints_src(self._h, B, C.byref(src), out.ctypes.data, gates.ctypes.data))
            raw = out.tobytes()
            cs = [[int.from_bytes(raw[32 * (b * Q + q):32 * (b * Q + q) + 32], "little") for q in range(Q)] for b in range(B)]
            return cs, [(int(c), int(f)) for c, f in gates]
        if assignments is None:
            B, ptrs = 1, (None, None, None)
        else:
            assignments = list(assignments)
            B = len(assignments)
            if B < 1:
                raise ValueError("eval_constraints: need at least one assignment (or None: the resident one)")
            keep = [np.ascontiguousarray(np.stack([fr_array(getattr(a, k)) for a in assignments])) for k in ("aL", "aR", "aO")]
            if any(a.shape != (B, n, 32) for a in keep):
                raise ValueError(f"eval_constraints: every assignment needs n = {n} values in aL, aR, aO")
            ptrs = tuple(a.ctypes.data for a in keep)
        out = np.zeros((B, Q, 32), np.uint8)
        gates = np.zeros((B, 2), np.int64)
        _lib.check(_lib.lib().sonic_prover_eval_constraints(self._h, B, *ptrs, out.ctypes.data, gates.ctypes.data))
        raw = out.tobytes()
        cs = [[int.from_bytes(raw[32 * (b * Q + q):32 * (b * Q + q) + 32], "little") for q in range(Q)] for b in range(B)]
        return cs, [(int(c), int(f)) for c, f in gates]

    def prove_bytes(self, transcript) -> bytes:
        tr = fr_array(transcript)
        assert tr.shape[0] == transcript_len(self.Q)
        out = C.create_string_buffer(_lib.lib().sonic_proof_size(self.Q))
        _lib.check(_lib.lib().sonic_prover_prove(self._h, tr.ctypes.data, out))
        return out.raw

    def submit(self, transcript) -> None:
        """queue one proof on the GPU and return without waiting (sonic_prover_submit); one proof in flight per handle"""
        tr = fr_array(transcript)
        assert tr.shape[0] == transcript_len(self.Q)
        _lib.check(_lib.lib().sonic_prover_submit(self._h, tr.ctypes.data))

    def collect(self) -> bytes:
        """wait for the submitted proof, finish it on the host, return its bytes (sonic_prover_collect)"""
        out = C.create_string_buffer(_lib.lib().sonic_proof_size(self.Q))
        _lib.check(_lib.lib().sonic_prover_collect(self._h, out))
        return out.raw

    # ---- core proofs: R, T and the openings, no signature (include/sonic_hip.h, "Core proofs") ----
    def prove_core_bytes(self, transcript) -> bytes:
        """the 576 bytes of a core proof (sonic_prover_prove_core); transcript: the four blinders, y, z.  Equal to the first 576 bytes of
        prove_bytes for every transcript that starts with these six."""
        tr = fr_array(transcript)
        assert tr.shape[0] == 6
        out = C.create_string_buffer(_lib.CORE_PROOF_SIZE)
        _lib.check(_lib.lib().sonic_prover_prove_core(self._h, tr.ctypes.data, out))
        return out.raw

    def submit_core(self, transcript) -> None:
        """queue one core proof and return without waiting (sonic_prover_submit_core); one proof in flight per handle"""
        tr = fr_array(transcript)
        assert tr.shape[0] == 6
        _lib.check(_lib.lib().sonic_prover_submit_core(self._h, tr.ctypes.data))

    def collect_core(self) -> bytes:
        """wait for the core proof submit_core queued and return its bytes (sonic_prover_collect_core)"""
        out = C.create_string_buffer(_lib.CORE_PROOF_SIZE)
        _lib.check(_lib.lib().sonic_prover_collect_core(self._h, out))
        return out.raw

    def prove_core_fs(self, circuit_digest: bytes, blinder_seed: bytes):
        """a core proof under its own Fiat-Shamir transcript (sonic_prover_prove_core_fs): (proof bytes, y, z); blinders from witness digest v2"""
        circuit_digest, blinder_seed = bytes(circuit_digest), bytes(blinder_seed)
        if len(circuit_digest) != 32 or len(blinder_seed) != 32:      # the C side reads 32 bytes of each
            raise ValueError("prove_core_fs: circuit_digest and blinder_seed must be 32 bytes each")
        out = C.create_string_buffer(_lib.CORE_PROOF_SIZE)
        yz = C.create_string_buffer(64)
        _lib.check(_lib.lib().sonic_prover_prove_core_fs(self._h, circuit_digest, blinder_seed, out, yz))
        return out.raw, int.from_bytes(yz.raw[:32], "little"), int.from_bytes(yz.raw[32:], "little")

    # ---- ONE proof over several GPUs (sonic_prover_set_share): this handle runs rank's pieces of the proof's MSMs ----
    def set_share(self, rank: int, world: int) -> None:
        _lib.check(_lib.lib().sonic_prover_set_share(self._h, rank, world))

    def prove_share(self, transcript) -> bytes:
        tr = fr_array(transcript)
        assert tr.shape[0] == transcript_len(self.Q)
        out = C.create_string_buffer(_lib.lib().sonic_proof_share_size(self.Q))
        _lib.check(_lib.lib().sonic_prover_prove_share(self._h, tr.ctypes.data, out))
        return out.raw

    def collect_share(self) -> bytes:
        """wait for the submitted share (submit() queues it like a whole proof) and return its bytes"""
        out = C.create_string_buffer(_lib.lib().sonic_proof_share_size(self.Q))
        _lib.check(_lib.lib().sonic_prover_collect_share(self._h, out))
        return out.raw

    def prove_fs(self, circuit_digest: bytes, blinder_seed: bytes):
        """prove with the opt-in Fiat-Shamir transcript (sonic_prover_prove_fs): returns (proof bytes, the 8 + 2Q transcript values
        the proof was made with); six waits for the GPU instead of one"""
        circuit_digest, blinder_seed = bytes(circuit_digest), bytes(blinder_seed)
        if len(circuit_digest) != 32 or len(blinder_seed) != 32:      # the C side reads 32 bytes of each
            raise ValueError("prove_fs: circuit_digest and blinder_seed must be 32 bytes each")
        out = C.create_string_buffer(_lib.lib().sonic_proof_size(self.Q))
        tr = C.create_string_buffer(32 * transcript_len(self.Q))
        _lib.check(_lib.lib().sonic_prover_prove_fs(self._h, bytes(circuit_digest), bytes(blinder_seed), out, tr))
        return out.raw, [int.from_bytes(tr.raw[32 * i:32 * i + 32], "little") for i in range(transcript_len(self.Q))]

    def witness_digest(self) -> bytes:
        """witness digest v2 of the resident assignment (sonic_prover_witness_digest_v2): the SHA-256 tree the GPU computes over aL, aR, aO
        where they lie; cached until the assignment changes"""
        out = C.create_string_buffer(32)
        _lib.check(_lib.lib().sonic_prover_witness_digest_v2(self._h, out))
        return out.raw

    def weights_digest_v2(self) -> bytes:
        """weights digest v2 of the handle's circuit (sonic_prover_weights_digest_v2): the SHA-256 tree the GPU computes over the entries of
        the resident CSR; cached.  A handle made from dense weights is refused: make it from a SparseCircuit."""
        out = C.create_string_buffer(32)
        _lib.check(_lib.lib().sonic_prover_weights_digest_v2(self._h, out))
        return out.raw

    @property
    def device_bytes(self) -> int:
        """the device memory the handle owns now (sonic_prover_device_bytes): every buffer of its own, lane workspaces included, not the
        SRS it borrows.  The signature's state -- the MSM slots 5 and above and the Q buffers of the pairs -- appears with the first full
        proof; core proofs never make it."""
        out = C.c_int64(0)
        _lib.check(_lib.lib().sonic_prover_device_bytes(self._h, C.byref(out)))
        return int(out.value)

    @property
    def host_bytes(self) -> int:
        """the pinned host memory the handle owns now (sonic_prover_host_bytes): the staging of a core proof until the first full proof,
        whose 5 Q + 8 MSM slots then have their pinned twins here"""
        out = C.c_int64(0)
        _lib.check(_lib.lib().sonic_prover_host_bytes(self._h, C.byref(out)))
        return int(out.value)

    def submit_fs(self, circuit_digest: bytes, blinder_seed: bytes) -> None:
        """hand one Fiat-Shamir proof to the handle's host worker and return without waiting (sonic_prover_submit_fs); one proof in flight
        per handle.  The blinders come from witness digest v2, so the bytes differ from prove_fs's for the same seed."""
        circuit_digest, blinder_seed = bytes(circuit_digest), bytes(blinder_seed)
        if len(circuit_digest) != 32 or len(blinder_seed) != 32:      # the C side reads 32 bytes of each
            raise ValueError("submit_fs: circuit_digest and blinder_seed must be 32 bytes each")
        _lib.check(_lib.lib().sonic_prover_submit_fs(self._h, circuit_digest, blinder_seed))

    def collect_fs(self):
        """wait for the proof submit_fs started (sonic_prover_collect_fs): (proof bytes, the 8 + 2Q transcript values it was made with)"""
        out = C.create_string_buffer(_lib.lib().sonic_proof_size(self.Q))
        tr = C.create_string_buffer(32 * transcript_len(self.Q))
        _lib.check(_lib.lib().sonic_prover_collect_fs(self._h, out, tr))
        return out.raw, [int.from_bytes(tr.raw[32 * i:32 * i + 32], "little") for i in range(transcript_len(self.Q))]

    def hsc_prove(self, yzs, u: int, v: int) -> HscProof:
        """hscProve srs sXY yzs (Signature.hs:32-72) for the s(X,Y) of this handle's circuit; u, v: its two `rnd` draws"""
        yzs = list(yzs)
        flat = fr_array([x for pair in yzs for x in pair])
        out = C.create_string_buffer(_lib.lib().sonic_hsc_proof_size(len(yzs)))
        _lib.check(_lib.lib().sonic_prover_hsc_prove(self._h, len(yzs), flat.ctypes.data, fr_to_bytes(u), fr_to_bytes(v), out))
        return _hsc_from_bytes(out.raw, len(yzs))

    def aggregate_core(self, yzs, weights_digest: Optional[bytes] = None) -> bytes:
        """the helper of helped verification (sonic_prover_aggregate_core): ONE signature of correct computation over the (y_k, z_k) of K
        core proofs of this handle's circuit -- the bytes of an HscProof with m = K whose s_k is s(z_k, y_k) and whose u, v come from the
        aggregate's own transcript (fs_aggregate_challenges).  weights_digest: fs_weights_digest of the circuit (default: computed from
        the circuit the handle was made with, once).  Needs no assignment."""
        yzs = list(yzs)
        if not yzs or any(len(pair) != 2 for pair in yzs):
            raise ValueError("aggregate_core: yzs must hold at least one (y_k, z_k) pair")
        if weights_digest is None:
            if self._weights_digest is None:
                self._weights_digest = fs_weights_digest(self._circuit)
            weights_digest = self._weights_digest
        if len(bytes(weights_digest)) != 32:
            raise ValueError("aggregate_core: a weights digest is 32 bytes")
        flat = fr_array([x for pair in yzs for x in pair])
        out = C.create_string_buffer(_lib.lib().sonic_hsc_proof_size(len(yzs)))
        _lib.check(_lib.lib().sonic_prover_aggregate_core(self._h, bytes(weights_digest), len(yzs), flat.ctypes.data, out))
        return out.raw

    def close(self):
        if self._h:
            _lib.lib().sonic_prover_free(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def proof_from_shares(Q: int, shares, transcript) -> bytes:
    """the shares of all ranks (any order) -> canonical proof bytes (sonic_proof_from_shares; host only)"""
    shares = list(shares)
    blob = b"".join(bytes(s) for s in shares)
    tr = fr_array(transcript)
    out = C.create_string_buffer(_lib.lib().sonic_proof_size(Q))
    _lib.check(_lib.lib().sonic_proof_from_shares(Q, len(shares), blob, tr.ctypes.data, out))
    return out.raw


def share_plan(n: int, Q: int, prepared: bool, world: int, nb: int = 0, w: int = 0):
    """the plan of one proof over `world` ranks: per rank (pieces, cost) with pieces = 7 + 4Q pairs (lo, hi) in units of 1 / 2^20 of
    each MSM's terms (slot order R, T, W_a, W_b, W_t, [S_j, W_j]_j, [W'_j, Q_j]_j, Q_v, C)"""
    K = 7 + 4 * Q
    out = []
    for r in range(world):
        buf = (C.c_uint32 * (2 * K))()
        cost = C.c_double()
        _lib.check(_lib.lib().sonic_prove_share_plan(n, Q, int(prepared), world, r, nb, w, buf, C.byref(cost)))
        out.append(([(buf[2 * i], buf[2 * i + 1]) for i in range(K)], cost.value))
    return out


def device_count() -> int:
    """GPUs this process can drive (sonic_device_count)"""
    n = C.c_int(0)
    _lib.check(_lib.lib().sonic_device_count(C.byref(n)))
    return n.value


def _handle_array(provers):
    arr = (C.c_void_p * len(provers))(*[p._h for p in provers])
    return arr


def prove_shared(provers, transcript) -> bytes:
    """ONE proof made by several prover handles of the same circuit and assignment, one per GPU (or several on one GPU), from this
    one process: sonic_prove_shared runs handle r as rank r of len(provers) on a host thread of its own and combines the shares on
    the host.  Byte-identical to Prover.prove_bytes on one GPU.  No torch, no RCCL (the one-process-per-GPU form is
    sonic_amd.distributed.ShardedProver)."""
    provers = list(provers)
    Q = provers[0].Q
    tr = fr_array(transcript)
    assert tr.shape[0] == transcript_len(Q)
    out = C.create_string_buffer(_lib.lib().sonic_proof_size(Q))
    _lib.check(_lib.lib().sonic_prove_shared(_handle_array(provers), len(provers), tr.ctypes.data, out))
    return out.raw


def _constants_bytes(cs, Q: int, who: str) -> bytes:
    """one statement's constants as Q x 32 bytes: bytes as they are (a non-canonical value must reach the library, which refuses it),
    ints little-endian without reduction"""
    raw = bytes(cs) if isinstance(cs, (bytes, bytearray, memoryview)) else b"".join(int(c).to_bytes(32, "little") for c in cs)
    if len(raw) != 32 * Q:
        raise ValueError(f"{who}: need Q = {Q} constants (32 bytes each)")
    return raw


def prove_batch(provers, transcripts, assignments=None, constants=None) -> List[bytes]:
    """`mapM prove` over K statements of one circuit, spread over several prover handles (sonic_prove_batch: proof i on handle
    i % len(provers), one host thread per handle, no collective): the throughput mode of BASELINE's "batch of 64 independent proofs
    streamed over 8 GPUs".  assignments: K Assignment objects, a WitnessBatch of K assignments (sonic_prove_batch_src: tensors or
    arrays read where they lie), or None to prove every statement with the handles' resident assignment (then only the transcripts
    differ).  constants: None, or one cs (Q ints or Q x 32 bytes) per proof -- one statement
    per proof (sonic_prove_batch_statements); afterwards each handle holds the constants of the last proof it ran."""
    provers = list(provers)
    Q, n = provers[0].Q, provers[0].n
    K = len(transcripts)
    tr = np.ascontiguousarray(np.stack([fr_array(t) for t in transcripts]) if K else np.zeros((0, transcript_len(Q), 32), np.uint8))
    assert tr.shape[1] == transcript_len(Q)
    psz = _lib.lib().sonic_proof_size(Q)
    out = np.zeros((max(K, 1), psz), np.uint8)
    status = (C.c_int * max(K, 1))()
    aL = aR = aO = None
    if isinstance(assignments, WitnessBatch):
        if len(assignments) != K:
            raise ValueError("prove_batch: one assignment per proof")
        cs = None
        if constants is not None:
            constants = list(constants)
            if len(constants) != K:
                raise ValueError("prove_batch: one set of constants per proof")
            cs = b"".join(_constants_bytes(c, Q, "prove_batch") for c in constants) or bytes(32)
        w = assignments
        src, _keep = _witness_src(w.aL, w.aR, w.aO, w.stream, n, K, [p.device for p in provers], "prove_batch") if K else (_lib.WitnessSrc(), None)
        _lib.check(_lib.lib().sonic_prove_batch_src(_handle_array(provers), len(provers), K, C.byref(src), cs, tr.ctypes.data, out.ctypes.data, status))
        return [out[i].tobytes() for i in range(K)]
    if assignments is not None:
        assert len(assignments) == K
        aL = np.ascontiguousarray(np.stack([fr_array(a.aL) for a in assignments]))
        aR = np.ascontiguousarray(np.stack([fr_array(a.aR) for a in assignments]))
        aO = np.ascontiguousarray(np.stack([fr_array(a.aO) for a in assignments]))
        assert aL.shape[1] == n and aR.shape == aL.shape and aO.shape == aL.shape
    ptr = lambda a: None if a is None else a.ctypes.data       # noqa: E731
    if constants is not None:
        constants = list(constants)
        if len(constants) != K:
            raise ValueError("prove_batch: one set of constants per proof")
        cs = b"".join(_constants_bytes(c, Q, "prove_batch") for c in constants) or bytes(32)
        _lib.check(_lib.lib().sonic_prove_batch_statements(_handle_array(provers), len(provers), K, ptr(aL), ptr(aR), ptr(aO), cs, tr.ctypes.data, out.ctypes.data, status))
        return [out[i].tobytes() for i in range(K)]
    _lib.check(_lib.lib().sonic_prove_batch(_handle_array(provers), len(provers), K, ptr(aL), ptr(aR), ptr(aO), tr.ctypes.data, out.ctypes.data, status))
    return [out[i].tobytes() for i in range(K)]


def prove_batch_fs(provers, digests, seeds, assignments=None, constants=None):
    """K Fiat-Shamir proofs of one circuit spread over several prover handles (sonic_prove_batch_fs: proof i on handle i % len(provers), one
    host thread per handle walking the six passes): [(proof bytes, transcript values), ...].  digests, seeds: one circuit digest and one
    blinder seed (32 bytes each) per proof -- with per-proof constants, digests[i] = fs_circuit_digest_resume(midstate, constants[i]).
    assignments: K Assignment objects, a WitnessBatch (sonic_prove_batch_fs_src), or None (the handles' resident assignments);
    constants: one cs per proof, or None."""
    provers = list(provers)
    Q, n = provers[0].Q, provers[0].n
    digests, seeds = [bytes(d) for d in digests], [bytes(s) for s in seeds]
    K = len(digests)
    if len(seeds) != K or any(len(b) != 32 for b in digests + seeds):
        raise ValueError("prove_batch_fs: one 32-byte circuit digest and one 32-byte seed per proof")
    psz, tl = _lib.lib().sonic_proof_size(Q), transcript_len(Q)
    out = np.zeros((max(K, 1), psz), np.uint8)
    tr = np.zeros((max(K, 1), tl, 32), np.uint8)
    status = (C.c_int * max(K, 1))()
    aL = aR = aO = None
    wsrc = None
    if isinstance(assignments, WitnessBatch):
        if len(assignments) != K:
            raise ValueError("prove_batch_fs: one assignment per proof")
        w = assignments
        wsrc, _keep = _witness_src(w.aL, w.aR, w.aO, w.stream, n, K, [p.device for p in provers], "prove_batch_fs") if K else (_lib.WitnessSrc(), None)
    elif assignments is not None:
        if len(assignments) != K:
            raise ValueError("prove_batch_fs: one assignment per proof")
        aL, aR, aO = (np.ascontiguousarray(np.stack([fr_array(getattr(a, k)) for a in assignments])) for k in ("aL", "aR", "aO"))
        if any(a.shape != (K, n, 32) for a in (aL, aR, aO)):
            raise ValueError(f"prove_batch_fs: every assignment needs n = {n} values in aL, aR, aO")
    cs = None
    if constants is not None:
        constants = list(constants)
        if len(constants) != K:
            raise ValueError("prove_batch_fs: one set of constants per proof")
        cs = b"".join(_constants_bytes(c, Q, "prove_batch_fs") for c in constants) or bytes(32)
    ptr = lambda a: None if a is None else a.ctypes.data       # noqa: E731
    if wsrc is not None:
        _lib.check(_lib.lib().sonic_prove_batch_fs_src(_handle_array(provers), len(provers), K, C.byref(wsrc), cs, b"".join(digests) or bytes(32),
                                                       b"".join(seeds) or bytes(32), out.ctypes.data, tr.ctypes.data, status))
    else:
        _lib.check(_lib.lib().sonic_prove_batch_fs(_handle_array(provers), len(provers), K, ptr(aL), ptr(aR), ptr(aO), cs, b"".join(digests) or bytes(32),
                                                   b"".join(seeds) or bytes(32), out.ctypes.data, tr.ctypes.data, status))
    raw_tr = tr.tobytes()
    return [(out[i].tobytes(), [int.from_bytes(raw_tr[32 * (i * tl + k):32 * (i * tl + k) + 32], "little") for k in range(tl)]) for i in range(K)]


def _core_batch_args(provers, K, assignments, constants, who):
    """what the two core batch calls share: the witness source (or None: the resident assignments) and the constants (or None)"""
    Q, n = provers[0].Q, provers[0].n
    src = keep = None
    if assignments is not None:
        if not isinstance(assignments, WitnessBatch):
            assignments = list(assignments)
            cols = [np.ascontiguousarray(np.stack([fr_array(getattr(a, k)) for a in assignments])) if assignments else np.zeros((0, n, 32), np.uint8) for k in ("aL", "aR", "aO")]
            assignments = WitnessBatch(*cols)
        if len(assignments) != K:
            raise ValueError(f"{who}: one assignment per proof")
        if K:
            src, keep = _witness_src(assignments.aL, assignments.aR, assignments.aO, assignments.stream, n, K, [p.device for p in provers], who)
    cs = None
    if constants is not None:
        constants = list(constants)
        if len(constants) != K:
            raise ValueError(f"{who}: one set of constants per proof")
        cs = b"".join(_constants_bytes(c, Q, who) for c in constants) or bytes(32)
    return (C.byref(src) if src is not None else None), cs, keep


def prove_core_batch(provers, transcripts, assignments=None, constants=None) -> List[bytes]:
    """K core proofs of one circuit over several prover handles (sonic_prove_batch_core_src; proof i on handle i % len(provers)).
    transcripts: six values per proof; assignments: Assignment objects, a WitnessBatch, or None (the resident assignments);
    constants: one cs per proof, or None."""
    provers = list(provers)
    K = len(transcripts)
    tr = np.ascontiguousarray(np.stack([fr_array(t) for t in transcripts]) if K else np.zeros((0, 6, 32), np.uint8))
    assert tr.shape[1] == 6
    src, cs, _keep = _core_batch_args(provers, K, assignments, constants, "prove_core_batch")
    out = np.zeros((max(K, 1), _lib.CORE_PROOF_SIZE), np.uint8)
    status = (C.c_int * max(K, 1))()
    _lib.check(_lib.lib().sonic_prove_batch_core_src(_handle_array(provers), len(provers), K, src, cs, tr.ctypes.data, out.ctypes.data, status))
    return [out[i].tobytes() for i in range(K)]


def prove_core_batch_fs(provers, digests, seeds, assignments=None, constants=None):
    """K Fiat-Shamir core proofs (sonic_prove_batch_core_fs_src): [(proof bytes, y, z), ...]; digests, seeds, assignments, constants as
    for prove_batch_fs"""
    provers = list(provers)
    digests, seeds = [bytes(d) for d in digests], [bytes(s) for s in seeds]
    K = len(digests)
    if len(seeds) != K or any(len(b) != 32 for b in digests + seeds):
        raise ValueError("prove_core_batch_fs: one 32-byte circuit digest and one 32-byte seed per proof")
    src, cs, _keep = _core_batch_args(provers, K, assignments, constants, "prove_core_batch_fs")
    out = np.zeros((max(K, 1), _lib.CORE_PROOF_SIZE), np.uint8)
    yz = np.zeros((max(K, 1), 64), np.uint8)
    status = (C.c_int * max(K, 1))()
    _lib.check(_lib.lib().sonic_prove_batch_core_fs_src(_handle_array(provers), len(provers), K, src, cs, b"".join(digests) or bytes(32),
                                                        b"".join(seeds) or bytes(32), out.ctypes.data, yz.ctypes.data, status))
    return [(out[i].tobytes(), int.from_bytes(yz[i, :32].tobytes(), "little"), int.from_bytes(yz[i, 32:].tobytes(), "little")) for i in range(K)]


class _Statement(C.Structure):          # sonic_statement_t
    _fields_ = [(k, C.c_void_p) for k in ("wL", "wR", "wO", "cs", "aL", "aR", "aO", "transcript")]


def prove_many(replicas, statements) -> List[bytes]:
    """`mapM (\\(asg, circ, tr) -> prove srs asg circ)` over K INDEPENDENT statements of one shape (n, Q) -- every proof its own circuit,
    assignment and transcript -- spread over the SRS replicas, one per GPU (sonic_prove_many: two host threads per replica making
    one-shot calls; no collective).  statements: (Assignment, ArithCircuit, transcript) triples.  BASELINE's "batch of 64 independent
    proofs streamed over 8 GPUs"."""
    replicas, statements = list(replicas), list(statements)
    K = len(statements)
    if K == 0:
        return []
    keep, arr = [], (_Statement * K)()
    n = Q = None
    for i, (asg, circ, tr) in enumerate(statements):
        wL, wR, wO, cs, n_i, Q_i = _circuit_arrays(circ)
        aL, aR, aO, t = fr_array(asg.aL), fr_array(asg.aR), fr_array(asg.aO), fr_array(tr)
        if n is None:
            n, Q = n_i, Q_i
        if (n_i, Q_i) != (n, Q) or aL.shape[0] != n or aR.shape[0] != n or aO.shape[0] != n or t.shape[0] != transcript_len(Q):
            raise ValueError(f"prove_many: statement {i} has another shape than statement 0 (n = {n}, Q = {Q})")
        bufs = (wL, wR, wO, cs, aL, aR, aO, t)
        keep.append(bufs)
        for name, b in zip(("wL", "wR", "wO", "cs", "aL", "aR", "aO", "transcript"), bufs):
            setattr(arr[i], name, b.ctypes.data)
    psz = _lib.lib().sonic_proof_size(Q)
    out = np.zeros((K, psz), np.uint8)
    status = (C.c_int * K)()
    srs_arr = (C.c_void_p * len(replicas))(*[r._h for r in replicas])
    _lib.check(_lib.lib().sonic_prove_many(srs_arr, len(replicas), n, Q, arr, K, out.ctypes.data, status))
    return [out[i].tobytes() for i in range(K)]


class ProverPipeline:
    """`mapM prove` over a stream of statements of one circuit, from one host thread: `depth` prover handles used in turn, so that
    while proof i is being waited for and finished, proof i + 1 is already running (its polynomial building and sorts fill the
    reduction tail of proof i).  Same bytes as proving one after the other."""

    def __init__(self, srs: SRS, circuit: ArithCircuit, depth: int = 2, prepare: bool = True):
        self.provers = [Prover(srs, circuit, prepare) for _ in range(max(1, depth))]

    def set_assignment(self, assignment: Assignment):
        for p in self.provers:
            p.set_assignment(assignment)

    def prove_all(self, transcripts) -> List[bytes]:
        k = len(self.provers)
        out: List[bytes] = []
        inflight: List[int] = []          # indices of the submitted, not yet collected proofs, oldest first
        try:
            for i, tr in enumerate(transcripts):
                if len(inflight) == k:
                    out.append(self.provers[inflight.pop(0) % k].collect())
                self.provers[i % k].submit(tr)
                inflight.append(i)
            while inflight:
                out.append(self.provers[inflight.pop(0) % k].collect())
        finally:
            for i in inflight:            # an error on the way: leave no handle with a proof in flight
                try:
                    self.provers[i % k].collect()
                except Exception:
                    pass
        return out

    def close(self):
        for p in self.provers:
            p.close()


def prove(srs: SRS, assignment: Assignment, circuit: ArithCircuit, transcript: Optional[list] = None, rng=None):
    """prove :: SRS -> Assignment Fr -> ArithCircuit Fr -> m (Proof, RndOracle) (Protocol.hs:47-52).
    `transcript` makes the MonadRandom draws explicit (reproducible proofs); default: fresh draws."""
    n, Q, suffix, args, _keep = _circuit_args(circuit)
    if srs.srsD < 7 * n:   # Protocol.hs:54-55 (checked again by the library)
        raise _lib.SonicError(1, f"Parameter d is not large enough: {srs.srsD} should be greater than {7 * n}")
    if transcript is None:
        transcript = draw_transcript(Q, rng)
    # the one-shot entry point (sonic_prove, sonic_prove_csr): circuit, assignment and transcript as host buffers, like the reference's
    # call; the library parks the handle's shell (streams, workspaces, twiddle tables) for the next call of the same shape -- making and
    # freeing a handle per call cost ~7 ms of stream / pinned-memory set-up around a 2-ms proof at the reference's own benchmark sizes
    aL, aR, aO = fr_array(assignment.aL), fr_array(assignment.aR), fr_array(assignment.aO)
    if aL.shape[0] != n or aR.shape[0] != n or aO.shape[0] != n:
        raise ValueError(f"assignment and {'circuit' if suffix else 'weight rows'} differ in length")
    tr = fr_array(transcript)
    if tr.shape[0] != 8 + 2 * Q:
        raise ValueError(f"transcript needs 8 + 2Q = {8 + 2 * Q} elements")
    out = C.create_string_buffer(_lib.lib().sonic_proof_size(Q))
    _lib.check(getattr(_lib.lib(), "sonic_prove" + suffix)(srs._h, n, Q, *args, aL.ctypes.data, aR.ctypes.data, aO.ctypes.data, tr.ctypes.data, out))
    t = [int(v) % R_MODULUS for v in transcript]
    oracle = RndOracle(t[4], t[5], list(zip(t[6:6 + Q], t[6 + Q:6 + 2 * Q])))
    return Proof.from_bytes(out.raw, Q), oracle


def _circuit_arrays(circuit: ArithCircuit, who: str = ""):
    w = circuit.weights
    wL, wR, wO = fr_matrix(w.wL), fr_matrix(w.wR), fr_matrix(w.wO)
    cs = fr_array(circuit.cs)
    Q = cs.shape[0]
    if Q < 1 or wL.shape[0] % Q or wL.shape[0] == 0 or wR.shape != wL.shape or wO.shape != wL.shape:
        raise ValueError(who + "need Q >= 1 weight rows of equal length n >= 1 in wL, wR, wO")
    return wL, wR, wO, cs, wL.shape[0] // Q, Q


def _circuit_args(circuit, who: str = ""):
    """either circuit type, shapes checked -> (n, Q, suffix, args, keep): the entry points that take a circuit are called
    `sonic_<name><suffix>` ("" dense, "_csr" sparse) with the pointers `args` (gate weights, then cs) where the circuit goes; `keep`
    holds the arrays they point into"""
    if isinstance(circuit, SparseCircuit):
        return circuit.n, circuit.Q, "_csr", (*circuit._args(), circuit.cs.ctypes.data), circuit
    wL, wR, wO, cs, n, Q = keep = _circuit_arrays(circuit, who)
    return n, Q, "", (wL.ctypes.data, wR.ctypes.data, wO.ctypes.data, cs.ctypes.data), keep


def fs_circuit_digest(circuit: ArithCircuit) -> bytes:
    """SHA-256 of (n, Q, wL, wR, wO, cs): the statement part of the Fiat-Shamir transcript, once per circuit"""
    n, Q, suffix, args, _keep = _circuit_args(circuit)         # (sparse: the same digest from the rows; host only)
    out = C.create_string_buffer(32)
    _lib.check(getattr(_lib.lib(), "sonic_fs_circuit_digest" + suffix)(n, Q, *args, out))
    return out.raw


def fs_circuit_midstate(circuit) -> bytes:
    """the SHA-256 state of the circuit digest after the gate weights (sonic_fs_circuit_midstate[_csr]; the circuit's cs is not read):
    O(Q n) hashing once per circuit, after which fs_circuit_digest_resume gives each statement's digest from Q x 32 bytes"""
    n, Q, suffix, args, _keep = _circuit_args(circuit)
    out = C.create_string_buffer(_lib.FS_MIDSTATE_SIZE)
    _lib.check(getattr(_lib.lib(), "sonic_fs_circuit_midstate" + suffix)(n, Q, *args[:-1], out))
    return out.raw


def fs_circuit_digest_resume(state: bytes, cs) -> bytes:
    """fs_circuit_digest of the circuit behind `state` with the constants cs (Q ints or Q x 32 bytes), byte for byte"""
    state = bytes(state)
    if len(state) != _lib.FS_MIDSTATE_SIZE:
        raise ValueError(f"fs_circuit_digest_resume: a midstate is {_lib.FS_MIDSTATE_SIZE} bytes")
    Q = int.from_bytes(state[104:112], "little")
    raw = _constants_bytes(cs, Q, "fs_circuit_digest_resume") if 0 < Q < 1 << 40 else bytes(32)      # (a bad Q: the library refuses the midstate)
    out = C.create_string_buffer(32)
    _lib.check(_lib.lib().sonic_fs_circuit_digest_resume(state, raw, out))
    return out.raw


def fs_srs_id(srs: SRS) -> bytes:
    """SHA-256 of d, g^x, g^{alpha x}, g^{1/x}, g^{alpha/x}: what binds a Fiat-Shamir transcript to one reference string"""
    out = C.create_string_buffer(32)
    _lib.check(_lib.lib().sonic_fs_srs_id(srs._h, out))
    return out.raw


def fs_challenges(srs: SRS, circuit: ArithCircuit, proof: Proof) -> RndOracle:
    """the RndOracle a Fiat-Shamir proof determines (sonic_fs_challenges_v2)"""
    n, Q = _circuit_args(circuit)[:2]
    raw = proof.to_bytes()
    if len(raw) != _lib.lib().sonic_proof_size(Q):
        raise ValueError("fs_challenges: the proof does not have Q entries in its hsc lists")
    out = C.create_string_buffer(32 * (4 + 2 * Q))
    _lib.check(_lib.lib().sonic_fs_challenges_v2(n, Q, srs.srsD, fs_circuit_digest(circuit), fs_srs_id(srs), raw, out))
    v = [int.from_bytes(out.raw[32 * i:32 * i + 32], "little") for i in range(4 + 2 * Q)]
    return RndOracle(v[0], v[1], list(zip(v[2:2 + Q], v[2 + Q:2 + 2 * Q])))


def prove_fs(srs: SRS, assignment: Assignment, circuit: ArithCircuit, blinder_seed: Optional[bytes] = None):
    """prove with every `rnd` draw of the reference (Protocol.hs:58,66,76,84-85; Signature.hs:48,60) replaced by the hash of what
    precedes it: (Proof, RndOracle); the blinders come from `blinder_seed` (32 bytes, default fresh)"""
    seed = secrets.token_bytes(32) if blinder_seed is None else bytes(blinder_seed)
    p = Prover(srs, circuit, prepare=False)
    try:
        p.set_assignment(assignment)
        raw, t = p.prove_fs(fs_circuit_digest(circuit), seed)
    finally:
        p.close()
    Q = p.Q
    return Proof.from_bytes(raw, Q), RndOracle(t[4], t[5], list(zip(t[6:6 + Q], t[6 + Q:6 + 2 * Q])))


def verify_fs(srs: SRS, circuit: ArithCircuit, proof: Proof) -> bool:
    """verify for a Fiat-Shamir proof: the challenges are recomputed from the circuit and the proof (sonic_verify_fs)"""
    n, Q, suffix, args, _keep = _circuit_args(circuit)
    h = proof.prHscProof
    if len(h.hscS) != Q or len(h.hscW) != Q:
        return False
    ok = C.c_int(0)
    _lib.check(getattr(_lib.lib(), "sonic_verify_fs" + suffix)(srs._h, n, Q, *args, proof.to_bytes(), C.byref(ok)))
    return bool(ok.value)


def hsc_prove(srs: SRS, circuit: ArithCircuit, yzs, u: Optional[int] = None, v: Optional[int] = None, rng=None) -> HscProof:
    """hscProve :: SRS -> BiVLaurent Fr -> [(Fr, Fr)] -> m HscProof (Signature.hs:32-72), with sXY = sPoly of `circuit`'s weights
    (Constraints.hs:34-53); u, v default to fresh draws"""
    draw = (lambda: rng.randrange(1, R_MODULUS)) if rng is not None else (lambda: secrets.randbelow(R_MODULUS - 1) + 1)
    p = Prover(srs, circuit, prepare=False)
    try:
        return p.hsc_prove(yzs, draw() if u is None else u, draw() if v is None else v)
    finally:
        p.close()


def from_x(p) -> dict:
    """fromX :: VLaurent f -> BiVLaurent f (Utils.hs:23-24): the univariate polynomial {exponent: coeff} in X as a bivariate one,
    constant in Y -- in the nested form hsc_prove_poly takes.  The prover itself never lifts: evaluating Y := y is a ring
    homomorphism, so tPoly's product (Constraints.hs:56-65) is formed in the univariate ring."""
    return {int(ex): {0: int(c)} for ex, c in (p.items() if isinstance(p, dict) else p) if int(c) % R_MODULUS}


def from_y(p) -> dict:
    """fromY :: VLaurent f -> BiVLaurent f (Utils.hs:26-27): `monomial 0` -- a polynomial in Y as the X^0 coefficient"""
    inner = {int(ey): int(c) for ey, c in (p.items() if isinstance(p, dict) else p) if int(c) % R_MODULUS}
    return {0: inner} if inner else {}


def biv_add(a: dict, b: dict) -> dict:
    """sum of two BiVLaurent polynomials in the nested form (coefficients mod r, zero terms dropped)"""
    out = {ex: dict(inner) for ex, inner in a.items()}
    for ex, inner in b.items():
        row = out.setdefault(ex, {})
        for ey, c in inner.items():
            row[ey] = (row.get(ey, 0) + c) % R_MODULUS
    return {ex: {ey: c for ey, c in inner.items() if c} for ex, inner in out.items() if any(inner.values())}


def _biv_terms(sXY):
    """BiVLaurent Fr as {x_exp: {y_exp: coeff}} (X outside, Y inside, like poly's nested sparse form) or [(x_exp, y_exp, coeff)]"""
    if isinstance(sXY, dict):
        items = [(ex, ey, c) for ex, inner in sXY.items() for ey, c in inner.items()]
    else:
        items = [(ex, ey, c) for ex, ey, c in sXY]
    xe = np.array([t[0] for t in items], dtype=np.int64)
    ye = np.array([t[1] for t in items], dtype=np.int64)
    return xe, ye, fr_array([t[2] for t in items])


def hsc_prove_poly(srs: SRS, sXY, yzs, u: Optional[int] = None, v: Optional[int] = None, rng=None) -> HscProof:
    """hscProve :: SRS -> BiVLaurent Fr -> [(Fr, Fr)] -> m HscProof (Signature.hs:32-72) for ANY sparse bivariate Laurent
    polynomial (sonic_hsc_prove_poly); u, v: its two `rnd` draws (default fresh)"""
    draw = (lambda: rng.randrange(1, R_MODULUS)) if rng is not None else (lambda: secrets.randbelow(R_MODULUS - 1) + 1)
    xe, ye, cf = _biv_terms(sXY)
    yzs = list(yzs)
    flat = fr_array([x for pair in yzs for x in pair])
    out = C.create_string_buffer(_lib.lib().sonic_hsc_proof_size(len(yzs)))
    _lib.check(_lib.lib().sonic_hsc_prove_poly(srs._h, len(xe), xe.ctypes.data, ye.ctypes.data, cf.ctypes.data, len(yzs), flat.ctypes.data,
                                               fr_to_bytes(draw() if u is None else u), fr_to_bytes(draw() if v is None else v), out))
    return _hsc_from_bytes(out.raw, len(yzs))


def hsc_verify_poly(srs: SRS, sXY, yzs, proof: HscProof) -> bool:
    """hscVerify :: SRS -> BiVLaurent Fr -> [(Fr, Fr)] -> HscProof -> Bool (Signature.hs:74-90) for any sparse bivariate polynomial"""
    xe, ye, cf = _biv_terms(sXY)
    yzs = list(yzs)
    if len(proof.hscS) != len(yzs) or len(proof.hscW) != len(yzs):
        return False
    flat = fr_array([x for pair in yzs for x in pair])
    ok = C.c_int(0)
    _lib.check(_lib.lib().sonic_hsc_verify_poly(srs._h, len(xe), xe.ctypes.data, ye.ctypes.data, cf.ctypes.data, len(yzs), flat.ctypes.data,
                                                _hsc_to_bytes(proof), C.byref(ok)))
    return bool(ok.value)


def hsc_verify(srs: SRS, circuit: ArithCircuit, yzs, proof: HscProof) -> bool:
    """hscVerify :: SRS -> BiVLaurent Fr -> [(Fr, Fr)] -> HscProof -> Bool (Signature.hs:74-90); host CPU pairings"""
    wL, wR, wO, _cs, n, Q = _circuit_arrays(circuit, "hsc_verify: ")
    yzs = list(yzs)
    if any(len(pair) != 2 for pair in yzs):
        raise ValueError("hsc_verify: yzs must hold (y_j, z_j) pairs")
    if len(proof.hscS) != len(yzs) or len(proof.hscW) != len(yzs):
        return False
    flat = fr_array([x for pair in yzs for x in pair])
    ok = C.c_int(0)
    _lib.check(_lib.lib().sonic_hsc_verify(srs._h, n, Q, wL.ctypes.data, wR.ctypes.data, wO.ctypes.data, len(yzs), flat.ctypes.data,
                                           _hsc_to_bytes(proof), C.byref(ok)))
    return bool(ok.value)


def verify(srs: SRS, circuit: ArithCircuit, proof: Proof, y: int, z: int, yzs) -> bool:
    """verify :: SRS -> ArithCircuit Fr -> Proof -> Fr -> Fr -> [(Fr, Fr)] -> Bool (Protocol.hs:111-130), with
    hscVerify (Signature.hs:74-90).  Runs on the host CPU (pairings); the SRS needs its G2 half (SRS.new, or a file
    that carries it).  Shapes are checked here because the C side reads 64 Q bytes of yzs and sonic_proof_size(Q)
    bytes of proof; a Proof whose hsc lists do not have Q entries is rejected (False), like any other malformed proof."""
    n, Q, suffix, args, _keep = _circuit_args(circuit, "verify: ")
    yzs = list(yzs)
    if len(yzs) != Q or any(len(pair) != 2 for pair in yzs):
        raise ValueError(f"verify: yzs must hold {Q} (y_j, z_j) pairs, got {len(yzs)}")
    h = proof.prHscProof
    if len(h.hscS) != Q or len(h.hscW) != Q:
        return False
    raw = proof.to_bytes()
    if len(raw) != _lib.lib().sonic_proof_size(Q):
        return False
    flat = fr_array([v for pair in yzs for v in pair])
    ok = C.c_int(0)
    _lib.check(getattr(_lib.lib(), "sonic_verify" + suffix)(srs._h, n, Q, *args, raw, fr_to_bytes(y), fr_to_bytes(z), flat.ctypes.data, C.byref(ok)))
    return bool(ok.value)


def _core_bytes(proof) -> bytes:
    """a core proof as its 576 bytes: a CoreProof, a Proof (its head), or bytes in either encoding"""
    if isinstance(proof, Proof):
        proof = proof.core()
    if isinstance(proof, CoreProof):
        return proof.to_bytes()
    raw = bytes(proof)
    return CoreProof.from_bytes(raw).to_bytes() if len(raw) == _lib.CORE_PROOF_SIZE_COMPRESSED else raw


def verify_core(srs: SRS, circuit, proof, y: int, z: int) -> bool:
    """the sound check of a proof's head (sonic_verify_core[_csr]): the proof's s must be s(z, y) of the circuit -- evaluated here, since
    nothing in `verify` ties it down -- and the three pcV equations of R, T and their openings must hold.  proof: a CoreProof, its bytes,
    or a Proof, whose head is checked: verify_core(proof, y, z) with the proof's own y, z (fs_challenges for a Fiat-Shamir proof) is the
    sound verification of an existing full proof."""
    n, Q, suffix, args, _keep = _circuit_args(circuit, "verify_core: ")
    raw = _core_bytes(proof)
    if len(raw) != _lib.CORE_PROOF_SIZE:
        return False
    ok = C.c_int(0)
    _lib.check(getattr(_lib.lib(), "sonic_verify_core" + suffix)(srs._h, n, Q, *args, raw, fr_to_bytes(y), fr_to_bytes(z), C.byref(ok)))
    return bool(ok.value)


def verify_core_fs(srs: SRS, circuit, proof) -> bool:
    """verify_core for a proof made by Prover.prove_core_fs: y, z are recomputed from the circuit and the proof (sonic_verify_core_fs[_csr])"""
    n, Q, suffix, args, _keep = _circuit_args(circuit, "verify_core_fs: ")
    raw = _core_bytes(proof)
    if len(raw) != _lib.CORE_PROOF_SIZE:
        return False
    ok = C.c_int(0)
    _lib.check(getattr(_lib.lib(), "sonic_verify_core_fs" + suffix)(srs._h, n, Q, *args, raw, C.byref(ok)))
    return bool(ok.value)


def fs_core_challenges(srs: SRS, circuit, proof):
    """(y, z) of a Fiat-Shamir core proof (sonic_fs_core_challenges; host only)"""
    n, Q = _circuit_args(circuit)[:2]
    raw = _core_bytes(proof)
    if len(raw) != _lib.CORE_PROOF_SIZE:
        raise ValueError(f"fs_core_challenges: a core proof is {_lib.CORE_PROOF_SIZE} bytes")
    out = C.create_string_buffer(64)
    _lib.check(_lib.lib().sonic_fs_core_challenges(n, Q, srs.srsD, fs_circuit_digest(circuit), fs_srs_id(srs), raw, out))
    return int.from_bytes(out.raw[:32], "little"), int.from_bytes(out.raw[32:], "little")


def fs_weights_digest(circuit) -> bytes:
    """SHA-256 of the gate weights alone (sonic_fs_weights_digest over fs_circuit_midstate; host only): what the transcript of an aggregate
    binds, since s(X, Y) does not depend on the constants.  circuit: an ArithCircuit, a SparseCircuit, or the 112 bytes of a midstate."""
    mid = bytes(circuit) if isinstance(circuit, (bytes, bytearray)) else fs_circuit_midstate(circuit)
    if len(mid) != _lib.FS_MIDSTATE_SIZE:
        raise ValueError(f"fs_weights_digest: a midstate is {_lib.FS_MIDSTATE_SIZE} bytes")
    out = C.create_string_buffer(32)
    _lib.check(_lib.lib().sonic_fs_weights_digest(mid, out))
    return out.raw


def fs_weights_digest_v2(circuit) -> bytes:
    """weights digest v2 (sonic_fs_weights_digest_v2_csr; host only): SHA-256 tree over the ENTRIES of the stacked CSR, O(nnz) where
    fs_weights_digest hashes 96 Q n bytes.  circuit: a SparseCircuit, hashed as given -- an explicit zero is an entry, so two CSRs of one
    matrix that differ in explicit zeros have different digests -- or an ArithCircuit, which goes through SparseCircuit.from_circuit
    (its non-zero entries)."""
    sp = circuit if isinstance(circuit, SparseCircuit) else SparseCircuit.from_circuit(circuit)
    out = C.create_string_buffer(32)
    _lib.check(_lib.lib().sonic_fs_weights_digest_v2_csr(sp.n, sp.Q, *sp._args(), out))
    return out.raw


def fs_circuit_digest_v2(weights_digest: bytes, cs) -> bytes:
    """circuit digest v2 of one statement (sonic_fs_circuit_digest_v2; host only): SHA-256 over weights digest v2, Q and the constants
    cs (ints or Q x 32 bytes) -- 32 Q bytes of hashing per statement.  What prove_core_fs and its batches take as `circuit_digest` for a
    Verifier(..., digest=2)."""
    weights_digest = bytes(weights_digest)
    if len(weights_digest) != 32:
        raise ValueError("fs_circuit_digest_v2: a weights digest is 32 bytes")
    # (bytes as they are, ints without reduction: a non-canonical constant must reach the library, which refuses it)
    if isinstance(cs, np.ndarray) and cs.dtype == np.uint8:
        raw = cs.tobytes()
    else:
        raw = bytes(cs) if isinstance(cs, (bytes, bytearray, memoryview)) else b"".join(int(c).to_bytes(32, "little") for c in cs)
    if not raw or len(raw) % 32:
        raise ValueError("fs_circuit_digest_v2: need Q >= 1 constants of 32 bytes each")
    out = C.create_string_buffer(32)
    _lib.check(_lib.lib().sonic_fs_circuit_digest_v2(weights_digest, len(raw) // 32, raw, out))
    return out.raw


def fs_aggregate_challenges(srs: SRS, circuit, yzs, aggregate: bytes, weights_digest: Optional[bytes] = None):
    """(u, v) that the bytes of an aggregate for the pairs yzs determine (sonic_fs_aggregate_challenges; host only): a verifier compares
    them with the aggregate's own last 64 bytes"""
    n, Q = _circuit_args(circuit)[:2]
    yzs = list(yzs)
    aggregate = bytes(aggregate)
    if not yzs or len(aggregate) != _lib.lib().sonic_hsc_proof_size(len(yzs)):
        raise ValueError("fs_aggregate_challenges: an aggregate for K >= 1 pairs is sonic_hsc_proof_size(K) bytes")
    flat = fr_array([x for pair in yzs for x in pair])
    out = C.create_string_buffer(64)
    wd = weights_digest if weights_digest is not None else fs_weights_digest(circuit)
    _lib.check(_lib.lib().sonic_fs_aggregate_challenges(n, Q, srs.srsD, bytes(wd), fs_srs_id(srs), len(yzs), flat.ctypes.data, aggregate, out))
    return int.from_bytes(out.raw[:32], "little"), int.from_bytes(out.raw[32:], "little")


def aggregate_core(prover: "Prover", proofs, yzs):
    """what a helper ships for K core proofs: (aggregate, mismatched) -- Prover.aggregate_core over their (y_k, z_k), and the k whose proof's
    s is not the aggregate's s_k = s(z_k, y_k): no verifier will accept those, so the helper can drop them first"""
    yzs = list(yzs)
    raws = [_core_bytes(p) for p in proofs]
    if len(raws) != len(yzs):
        raise ValueError("aggregate_core: one (y_k, z_k) pair per proof")
    agg = prover.aggregate_core(yzs)
    mismatched = [k for k, raw in enumerate(raws) if len(raw) != _lib.CORE_PROOF_SIZE or raw[544:576] != agg[224 * k + 96:224 * k + 128]]
    return agg, mismatched


class Verifier:
    """The batched verifier (sonic_verifier_* of the C ABI): the circuit resident in HBM, K proofs folded into ONE pairing product --
    four Miller loops and one final exponentiation per batch; point validation, s(u, v) and the G1 sums run on the GPU.  `circuit` is an
    ArithCircuit or a SparseCircuit.  A malformed proof is a rejected proof (False), never an exception."""

    def __init__(self, srs: SRS, circuit, digest: int = 1):
        """digest: which circuit digest the handle's Fiat-Shamir and helped calls derive.  1: circuit digest v1 (fs_circuit_digest; O(Q n)
        hashing here).  2: circuit digest v2 (sonic_verifier_new_digest): the GPU hashes the CSR entries, nothing dense; proofs must be made
        under fs_circuit_digest_v2(wd2, cs) and aggregates under weights_digest=wd2.  A dense circuit goes through
        SparseCircuit.from_circuit first."""
        if digest not in (1, 2):
            raise ValueError("Verifier: digest must be 1 or 2")
        if digest == 2 and not isinstance(circuit, SparseCircuit):
            circuit = SparseCircuit.from_circuit(circuit)
        self.n, self.Q, suffix, args, _keep = _circuit_args(circuit, "Verifier: ")
        self._srs = srs                  # the handle borrows the SRS
        self._h = C.c_void_p()
        if digest == 2:
            _lib.check(_lib.lib().sonic_verifier_new_digest(srs._h, self.n, self.Q, *args, 2, C.byref(self._h)))
        else:
            _lib.check(getattr(_lib.lib(), "sonic_verifier_new" + suffix)(srs._h, self.n, self.Q, *args, C.byref(self._h)))

    @property
    def digest_kind(self) -> int:
        """1 or 2 (sonic_verifier_digest_kind)"""
        return int(_lib.lib().sonic_verifier_digest_kind(self._h))

    def weights_digest_v2(self) -> bytes:
        """weights digest v2 of the handle's resident CSR, computed on the GPU (sonic_verifier_weights_digest_v2); a handle made from dense
        weights holds their non-zero entries"""
        out = C.create_string_buffer(32)
        _lib.check(_lib.lib().sonic_verifier_weights_digest_v2(self._h, out))
        return out.raw

    def _proof_bytes(self, proofs):
        """the batch as one buffer, and the suffix of the entry point that reads it: "" for proof bytes / Proof objects, "_z" when every
        proof is given as compressed bytes (told apart by length)"""
        size, zsize = _lib.lib().sonic_proof_size(self.Q), _lib.lib().sonic_proof_size_compressed(self.Q)
        raws = [p.to_bytes() if isinstance(p, Proof) else bytes(p) for p in proofs]
        if raws and all(len(r) == zsize for r in raws):
            return b"".join(raws), "_z"
        if not raws or any(len(r) != size for r in raws):
            raise ValueError(f"Verifier: need at least one proof, each of {size} bytes, or each of {zsize} compressed (Q = {self.Q})")
        return b"".join(raws), ""

    @staticmethod
    def _seed(seed):
        if seed is not None and len(bytes(seed)) != 32:
            raise ValueError("Verifier: seed must be 32 bytes (or None: the library draws it)")
        return None if seed is None else bytes(seed)

    def _result(self, K, call, each):
        ok = C.c_int(0)
        flags = C.create_string_buffer(K) if each else None
        _lib.check(call(C.byref(ok), flags))
        return (bool(ok.value), [bool(b) for b in flags.raw]) if each else bool(ok.value)

    def _constants(self, constants, K):
        constants = list(constants)
        if len(constants) != K:
            raise ValueError("Verifier: one set of constants per proof")
        return b"".join(_constants_bytes(c, self.Q, "Verifier") for c in constants)

    def verify_batch(self, proofs, transcripts, seed=None, each: bool = False, constants=None):
        """proofs: Proof objects, proof bytes, or compressed proof bytes (all of them: the `_z` entry point); transcripts: one (y, z, yzs) per proof, as for verify().  True iff every proof is
        accepted; with each=True also the per-proof verdicts.  constants: None -- every proof against the circuit's cs -- or one cs per
        proof (Q ints or Q x 32 bytes): proof k against the handle's weights and ITS constants (sonic_verifier_verify_batch_cs)."""
        proofs, transcripts = list(proofs), list(transcripts)
        if len(transcripts) != len(proofs):
            raise ValueError("verify_batch: one (y, z, yzs) transcript per proof")
        fr = lambda v: int(v).to_bytes(32, "little")     # noqa: E731  (as is: a non-canonical challenge rejects its proof)
        blocks = []
        for y, z, yzs in transcripts:
            yzs = list(yzs)
            if len(yzs) != self.Q or any(len(pair) != 2 for pair in yzs):
                raise ValueError(f"verify_batch: yzs must hold {self.Q} (y_j, z_j) pairs")
            blocks.append(fr(y) + fr(z) + b"".join(fr(a) + fr(b) for a, b in yzs))
        (raw, z), chal, sd, K = self._proof_bytes(proofs), b"".join(blocks), self._seed(seed), len(proofs)
        if constants is not None:
            cs, call = self._constants(constants, K), _lib.lib().sonic_verifier_verify_batch_cs
            return self._result(K, lambda ok, flags: call(self._h, K, raw, int(z == "_z"), chal, cs, sd, ok, flags), each)
        call = getattr(_lib.lib(), "sonic_verifier_verify_batch" + z)
        return self._result(K, lambda ok, flags: call(self._h, K, raw, chal, sd, ok, flags), each)

    def verify_fs_batch(self, proofs, seed=None, each: bool = False, constants=None):
        """the same for Fiat-Shamir proofs (prove_fs): every proof's challenges are recomputed from the circuit and the proof -- with
        constants (one cs per proof), from the digest of that proof's own statement (sonic_verifier_verify_fs_batch_cs)"""
        proofs = list(proofs)
        (raw, z), sd, K = self._proof_bytes(proofs), self._seed(seed), len(proofs)
        if constants is not None:
            cs, call = self._constants(constants, K), _lib.lib().sonic_verifier_verify_fs_batch_cs
            return self._result(K, lambda ok, flags: call(self._h, K, raw, int(z == "_z"), cs, sd, ok, flags), each)
        call = getattr(_lib.lib(), "sonic_verifier_verify_fs_batch" + z)
        return self._result(K, lambda ok, flags: call(self._h, K, raw, sd, ok, flags), each)

    def _core_proof_bytes(self, proofs):
        """a batch of core proofs as one buffer and whether it is the compressed form (told apart by length)"""
        raws = [p.core().to_bytes() if isinstance(p, Proof) else p.to_bytes() if isinstance(p, CoreProof) else bytes(p) for p in proofs]
        if raws and all(len(r) == _lib.CORE_PROOF_SIZE_COMPRESSED for r in raws):
            return b"".join(raws), 1
        if not raws or any(len(r) != _lib.CORE_PROOF_SIZE for r in raws):
            raise ValueError(f"Verifier: need at least one core proof, each of {_lib.CORE_PROOF_SIZE} bytes, or each of {_lib.CORE_PROOF_SIZE_COMPRESSED} compressed")
        return b"".join(raws), 0

    def verify_core_batch(self, proofs, yzs, seed=None, each: bool = False, constants=None):
        """K core proofs in one pairing product (sonic_verifier_verify_core_batch): s(z_k, y_k) on the GPU held against each proof's s,
        then the 3K checks of the heads folded.  proofs: CoreProof objects, Proofs (their heads), 576-byte or 336-byte (compressed) core
        proofs; yzs: one (y, z) per proof; constants: None, or one cs per proof.  A proof whose s is not s(z, y) is a rejected proof."""
        proofs, yzs = list(proofs), list(yzs)
        if len(yzs) != len(proofs) or any(len(pair) != 2 for pair in yzs):
            raise ValueError("verify_core_batch: one (y, z) pair per proof")
        fr = lambda v: int(v).to_bytes(32, "little")     # noqa: E731  (as is: a non-canonical challenge rejects its proof)
        (raw, z), yz, sd, K = self._core_proof_bytes(proofs), b"".join(fr(y) + fr(zz) for y, zz in yzs), self._seed(seed), len(proofs)
        cs = self._constants(constants, K) if constants is not None else None
        call = _lib.lib().sonic_verifier_verify_core_batch
        return self._result(K, lambda ok, flags: call(self._h, K, raw, z, yz, cs, sd, ok, flags), each)

    def verify_core_fs_batch(self, proofs, seed=None, each: bool = False, constants=None):
        """the same for Fiat-Shamir core proofs (Prover.prove_core_fs): y_k, z_k recomputed from the circuit (with constants: from the
        digest of proof k's own statement) and the proof"""
        proofs = list(proofs)
        (raw, z), sd, K = self._core_proof_bytes(proofs), self._seed(seed), len(proofs)
        cs = self._constants(constants, K) if constants is not None else None
        call = _lib.lib().sonic_verifier_verify_core_fs_batch
        return self._result(K, lambda ok, flags: call(self._h, K, raw, z, cs, sd, ok, flags), each)

    def _aggregate(self, aggregate, K):
        aggregate = _hsc_to_bytes(aggregate) if isinstance(aggregate, HscProof) else bytes(aggregate)
        if len(aggregate) != _lib.lib().sonic_hsc_proof_size(K):
            raise ValueError(f"Verifier: an aggregate for {K} proofs is {_lib.lib().sonic_hsc_proof_size(K)} bytes")
        return aggregate

    def verify_core_batch_helped(self, proofs, yzs, aggregate, seed=None, each: bool = False, constants=None):
        """verify_core_batch with a helper's aggregate signature over the same (y_k, z_k) (Prover.aggregate_core;
        sonic_verifier_verify_core_batch_helped): each proof's s is held against the aggregate's s_k, s(u, v) is evaluated once for the
        batch instead of s(z_k, y_k) per proof, and the 6K + 1 checks fold into the same four Miller loops.  An aggregate that is
        malformed, not under its own transcript, or fails its global check rejects every proof."""
        proofs, yzs = list(proofs), list(yzs)
        if len(yzs) != len(proofs) or any(len(pair) != 2 for pair in yzs):
            raise ValueError("verify_core_batch_helped: one (y, z) pair per proof")
        fr = lambda v: int(v).to_bytes(32, "little")     # noqa: E731  (as is: a non-canonical challenge rejects its proof)
        (raw, z), yz, sd, K = self._core_proof_bytes(proofs), b"".join(fr(y) + fr(zz) for y, zz in yzs), self._seed(seed), len(proofs)
        cs = self._constants(constants, K) if constants is not None else None
        agg, call = self._aggregate(aggregate, K), _lib.lib().sonic_verifier_verify_core_batch_helped
        return self._result(K, lambda ok, flags: call(self._h, K, raw, z, yz, cs, agg, sd, ok, flags), each)

    def verify_core_fs_batch_helped(self, proofs, aggregate, seed=None, each: bool = False, constants=None):
        """the same for Fiat-Shamir core proofs: y_k, z_k recomputed per proof as verify_core_fs_batch does; the aggregate is over those"""
        proofs = list(proofs)
        (raw, z), sd, K = self._core_proof_bytes(proofs), self._seed(seed), len(proofs)
        cs = self._constants(constants, K) if constants is not None else None
        agg, call = self._aggregate(aggregate, K), _lib.lib().sonic_verifier_verify_core_fs_batch_helped
        return self._result(K, lambda ok, flags: call(self._h, K, raw, z, cs, agg, sd, ok, flags), each)

    def eval_s(self, uvs) -> List[int]:
        """s(u, v) of the circuit's s(X, Y) for every (u, v) of `uvs`, on the GPU (raises SonicError INEXACT_DIVISION for u = 0 or v = 0)"""
        uvs = list(uvs)
        flat = fr_array([x for pair in uvs for x in pair])
        out = C.create_string_buffer(32 * len(uvs))
        _lib.check(_lib.lib().sonic_verifier_eval_s(self._h, len(uvs), flat.ctypes.data, out))
        return [int.from_bytes(out.raw[32 * i:32 * i + 32], "little") for i in range(len(uvs))]

    def close(self):
        if self._h:
            _lib.lib().sonic_verifier_free(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def verify_batch(srs: SRS, circuit, proofs, transcripts, seed=None, each: bool = False):
    """Verifier(srs, circuit).verify_batch(...) for one batch"""
    v = Verifier(srs, circuit)
    try:
        return v.verify_batch(proofs, transcripts, seed=seed, each=each)
    finally:
        v.close()
