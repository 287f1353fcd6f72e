"""Sonic.SRS (src/Sonic/SRS.hs): the structured reference string, resident in HBM."""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib
from .encoding import R_MODULUS, fr_to_bytes, g1_from_bytes


UPDATE_PROOF_SIZE = 448         # SONIC_SRS_UPDATE_PROOF_SIZE


def check_names(failed: int) -> str:
    """the relations a failed_mask of SRS.check names, as in 'R1, R3'"""
    return ", ".join(f"R{i}" for i in range(5) if failed >> i & 1)


def srs_verify_update(old: "SRS", new: "SRS", proof: bytes, check: bool = True) -> bool:
    """whether `new` is `old` updated by someone who knew the shares behind `proof` (sonic_srs_verify_update): the proof's two Schnorr
    equations, the two pairing equations that link the strings and -- with check, the default -- the structure check of the new string.
    check=False is for a string that is checked elsewhere: the link equations alone say nothing about the other 8d + 2 points.
    A malformed proof is False, not an error."""
    if len(proof) != UPDATE_PROOF_SIZE:
        return False
    ok = C.c_int(0)
    _lib.check(_lib.lib().sonic_srs_verify_update(old._h, new._h, bytes(proof), 1 if check else 0, C.byref(ok)))
    return bool(ok.value)


class SRS:
    """`data SRS` (SRS.hs:11-22), prover half.  Device layout: two arrays of 2d+1 affine points,
    basis 0 = g^{x^e}, basis 1 = g^{alpha x^e}, slot e + d; the reference's four G1 vectors are views:
    gNegativeX[k] = basis0[-(k+1)], gPositiveX[k] = basis0[k], gNegativeAlphaX[k] = basis1[-(k+1)],
    gPositiveAlphaX[k] = basis1[k+1].  The G2 vectors (verifier only) are generated lazily on first access, after which
    the handle forgets x and alpha."""

    def __init__(self, handle: C.c_void_p, d: int):
        self._h = handle
        self.srsD = d

    @classmethod
    def new(cls, d: int, x: int, alpha: int, device: int = -1) -> "SRS":
        """SRS.new :: Int -> Fr -> Fr -> SRS (SRS.hs:27-43), generated on the GPU `device` (-1: the default device)."""
        h = C.c_void_p()
        _lib.check(_lib.lib().sonic_srs_new_on(device, d, fr_to_bytes(x), fr_to_bytes(alpha), C.byref(h)))
        return cls(h, d)

    @classmethod
    def from_points(cls, d: int, basis0: np.ndarray, basis1: np.ndarray, device: int = -1) -> "SRS":
        """The record constructor: caller-supplied points, uint8 [(2d+1), 96] per basis."""
        b0 = np.ascontiguousarray(basis0, np.uint8)
        b1 = np.ascontiguousarray(basis1, np.uint8)
        assert b0.size == 96 * (2 * d + 1) and b1.size == 96 * (2 * d + 1)
        h = C.c_void_p()
        _lib.check(_lib.lib().sonic_srs_from_points_on(device, d, b0.ctypes.data, b1.ctypes.data, C.byref(h)))
        return cls(h, d)

    def replicate(self, device: int) -> "SRS":
        """a replica of this SRS on another GPU of the process, copied device to device with its window tables (sonic_srs_replicate)"""
        h = C.c_void_p()
        _lib.check(_lib.lib().sonic_srs_replicate(self._h, device, C.byref(h)))
        return SRS(h, self.srsD)

    @property
    def device(self) -> int:
        """the GPU the handle lives on"""
        return int(_lib.lib().sonic_srs_device(self._h))

    @property
    def srsPairing(self):
        """srsPairing = e(g, h^alpha) (SRS.hs:21,42): the Fq12 element as nested tuples ((c00, c01, c02), (c10, c11, c12)) of Fq2
        pairs -- Fq12 = Fq6[w]/(w^2 - v), Fq6 = Fq2[v]/(v^3 - (1 + u)) -- from sonic_srs_pairing (host pairing; needs the G2 half)"""
        out = C.create_string_buffer(576)
        _lib.check(_lib.lib().sonic_srs_pairing(self._h, out))
        v = [int.from_bytes(out.raw[48 * i:48 * i + 48], "little") for i in range(12)]
        return tuple(tuple((v[6 * i + 2 * j], v[6 * i + 2 * j + 1]) for j in range(3)) for i in range(2))

    def set_g2_points(self, basis0: np.ndarray, basis1: np.ndarray) -> None:
        """attach the verifier half to a handle built from G1 points: uint8 [(2d+1), 192] per basis, validated"""
        b0 = np.ascontiguousarray(basis0, np.uint8)
        b1 = np.ascontiguousarray(basis1, np.uint8)
        assert b0.size == 192 * (2 * self.srsD + 1) and b1.size == 192 * (2 * self.srsD + 1)
        _lib.check(_lib.lib().sonic_srs_set_g2_points(self._h, b0.ctypes.data, b1.ctypes.data))

    def has_g2(self) -> bool:
        """whether the handle holds the verifier half or can still generate it (sonic_srs_has_g2)"""
        return bool(_lib.lib().sonic_srs_has_g2(self._h))

    def save(self, path: str, g2=None, compressed: bool = False) -> None:
        """write the SRS to disk (format in include/sonic_hip.h): the G1 bases and, with g2, the G2 bases, so that the
        loaded handle can verify as well as prove.  g2=None (default): include the G2 half if the handle has it -- handles made
        from G1 points only, or loaded from a version-1 file, save as they are.  The file never holds the trapdoor.
        compressed=True writes the "SONICSRZ" container instead: every point in its compressed encoding, half the size; load() takes either."""
        save = _lib.lib().sonic_srs_save_compressed if compressed else _lib.lib().sonic_srs_save
        _lib.check(save(self._h, str(path).encode(), 2 if g2 is None else (1 if g2 else 0)))

    @classmethod
    def load(cls, path: str, device: int = -1, circuit=None, check: bool = False) -> "SRS":
        """read either container.  circuit=(n, Q): a circuit-sized view (see for_circuit) made by reading only the byte ranges of its
        windows, and the four G2 points where the file has a G2 half (sonic_srs_load_for_circuit_on).
        check=True runs the structure check (see check) on the loaded string and raises SonicError(BAD_ENCODING) naming the relations
        that fail: loading alone validates every point on its own and nothing else.  A view cannot be checked: check the whole string."""
        if check and circuit is not None:
            raise ValueError("SRS.load: check=True needs the whole string, not a circuit-sized view")
        h = C.c_void_p()
        if circuit is None:
            _lib.check(_lib.lib().sonic_srs_load_on(device, str(path).encode(), C.byref(h)))
        else:
            n, Q = circuit
            _lib.check(_lib.lib().sonic_srs_load_for_circuit_on(device, str(path).encode(), n, Q, C.byref(h)))
        srs = cls(h, int(_lib.lib().sonic_srs_d(h)))
        if check:
            ok, failed = srs.check()
            if not ok:
                srs.close()
                raise _lib.SonicError(3, f"SRS.load: {path} is no reference string: relations {check_names(failed)} fail")
        return srs

    def check(self, seed: bytes = None):
        """(ok, failed_mask): whether the handle's points ARE a reference string -- the consecutive powers of one x over the fixed
        generators, with the alpha basis and the G2 half belonging to them (sonic_srs_check: relations R0 .. R4 under 128-bit
        randomizers, the G1 sums as MSMs, the G2 sums and the pairings beside them).  failed_mask has bit i set when Ri fails.
        seed=None draws the randomizers' seed from the operating system; a 32-byte seed is for reproducible tests only."""
        if seed is not None and len(seed) != 32:
            raise ValueError("SRS.check: the seed is 32 bytes")
        failed = C.c_int(0)
        _lib.check(_lib.lib().sonic_srs_check(self._h, seed, C.byref(failed)))
        return failed.value == 0, int(failed.value)

    def update(self, x: int = None, alpha: int = None, seed: bytes = None):
        """(new_srs, proof): a contribution to the string (sonic_srs_update).  The new handle holds the string of trapdoor
        (x_old * x, alpha_old * alpha) on the same GPU; this handle is untouched.  proof: 448 bytes for srs_verify_update.
        x=None / alpha=None: the share is drawn with `secrets` and never returned -- what a real contribution does.  seed: 32 bytes that
        make the proof's nonces reproducible, for tests."""
        import secrets
        if seed is not None and len(seed) != 32:
            raise ValueError("SRS.update: the seed is 32 bytes")
        xs = [1 + secrets.randbelow(R_MODULUS - 1) if v is None else v for v in (x, alpha)]
        for v in xs:
            if not 0 <= v < 1 << 256:
                raise ValueError("SRS.update: a share is a non-negative integer below 2^256")
        h = C.c_void_p()
        proof = C.create_string_buffer(UPDATE_PROOF_SIZE)
        _lib.check(_lib.lib().sonic_srs_update(self._h, xs[0].to_bytes(32, "little"), xs[1].to_bytes(32, "little"), seed, C.byref(h), proof))
        return SRS(h, self.srsD), proof.raw

    def for_circuit(self, n: int, Q: int) -> "SRS":
        """a circuit-sized VIEW of this string on the same GPU (sonic_srs_for_circuit): the same d, Fiat-Shamir id, commitments and
        proofs, over copies of only the exponents a circuit of (n, Q) touches -- [-4n-8, max(3n, n+Q)] and [d-3n-4, d] -- with tables
        sized for those windows and the window width of a string of d = 8n.  The view owns what it holds: this handle may be closed.
        It needs d >= max(7n, 4n + 8); it refuses (SONIC_ERR_INVALID_ARG) exponents it does not hold, provers for circuits whose
        windows it does not contain, verifiers for another n, save() and set_g2_points().  Measured against the whole string in
        profiles/r14_srs_view.txt (README, "Circuit-sized SRS views")."""
        h = C.c_void_p()
        _lib.check(_lib.lib().sonic_srs_for_circuit(self._h, n, Q, C.byref(h)))
        return SRS(h, self.srsD)

    @property
    def windows(self):
        """(lo0, hi0, lo1, hi1): the exponent windows the handle holds; one window -- every whole string: (-d, d) -- has lo1 = 1, hi1 = 0"""
        w = (C.c_int64 * 4)()
        _lib.check(_lib.lib().sonic_srs_windows(self._h, w))
        return tuple(int(v) for v in w)

    @property
    def device_bytes(self) -> int:
        """device memory of the G1 side: both bases with their window tables, the running sums, the symmetric sums"""
        out = C.c_size_t()
        _lib.check(_lib.lib().sonic_srs_device_bytes(self._h, C.byref(out)))
        return int(out.value)

    def points(self, basis: int, e0: int, n: int) -> np.ndarray:
        out = np.zeros((n, 96), np.uint8)
        _lib.check(_lib.lib().sonic_srs_get_points(self._h, basis, e0, n, out.ctypes.data))
        return out

    def g2_points(self, basis: int, e0: int, n: int) -> np.ndarray:
        """G2 half (generated on the GPU on first use): uint8 [n, 192], x.c0 || x.c1 || y.c0 || y.c1"""
        out = np.zeros((n, 192), np.uint8)
        _lib.check(_lib.lib().sonic_srs_get_g2_points(self._h, basis, e0, n, out.ctypes.data))
        return out

    def _one_g2(self, name, basis, e, k, length):
        if not (0 <= k < length):
            raise IndexError(f"{name} is not long enough: {k} >= {length}")
        b = self.g2_points(basis, e, 1)[0].tobytes()
        if b == bytes(192):
            return None
        v = [int.from_bytes(b[i:i + 48], "little") for i in range(0, 192, 48)]
        return ((v[0], v[1]), (v[2], v[3]))

    def hNegativeX(self, k):            # SRS.hs:35
        return self._one_g2("hNegativeX", 0, -(k + 1), k, self.srsD)

    def hPositiveX(self, k):            # SRS.hs:36
        return self._one_g2("hPositiveX", 0, k, k, self.srsD + 1)

    def hNegativeAlphaX(self, k):       # SRS.hs:40
        return self._one_g2("hNegativeAlphaX", 1, -(k + 1), k, self.srsD)

    def hPositiveAlphaX(self, k):       # SRS.hs:41
        return self._one_g2("hPositiveAlphaX", 1, k, k, self.srsD + 1)

    def _one(self, name, basis, e, k, length):
        if not (0 <= k < length):   # CommitmentScheme.hs:70-73
            raise IndexError(f"{name} is not long enough: {k} >= {length}")
        return g1_from_bytes(self.points(basis, e, 1)[0].tobytes())

    def gNegativeX(self, k):
        return self._one("gNegativeX", 0, -(k + 1), k, self.srsD)

    def gPositiveX(self, k):
        return self._one("gPositiveX", 0, k, k, self.srsD + 1)

    def gNegativeAlphaX(self, k):
        return self._one("gNegativeAlphaX", 1, -(k + 1), k, self.srsD)

    def gPositiveAlphaX(self, k):
        return self._one("gPositiveAlphaX", 1, k + 1, k, self.srsD)

    def close(self):
        if self._h:
            _lib.lib().sonic_srs_free(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
