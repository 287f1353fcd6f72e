"""The updatable SRS on the GPU (include/sonic_hip.h, "Updatable SRS"): SRS.check, SRS.update, srs_verify_update.  Bytes and verdicts only.

Sizes, and the boundary each crosses:
  d = 12      25 points per basis: the smallest a circuit can use, under one 64-point normalisation chunk and one block of every kernel
  d = 300     601 points: crosses the 64-point chunks of k_batch_affine / k_g2_batch_affine, the 64-thread blocks of k_g2_sum and the
              256-thread blocks of k_g1_scale_each / k_g2_scale_each, each with a remainder
  d = 8200    16401 points: 17 more than the 256 x 64 threads of k_g2_sum's grid, so some threads add a second point (check only)
  d = 2^19+3  1048583 points: 7 more than the 2^20-point slab of the G1 scaling (srs_scale_g1_enqueue) and 7 more than two 2^19-point
              slabs of the G2 scaling and of the G2 sums (srs_scale_g2, g2_weighted_sum), so in both groups a later slab's exponent
              origin, its reads and writes at the slab's base and the reuse of the slab buffers are compared with the oracle, and the
              host adds the block totals of three slabs (one update, one check)

Masks of SRS.check: bit i set when Ri fails.  A mutant's expected mask is worked out from the relations (in the header), not observed:
an element enters a relation when it is a term of one of its sums or one of its fixed G2 points H0[1], H1[0]."""
import random

import numpy as np
import pytest

from util import R, circuit_arrays

pytestmark = pytest.mark.gpu

INVALID_ARG, BAD_ENCODING = 7, 3
R0, R1, R2, R3, R4 = 1, 2, 4, 8, 16
SEED = bytes(range(100, 132))
SIZES = (12, 300)
D_GRID, D_SLAB = 8200, (1 << 19) + 3
ZERO_RUN = (1 << 254) + 1              # two bits set, 253 zero bits between them


def trapdoor(d, k=0):
    pyr = random.Random(1000 * d + k)
    return pyr.randrange(2, R), pyr.randrange(2, R)


class Honest:
    """one honest string of d with its G2 half, and its four bases as arrays, made once per d"""

    def __init__(self, sonic, d):
        self.d, self.n = d, 2 * d + 1
        self.x, self.alpha = trapdoor(d)
        self.srs = sonic.SRS.new(d, self.x, self.alpha)
        self.arrays = bases(self.srs)


def bases(srs):
    d, n = srs.srsD, 2 * srs.srsD + 1
    return [srs.points(0, -d, n), srs.points(1, -d, n), srs.g2_points(0, -d, n), srs.g2_points(1, -d, n)]


_HONEST = {}


@pytest.fixture
def honest(sonic):
    def get(d):
        if d not in _HONEST:
            _HONEST[d] = Honest(sonic, d)
        return _HONEST[d]
    return get


def assemble(sonic, d, arrays):
    """a handle from four arrays of valid points: loading must accept it whatever its structure"""
    s = sonic.SRS.from_points(d, arrays[0], arrays[1])
    s.set_g2_points(arrays[2], arrays[3])
    return s


def same_string(a, b):
    d = a.srsD
    for got, want in zip(bases(a), bases(b)):
        assert np.array_equal(got, want)
    # the places a scaling by x1^e can go wrong on its own: both ends, both sides of the centre, the empty slot
    for basis in (0, 1):
        for e in (-d, -1, 1, d):
            assert a.points(basis, e, 1).tobytes() == b.points(basis, e, 1).tobytes() != bytes(96)
            assert a.g2_points(basis, e, 1).tobytes() == b.g2_points(basis, e, 1).tobytes() != bytes(192)
    assert a.points(1, 0, 1).tobytes() == bytes(96)
    assert a.g2_points(1, 0, 1).tobytes() == b.g2_points(1, 0, 1).tobytes() != bytes(192)


# ---- update against the oracle ------------------------------------------------------------------------------------------------------------
SHARES = {"random": None, "ones": (1, 1), "top-bit": (R - 1, 3), "zero-run": (ZERO_RUN, 1 << 200)}


@pytest.mark.parametrize("case", sorted(SHARES))
@pytest.mark.parametrize("d", SIZES)
def test_update_holds_the_points_of_new_with_the_product_trapdoor(sonic, honest, d, case):
    h = honest(d)
    x1, a1 = SHARES[case] or trapdoor(d, 1)
    new, proof = h.srs.update(x1, a1, seed=SEED)
    assert len(proof) == 448 and new.srsD == d and new.device == h.srs.device
    same_string(new, sonic.SRS.new(d, h.x * x1 % R, h.alpha * a1 % R))
    assert np.array_equal(bases(h.srs)[0], h.arrays[0]) and np.array_equal(bases(h.srs)[3], h.arrays[3])        # the source is untouched
    x2, a2 = trapdoor(d, 2)
    again, _ = new.update(x2, a2, seed=SEED)
    same_string(again, sonic.SRS.new(d, h.x * x1 * x2 % R, h.alpha * a1 * a2 % R))


def test_update_and_check_across_the_slab_boundary(sonic):
    d = D_SLAB
    x, alpha = trapdoor(d)
    x1, a1 = trapdoor(d, 1)
    old = sonic.SRS.new(d, x, alpha)
    new, proof = old.update(x1, a1, seed=SEED)
    want = sonic.SRS.new(d, x * x1 % R, alpha * a1 % R)
    n = 2 * d + 1
    for basis in (0, 1):
        assert np.array_equal(new.points(basis, -d, n), want.points(basis, -d, n))
        assert np.array_equal(new.g2_points(basis, -d, n), want.g2_points(basis, -d, n))
    assert new.check(SEED) == (True, 0)
    assert sonic.srs_verify_update(old, new, proof, check=False)


# ---- check accepts ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d", SIZES + (D_GRID,))
def test_check_accepts_a_generated_string(honest, d):
    assert honest(d).srs.check(SEED) == (True, 0)
    assert honest(d).srs.check() == (True, 0)                     # a seed from the operating system


@pytest.mark.parametrize("compressed", (False, True))
@pytest.mark.parametrize("d", SIZES)
def test_check_accepts_a_saved_and_loaded_string(sonic, honest, tmp_path, d, compressed):
    path = tmp_path / "srs.bin"
    honest(d).srs.save(path, g2=True, compressed=compressed)
    assert sonic.SRS.load(path).check(SEED) == (True, 0)
    assert sonic.SRS.load(path, check=True).srsD == d


@pytest.mark.parametrize("d", SIZES)
def test_check_accepts_an_updated_string(honest, d):
    new, _ = honest(d).srs.update(seed=SEED)                      # shares drawn with `secrets`
    assert new.check(SEED) == (True, 0)


# ---- check rejects ------------------------------------------------------------------------------------------------------------------------
def idx(d, e):
    return e + d


def mutants(d):
    """name -> (which array, mutation on the copy, expected mask).  Entries are replaced by other honest entries: every point stays valid."""
    out = {}
    # G0[e] is a term of P (e <= d-1), of P+ (e >= -d+1), of A0 (e != 0) and of the sum over all of basis 0: R1, R2, R3, R4
    for e in (-d, -1, 1, d - 1):
        out[f"G0[{e}] := G0[{e + 1}]"] = (0, lambda a, e=e: a.__setitem__(idx(d, e), a[idx(d, e + 1)].copy()), R1 | R2 | R3 | R4)
    out[f"G0[{d}] := G0[{d - 1}]"] = (0, lambda a: a.__setitem__(idx(d, d), a[idx(d, d - 1)].copy()), R1 | R2 | R3 | R4)
    # G1[e] is a term of A alone; its neighbour away from the empty slot
    for e, nb in ((-d, -d + 1), (-1, -2), (1, 2), (d, d - 1)):
        def swap(a, e=e, nb=nb):
            a[[idx(d, e), idx(d, nb)]] = a[[idx(d, nb), idx(d, e)]]
        out[f"G1[{e}] <-> G1[{nb}]"] = (1, swap, R2)
    # H0[e] is a term of B; H0[1] is also the fixed point of R1
    for e, src, mask in ((-d, -d + 1, R3), (1, 2, R1 | R3), (d, d - 1, R3)):
        out[f"H0[{e}] := H0[{src}]"] = (2, lambda a, e=e, src=src: a.__setitem__(idx(d, e), a[idx(d, src)].copy()), mask)
    # H1[e] is a term of C; H1[0] is also the fixed point of R2 and of R4
    for e, src, mask in ((-d, -d + 1, R4), (0, 1, R2 | R4), (d, d - 1, R4)):
        out[f"H1[{e}] := H1[{src}]"] = (3, lambda a, e=e, src=src: a.__setitem__(idx(d, e), a[idx(d, src)].copy()), mask)
    return out


MUTANT_NAMES = {d: sorted(mutants(d)) for d in SIZES}


@pytest.mark.parametrize("d,name", [(d, n) for d in SIZES for n in MUTANT_NAMES[d]])
def test_check_rejects_one_wrong_element_and_names_the_relation(sonic, honest, d, name):
    h = honest(d)
    which, mutate, mask = mutants(d)[name]
    arrays = [a.copy() for a in h.arrays]
    mutate(arrays[which])
    assert not np.array_equal(arrays[which], h.arrays[which])
    bad = assemble(sonic, d, arrays)                              # from_points / set_g2_points still accept it
    assert bad.check(SEED) == (False, mask)
    assert h.srs.check(SEED) == (True, 0)                         # the honest string under the same seed


@pytest.mark.parametrize("d", SIZES)
def test_check_rejects_halves_of_two_trapdoors(sonic, honest, d):
    h = honest(d)
    x2, alpha2 = trapdoor(d, 5)
    other_alpha = bases(sonic.SRS.new(d, h.x, alpha2))
    other_x = bases(sonic.SRS.new(d, x2, h.alpha))
    # G2 half of another alpha: every relation inside the G2 half and inside the G1 half holds; R2 ties the alpha basis to H1[0]
    assert assemble(sonic, d, h.arrays[:2] + other_alpha[2:]).check(SEED) == (False, R2)
    # G2 half of another x: H0[1] no longer is the step of the G1 powers (R1), and neither G2 basis matches basis 0 (R3, R4); R2 reads
    # H1[0] = alpha h alone, which both strings share
    assert assemble(sonic, d, h.arrays[:2] + other_x[2:]).check(SEED) == (False, R1 | R3 | R4)
    # negative powers of all four bases from x2: every sum is consistent term by term, but the step from e = -1 to e = 0 is not x
    mixed = [np.concatenate([o[:d], a[d:]]) for a, o in zip(h.arrays, other_x)]
    assert assemble(sonic, d, mixed).check(SEED) == (False, R1)


def test_check_randomizers_are_the_specified_hash_and_differ_between_elements(sonic, honest, ref):
    """A string that is wrong in two elements of the alpha basis in a way that cancels under the randomizers of SEED and of no other
    seed: G1[a] + rho_b T and G1[b] - rho_a T change A by rho_a rho_b T - rho_b rho_a T = 0.  It passes under SEED only if the device
    made exactly the rho_e of the header for e = a and e = b (with all rho_e equal to any constant it fails, as rho_a != rho_b), and it
    fails R2 under any other seed -- which is also why a caller-supplied seed is for tests only."""
    import srs_update_ref as uref
    from sonic_amd import encoding as enc
    d = 12
    h = honest(d)
    a, b = idx(d, -7), idx(d, 5)
    ra, rb = uref.rho(SEED, a), uref.rho(SEED, b)
    assert ra != rb
    T = ref.g1_mul(ref.G1_GEN, 0xBADC0DE)
    arrays = [x.copy() for x in h.arrays]
    pa, pb = enc.g1_from_bytes(arrays[1][a].tobytes()), enc.g1_from_bytes(arrays[1][b].tobytes())
    arrays[1][a] = np.frombuffer(enc.g1_to_bytes(ref.g1_add(pa, ref.g1_mul(T, rb))), np.uint8)
    arrays[1][b] = np.frombuffer(enc.g1_to_bytes(ref.g1_add(pb, ref.g1_mul(T, R - ra))), np.uint8)
    crafted = assemble(sonic, d, arrays)
    assert crafted.check(SEED) == (True, 0)
    assert crafted.check(bytes(32)) == (False, R2)
    assert crafted.check()[1] == R2


def test_check_rejects_a_string_over_another_generator(sonic, honest, ref):
    """d = 12, built with the oracle's Python integers: the G1 half over c g instead of g.  R0 names it.  R1 and R2 compare G1 sums with
    G1 sums and hold; R3 and R4 compare basis 0 with the G2 half over h and fail with it: R1 and R3 together imply G0[0] = g, so no
    string fails R0 alone."""
    from sonic_amd import encoding as enc
    d, c = 12, 0xC0FFEE
    h = honest(d)
    xs = [pow(h.x, e, R) for e in range(-d, d + 1)]
    g0 = np.frombuffer(b"".join(enc.g1_to_bytes(ref.g1_mul(ref.G1_GEN, c * p % R)) for p in xs), np.uint8).reshape(-1, 96)
    g1 = np.frombuffer(b"".join(enc.g1_to_bytes(None if e == d else ref.g1_mul(ref.G1_GEN, c * h.alpha * p % R)) for e, p in enumerate(xs)), np.uint8).reshape(-1, 96)
    failed = assemble(sonic, d, [g0, g1] + h.arrays[2:]).check(SEED)
    assert failed == (False, R0 | R3 | R4)


# ---- update proofs ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d", SIZES)
def test_update_proofs(sonic, honest, d):
    h = honest(d)
    x1, a1 = trapdoor(d, 1)
    new, proof = h.srs.update(x1, a1, seed=SEED)
    assert sonic.srs_verify_update(h.srs, new, proof) is True
    assert h.srs.update(x1, a1, seed=SEED)[1] == proof                       # a seeded contribution is reproducible
    fresh_new, fresh = h.srs.update(x1, a1)                                  # nonces from the operating system: X, A stay, the rest moves
    assert fresh[:192] == proof[:192] and fresh[192:288] != proof[192:288] and fresh[288:384] != proof[288:384]
    assert sonic.srs_verify_update(h.srs, fresh_new, fresh, check=False) is True
    for name, off in dict(X=0, A=96, Rx=192, Ra=288, sx=384, sa=416).items():
        flipped = proof[:off + 5] + bytes([proof[off + 5] ^ 0x10]) + proof[off + 6:]
        assert sonic.srs_verify_update(h.srs, new, flipped) is False, name
    assert sonic.srs_verify_update(h.srs, new, proof[:-1]) is False
    # a proof from another contribution to the same old string
    x2, a2 = trapdoor(d, 2)
    other, other_proof = h.srs.update(x2, a2, seed=SEED)
    assert sonic.srs_verify_update(h.srs, other, other_proof) is True
    assert sonic.srs_verify_update(h.srs, new, other_proof) is False
    # the right proof against a different old string of the same d
    stranger = sonic.SRS.new(d, *trapdoor(d, 3))
    assert sonic.srs_verify_update(stranger, new, proof) is False
    # new made with a different x1 than the proof's
    assert sonic.srs_verify_update(h.srs, h.srs.update(x1 + 1, a1, seed=SEED)[0], proof) is False
    # a new string that passes both link equations (they read G0'[1] and H1'[0]) but is no reference string: one far element replaced
    arrays = bases(new)
    arrays[0][idx(d, -d)] = arrays[0][idx(d, -d + 1)]
    broken = assemble(sonic, d, arrays)
    assert sonic.srs_verify_update(h.srs, broken, proof, check=False) is True
    assert sonic.srs_verify_update(h.srs, broken, proof) is False
    # a chain of two updates verifies link by link, and not across
    third, proof2 = new.update(x2, a2, seed=SEED)
    assert sonic.srs_verify_update(new, third, proof2) is True
    assert sonic.srs_verify_update(h.srs, third, proof2) is False and sonic.srs_verify_update(h.srs, third, proof) is False


# ---- the string is usable -----------------------------------------------------------------------------------------------------------------
def test_an_updated_string_proves_and_verifies(sonic, honest, ref):
    d, n, Q = 300, 16, 2
    h = honest(d)
    new, _ = h.srs.update(*trapdoor(d, 1), seed=SEED)
    pyr = random.Random(99)
    circ, asg, _ = circuit_arrays(ref, pyr, n, Q)
    circuit = sonic.ArithCircuit(sonic.GateWeights(circ[0], circ[1], circ[2]), circ[3])
    assignment = sonic.Assignment(*asg)
    tr = [pyr.randrange(1, R) for _ in range(8 + 2 * Q)]
    proof, o = sonic.prove(new, assignment, circuit, transcript=tr)
    assert sonic.verify(new, circuit, proof, o.rndOracleY, o.rndOracleZ, o.rndOracleYZs) is True
    old_proof, oo = sonic.prove(h.srs, assignment, circuit, transcript=tr)
    assert old_proof.to_bytes() != proof.to_bytes()
    assert sonic.verify(h.srs, circuit, old_proof, oo.rndOracleY, oo.rndOracleZ, oo.rndOracleYZs) is True
    assert sonic.verify(new, circuit, old_proof, oo.rndOracleY, oo.rndOracleZ, oo.rndOracleYZs) is False
    assert sonic.fs_srs_id(new) != sonic.fs_srs_id(h.srs)
    view = new.for_circuit(n, Q)
    assert sonic.prove(view, assignment, circuit, transcript=tr)[0].to_bytes() == proof.to_bytes()


# ---- refusals -----------------------------------------------------------------------------------------------------------------------------
def refused(sonic, code, call, *needles):
    with pytest.raises(sonic.SonicError) as e:
        call()
    assert e.value.code == code, (e.value.code, e.value.message)
    assert e.value.message, "a refusal carries a message"
    for s in needles:
        assert s in e.value.message, (s, e.value.message)


def test_refusals(sonic, honest):
    d = 300
    h = honest(d)
    view = h.srs.for_circuit(16, 2)
    refused(sonic, INVALID_ARG, lambda: view.check(SEED), "view")
    refused(sonic, INVALID_ARG, lambda: view.update(2, 3), "view")
    new, proof = h.srs.update(2, 3, seed=SEED)
    refused(sonic, INVALID_ARG, lambda: sonic.srs_verify_update(view, new, proof), "view")
    g1_only = sonic.SRS.from_points(d, h.arrays[0], h.arrays[1])
    assert not g1_only.has_g2()
    refused(sonic, INVALID_ARG, lambda: g1_only.check(SEED), "G2")
    refused(sonic, INVALID_ARG, lambda: g1_only.update(2, 3), "G2")
    refused(sonic, INVALID_ARG, lambda: h.srs.update(0, 3), "zero")
    refused(sonic, INVALID_ARG, lambda: h.srs.update(2, 0), "zero")
    refused(sonic, BAD_ENCODING, lambda: h.srs.update(R, 3), "< r")
    refused(sonic, BAD_ENCODING, lambda: h.srs.update(2, R + 5), "< r")
    assert h.srs.check(SEED) == (True, 0)                          # and the handle is as it was
