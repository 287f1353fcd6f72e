"""The compressed encodings on the GPU (include/sonic_hip.h, "Compressed encodings"; sonic_amd/csrc/compress.hip): the four bulk kernels
against the pure-Python mirror (sonic_amd/encoding.py, itself pinned by tests/test_compress_host.py), the compressed SRS container, and
the batched verifier's `_z` entry points against the uncompressed ones.  Every comparison is byte-exact."""
import ctypes as C
import hashlib
import os
import random

import numpy as np
import pytest

from util import R, circuit_arrays

pytestmark = pytest.mark.gpu

QMOD = 0x1a0111ea397fe69a4b1ba7b6434bacd764774b84f38512bf6730d2a0f6b0f6241eabfffeb153ffffb9feffffffffaaab
SEED = bytes(range(32))


def be(v, flags=0x80):
    return (v | flags << 376).to_bytes(48, "big")


def is_square(a):
    return a % QMOD == 0 or pow(a, (QMOD - 1) // 2, QMOD) == 1


OFF_CURVE_X = next(x for x in range(1, 100) if not is_square(x ** 3 + 4))
# (0, 2) and (0, -2) of order 3; infinity; then the refusals: no compression bit, infinity with a sign / with a byte set, x = q, x off the curve
G1_EDGES = [be(0), be(0, 0xA0), be(0, 0xC0), be(5, 0x00), be(0, 0xE0), be(1, 0xC0), be(QMOD), be(OFF_CURVE_X)]


@pytest.fixture(scope="module")
def enc():
    from sonic_amd import encoding
    return encoding


def g1_expect(enc, ref, z, check_subgroup, trusted):
    """(96 bytes, flag) of one encoding by the mirror; `trusted`: a point of an SRS, known to lie in the subgroup"""
    try:
        p = enc.g1_decompress(z)
    except enc.PointRefused as r:
        return bytes(96), r.verdict
    if check_subgroup and p is not None and not trusted and ref.g1_add(ref.g1_mul(p, R - 1), p) is not ref.INF:
        return bytes(96), enc.Z_OUTSIDE_SUBGROUP
    return enc.g1_to_bytes(p), 0


@pytest.fixture(scope="module")
def g1_world(sonic, enc):
    """257 encodings: points of an SRS at d = 200 with the edge encodings at positions 0, 255, 256 (and the rest of them from 1 on)"""
    srs = sonic.SRS.new(200, 0x1234567, 0x7654321)
    pts = srs.points(0, -200, 401)
    srs.close()
    zs = [enc.g1_compress(enc.g1_from_bytes(bytes(pts[i]))) for i in range(257)]
    trusted = [True] * 257
    for pos, e in zip([0, 255, 256, 1, 2, 3, 4, 5], [G1_EDGES[0], G1_EDGES[7], G1_EDGES[6], G1_EDGES[1], G1_EDGES[2], G1_EDGES[3], G1_EDGES[4], G1_EDGES[5]]):
        zs[pos], trusted[pos] = e, False
    assert {z[0] & 0x20 for z in zs[6:255]} == {0, 0x20}             # both signs among the SRS points
    return zs, trusted, pts


@pytest.mark.parametrize("n", [0, 1, 255, 256, 257])
@pytest.mark.parametrize("check", [1, 0])
def test_g1_decompress_matches_the_mirror(sonic, enc, ref, g1_world, n, check):
    zs, trusted, _ = g1_world
    zin = np.frombuffer(b"".join(zs[:n]), np.uint8).reshape(n, 48)
    out, flags = sonic.g1_decompress(zin, check_subgroup=bool(check), flags=True)
    assert out.shape == (n, 96) and flags.shape == (n,)
    for i in range(n):
        want, fl = g1_expect(enc, ref, zs[i], check, trusted[i])
        assert (bytes(out[i]), int(flags[i])) == (want, fl), (i, zs[i].hex())
    if n:
        assert int(flags[0]) == (4 if check else 0)                   # (0, 2): on the curve, outside the subgroup
        if not check:
            assert bytes(out[0]) == bytes(48) + (2).to_bytes(48, "little")
    if n >= 2 and not check:
        assert bytes(out[1]) == bytes(48) + (QMOD - 2).to_bytes(48, "little")      # 0xa0...: y = q - 2


def test_g1_refusals_without_flags_and_round_trip(sonic, g1_world):
    zs, _, pts = g1_world
    with pytest.raises(sonic.SonicError) as e:
        sonic.g1_decompress(np.frombuffer(b"".join(zs[250:257]), np.uint8).reshape(-1, 48))      # one refused point, flags = NULL
    assert e.value.code == 3
    good = np.frombuffer(b"".join(zs[6:255] + [G1_EDGES[2]]), np.uint8).reshape(-1, 48)           # SRS points and infinity
    back = sonic.g1_decompress(good)
    assert bytes(back[:-1]) == bytes(pts[6:255]) and bytes(back[-1]) == bytes(96)
    assert bytes(sonic.g1_compress(back)) == bytes(good)
    with pytest.raises(sonic.SonicError) as e:
        sonic.g1_compress(np.frombuffer(bytes(48) + (2).to_bytes(48, "little"), np.uint8).reshape(1, 96))   # (0, 2) uncompressed
    assert e.value.code == 3
    assert sonic.g1_compress(np.zeros((0, 96), np.uint8)).shape == (0, 48)


# ---- G2 ----
@pytest.fixture(scope="module")
def g2_world(sonic, enc):
    from oracle import pairing as pr
    srs = sonic.SRS.new(40, 0x1234567, 0x7654321)
    pts = srs.g2_points(1, -40, 81)
    srs.close()
    zs = [enc.g2_compress(enc.g2_from_bytes(bytes(pts[i]))) for i in range(65)]
    trusted = [True] * 65
    # a point of the twist outside the subgroup (no cofactor clearing), and an x off the twist
    x = 1
    while True:
        try:
            rogue = enc.g2_decompress(be(0) + x.to_bytes(48, "big"))
            if pr.g2_add(pr.g2_mul(rogue, R - 1), rogue) is not None:
                break
        except enc.PointRefused:
            pass
        x += 1
    off = next(be(0) + v.to_bytes(48, "big") for v in range(1, 100) if not is_square((((v ** 3 + 4) % QMOD) ** 2 + 16) % QMOD))
    edges = {0: enc.g2_compress(rogue), 63: off, 64: be(QMOD) + bytes(48), 1: be(0, 0xC0) + bytes(48), 2: be(0, 0xE0) + bytes(48),
             3: be(7, 0x00) + bytes(48), 4: enc.g2_compress(pr.G2_GEN), 5: zs[5][:48] + bytes([0x80]) + zs[5][49:]}
    for pos, e in edges.items():
        zs[pos], trusted[pos] = e, pos == 4
    assert {z[0] & 0x20 for z in zs[6:63]} == {0, 0x20}
    return zs, trusted, pts, rogue


@pytest.mark.parametrize("n", [0, 1, 63, 64, 65])
@pytest.mark.parametrize("check", [1, 0])
def test_g2_decompress_matches_the_mirror(sonic, enc, g2_world, n, check):
    zs, trusted, _, rogue = g2_world
    zin = np.frombuffer(b"".join(zs[:n]), np.uint8).reshape(n, 96)
    out, flags = sonic.g2_decompress(zin, check_subgroup=bool(check), flags=True)
    for i in range(n):
        try:
            p, fl = enc.g2_decompress(zs[i]), 0
            if check and i == 0:
                p, fl = None, enc.Z_OUTSIDE_SUBGROUP                # the rogue point (its verdict by Python: the fixture)
        except enc.PointRefused as r:
            p, fl = None, r.verdict
        assert (bytes(out[i]), int(flags[i])) == (enc.g2_to_bytes(p), fl), (i, zs[i].hex())
    if n and not check:
        assert bytes(out[0]) == enc.g2_to_bytes(rogue)


def test_g2_known_answer_refusals_and_round_trip(sonic, enc, g2_world):
    from oracle import pairing as pr
    zs, _, pts, rogue = g2_world
    gen = np.frombuffer(enc.g2_to_bytes(pr.G2_GEN), np.uint8).reshape(1, 192)
    z = sonic.g2_compress(gen)
    (x0, x1), _ = pr.G2_GEN
    assert bytes(z[0]) == (x1 | 1 << 383).to_bytes(48, "big") + x0.to_bytes(48, "big") and bytes(z[0]).hex().startswith("93e02b60")
    assert bytes(sonic.g2_decompress(z)) == bytes(gen)
    with pytest.raises(sonic.SonicError) as e:
        sonic.g2_decompress(np.frombuffer(b"".join(zs[60:65]), np.uint8).reshape(-1, 96))
    assert e.value.code == 3
    good = np.frombuffer(b"".join(zs[6:63] + [be(0, 0xC0) + bytes(48)]), np.uint8).reshape(-1, 96)
    back = sonic.g2_decompress(good)
    assert bytes(back[:-1]) == bytes(pts[6:63]) and bytes(back[-1]) == bytes(192)
    assert bytes(sonic.g2_compress(back)) == bytes(good)
    with pytest.raises(sonic.SonicError) as e:
        sonic.g2_compress(np.frombuffer(enc.g2_to_bytes(rogue), np.uint8).reshape(1, 192))
    assert e.value.code == 3


# ---- the compressed SRS container ----
@pytest.fixture(scope="module")
def small_statement(sonic, ref):
    pyr = random.Random(1602)
    n, Q = 16, 2
    _, _, e = circuit_arrays(ref, pyr, n, Q)
    circuit = sonic.ArithCircuit(sonic.GateWeights(e["wL"], e["wR"], e["wO"]), e["cs"])
    asg = sonic.Assignment(e["aL"], e["aR"], e["aO"])
    tr = [pyr.randrange(1, R) for _ in range(8 + 2 * Q)]
    return n, Q, circuit, asg, tr


def prove_bytes(sonic, srs, circuit, asg, tr):
    p = sonic.Prover(srs, circuit)
    p.set_assignment(asg)
    raw = p.prove_bytes(tr)
    p.close()
    return raw


def test_srs_compressed_container(sonic, enc, small_statement, tmp_path):
    d, m = 200, 401
    srs = sonic.SRS.new(d, 0xabcdef01, 0x10fedcba)
    want = [srs.points(b, -d, m) for b in (0, 1)], [srs.g2_points(b, -d, m) for b in (0, 1)]
    path = str(tmp_path / "srs.z")
    srs.save(path, g2=True, compressed=True)
    assert os.path.getsize(path) == 24 + 2 * m * 48 + 2 * m * 96
    blob = open(path, "rb").read()
    assert blob[:8] == b"SONICSRZ" and blob[24 + 48 * (m + d):24 + 48 * (m + d + 1)] == b"\xc0" + bytes(47)       # basis 1, e = 0: the omitted g^alpha
    assert blob[24:72] == enc.g1_compress(enc.g1_from_bytes(bytes(want[0][0][0])))
    loaded = sonic.SRS.load(path)
    for b in (0, 1):
        assert bytes(loaded.points(b, -d, m)) == bytes(want[0][b]) and bytes(loaded.g2_points(b, -d, m)) == bytes(want[1][b])
    # a proof over the loaded handle is the proof over the original, and verifies
    n, Q, circuit, asg, tr = small_statement
    raw = prove_bytes(sonic, srs, circuit, asg, tr)
    assert prove_bytes(sonic, loaded, circuit, asg, tr) == raw
    assert sonic.verify(loaded, circuit, sonic.Proof.from_bytes(raw, Q), tr[4], tr[5], list(zip(tr[6:6 + Q], tr[6 + Q:6 + 2 * Q])))
    loaded.close()
    # one sign bit flipped: -P is in the subgroup, the handle loads and differs at exactly that slot
    k = 137
    off = 24 + 48 * k
    flipped = str(tmp_path / "flipped.z")
    open(flipped, "wb").write(blob[:off] + bytes([blob[off] ^ 0x20]) + blob[off + 1:])
    other = sonic.SRS.load(flipped)
    got = other.points(0, -d, m)
    other.close()
    diff = [i for i in range(m) if bytes(got[i]) != bytes(want[0][0][i])]
    x, y = enc.g1_from_bytes(bytes(want[0][0][k]))
    assert diff == [k] and enc.g1_from_bytes(bytes(got[k])) == (x, QMOD - y)
    # an x off the curve, and infinity where none may be: refused
    for name, patch in (("offcurve.z", be(OFF_CURVE_X)), ("inf.z", be(0, 0xC0))):
        bad = str(tmp_path / name)
        open(bad, "wb").write(blob[:off] + patch + blob[off + 48:])
        with pytest.raises(sonic.SonicError) as e:
            sonic.SRS.load(bad)
        assert e.value.code == 3, name
    # the uncompressed container still round-trips beside it
    plain = str(tmp_path / "srs.bin")
    srs.save(plain, g2=True)
    again = sonic.SRS.load(plain)
    assert bytes(again.points(1, -d, m)) == bytes(want[0][1])
    again.close()
    srs.close()


# ---- the batched verifier over compressed proofs ----
def layout(Q, g=96):
    """offsets of the points and field elements of a proof whose points take g bytes"""
    g1, fr, o = [], [], 0
    for kind in "GGFGFGGF" + "GFG" * Q + "FGG" * Q + "GGFF":
        (g1 if kind == "G" else fr).append(o)
        o += g if kind == "G" else 32
    return g1, fr, o


def put(raw, off, b):
    return raw[:off] + b + raw[off + len(b):]


class Batch:
    def __init__(self, sonic, ref, Q, fs):
        pyr = random.Random(77 + Q)
        n, K = 16, 5
        self.Q, self.fs = Q, fs
        self.srs = sonic.SRS.new(7 * n + 12, pyr.randrange(2, R), pyr.randrange(2, R))
        _, _, e = circuit_arrays(ref, pyr, n, Q)
        circuit = sonic.ArithCircuit(sonic.GateWeights(e["wL"], e["wR"], e["wO"]), e["cs"])
        p = sonic.Prover(self.srs, circuit)
        p.set_assignment(sonic.Assignment(e["aL"], e["aR"], e["aO"]))
        digest = sonic.fs_circuit_digest(circuit) if fs else None
        self.proofs, self.trs = [], []
        for k in range(K):
            if fs:
                raw, tr = p.prove_fs(digest, hashlib.sha256(b"z%d" % k).digest())
            else:
                tr = [pyr.randrange(1, R) for _ in range(8 + 2 * Q)]
                raw = p.prove_bytes(tr)
            self.proofs.append(bytes(raw))
            self.trs.append((tr[4], tr[5], list(zip(tr[6:6 + Q], tr[6 + Q:6 + 2 * Q]))))
        p.close()
        self.ver = sonic.Verifier(self.srs, circuit)

    def verdicts(self, proofs):
        if self.fs:
            return self.ver.verify_fs_batch(proofs, seed=SEED, each=True)
        return self.ver.verify_batch(proofs, self.trs, seed=SEED, each=True)

    def close(self):
        self.ver.close()
        self.srs.close()


@pytest.fixture(scope="module")
def batches(sonic, ref):
    made = {}

    def get(Q, fs):
        if (Q, fs) not in made:
            made[(Q, fs)] = Batch(sonic, ref, Q, fs)
        return made[(Q, fs)]
    yield get
    for b in made.values():
        b.close()


@pytest.mark.parametrize("fs", [False, True], ids=["transcript", "fiat-shamir"])
@pytest.mark.parametrize("Q", [1, 2])
def test_verify_batch_z_is_verify_batch(sonic, batches, Q, fs):
    b = batches(Q, fs)
    g96, fr96, _ = layout(Q)
    g48, fr48, zsize = layout(Q, 48)
    plain = list(b.proofs)
    comp = [sonic.proof_compress(p, Q) for p in plain]
    assert all(len(z) == zsize for z in comp)
    # all valid
    assert b.verdicts(comp) == b.verdicts(plain) == (True, [True] * 5)
    # proof 2 with one evaluation altered (the field elements travel as they are)
    a = (int.from_bytes(plain[2][fr96[0]:fr96[0] + 32], "little") + 1) % R
    plain2, comp2 = list(plain), list(comp)
    plain2[2] = put(plain[2], fr96[0], a.to_bytes(32, "little"))
    comp2[2] = put(comp[2], fr48[0], a.to_bytes(32, "little"))
    assert comp2[2] == sonic.proof_compress(plain2[2], Q)
    want = b.verdicts(plain2)
    assert b.verdicts(comp2) == want and want == (False, [True, True, False, True, True])
    # proof 3 with the sign bit of T flipped: the compressed form of the proof with -T
    comp3 = list(comp)
    comp3[3] = put(comp[3], g48[1], bytes([comp[3][g48[1]] ^ 0x20]))
    plain3 = list(plain)
    plain3[3] = sonic.proof_decompress(comp3[3], Q)
    assert plain3[3] != plain[3]
    want = b.verdicts(plain3)
    assert b.verdicts(comp3) == want and want == (False, [True, True, True, False, True])
    # proof 4 with an x off the curve for R: rejected, and the others keep their verdicts
    comp4 = list(comp)
    comp4[4] = put(comp[4], g48[0], be(OFF_CURVE_X))
    plain4 = list(plain)
    plain4[4] = put(plain[4], g96[0], OFF_CURVE_X.to_bytes(48, "little") + (1).to_bytes(48, "little"))     # the uncompressed comparison: R off the curve
    want = b.verdicts(plain4)
    assert b.verdicts(comp4) == want and want == (False, [True, True, True, True, False])
    # a malformed point (no compression bit) in proof 0 beside the altered proof 2
    comp5 = list(comp2)
    comp5[0] = put(comp[0], g48[2], bytes(48))
    assert b.verdicts(comp5) == (False, [False, True, False, True, True])


def test_compressed_bytes_take_the_z_path(sonic, batches):
    from sonic_amd import _lib
    L = _lib.lib()
    b = batches(2, False)
    comp = [sonic.proof_compress(p, 2) for p in b.proofs]

    def launches(name):
        ms, cnt = C.c_double(0), C.c_int64(0)
        L.sonic_profile_get(name.encode(), C.byref(ms), C.byref(cnt))
        return cnt.value
    L.sonic_profile_enable(1)
    try:
        L.sonic_profile_reset()
        assert b.ver.verify_batch(comp, b.trs, seed=SEED) is True
        assert launches("k_g1_decompress") == 1 and launches("k_g1_validate") == 0
        L.sonic_profile_reset()
        assert b.ver.verify_batch([sonic.Proof.from_bytes(p, 2) for p in b.proofs], b.trs, seed=SEED) is True
        assert launches("k_g1_decompress") == 0 and launches("k_g1_validate") == 1
    finally:
        L.sonic_profile_enable(0)
        L.sonic_profile_reset()
