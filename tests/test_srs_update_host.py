"""The updatable SRS without a GPU: the HD scaling functions of both groups, the G2 addition, the randomizers of the structure check and the
proof of a contribution as the host compiles them (tests/host/srs_update_host.cpp, plain and under ASan / UBSan with the flags of
tests/host/Makefile), against Python integers over oracle/ and the restatement in tests/srs_update_ref.py -- which also makes, updates
and verifies whole strings at d = 12 with oracle/pairing.py.  Every comparison is of bytes or verdicts."""
import os
import random
import re
import subprocess

import pytest

import srs_update_ref as ref
from oracle import pairing as pr
from oracle.sonic_ref import G1_GEN, g1_mul
from sonic_amd import _lib, encoding as enc

HERE = os.path.dirname(os.path.abspath(__file__))
HOST = os.path.join(HERE, "host")
ENV = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
R = ref.R
NEW_SYMBOLS = ["sonic_srs_check", "sonic_srs_update", "sonic_srs_verify_update"]
SEED = bytes(range(7, 39))
# 1, 2, r - 1 (every limb's top bit region in use), a 128-bit value, one bit above a long run of zeros, one bit below it
SCALARS = [1, 2, R - 1, (1 << 128) - 159, 1 << 200, (1 << 250) + 1]


@pytest.fixture(scope="module")
def drivers():
    subprocess.check_call(["make", "-C", HOST, "-s", "-f", "srs_update.mk", "srs_update_host", "srs_update_host_san"])
    return {"plain": os.path.join(HOST, "srs_update_host"), "san": os.path.join(HOST, "srs_update_host_san")}


def run_driver(path, lines):
    out = subprocess.run([path], input="\n".join(lines) + "\n", capture_output=True, text=True, timeout=600, env=ENV)
    assert out.returncode == 0 and out.stdout.endswith("srs_update_host ok\n"), out.stdout[-2000:] + out.stderr[-3000:]
    return out.stdout.splitlines()[:-1]


def fr(k):
    return enc.fr_to_bytes(k).hex()


@pytest.fixture(scope="module")
def scale_cases():
    rng = random.Random(1717)
    ks = SCALARS + [rng.randrange(1, R) for _ in range(4)]
    p1, p2 = g1_mul(G1_GEN, rng.randrange(1, R)), pr.g2_mul(pr.G2_GEN, rng.randrange(1, R))
    g1 = [(p, k, 8) for p in (G1_GEN, p1) for k in ks] + [(p1, k, 4) for k in (1, (1 << 128) - 159, rng.randrange(1 << 128))] + [(None, 5, 8)]
    g2 = [(p, k, 8) for p in (pr.G2_GEN, p2) for k in ks] + [(p2, k, 4) for k in (1, (1 << 128) - 159, rng.randrange(1 << 128))] + [(None, 5, 8)]
    # the expected points once, with the oracle's arithmetic
    want1 = [enc.g1_to_bytes(g1_mul(p, k) if p else None).hex() for p, k, _ in g1]
    want2 = [enc.g2_to_bytes(pr.g2_mul(p, k) if p else None).hex() for p, k, _ in g2]
    adds = [(pr.G2_GEN, p2), (p2, p2), (p2, (p2[0], pr.f2_neg(p2[1]))), (None, p2), (p2, None)]
    return g1, want1, g2, want2, adds


def check_scaling(driver, scale_cases):
    g1, want1, g2, want2, adds = scale_cases
    lines = ["g1s %s %s %d" % (enc.g1_to_bytes(p).hex(), fr(k), limbs) for p, k, limbs in g1] + \
            ["g2s %s %s %d" % (enc.g2_to_bytes(p).hex(), fr(k), limbs) for p, k, limbs in g2] + \
            ["g2a %s %s" % (enc.g2_to_bytes(p).hex(), enc.g2_to_bytes(q).hex()) for p, q in adds]
    got = run_driver(driver, lines)
    assert got[:len(g1)] == want1
    assert got[len(g1):len(g1) + len(g2)] == want2
    assert got[len(g1) + len(g2):] == [enc.g2_to_bytes(pr.g2_add(p, q)).hex() for p, q in adds]


def test_scaling_functions_against_python_integers(drivers, scale_cases):
    check_scaling(drivers["plain"], scale_cases)


def test_scaling_functions_under_sanitizers(drivers, scale_cases):
    check_scaling(drivers["san"], scale_cases)


def test_check_randomizers_are_the_restated_hash(drivers):
    idx = [0, 1, 24, 255, 256, 65535, (1 << 22), (1 << 33) + 5]
    for name in ("plain", "san"):
        got = run_driver(drivers[name], ["rho %s %d" % (SEED.hex(), i) for i in idx] + ["rho %s 3" % bytes(32).hex()])
        assert [int.from_bytes(bytes.fromhex(g), "little") for g in got] == [ref.rho(SEED, i) for i in idx] + [ref.rho(bytes(32), 3)]
        assert all(len(g) == 32 for g in got)


@pytest.fixture(scope="module")
def contribution():
    rng = random.Random(448)
    d, old_id = 12, bytes(rng.randrange(256) for _ in range(32))
    x1, a1 = rng.randrange(1, R), rng.randrange(1, R)
    kx, ka = ref.seeded_nonce(SEED, x1, a1, old_id, 0), ref.seeded_nonce(SEED, x1, a1, old_id, 1)
    return d, old_id, x1, a1, kx, ka, ref.make_proof(d, old_id, x1, a1, kx, ka)


def test_proof_layout_challenge_and_nonces(drivers, contribution):
    d, old_id, x1, a1, kx, ka, proof = contribution
    assert len(proof) == ref.PROOF_BYTES == 448
    for name in ("plain", "san"):
        got = run_driver(drivers[name], ["nonce %s %s %s %s %d" % (SEED.hex(), fr(x1), fr(a1), old_id.hex(), i) for i in (0, 1)] +
                         ["chal %d %s %s" % (d, old_id.hex(), proof[:384].hex()), "make %d %s %s %s %s %s" % (d, old_id.hex(), fr(x1), fr(a1), fr(kx), fr(ka)),
                          "schnorr %d %s %s" % (d, old_id.hex(), proof.hex())])
        assert got[0] == fr(kx) and got[1] == fr(ka) and kx != ka
        assert got[2] == fr(ref.challenge(d, old_id, proof[:384]))
        assert got[3] == proof.hex()
        # the layout: X, A, Rx, Ra as multiples of g, then the two responses
        assert proof[:96] == enc.g1_to_bytes(g1_mul(G1_GEN, x1)) and proof[96:192] == enc.g1_to_bytes(g1_mul(G1_GEN, a1))
        assert proof[192:288] == enc.g1_to_bytes(g1_mul(G1_GEN, kx)) and proof[288:384] == enc.g1_to_bytes(g1_mul(G1_GEN, ka))
        c = ref.challenge(d, old_id, proof[:384])
        assert proof[384:416] == enc.fr_to_bytes((kx + c * x1) % R) and proof[416:] == enc.fr_to_bytes((ka + c * a1) % R)
        assert got[4].split() == ["1", proof[:96].hex(), proof[96:192].hex()]
    assert ref.schnorr_ok(d, old_id, proof) == (g1_mul(G1_GEN, x1), g1_mul(G1_GEN, a1))


def malformed(proof):
    """one mutant per field and per way a field can be wrong; every one must be refused"""
    order3 = (0).to_bytes(48, "little") + (2).to_bytes(48, "little")                # (0, 2): on the curve, order 3
    off = (1).to_bytes(48, "little") + (1).to_bytes(48, "little")
    out = {}
    for name, o in ref.OFF.items():
        width = 96 if o < 384 else 32
        out["flip " + name] = proof[:o] + bytes([proof[o] ^ 1]) + proof[o + 1:]
        if width == 96:
            out["infinity " + name] = proof[:o] + bytes(96) + proof[o + 96:]
            out["order-3 " + name] = proof[:o] + order3 + proof[o + 96:]
            out["off-curve " + name] = proof[:o] + off + proof[o + 96:]
            out["x = q " + name] = proof[:o] + pr.Q.to_bytes(48, "little") + proof[o + 48:]
        else:
            out["non-canonical " + name] = proof[:o] + enc.fr_to_bytes(0)[:0] + R.to_bytes(32, "little") + proof[o + 32:]
    out["swapped responses"] = proof[:384] + proof[416:] + proof[384:416]
    return out


def test_verifier_refuses_each_malformed_field(drivers, contribution):
    d, old_id, *_, proof = contribution
    bad = malformed(proof)
    others = {"another d": (d + 1, old_id, proof), "another old id": (d, bytes(32), proof)}
    lines = ["schnorr %d %s %s" % (d, old_id.hex(), p.hex()) for p in bad.values()] + ["schnorr %d %s %s" % (dd, i.hex(), p.hex()) for dd, i, p in others.values()]
    for name in ("plain", "san"):
        got = run_driver(drivers[name], lines)
        assert got == ["0"] * len(lines), [k for k, g in zip(list(bad) + list(others), got) if g != "0"]
    for k, p in bad.items():
        assert ref.schnorr_ok(d, old_id, p) is False, k


@pytest.fixture(scope="module")
def strings():
    """a string at d = 12 over Python integers, one contribution to it, and the proof"""
    rng = random.Random(12)
    d, x, alpha, x1, a1 = 12, rng.randrange(1, R), rng.randrange(1, R), rng.randrange(1, R), rng.randrange(1, R)
    old = ref.make_string(d, x, alpha)
    new = ref.update_string(old, x1, a1)
    old_id = ref.string_id(old)
    proof = ref.make_proof(d, old_id, x1, a1, ref.seeded_nonce(SEED, x1, a1, old_id, 0), ref.seeded_nonce(SEED, x1, a1, old_id, 1))
    return d, x, alpha, x1, a1, old, new, proof


def test_update_of_a_string_is_the_string_of_the_product(strings):
    d, x, alpha, x1, a1, old, new, proof = strings
    assert new == ref.make_string(d, x * x1 % R, alpha * a1 % R)
    assert ref.string_id(new) != ref.string_id(old)


def test_reference_verifier_and_host_pairing_agree_on_the_link_equations(drivers, strings):
    d, x, alpha, x1, a1, old, new, proof = strings
    assert ref.verify_update_links(old, new, proof)
    other = ref.update_string(old, x1 + 1, a1)                      # another contribution: the proof's X no longer links the strings
    assert not ref.verify_update_links(old, other, proof)
    assert not ref.verify_update_links(new, new, proof)             # the right proof against another old string
    X, A = g1_mul(G1_GEN, x1), g1_mul(G1_GEN, a1)
    g1b, g2b = (lambda p: enc.g1_to_bytes(p).hex()), (lambda p: enc.g2_to_bytes(p).hex())
    lines = ["peq %s %s %s %s" % (g1b(new["G0"][d + 1]), g2b(pr.G2_GEN), g1b(X), g2b(old["H0"][d + 1])),
             "peq %s %s %s %s" % (g1b(G1_GEN), g2b(new["H1"][d]), g1b(A), g2b(old["H1"][d])),
             "peq %s %s %s %s" % (g1b(other["G0"][d + 1]), g2b(pr.G2_GEN), g1b(X), g2b(old["H0"][d + 1])),
             "peq %s %s %s %s" % (g1b(G1_GEN), g2b(new["H1"][d]), g1b(A), g2b(new["H1"][d]))]
    assert run_driver(drivers["plain"], lines) == ["1", "1", "0", "0"]


def test_reference_check_accepts_and_names_the_relation(strings):
    d, x, alpha, x1, a1, old, new, proof = strings
    assert ref.check_string(new, SEED) == 0
    bad = dict(new, G0=list(new["G0"]))
    bad["G0"][2 * d] = bad["G0"][2 * d - 1]                          # G0[d] := G0[d-1]: R1 (P+), R2 (A0) and the full sum of R3, R4
    assert ref.check_string(bad, SEED) == 2 | 4 | 8 | 16


def test_new_symbols_declared_exported_and_bound():
    hdr = open(os.path.join(os.path.dirname(HERE), "include", "sonic_hip.h")).read()
    L = _lib.lib()
    for name in NEW_SYMBOLS:
        assert re.search(r"\b%s\s*\(" % name, hdr), name
        assert name in _lib.EXPORTED and getattr(L, name).argtypes is not None, name
    assert "SONIC_SRS_UPDATE_PROOF_SIZE 448" in hdr
    assert L.sonic_abi_version() == 7 and _lib.ABI_VERSION == 7
