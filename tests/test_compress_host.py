"""The compressed point encodings without a GPU: the HD field functions and point codecs as the host compiles them
(tests/host/compress_host.cpp, plain and under ASan / UBSan with the flags of tests/host/Makefile), the pure-Python mirror
(sonic_amd/encoding.py), one proof's re-encoding through the C ABI (sonic_proof_compress / sonic_proof_decompress), the compressed SRS
container's reader on hostile files, and the new symbols.  Every comparison is byte-exact."""
import ctypes as C
import json
import os
import random
import re
import struct
import subprocess

import pytest

from oracle import pairing as pr
from oracle.sonic_ref import G1_GEN, Q, g1_add, g1_mul
from sonic_amd import _lib, encoding as enc

HERE = os.path.dirname(os.path.abspath(__file__))
HOST = os.path.join(HERE, "host")
ENV = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
G1_GEN_Z = "97f1d3a73197d7942695638c4fa9ac0fc3688c4f9774b905a14e3a3f171bac586c55e83ff97a1aeffb3af00adb22c6bb"
NEW_SYMBOLS = ["sonic_g1_compress", "sonic_g1_decompress", "sonic_g2_compress", "sonic_g2_decompress", "sonic_proof_size_compressed", "sonic_proof_compress",
               "sonic_proof_decompress", "sonic_verifier_verify_batch_z", "sonic_verifier_verify_fs_batch_z", "sonic_srs_save_compressed"]


@pytest.fixture(scope="module")
def drivers():
    subprocess.check_call(["make", "-C", HOST, "-s", "-f", "compress.mk", "compress_host", "compress_host_san"])
    return {"plain": os.path.join(HOST, "compress_host"), "san": os.path.join(HOST, "compress_host_san")}


def run_driver(path, lines):
    out = subprocess.run([path], input="\n".join(lines) + "\n", capture_output=True, text=True, timeout=600, env=ENV)
    assert out.returncode == 0 and out.stdout.endswith("compress_host ok\n"), out.stdout[-2000:] + out.stderr[-3000:]
    return out.stdout.splitlines()[:-1]


def is_square(a):
    return a % Q == 0 or pow(a, (Q - 1) // 2, Q) == 1


def f2_is_square(a):                       # the norm decides in Fq2
    return is_square((a[0] * a[0] + a[1] * a[1]) % Q)


@pytest.fixture(scope="module")
def field_cases():
    rng = random.Random(381)
    fq = [0, 1, 4, Q - 1] + [pow(rng.randrange(Q), 2, Q) for _ in range(64)] + [rng.randrange(Q) for _ in range(64)]
    rand = fq[-64:]
    assert any(is_square(a) for a in rand) and any(not is_square(a) for a in rand)          # the fixed seed gives both kinds
    sq, nsq = next(a for a in rand if is_square(a) and a), next(a for a in rand if not is_square(a))
    fq2 = [(sq, 0), (nsq, 0), (0, sq), (0, nsq), (0, 0)]
    for _ in range(64):
        e = (rng.randrange(Q), rng.randrange(Q))
        fq2.append(pr.f2_sqr(e))
    fq2 += [(rng.randrange(Q), rng.randrange(Q)) for _ in range(16)]
    assert any(not f2_is_square(a) for a in fq2)
    high = [0, 1, (Q - 1) // 2, (Q + 1) // 2, Q - 1] + rand[:8]
    return fq, fq2, high


def check_field_functions(driver, field_cases):
    fq, fq2, high = field_cases
    lines = ["sqrt %x" % a for a in fq] + ["sqrt2 %x %x" % a for a in fq2] + ["high %x" % y for y in high] + \
            ["high2 %x %x" % (c0, c1) for c0 in high[:5] for c1 in (0, 1, Q - 1)]
    got = iter(run_driver(driver, lines))
    for a in fq:
        ok, r = next(got).split()
        want = pow(a, (Q + 1) // 4, Q)
        assert int(r, 16) == want and int(ok) == int(want * want % Q == a), hex(a)
    for a in fq2:
        ok, r0, r1 = next(got).split()
        r = (int(r0, 16), int(r1, 16))
        assert int(ok) == int(f2_is_square(a)), a
        if int(ok):
            assert pr.f2_sqr(r) == a and r[0] < Q and r[1] < Q, a
            m = enc.fq2_sqrt(a)                                        # the mirror finds a root as well (its sign may differ)
            assert m is not None and pr.f2_sqr(m) == a
        else:
            assert enc.fq2_sqrt(a) is None
    for y in high:
        assert int(next(got)) == int(y > (Q - 1) // 2) == int(enc.fq_is_high(y))
    for c0 in high[:5]:
        for c1 in (0, 1, Q - 1):
            assert int(next(got)) == int(enc.fq2_is_high((c0, c1))) == int((c1 if c1 else c0) > (Q - 1) // 2)


def test_field_square_roots_and_signs(drivers, field_cases):
    check_field_functions(drivers["plain"], field_cases)


def test_field_square_roots_and_signs_under_sanitizers(drivers, field_cases):
    check_field_functions(drivers["san"], field_cases)


# ---- the pure-Python mirror ----
@pytest.fixture(scope="module")
def multiples():
    g1 = [g1_mul(G1_GEN, k) for k in range(1, 65)]
    g2 = [pr.g2_mul(pr.G2_GEN, k) for k in range(1, 65)]
    return g1, g2


def off_curve_x():
    return next(x for x in range(1, 100) if not is_square(x ** 3 + 4))


def test_known_answers():
    assert enc.g1_compress(G1_GEN).hex() == G1_GEN_Z and enc.g1_decompress(bytes.fromhex(G1_GEN_Z)) == G1_GEN
    (x0, x1), _ = pr.G2_GEN
    z = enc.g2_compress(pr.G2_GEN)
    assert z == (x1 | 1 << 383).to_bytes(48, "big") + x0.to_bytes(48, "big") and z.hex().startswith("93e02b60")
    assert enc.g2_decompress(z) == pr.G2_GEN
    assert enc.g1_compress(None) == b"\xc0" + bytes(47) and enc.g1_decompress(b"\xc0" + bytes(47)) is None
    assert enc.g2_compress(None) == b"\xc0" + bytes(95) and enc.g2_decompress(b"\xc0" + bytes(95)) is None


def test_round_trips_cover_both_signs(multiples):
    g1, g2 = multiples
    for pts, comp, dec in ((g1, enc.g1_compress, enc.g1_decompress), (g2, enc.g2_compress, enc.g2_decompress)):
        signs = []
        for p in pts:
            z = comp(p)
            assert dec(z) == p and z[0] & 0x80 and not z[0] & 0x40
            signs.append(bool(z[0] & 0x20))
        assert min(signs.count(True), signs.count(False)) >= len(pts) // 4          # a condition on the inputs, held here


def test_refusals():
    z = bytes.fromhex(G1_GEN_Z)
    bad = [bytes([z[0] & 0x7F]) + z[1:],                          # compression bit clear
           b"\xe0" + bytes(47), b"\xc0" + bytes(46) + b"\x01", bytes([0xC0 | z[0] & 0x1F]) + z[1:],      # infinity bit with anything else
           (Q | 1 << 383).to_bytes(48, "big")]                    # x = q
    for b in bad:
        with pytest.raises(enc.PointRefused) as e:
            enc.g1_decompress(b)
        assert e.value.verdict == enc.Z_MALFORMED
    with pytest.raises(enc.PointRefused) as e:
        enc.g1_decompress((off_curve_x() | 1 << 383).to_bytes(48, "big"))
    assert e.value.verdict == enc.Z_OFF_CURVE
    z2 = enc.g2_compress(pr.G2_GEN)
    for b in (bytes([z2[0] & 0x7F]) + z2[1:], b"\xc0" + bytes(94) + b"\x01", (Q | 1 << 383).to_bytes(48, "big") + bytes(48),
              z2[:48] + bytes([z2[48] | 0x80]) + z2[49:], z2[:48] + Q.to_bytes(48, "big")):
        with pytest.raises(enc.PointRefused) as e:
            enc.g2_decompress(b)
        assert e.value.verdict == enc.Z_MALFORMED
    x2 = next(x for x in range(1, 100) if not f2_is_square(((x ** 3 + 4) % Q, 4)))
    with pytest.raises(enc.PointRefused) as e:
        enc.g2_decompress((1 << 383).to_bytes(48, "big") + x2.to_bytes(48, "big"))
    assert e.value.verdict == enc.Z_OFF_CURVE


def check_point_codecs(driver, multiples):
    """the host build of compress.hpp's point functions against the mirror"""
    g1, g2 = multiples
    g1, g2 = g1[:8] + [None], g2[:4] + [None]
    edge = ["80" + "00" * 47, "a0" + "00" * 47, "c0" + "00" * 47, "e0" + "00" * 47, "00" * 48, (Q | 1 << 383).to_bytes(48, "big").hex(),
            (off_curve_x() | 1 << 383).to_bytes(48, "big").hex()]
    lines = ["g1c " + enc.g1_to_bytes(p).hex() for p in g1] + ["g1d %s 1" % enc.g1_compress(p).hex() for p in g1] + ["g1d %s %d" % (e, s) for e in edge for s in (0, 1)] + \
            ["g2c " + enc.g2_to_bytes(p).hex() for p in g2] + ["g2d %s 1" % enc.g2_compress(p).hex() for p in g2]
    got = iter(run_driver(driver, lines))
    for p in g1:
        assert next(got) == enc.g1_compress(p).hex()
    for p in g1:
        assert next(got).split() == ["0", enc.g1_to_bytes(p).hex()]
    for e in edge:
        for sub in (0, 1):
            try:
                p, verdict = enc.g1_decompress(bytes.fromhex(e)), 0
                if sub and p is not None and g1_add(g1_mul(p, pr.R - 1), p) is not None:          # r P != O (g1_mul reduces its scalar mod r)
                    p, verdict = None, enc.Z_OUTSIDE_SUBGROUP
            except enc.PointRefused as r:
                p, verdict = None, r.verdict
            assert next(got).split() == [str(verdict), enc.g1_to_bytes(p).hex()], (e, sub)
    for p in g2:
        assert next(got) == enc.g2_compress(p).hex()
    for p in g2:
        assert next(got).split() == ["0", enc.g2_to_bytes(p).hex()]


def test_point_codecs_host_build(drivers, multiples):
    check_point_codecs(drivers["plain"], multiples)
    # (0, 2) has order 3: on the curve, outside the subgroup
    assert enc.g1_decompress(bytes.fromhex("80" + "00" * 47)) == (0, 2) and enc.g1_decompress(bytes.fromhex("a0" + "00" * 47)) == (0, Q - 2)


def test_point_codecs_under_sanitizers(drivers, multiples):
    check_point_codecs(drivers["san"], multiples)


# ---- one proof through the C ABI (no device) ----
def golden_proofs():
    out = []
    for name in ("prove_small.json", "fs_small.json"):
        for c in json.load(open(os.path.join(HERE, "golden", name)))["cases"]:
            if "proof" in c:
                proof = bytes.fromhex(c["proof"])
                out.append(((len(proof) - 832) // 448, proof))                 # (7 + 4Q) 96 + (5 + 2Q) 32 bytes
    return out


def mirror_compress(proof: bytes, Qn: int) -> bytes:
    """the compressed proof by the mirror: record order R T a Wa b Wb Wt s [S s W]* [s' W' Q]* Qv C u v"""
    order = "GGFGFGGF" + "GFG" * Qn + "FGG" * Qn + "GGFF"
    out, pos = b"", 0
    for kind in order:
        if kind == "G":
            out += enc.g1_compress(enc.g1_from_bytes(proof[pos:pos + 96])); pos += 96
        else:
            out += proof[pos:pos + 32]; pos += 32
    assert pos == len(proof)
    return out


def c_compress(L, Qn, proof):
    out = C.create_string_buffer(L.sonic_proof_size_compressed(Qn))
    return L.sonic_proof_compress(Qn, proof, out), out.raw


def c_decompress(L, Qn, z):
    out = C.create_string_buffer(L.sonic_proof_size(Qn))
    return L.sonic_proof_decompress(Qn, z, out), out.raw


def test_proof_compress_round_trip_and_refusals():
    L = _lib.lib()
    for Qn in (1, 2, 5):
        assert L.sonic_proof_size_compressed(Qn) == (7 + 4 * Qn) * 48 + (5 + 2 * Qn) * 32 != L.sonic_proof_size(Qn)
    proofs = golden_proofs()
    assert len(proofs) >= 2
    for Qn, proof in proofs:
        rc, z = c_compress(L, Qn, proof)
        assert rc == 0 and z == mirror_compress(proof, Qn)
        rc, back = c_decompress(L, Qn, z)
        assert rc == 0 and back == proof
    Qn, proof = proofs[0]
    _, z = c_compress(L, Qn, proof)
    # T is the second point: its sign bit flipped is -T, another valid proof
    flipped = z[:48] + bytes([z[48] ^ 0x20]) + z[49:]
    rc, other = c_decompress(L, Qn, flipped)
    T = enc.g1_from_bytes(proof[96:192])
    assert rc == 0 and other != proof and other[:96] == proof[:96] and other[192:] == proof[192:] and enc.g1_from_bytes(other[96:192]) == (T[0], Q - T[1])
    for bad_point in ((off_curve_x() | 1 << 383).to_bytes(48, "big"), b"\x80" + bytes(47), bytes(48)):       # off the curve; (0, 2), order 3; no compression bit
        rc, _ = c_decompress(L, Qn, bad_point + z[48:])
        assert rc == 3, bad_point.hex()
    rc, _ = c_decompress(L, Qn, z[:-32] + b"\xff" * 32)                  # v is no canonical field element
    assert rc == 3
    rc, _ = c_compress(L, Qn, (0).to_bytes(48, "little") + (2).to_bytes(48, "little") + proof[96:])      # (0, 2) uncompressed: refused as load_g1 refuses it
    assert rc == 3


def test_python_proof_takes_either_length():
    import sonic_amd
    Qn, proof = golden_proofs()[0]
    p = sonic_amd.Proof.from_bytes(proof, Qn)
    z = p.to_bytes(compressed=True)
    assert len(z) == _lib.lib().sonic_proof_size_compressed(Qn) and z == mirror_compress(proof, Qn)
    assert sonic_amd.Proof.from_bytes(z, Qn) == p and p.to_bytes() == proof


# ---- the compressed SRS container's reader on hostile files ----
def zfile(d, flags=0, version=1, magic=b"SONICSRZ", body=None):
    n = 2 * d + 1 if 0 < d < 1000 else 3
    if body is None:
        body = bytes(range(256)) * ((2 * n * 48 + (2 * n * 96 if flags & 1 else 0)) // 256 + 1)
        body = body[:2 * n * 48 + (2 * n * 96 if flags & 1 else 0)]
    return magic + struct.pack("<IIq", version, flags, d) + body


def test_compressed_srs_file_reader_under_sanitizers(drivers, tmp_path):
    cases = {"good": (zfile(3), 0), "good_g2": (zfile(3, 1), 0), "truncated": (zfile(3, 1)[:-1], 3), "trailing": (zfile(3) + b"\0", 3), "d0": (zfile(0), 2),
             "dhuge": (zfile(1 << 40), 2), "flags": (zfile(3, 2), 2), "version2": (zfile(3, version=2), 2), "old_magic": (zfile(3, magic=b"SONICSRS"), 2)}
    for name, (blob, _) in cases.items():
        (tmp_path / name).write_bytes(blob)
    got = run_driver(drivers["san"], ["zfile %s" % (tmp_path / name) for name in cases] + ["zfile %s" % (tmp_path / "missing"), "sfile %s" % (tmp_path / "good")])
    for (name, (blob, want)), line in zip(cases.items(), got):
        f = [int(x) for x in line.split()]
        assert f[0] == want, (name, line)
        if want == 0:
            g2 = name == "good_g2"
            assert f[1:] == [1, int(g2), 3, 7 * 48, 7 * 48, 7 * 96 * g2, 7 * 96 * g2], line
        else:
            assert f[4:] == [0, 0, 0, 0], line                     # nothing is kept of a file that fails
    assert got[-2].split()[0] == "1"
    assert got[-1].split()[0] == "2"                               # srs_file_read refuses the compressed magic


def test_new_symbols_declared_exported_and_bound():
    hdr = open(os.path.join(os.path.dirname(HERE), "include", "sonic_hip.h")).read()
    L = _lib.lib()
    for name in NEW_SYMBOLS:
        assert re.search(r"\b%s\s*\(" % name, hdr), name
        assert name in _lib.EXPORTED and getattr(L, name).argtypes is not None, name
    assert L.sonic_abi_version() == 7 and _lib.ABI_VERSION == 7
