"""The body of tests/test_gpu_stream_pool.py: ONE process, whose pool size SONIC_STREAM_POOL fixed before the library made its pool.
  python stream_pool_child.py ref FILE     proofs made one at a time on a fresh handle per shape, written to FILE (json)
  python stream_pool_child.py check FILE   the same proofs from handles that share the device -- two handles alternately, five in a ring, one
                                           freed beside a proof in flight, sonic_prove_batch's thread per handle, a Fiat-Shamir proof beside
                                           a streamed one -- compared by bytes with FILE
Prints "stream_pool_child ok" last; any difference is an assertion."""
import hashlib
import json
import os
import random
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

# (n, Q, SONIC_PROVE_FUSED): two fused shapes (chain streams; Q = 3: two chains), one with the mixed accumulation kernels, and the unfused
# lane path that large proofs take, at a small size
SHAPES = [(40, 2, None), (300, 3, None), (5000, 2, None), (300, 3, "0")]
N_TR = 8


def main():
    mode, path = sys.argv[1], sys.argv[2]
    import sonic_amd
    from sonic_amd import _lib
    from sonic_amd.workload import big_circuit
    from sonic_amd.protocol import R_MODULUS as R
    _lib.check(_lib.lib().sonic_init(0))
    ref = json.load(open(path)) if mode == "check" else {}
    for si, (n, Q, fused) in enumerate(SHAPES):
        if fused is None:
            os.environ.pop("SONIC_PROVE_FUSED", None)
        else:
            os.environ["SONIC_PROVE_FUSED"] = fused
        key = "%d/%d/%s" % (n, Q, fused)
        pyr = random.Random(7000 + si)
        srs = sonic_amd.SRS.new(7 * n + 5, pyr.randrange(1, R), pyr.randrange(1, R))
        c = big_circuit(11 + si, n, Q)
        circuit = sonic_amd.ArithCircuit(sonic_amd.GateWeights(c["wL"], c["wR"], c["wO"]), c["cs"])
        asg = sonic_amd.Assignment(c["aL"], c["aR"], c["aO"])
        trs = [[pyr.randrange(1, R) for _ in range(8 + 2 * Q)] for _ in range(N_TR)]
        digest, seed = sonic_amd.fs_circuit_digest(circuit), hashlib.sha256(b"stream-pool-%d" % si).digest()

        def handle():
            p = sonic_amd.Prover(srs, circuit)
            p.set_assignment(asg)
            return p

        if mode == "ref":
            p = handle()
            proofs = [p.prove_bytes(t).hex() for t in trs]
            p.submit_fs(digest, seed)
            raw, tr = p.collect_fs()
            p.close()
            assert len(set(proofs)) == N_TR
            ref[key] = dict(proofs=proofs, fs=[raw.hex(), [str(v) for v in tr]])
            srs.close()
            continue
        want = [bytes.fromhex(h) for h in ref[key]["proofs"]]
        want_fs = (bytes.fromhex(ref[key]["fs"][0]), [int(v) for v in ref[key]["fs"][1]])
        # two handles, six transcripts alternately: a proof is submitted before the other handle's is collected
        A, B = handle(), handle()
        hs, got = [A, B], []
        hs[0].submit(trs[0])
        for i in range(1, 6):
            hs[i % 2].submit(trs[i])
            got.append(hs[(i - 1) % 2].collect())
        got.append(hs[5 % 2].collect())
        assert got == want[:6], (key, "two handles alternately")
        # five handles in a ring: all in flight, collected in order, then once more the other way round
        ring = [A, B] + [handle() for _ in range(3)]
        for i, p in enumerate(ring):
            p.submit(trs[i])
        assert [p.collect() for p in ring] == want[:5], (key, "ring")
        for i, p in enumerate(ring):
            p.submit(trs[7 - i])
        assert [p.collect() for p in reversed(ring)] == [want[7 - i] for i in reversed(range(5))], (key, "ring, reversed")
        # a handle freed while another has a proof in flight
        ring[2].submit(trs[6])
        ring[4].close()
        ring[3].close()
        assert ring[2].collect() == want[6], (key, "free beside a flight")
        ring[2].close()
        # sonic_prove_batch: one library thread per handle
        assert sonic_amd.prove_batch([A, B], trs) == want, (key, "prove_batch")
        # ... and with every proof's assignment handed over with the call (a pooled handle uploads it on a stream of its own)
        assert sonic_amd.prove_batch([A, B], trs, assignments=[asg] * N_TR) == want, (key, "prove_batch, assignments from the host")
        # a Fiat-Shamir proof in flight (six passes on a worker thread) beside a plain streamed proof
        A.submit_fs(digest, seed)
        B.submit(trs[3])
        assert B.collect() == want[3], (key, "streamed beside fs")
        assert A.collect_fs() == want_fs, (key, "fs beside streamed")
        A.close()
        B.close()
        srs.close()
    if mode == "ref":
        json.dump(ref, open(path, "w"))
    print("stream_pool_child ok")


if __name__ == "__main__":
    main()
