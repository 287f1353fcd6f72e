"""sonic_amd/csrc/proof_layout.hpp is the one place that numbers a proof's MSM slots, evaluations, transcript elements and bytes.  A
host program (tests/host/proof_layout_host.cpp, plain g++) prints what the header and share_plan.hpp::share_line say for Q in
{1, 2, 5}; here that is held against the independent Python restatements: proof_parts and fr_owner_slot (tests/test_share_cpu.py),
Proof.from_bytes and the transcript order (sonic_amd/protocol.py).  CPU only."""
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "tests", "host")
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
QS = (1, 2, 5)


@pytest.fixture(scope="module")
def printed():
    """{Q: {"slot": {name: index}, "side": .., "eval": .., "tr": .., "pair": .., "count": .., "owner": {i: slot},
    "field": [(offset, kind, index)], "line": {(n, prepared): [(slot, terms)]}}}"""
    subprocess.check_call(["make", "-C", HOST, "-s", "proof_layout_host"])
    out = subprocess.run([os.path.join(HOST, "proof_layout_host")], capture_output=True, text=True, timeout=60, check=True).stdout
    res, cur = {}, None
    for ln in out.splitlines():
        w = ln.split()
        if w[0] == "Q":
            cur = res.setdefault(int(w[1]), {k: {} for k in ("slot", "side", "eval", "tr", "pair", "count", "owner")})
            cur["field"], cur["line"] = [], {}
        elif w[0] == "owner":
            cur["owner"][int(w[1])] = int(w[2])
        elif w[0] == "field":
            cur["field"].append((int(w[1]), w[2], int(w[3])))
        elif w[0] == "line":
            cur["line"].setdefault((int(w[1]), int(w[2])), []).append((int(w[3]), int(w[4])))
        else:
            assert w[1] not in cur[w[0]], ln
            cur[w[0]][w[1]] = int(w[2])
    assert sorted(res) == list(QS)
    return res


@pytest.mark.parametrize("Q", QS)
def test_slots_are_a_permutation_and_side_slots_follow(printed, Q):
    d = printed[Q]
    K = d["count"]["K"]
    assert K == 7 + 4 * Q and d["count"]["F"] == 3 + 2 * Q and d["count"]["slots_total"] == K + Q + 1
    assert len(d["slot"]) == K and sorted(d["slot"].values()) == list(range(K))
    assert sorted(d["side"].values()) == list(range(K, K + Q + 1)) and d["side"]["C_extra"] == K + Q
    assert [d["side"][f"S_extra{j}"] for j in range(Q)] == list(range(K, K + Q))
    assert sorted(d["eval"].values()) == list(range(3 + 2 * Q))
    # transcript: the draw order of sonic_amd.protocol.draw_transcript -- 4 blinders, y, z, ys, zs, u, v -- and one pair per challenge + yz
    from sonic_amd.protocol import transcript_len
    assert d["count"]["transcript_len"] == transcript_len(Q)
    order = ["y", "z"] + [f"y_j{j}" for j in range(Q)] + [f"z_j{j}" for j in range(Q)] + ["u", "v"]
    assert d["tr"].pop("n_blinders") == 4 and [d["tr"][k] for k in order] == list(range(4, 8 + 2 * Q)) and len(d["tr"]) == len(order)
    assert sorted(d["pair"].values()) == list(range(d["count"]["n_pairs"])) and d["count"]["n_pairs"] == 5 + 2 * Q


@pytest.mark.parametrize("Q", QS)
def test_offsets_match_the_python_restatements(printed, Q):
    from test_share_cpu import _oracle_proof, fr_owner_slot, proof_parts
    from sonic_amd.protocol import Proof
    from sonic_amd.protocol import g1_to_bytes
    d = printed[Q]
    K, F = 7 + 4 * Q, 3 + 2 * Q
    size = d["count"]["proof_bytes"]
    assert size == K * 96 + (F + 2) * 32
    off = {(kind, i): o for o, kind, i in d["field"]}
    assert len(off) == len(d["field"]) == K + F + 2
    # the fields tile the proof
    at = 0
    for o, kind, _ in d["field"]:
        assert o == at
        at += 96 if kind == "G" else 32
    assert at == size
    # proof_parts: a "proof" whose every 32-byte block starts with its own offset
    marked = b"".join(o.to_bytes(4, "little") + bytes(28) for o in range(0, size, 32))
    pts, frs = proof_parts(marked, Q)
    assert [int.from_bytes(p[:4], "little") for p in pts] == [off[("G", i)] for i in range(K)]
    assert [int.from_bytes(f[:4], "little") for f in frs] == [off[("F", i)] for i in range(F)]
    assert off[("T", d["tr"]["u"])] == size - 64 and off[("T", d["tr"]["v"])] == size - 32
    assert [d["owner"][i] for i in range(F)] == [fr_owner_slot(i, Q) for i in range(F)]
    # Proof.from_bytes on a real proof: every record field sits at the offset of the slot / evaluation of that name
    proof, _ = _oracle_proof(8, Q, 20 + Q)
    pr = Proof.from_bytes(proof, Q)
    h = pr.prHscProof
    S, E = d["slot"], d["eval"]
    g = {S["R"]: pr.prR, S["T"]: pr.prT, S["Wa"]: pr.prWa, S["Wb"]: pr.prWb, S["Wt"]: pr.prWt, S["Qv"]: h.hscQv, S["C"]: h.hscC}
    f = {E["a"]: pr.prA, E["b"]: pr.prB, E["s"]: pr.prS}
    for j in range(Q):
        g[S[f"S{j}"]], (f[E[f"s_j{j}"]], g[S[f"W{j}"]]) = h.hscS[j]
        f[E[f"sp_j{j}"]], g[S[f"Wp{j}"]], g[S[f"Qj{j}"]] = h.hscW[j]
    assert len(g) == K and len(f) == F
    for i in range(K):
        assert g1_to_bytes(g[i]) == proof[off[("G", i)]:off[("G", i)] + 96], i
    for i in range(F):
        assert f[i] == int.from_bytes(proof[off[("F", i)]:off[("F", i)] + 32], "little"), i
    assert h.hscU == int.from_bytes(proof[size - 64:size - 32], "little") and h.hscV == int.from_bytes(proof[size - 32:], "little")


@pytest.mark.parametrize("Q", QS)
def test_share_line_covers_every_slot_once_with_the_documented_terms(printed, Q):
    d = printed[Q]
    S = d["slot"]
    assert sorted(d["line"]) == [(n, pr) for n in (1, 16, 257) for pr in (0, 1)]
    for (n, prepared), line in d["line"].items():
        assert sorted(s for s, _ in line) == list(range(7 + 4 * Q)), (n, prepared)
        want = {S["T"]: 7 * n + 9, S["Wt"]: 7 * n + 8, S["R"]: 3 * n + 4, S["Wa"]: 3 * n + 4, S["Wb"]: 3 * n + 4,
                S["C"]: 2 * n + Q + 1, S["Qv"]: 2 * n + Q}
        for j in range(Q):
            want.update({S[f"S{j}"]: n if prepared else 3 * n + 1, S[f"W{j}"]: 3 * n, S[f"Wp{j}"]: 3 * n, S[f"Qj{j}"]: 2 * n + Q})
        assert dict(line) == want, (n, prepared)
