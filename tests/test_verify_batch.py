"""Batch PLONK verification on the host path (nzcb_verify_batch with NZCB_VERIFY_HOST, no
GPU needed): the G1 group routine against the oracle's curve arithmetic, the verdicts against
nzcb.verify item by item, the random weights, the number of pairing checks of the bisection,
and the per-item points under a fixed seed. The same cases run on the device in
tests/test_gpu_verify_batch.py."""
import json
import os

import pytest

import nzcb
import verify_batch_cases as C
from oracle import binfmt, bn254 as bn, plonk, synth

GOLD = os.path.join(os.path.dirname(__file__), "golden")
HOST = nzcb.VERIFY_HOST
SEED = bytes(range(32))


def _gold(name):
    meta = json.load(open(os.path.join(GOLD, f"{name}.json")))
    zkey = open(os.path.join(GOLD, f"{name}.zkey"), "rb").read()
    items = [(bytes.fromhex(meta["proofs"][bl]["proof_bin"]), C.pub_bytes(meta["proofs"][bl]["publicSignals"]))
             for bl in ("zero", "fixed")]
    return nzcb.vk_from_zkey(zkey), items


@pytest.fixture(scope="module")
def synth_batch():
    """synth_circuit(5, 2, 3): the key, the oracle's key, and 8 valid proofs under distinct blindings."""
    c = synth.synth_circuit(5, 2, 3, seed=31)
    zk = plonk.setup(c, 777)
    items = []
    for k in range(8):
        bls = [(b + 1000003 * k) % bn.R_MOD for b in synth.fixed_blindings()]
        proof, pub = plonk.prove(zk, c["witness"], bls)
        items.append((plonk.proof_to_bytes(proof), C.pub_bytes(pub)))
    assert len({p for p, _ in items}) == 8
    return nzcb.vk_from_zkey(binfmt.write_zkey(zk)), plonk.vk_from_zkey(zk), items


def _each(vk, items, **kw):
    return [nzcb.verify(vk, p, u, **kw) for p, u in items]


def _batch(vk, items, **kw):
    return nzcb.verify_batch(vk, [p for p, _ in items], [u for _, u in items], device=HOST, **kw)


# ---------------------------------------------------------------- 1. group routine
def test_lincomb_edge_cases_match_oracle():
    groups = C.edge_groups()
    got = nzcb.Engine.g1_lincomb(*C.pack(groups), device=HOST)
    assert got == C.oracle_sums(groups)
    assert got[-1] == bytes(64) and got[-4] == bytes(64)          # empty group, P + (r-1) P


def test_lincomb_random_groups_match_oracle():
    groups = C.random_groups(41, [1, 2, 18], seed=7)
    assert nzcb.Engine.g1_lincomb(*C.pack(groups), device=HOST) == C.oracle_sums(groups)
    assert nzcb.Engine.g1_lincomb(b"", b"", [], device=HOST) == []


def test_lincomb_rejects_decreasing_ends():
    pts, scs, _ = C.pack([[(C.G, 1), (C.G, 2)]])
    with pytest.raises(nzcb.NzcbError):
        nzcb.Engine.g1_lincomb(pts, scs, [2, 1, 2], device=HOST)


# ---------------------------------------------------------------- 2. verdicts
def test_verdicts_match_single_verifier(synth_batch):
    vk, _, good = synth_batch
    items = [good[k % 8] for k in range(16)]
    # first, last, middle and two adjacent positions; each kind of tampering
    for pos, kind in ((0, "eval"), (15, "point"), (7, "pub"), (10, "eval"), (11, "point")):
        items[pos] = C.tamper(*items[pos], kind)
    want = _each(vk, items)
    assert want == [k not in (0, 7, 10, 11, 15) for k in range(16)]
    assert _batch(vk, items) == want
    assert _batch(vk, items, seed=SEED) == want


@pytest.mark.parametrize("name", ["p5", "p8"])
def test_golden_proofs(name):
    vk, items = _gold(name)
    assert _batch(vk, items) == [True, True]
    items = items + [C.tamper(*items[1], "eval"), items[0]]
    assert _batch(vk, items) == _each(vk, items) == [True, True, False, True]


def test_malformed_items_leave_neighbours(synth_batch):
    vk, _, good = synth_batch
    items = list(good[:6])
    items[1] = C.tamper(*items[1], "offcurve")
    items[4] = C.tamper(*items[4], "big")
    items[5] = C.tamper(*items[5], "eval")
    want = [True, False, True, True, False, False]
    assert _each(vk, items) == want
    assert _batch(vk, items) == want


def test_wrong_n_public_all_invalid(synth_batch):
    vk, _, good = synth_batch
    proofs = [p for p, _ in good[:3]]
    pubs = [u + bytes(32) for _, u in good[:3]]                    # three signals for a key of two
    assert nzcb.verify_batch(vk, proofs, pubs, device=HOST) == [False] * 3
    valid, pts, checks = nzcb.Engine.verify_batch(vk, proofs, [u[:32] for _, u in good[:3]], device=HOST)
    assert valid == [False] * 3 and checks == 0 and pts == [bytes(128)] * 3


def test_count_zero_and_one(synth_batch):
    vk, _, good = synth_batch
    assert nzcb.verify_batch(vk, [], [], device=HOST) == []
    assert nzcb.Engine.verify_batch(vk, [], [], device=HOST) == ([], [], 0)
    assert _batch(vk, good[:1]) == [True]
    assert _batch(vk, [C.tamper(*good[0], "pub")]) == [False]


def test_agrees_with_oracle_verifier(synth_batch):
    vk, ovk, good = synth_batch
    items = [good[2], C.tamper(*good[3], "eval")]
    want = [plonk.verify(ovk, [bn.from_le(u[i:i + 32]) for i in range(0, len(u), 32)], plonk.proof_from_bytes(p))
            for p, u in items]
    assert want == [True, False]
    assert _batch(vk, items) == want


def test_json_api(synth_batch):
    vk, _, good = synth_batch
    items = [good[0], C.tamper(*good[1], "point")]
    vkj = nzcb.vk_to_json(vk)
    pubs = [[str(bn.from_le(u[i:i + 32])) for i in range(0, len(u), 32)] for _, u in items]
    proofs = [nzcb.proof_to_json(p) for p, _ in items]
    assert nzcb.plonk.verify_batch(vkj, pubs, proofs, device=HOST) == [True, False]


# ---------------------------------------------------------------- 3. the weights matter
def test_cancelling_errors_are_caught():
    """Without the public inputs in the transcript the challenges do not depend on them, and a
    public signal enters R linearly (through PI(xi) in the scalar of the generator). The same
    proof with signal 0 at +delta and at -delta is invalid twice, and the two errors cancel in
    an unweighted sum: only distinct weights tell."""
    c = synth.synth_circuit(5, 2, 3, seed=31)
    zk = plonk.setup(c, 777)
    proof, pub = plonk.prove(zk, c["witness"], synth.fixed_blindings(), transcript_pub=False)
    vk = nzcb.vk_from_zkey(binfmt.write_zkey(zk))
    pb = plonk.proof_to_bytes(proof)
    assert nzcb.verify(vk, pb, C.pub_bytes(pub), transcript_public=False)
    delta = 12345
    plus = C.pub_bytes([(pub[0] + delta) % bn.R_MOD] + list(pub[1:]))
    minus = C.pub_bytes([(pub[0] - delta) % bn.R_MOD] + list(pub[1:]))
    # the premise: L is the same and the two R add up to twice the valid proof's R
    sums = []
    for u in (C.pub_bytes(pub), plus, minus):
        sums.append(_unweighted(vk, pb, u))
    assert sums[1][0] == sums[2][0] == sums[0][0]
    r = [_pt(s[1]) for s in sums]
    assert bn.g1_add(r[1], r[2]) == bn.g1_add(r[0], r[0]) and r[1] != r[0]
    for kw in ({}, {"seed": SEED}):
        assert nzcb.verify_batch(vk, [pb, pb], [plus, minus], transcript_public=False, device=HOST, **kw) == \
            [False, False]
    assert nzcb.verify_batch(vk, [pb, pb, pb], [plus, C.pub_bytes(pub), minus], transcript_public=False,
                             device=HOST) == [False, True, False]


def _pt(b):
    return None if b == bytes(64) else (bn.from_le(b[:32]), bn.from_le(b[32:]))


def _unweighted(vk, proof, pub):
    """(L, R) of one item: its weighted points divided by the weight of the fixed seed."""
    _, pts, _ = nzcb.Engine.verify_batch(vk, [proof], [pub], transcript_public=False, device=HOST, seed=SEED)
    inv = bn.fr_inv(_weight(SEED, 0))
    return [C.pt_bytes(bn.g1_mul(_pt(pts[0][o:o + 64]), inv)) for o in (0, 64)]


def _weight(seed, i):
    from oracle import keccak
    h = keccak.keccak256(seed + i.to_bytes(4, "little"))
    return (int.from_bytes(h, "big") & ((1 << 128) - 1)) or 1


# ---------------------------------------------------------------- 4. pairing counts
def test_pairing_counts(synth_batch):
    vk, _, good = synth_batch
    items = [good[k % 8] for k in range(16)]
    proofs, pubs = [p for p, _ in items], [u for _, u in items]
    valid, _, checks = nzcb.Engine.verify_batch(vk, proofs, pubs, device=HOST)
    assert valid == [True] * 16 and checks == 1
    for pos in (0, 9, 15):
        bad = list(items)
        bad[pos] = C.tamper(*bad[pos], "eval")
        valid, _, checks = nzcb.Engine.verify_batch(vk, [p for p, _ in bad], [u for _, u in bad], device=HOST)
        assert valid == [k != pos for k in range(16)]
        assert 2 <= checks <= 1 + 2 * 4
    # items rejected before the sums cost no pairing check
    bad = list(items)
    bad[3] = C.tamper(*bad[3], "offcurve")
    bad[12] = C.tamper(*bad[12], "big")
    valid, pts, checks = nzcb.Engine.verify_batch(vk, [p for p, _ in bad], [u for _, u in bad], device=HOST)
    assert valid == [k not in (3, 12) for k in range(16)] and checks == 1
    assert pts[3] == pts[12] == bytes(128) and bytes(128) not in pts[:3]


# ---------------------------------------------------------------- 5. fixed seed
def test_points_reproducible_under_seed(synth_batch):
    vk, _, good = synth_batch
    proofs, pubs = [p for p, _ in good[:3]], [u for _, u in good[:3]]
    a = nzcb.Engine.verify_batch(vk, proofs, pubs, device=HOST, seed=SEED)
    b = nzcb.Engine.verify_batch(vk, proofs, pubs, device=HOST, seed=SEED)
    assert a == b and a[0] == [True] * 3
    c = nzcb.Engine.verify_batch(vk, proofs, pubs, device=HOST, seed=bytes(32))
    d = nzcb.Engine.verify_batch(vk, proofs, pubs, device=HOST)
    assert c[1] != a[1] and d[1] != a[1] and c[0] == d[0] == a[0]
    # the documented weights: item i's points are rho_i times those under weight 1
    w0, w2 = _weight(SEED, 0), _weight(SEED, 2)
    assert 0 < w0 < 1 << 128 and w0 != w2
    l2 = _pt(a[1][2][:64])
    p2 = plonk.proof_from_bytes(proofs[2])
    u = plonk.verifier_challenges(p2, [bn.from_le(pubs[2][i:i + 32]) for i in (0, 32)])["u"]
    assert l2 == bn.g1_mul(bn.g1_add(p2["Wxi"], bn.g1_mul(p2["Wxiw"], u)), w2)
