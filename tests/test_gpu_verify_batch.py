"""Batch PLONK verification on the GPU (csrc/verify_batch.hip): the G1 group kernels byte for
byte against the host path (which tests/test_verify_batch.py pins to the oracle) on edge cases
and on shapes across the wavefront and workgroup boundaries, the per-item points and the
verdicts of nzcb_verify_batch on device 0, and the Node.js binding. The proofs come from the
GPU prover on the golden n = 2^5 and n = 2^8 keys under distinct fixed blindings."""
import hashlib
import json
import os
import shutil
import subprocess

import pytest

import nzcb
import verify_batch_cases as C
from oracle import bn254 as bn

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
HOST = nzcb.VERIFY_HOST
SEED = bytes(range(32, 64))


def _blinding(tag: str, k: int) -> bytes:
    out = b""
    for j in range(11):
        h = hashlib.sha256(f"verify-batch {tag} {k} {j}".encode()).digest()
        out += bn.to_le(int.from_bytes(h, "big") % bn.R_MOD)
    return out


def _proofs(name: str, count: int):
    zkey = open(os.path.join(GOLD, f"{name}.zkey"), "rb").read()
    wtns = open(os.path.join(GOLD, f"{name}.wtns"), "rb").read()
    ctx = nzcb.ProverContext(zkey, device=0)
    try:
        items = [ctx.prove_raw(wtns, _blinding(name, k)) for k in range(count)]
    finally:
        ctx.close()
    assert len({p for p, _ in items}) == count
    return nzcb.vk_from_zkey(zkey), items


@pytest.fixture(scope="module")
def p5():
    return _proofs("p5", 67)


@pytest.fixture(scope="module")
def p8():
    return _proofs("p8", 8)


def _split(items):
    return [p for p, _ in items], [u for _, u in items]


# ---------------------------------------------------------------- 6, 7. group kernels
def test_lincomb_edge_cases_equal_host():
    packed = C.pack(C.edge_groups())
    got = nzcb.Engine.g1_lincomb(*packed, device=0)
    assert got == nzcb.Engine.g1_lincomb(*packed, device=HOST)
    assert got[-1] == bytes(64)
    assert nzcb.Engine.g1_lincomb(b"", b"", [], device=0) == []
    assert nzcb.Engine.g1_lincomb(b"", b"", [0, 0], device=0) == [bytes(64)] * 2


@pytest.mark.parametrize("n_terms", [1, 63, 64, 65, 257, 1340])
def test_lincomb_shapes_equal_host(n_terms):
    sizes = [1, 2, 18, 300] + [1, 2, 18] * 500            # one group of 300 where there is room
    groups = C.random_groups(n_terms, sizes, seed=1000 + n_terms)
    if n_terms == 1340:
        assert 300 in [len(g) for g in groups] and len(groups) > 128
    packed = C.pack(groups)
    assert nzcb.Engine.g1_lincomb(*packed, device=0) == nzcb.Engine.g1_lincomb(*packed, device=HOST)


# ---------------------------------------------------------------- 8. per-item points
@pytest.mark.parametrize("count", [1, 3, 4, 13, 67])
def test_points_equal_host(p5, count):
    vk, good = p5
    items = list(good[:count])
    if count >= 13:
        items[5] = C.tamper(*items[5], "offcurve")
        items[count - 1] = C.tamper(*items[count - 1], "eval")
    proofs, pubs = _split(items)
    dev = nzcb.Engine.verify_batch(vk, proofs, pubs, device=0, seed=SEED)
    host = nzcb.Engine.verify_batch(vk, proofs, pubs, device=HOST, seed=SEED)
    assert dev == host
    bad = {5, count - 1} if count >= 13 else set()
    assert dev[0] == [k not in bad for k in range(count)]
    assert [k for k in range(count) if dev[1][k] == bytes(128)] == ([5] if count >= 13 else [])


# ---------------------------------------------------------------- 9. verdicts on the device
def test_verdicts_on_device(p5):
    vk, good = p5
    items = list(good[:64])
    for pos, kind in ((0, "eval"), (63, "point"), (31, "pub"), (40, "eval"), (41, "point")):
        items[pos] = C.tamper(*items[pos], kind)
    items[17] = C.tamper(*items[17], "offcurve")
    items[50] = C.tamper(*items[50], "big")
    bad = {0, 17, 31, 40, 41, 50, 63}
    want = [k not in bad for k in range(64)]
    for k in sorted(bad) + [1, 62]:
        assert nzcb.verify(vk, *items[k]) == want[k]
    assert nzcb.verify_batch(vk, *_split(items), device=0) == want


def test_small_batches_on_device(p8):
    vk, good = p8
    assert nzcb.verify_batch(vk, [], [], device=0) == []
    assert nzcb.verify_batch(vk, *_split(good[:1]), device=0) == [True]
    assert nzcb.verify_batch(vk, *_split([C.tamper(*good[0], "pub")]), device=0) == [False]
    proofs, pubs = _split(good)
    assert nzcb.verify_batch(vk, proofs, [u + bytes(32) for u in pubs], device=0) == [False] * 8
    items = list(good)
    items[3] = C.tamper(*items[3], "point")
    assert nzcb.verify_batch(vk, *_split(items), device=0) == [nzcb.verify(vk, *it) for it in items]


def test_cancelling_errors_on_device(p5):
    """The same proof with public signal 0 at +delta and -delta, transcript without the public
    inputs (tests/test_verify_batch.py test_cancelling_errors_are_caught): the prover makes the
    proof under that transcript, the two errors cancel in an unweighted sum."""
    zkey = open(os.path.join(GOLD, "p5.zkey"), "rb").read()
    wtns = open(os.path.join(GOLD, "p5.wtns"), "rb").read()
    ctx = nzcb.ProverContext(zkey, device=0, transcript_public=False)
    try:
        proof, pub = ctx.prove_raw(wtns, _blinding("p5-nopub", 0))
    finally:
        ctx.close()
    vk = p5[0]
    assert nzcb.verify(vk, proof, pub, transcript_public=False)
    s0 = bn.from_le(pub[:32])
    plus, minus = (bn.to_le((s0 + d) % bn.R_MOD) + pub[32:] for d in (777, -777))
    assert nzcb.verify_batch(vk, [proof] * 4, [plus, pub, minus, pub], transcript_public=False, device=0) == \
        [False, True, False, True]


def test_pairing_counts_on_device(p5):
    vk, good = p5
    proofs, pubs = _split(good[:64])
    valid, _, checks = nzcb.Engine.verify_batch(vk, proofs, pubs, device=0)
    assert valid == [True] * 64 and checks == 1
    for pos in (0, 37):
        items = list(good[:64])
        items[pos] = C.tamper(*items[pos], "eval")
        valid, _, checks = nzcb.Engine.verify_batch(vk, *_split(items), device=0)
        assert valid == [k != pos for k in range(64)]
        assert 2 <= checks <= 13                                   # 1 + 2 * ceil(log2 64)
    items = list(good[:64])
    items[9] = C.tamper(*items[9], "offcurve")
    valid, _, checks = nzcb.Engine.verify_batch(vk, *_split(items), device=0)
    assert valid == [k != 9 for k in range(64)] and checks == 1


def test_verify_while_a_context_proves(p5):
    """A call has its own stream and buffers: verdicts and points are the same while a prover
    context works on the same device from another thread, and the proofs made meanwhile verify."""
    import threading
    vk, good = p5
    items = list(good[:13])
    items[4] = C.tamper(*items[4], "eval")
    proofs, pubs = _split(items)
    want = nzcb.Engine.verify_batch(vk, proofs, pubs, device=0, seed=SEED)
    zkey = open(os.path.join(GOLD, "p5.zkey"), "rb").read()
    wtns = open(os.path.join(GOLD, "p5.wtns"), "rb").read()
    ctx = nzcb.ProverContext(zkey, device=0)
    made, errors = [], []

    def prove():
        try:
            for k in range(12):
                made.append(ctx.prove_raw(wtns, _blinding("p5-meanwhile", k)))
        except Exception as e:  # noqa: BLE001 (reported by the assertion below)
            errors.append(e)

    t = threading.Thread(target=prove)
    t.start()
    try:
        got = [nzcb.Engine.verify_batch(vk, proofs, pubs, device=0, seed=SEED) for _ in range(3)]
    finally:
        t.join()
        ctx.close()
    assert errors == [] and len(made) == 12
    assert got == [want] * 3 and want[0] == [k != 4 for k in range(13)]
    assert nzcb.verify_batch(vk, *_split(made), device=0) == [True] * 12


# ---------------------------------------------------------------- 10. Node
@pytest.mark.skipif(shutil.which("node") is None or
                    not os.path.exists(os.path.join(ROOT, "nzcb-circom_amd", "js", "build", "nzcb.node")),
                    reason="node or the built addon is unavailable")
def test_node_verify_batch(p8):
    vk, good = p8
    proofs = [nzcb.proof_to_json(p) for p, _ in good]
    pubs = [nzcb.public_to_json(u, len(u) // 32) for _, u in good]
    proofs[5] = dict(proofs[5], eval_b=str((int(proofs[5]["eval_b"]) + 1) % bn.R_MOD))
    script = f"""
const m = require('./');
(async () => {{
  const vk = {json.dumps(nzcb.vk_to_json(vk))};
  const ok = await m.plonk.verifyBatch(vk, {json.dumps(pubs)}, {json.dumps(proofs)}, null, {{device: 0}});
  console.log(JSON.stringify(ok));
}})().catch((err) => {{ console.error(err); process.exit(1); }});
"""
    p = subprocess.run(["node", "-e", script], capture_output=True, text=True, timeout=120,
                       cwd=os.path.join(ROOT, "nzcb-circom_amd", "js"))
    assert p.returncode == 0, p.stderr
    assert json.loads(p.stdout) == [k != 5 for k in range(8)]
