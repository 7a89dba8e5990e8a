"""The key material check on device 0 against the host path, field for field, and against the
exact-integer expectations of tests/key_check_cases.py: k_srs_points, k_srs_weights and the two
MSMs behind nzcb.ptau_check, k_fr_compare and the transforms behind nzcb.zkey_check."""
import threading

import pytest

import key_check_cases as kc
import nzcb
from oracle import bn254 as bn

pytestmark = pytest.mark.gpu

HOST = nzcb.KEY_HOST
POWERS = {3: 15, 5: 63}
SPOILERS = (kc.spoil_range, kc.spoil_y, kc.spoil_zero, kc.spoil_other_point, kc.spoil_swap, kc.spoil_tail)


def both_paths(pts, g2, tau, chunk):
    """Device 0 and the host on one case, each held against the expectations; the same finding
    and the same L || R bytes."""
    dev = kc.check_srs(nzcb, 0, pts, g2, tau, chunk)
    host = kc.check_srs(nzcb, HOST, pts, g2, tau, chunk)
    assert dev == host
    return dev[0]


@pytest.mark.parametrize("chunk", [0, 8, 16])
@pytest.mark.parametrize("power", [3, 5])
def test_clean_points(power, chunk):
    pts = kc.raw_points(kc.TAU, POWERS[power])
    for count in (1, 2, 3, 9, len(pts)):
        f = both_paths(pts[:count], kc.g2_of(kc.TAU), kc.TAU, chunk)
        assert f["status"] == "OK" and f["pairing_checks"] == (1 if count > 1 else 0)


@pytest.mark.parametrize("chunk", [2, 3, 62, 63, 64])
def test_chunk_edges(chunk):
    """Chunks of one pair, and a chunk that ends one point before, at and past the last point."""
    pts = kc.raw_points(kc.TAU, 63)
    assert both_paths(pts, kc.g2_of(kc.TAU), kc.TAU, chunk)["status"] == "OK"


@pytest.mark.parametrize("k", kc.BAD_INDICES)
@pytest.mark.parametrize("spoil", SPOILERS, ids=lambda f: f.__name__)
@pytest.mark.parametrize("power", [3, 5])
def test_one_defect(power, spoil, k):
    pts = kc.raw_points(kc.TAU, POWERS[power])
    k %= len(pts)
    if spoil is kc.spoil_swap and k == len(pts) - 1:
        k -= 1  # the last pair
    spoil(pts, k)
    f = both_paths(pts, kc.g2_of(kc.TAU), kc.TAU, 8)
    assert f["status"] != "OK"


def test_three_bad_points_of_mixed_kinds():
    pts = kc.raw_points(kc.TAU, 63)
    kc.spoil_zero(pts, 40)
    kc.spoil_y(pts, 9)
    kc.spoil_range(pts, 17)
    for chunk in (0, 8):
        f = both_paths(pts, kc.g2_of(kc.TAU), kc.TAU, chunk)
        assert (f["status"], f["index"], f["n_bad"]) == ("CURVE", 9, 3)


@pytest.mark.parametrize("g2, want", [
    (lambda: kc.g2_of(kc.TAU2), ("SEQUENCE", 1)),
    (kc.g2_outside_subgroup, ("G2", 0)),
    (kc.g2_off_twist, ("G2", 0)),
], ids=["other-tau", "outside-subgroup", "off-twist"])
def test_g2_defects(g2, want):
    tau = kc.TAU2 if want[0] == "SEQUENCE" else kc.TAU
    f = both_paths(kc.raw_points(kc.TAU, 15), g2(), tau, 8)
    assert (f["status"], f["index"]) == want


def test_many_blocks_of_points():
    """2^10 + 6 points: the point kernel runs five blocks; defects in the first and the last
    block, and a sequence broken in the last one."""
    zkey, _ = nzcb.synth_setup(power=10)
    n = kc.zkey_n(zkey)
    off = kc.ptau_offset(zkey, 0)
    pts = [zkey[off + 64 * i:off + 64 * i + 64] for i in range(n + 6)]
    g2 = zkey[kc.header_offset(zkey, "X_2"):][:128]

    def run(points, device):
        return nzcb.Engine.srs_check(b"".join(points), g2, device=device, seed=kc.SEED)

    assert run(pts, 0) == run(pts, HOST) and run(pts, 0)[0]["status"] == "OK"
    bad = list(pts)
    kc.spoil_y(bad, n + 3)
    kc.spoil_range(bad, 70)
    kc.spoil_zero(bad, 700)
    f, _ = run(bad, 0)
    assert (f["status"], f["index"], f["n_bad"]) == ("RANGE", 70, 3) and (f, bytes(128)) == run(bad, HOST)
    bad = list(pts)
    kc.spoil_other_point(bad, n + 2)
    f, lr = run(bad, 0)
    assert (f["status"], f["index"]) == ("SEQUENCE", n + 2) and (f, lr) == run(bad, HOST)
    assert kc.checks_ok(f, n + 6)


# ---------------------------------------------------------------- files
def test_ptau_check_device():
    pts = kc.raw_points(kc.TAU, 63)
    ptau = kc.make_ptau(5, pts)
    for count in (0, 1, 2, 38):
        f = nzcb.ptau_check(ptau, count=count, device=0, seed=kc.SEED)
        assert f == nzcb.ptau_check(ptau, count=count, device=HOST, seed=kc.SEED) and f["status"] == "OK"
    kc.spoil_other_point(pts, 33)
    for g2s, want in ((None, ("SEQUENCE", 33)), ([kc.g2_of(2), kc.g2_of(kc.TAU)], ("GENERATOR", 0))):
        f = nzcb.ptau_check(kc.make_ptau(5, pts, g2s), device=0, seed=kc.SEED)
        assert (f["status"], f["index"]) == want
        assert f == nzcb.ptau_check(kc.make_ptau(5, pts, g2s), device=HOST, seed=kc.SEED)
    assert nzcb.ptau_check(nzcb.ptau_synth(4, kc.TAU), device=0)["status"] == "OK"  # the library's own file, OS seed


@pytest.mark.parametrize("name", ["p5", "p8"])
def test_golden_keys_are_ok(name):
    z = kc.golden_zkey(name)
    r = nzcb.zkey_check(z, device=0, seed=kc.SEED)
    assert r["ok"] and len(r["parts"]) == 11 and kc.all_ok_except(r) == []
    assert r == nzcb.zkey_check(z, device=HOST, seed=kc.SEED)


ZKEY_MUTATIONS = kc.zkey_mutations()


@pytest.mark.parametrize("name, data, expected, extra", ZKEY_MUTATIONS, ids=[m[0] for m in ZKEY_MUTATIONS])
def test_zkey_mutation(name, data, expected, extra):
    r = nzcb.zkey_check(data, device=0, seed=kc.SEED)
    assert kc.all_ok_except(r, **expected) == []
    assert extra is None or extra(r)
    assert r == nzcb.zkey_check(data, device=HOST, seed=kc.SEED)


def test_key_made_on_the_gpu():
    """n = 2^10: the compare kernel runs 16 blocks over the 4n evaluations and the commitment
    MSMs leave their tiny-n windows."""
    zkey, _ = nzcb.synth_setup(power=10)
    n = kc.zkey_n(zkey)
    r = nzcb.zkey_check(zkey, device=0, seed=kc.SEED)
    assert r["ok"] and kc.all_ok_except(r) == [] and all(p["checked"] == 5 * n for p in r["parts"].values())
    at = 4 * n - 37  # in the last block of the 4096
    off = kc.part_offset(zkey, "S3") + 32 * (n + at)
    r = nzcb.zkey_check(kc.patch(zkey, off + 9, bytes([zkey[off + 9] ^ 0x10])), device=0, seed=kc.SEED)
    assert kc.all_ok_except(r, S3="EVALS") == []
    assert (r["parts"]["S3"]["index"], r["parts"]["S3"]["n_bad"]) == (at, 1)
    qr = bn.g1_from_lem(zkey[kc.header_offset(zkey, "Qr"):][:64])
    r = nzcb.zkey_check(kc.patch(zkey, kc.header_offset(zkey, "Qr"), bn.g1_to_lem(bn.g1_neg(qr))), device=0)
    assert kc.all_ok_except(r, Qr="COMMIT") == []


def test_check_while_a_context_proves():
    import json
    import os
    z = kc.golden_zkey("p8")
    with open(os.path.join(kc.GOLD, "p8.json")) as f:
        exp = json.load(f)["proofs"]["fixed"]
    with open(os.path.join(kc.GOLD, "p8.wtns"), "rb") as f:
        wtns = f.read()
    ctx = nzcb.ProverContext(z, device=0)
    got = {}

    def check():
        try:
            got["check"] = nzcb.zkey_check(z, device=0, seed=kc.SEED)
        except Exception as e:  # surfaced by the assertion below
            got["check"] = e

    try:
        ctx.prove_raw(wtns, bytes.fromhex(exp["blinding"]))  # warm
        t = threading.Thread(target=check)
        t.start()
        proofs = [ctx.prove_raw(wtns, bytes.fromhex(exp["blinding"]))[0] for _ in range(4)]
        t.join()
    finally:
        ctx.close()
    assert all(p.hex() == exp["proof_bin"] for p in proofs)
    assert isinstance(got["check"], dict) and got["check"]["ok"] and kc.all_ok_except(got["check"]) == []
