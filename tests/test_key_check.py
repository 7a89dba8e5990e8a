"""The key material check on the host path (nzcb.KEY_HOST) against exact-integer expectations
(tests/key_check_cases.py): the SRS check behind nzcb.ptau_check and nzcb.zkey_check, the
files' readers, and every rule of the zkey check on the golden keys."""
import pytest

import key_check_cases as kc
import nzcb
from oracle import bn254 as bn

HOST = nzcb.KEY_HOST
POWERS = {3: 15, 5: 63}
SPOILERS = (kc.spoil_range, kc.spoil_y, kc.spoil_zero, kc.spoil_other_point, kc.spoil_swap, kc.spoil_tail)


def points_of(power: int) -> list:
    return kc.raw_points(kc.TAU, POWERS[power])


# ---------------------------------------------------------------- the SRS check
@pytest.mark.parametrize("chunk", [0, 8, 16])
@pytest.mark.parametrize("power", [3, 5])
def test_clean_points(power, chunk):
    pts = points_of(power)
    for count in (1, 2, 3, 9, len(pts)):
        finding, _ = kc.check_srs(nzcb, HOST, pts[:count], kc.g2_of(kc.TAU), kc.TAU, chunk)
        assert finding["status"] == "OK" and finding["pairing_checks"] == (1 if count > 1 else 0)


@pytest.mark.parametrize("k", kc.BAD_INDICES)
@pytest.mark.parametrize("spoil", SPOILERS, ids=lambda f: f.__name__)
@pytest.mark.parametrize("power", [3, 5])
def test_one_defect(power, spoil, k):
    pts = points_of(power)
    k %= len(pts)
    if spoil is kc.spoil_swap and k == len(pts) - 1:
        k -= 1  # the last pair
    spoil(pts, k)
    finding, _ = kc.check_srs(nzcb, HOST, pts, kc.g2_of(kc.TAU), kc.TAU, 8)
    want = {kc.spoil_range: "RANGE", kc.spoil_y: "CURVE", kc.spoil_zero: "CURVE"}.get(spoil, "SEQUENCE")
    if want == "SEQUENCE" and k == 0:
        want = "SEQUENCE" if spoil is kc.spoil_tail else "GENERATOR"
    assert finding["status"] == want
    assert finding["index"] == (0 if want == "GENERATOR" else max(k, 1) if want == "SEQUENCE" else k)


def test_three_bad_points_of_mixed_kinds():
    pts = points_of(5)
    kc.spoil_zero(pts, 40)
    kc.spoil_y(pts, 9)
    kc.spoil_range(pts, 17)
    finding, _ = kc.check_srs(nzcb, HOST, pts, kc.g2_of(kc.TAU), kc.TAU, 8)
    assert (finding["status"], finding["index"], finding["n_bad"]) == ("CURVE", 9, 3)
    kc.spoil_range(pts, 2)
    finding, _ = kc.check_srs(nzcb, HOST, pts, kc.g2_of(kc.TAU), kc.TAU, 16)
    assert (finding["status"], finding["index"], finding["n_bad"]) == ("RANGE", 2, 4)


@pytest.mark.parametrize("g2, want", [
    (lambda: kc.g2_of(kc.TAU2), ("SEQUENCE", 1)),
    (kc.g2_outside_subgroup, ("G2", 0)),
    (kc.g2_off_twist, ("G2", 0)),
    (lambda: bytes(128), ("G2", 0)),
    (lambda: bn.to_le(kc.P) + kc.g2_of(kc.TAU)[32:], ("G2", 0)),
], ids=["other-tau", "outside-subgroup", "off-twist", "infinity", "x-is-q"])
def test_g2_defects(g2, want):
    tau = kc.TAU2 if want[0] == "SEQUENCE" else kc.TAU
    finding, _ = kc.check_srs(nzcb, HOST, points_of(3), g2(), tau, 8)
    assert (finding["status"], finding["index"]) == want


def test_weights_are_the_batch_verifiers_rule():
    """rho_i = low 128 bits of keccak256(seed || LE32(i)): with two points L = rho_0 G."""
    pts = points_of(3)[:2]
    _, lr = nzcb.Engine.srs_check(b"".join(pts), kc.g2_of(kc.TAU), device=HOST, seed=kc.SEED)
    want = bn.g1_mul(bn.G1_GEN, kc.weight(kc.SEED, 0))
    assert lr[:64] == bn.to_le(want[0]) + bn.to_le(want[1])


def test_own_seed_and_bad_arguments():
    pts = points_of(3)
    finding, _ = nzcb.Engine.srs_check(b"".join(pts), kc.g2_of(kc.TAU), device=HOST)  # OS seed
    assert finding["status"] == "OK"
    with pytest.raises(nzcb.NzcbError) as e:
        nzcb.Engine.srs_check(b"".join(pts), kc.g2_of(kc.TAU), device=HOST, chunk_points=1)
    assert e.value.code == 1
    with pytest.raises(nzcb.NzcbError) as e:
        nzcb.Engine.srs_check(b"", kc.g2_of(kc.TAU), device=HOST)
    assert e.value.code == 1


# ---------------------------------------------------------------- ptau files
@pytest.mark.parametrize("power", [3, 5])
def test_ptau_check_counts(power, tmp_path):
    pts = points_of(power)
    ptau = kc.make_ptau(power, pts)
    for count in (0, 1, 2, 3, 9, len(pts)):
        f = nzcb.ptau_check(ptau, count=count, device=HOST, seed=kc.SEED)
        assert kc.strip(f) == {"status": "OK", "index": 0, "n_bad": 0, "checked": count or len(pts)}
    path = tmp_path / "t.ptau"
    path.write_bytes(ptau)
    assert nzcb.ptau_check(str(path), device=HOST, seed=kc.SEED) == nzcb.ptau_check(ptau, device=HOST, seed=kc.SEED)


def test_ptau_check_matches_the_setup_reader():
    """The file oracle.r1cs.write_ptau makes for `plonk setup` passes."""
    from oracle import r1cs
    assert nzcb.ptau_check(r1cs.write_ptau(kc.TAU, 3), device=HOST)["status"] == "OK"


def test_ptau_check_defects():
    pts = points_of(3)
    kc.spoil_other_point(pts, 9)
    f = nzcb.ptau_check(kc.make_ptau(3, pts), device=HOST, seed=kc.SEED)
    assert (f["status"], f["index"]) == ("SEQUENCE", 9)
    assert nzcb.ptau_check(kc.make_ptau(3, pts), count=9, device=HOST, seed=kc.SEED)["status"] == "OK"
    good = points_of(3)
    f = nzcb.ptau_check(kc.make_ptau(3, good, [kc.g2_of(2), kc.g2_of(kc.TAU)]), device=HOST, seed=kc.SEED)
    assert (f["status"], f["index"]) == ("GENERATOR", 0)
    f = nzcb.ptau_check(kc.make_ptau(3, good, [kc.G2_ONE, kc.g2_of(kc.TAU2)]), device=HOST, seed=kc.SEED)
    assert (f["status"], f["index"]) == ("SEQUENCE", 1)
    f = nzcb.ptau_check(kc.make_ptau(3, good, [kc.G2_ONE, kc.g2_outside_subgroup()]), device=HOST, seed=kc.SEED)
    assert f["status"] == "G2"


def test_ptau_format_and_argument_errors():
    pts = points_of(3)
    ptau = kc.make_ptau(3, pts)

    def code(data, **kw):
        with pytest.raises(nzcb.NzcbError) as e:
            nzcb.ptau_check(data, device=HOST, seed=kc.SEED, **kw)
        return e.value.code

    off, size = kc.section_span(ptau, b"ptau", 2)
    assert code(ptau[:off + size - 1]) == 2                         # section 2 cut short
    assert code(kc.make_ptau(3, pts[:-1])) == 2                     # fewer points than the header's power
    assert code(kc.make_ptau(3, pts, sections=(1, 2))) == 2         # no section 3
    assert code(kc.make_ptau(3, pts, [kc.G2_ONE])) == 2             # no [tau]G2
    assert code(ptau, count=16) == 1                                # count past the section
    assert code(b"zkey" + ptau[4:]) == 2
    assert nzcb.ptau_check(kc.make_ptau(3, pts[:-1]), count=14, device=HOST, seed=kc.SEED)["status"] == "OK"
    for cut in kc.section_edges(ptau, b"ptau"):
        for at in (cut - 1, cut + 1):
            if 0 <= at < len(ptau):
                assert code(ptau[:at]) == 2


# ---------------------------------------------------------------- zkey files
@pytest.mark.parametrize("name", ["p5", "p8"])
def test_golden_keys_are_ok(name):
    r = nzcb.zkey_check(kc.golden_zkey(name), device=HOST, seed=kc.SEED)
    assert r["ok"] and len(r["parts"]) == 11 and kc.all_ok_except(r) == []
    n = kc.zkey_n(kc.golden_zkey(name))
    assert r["srs"]["checked"] == n + 6 and r["srs"]["pairing_checks"] == 1
    assert all(p["checked"] == 5 * n for p in r["parts"].values())
    assert [p["commit_checked"] for p in r["parts"].values()] == [True] * 8 + [False] * 3


ZKEY_MUTATIONS = kc.zkey_mutations()


@pytest.mark.parametrize("name, data, expected, extra", ZKEY_MUTATIONS, ids=[m[0] for m in ZKEY_MUTATIONS])
def test_zkey_mutation(name, data, expected, extra):
    r = nzcb.zkey_check(data, device=HOST, seed=kc.SEED)
    assert kc.all_ok_except(r, **expected) == []
    assert extra is None or extra(r)


def test_zkey_check_file_and_short_parts(tmp_path):
    import ctypes
    z = kc.golden_zkey("p5")
    path = tmp_path / "k.zkey"
    path.write_bytes(z)
    assert nzcb.zkey_check(str(path), device=HOST, seed=kc.SEED) == nzcb.zkey_check(z, device=HOST, seed=kc.SEED)
    lib = nzcb.load()
    ok, n_parts, err = ctypes.c_int(0), ctypes.c_uint32(0), nzcb._Err()
    hdr, parts = (nzcb.KeyFinding * 2)(), (nzcb.KeyFinding * 3)()
    parts[2].status = 77  # past parts_cap = 2: left alone
    rc = lib.nzcb_zkey_check(ctypes.cast(ctypes.c_char_p(z), ctypes.c_void_p), len(z), HOST, None, ctypes.byref(ok),
                             hdr, parts, 2, ctypes.byref(n_parts), ctypes.byref(err))
    assert (rc, ok.value, n_parts.value, parts[2].status) == (0, 1, 11, 77)
    with pytest.raises(nzcb.NzcbError) as e:
        nzcb.zkey_check(z[:len(z) // 2], device=HOST)
    assert e.value.code == 2
