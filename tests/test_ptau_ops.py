"""The powers-of-tau operations on the host path (nzcb.PTAU_HOST) against the restatement of
tests/ptau_ops_cases.py: nzcb.ptau_new, ptau_contribute and ptau_prepare_phase2, whole files byte
for byte, the degenerate and composition properties, and every error the operations name."""
import os

import pytest

import nzcb
import ptau_ops_cases as pc
from oracle import bn254 as bn

HOST = nzcb.PTAU_HOST
A, B = pc.SECRETS_A, pc.SECRETS_B


@pytest.mark.parametrize("power", [1, 3])
def test_new_exact_bytes(power):
    assert nzcb.ptau_new(power) == pc.expected_file(power)


@pytest.mark.parametrize("power", [1, 2, 4])
def test_contribute_and_prepare_against_the_restatement(power):
    got = nzcb.ptau_contribute(nzcb.ptau_new(power), secrets=A, device=HOST)
    assert got == pc.expected_file(power, A)
    assert nzcb.ptau_prepare_phase2(got, device=HOST) == pc.expected_file(power, A, prepared=True)


def test_prepare_of_new_is_degenerate():
    """tau = 1, all points equal: every level is its source's P_0 followed by points at infinity,
    which needs complete additions (P + P, P - P) and infinity stored as zero bytes. Section 12's
    top level has a source padded with infinity and comes from the definition."""
    power = 3
    new = nzcb.ptau_new(power)
    got = nzcb.ptau_prepare_phase2(new, device=HOST)
    for src, lag in ((2, 12), (3, 13), (4, 14), (5, 15)):
        p0, w = pc.points(new, src)[0], pc.point_bytes(src)
        for p in range(power + 1):
            assert pc.level(got, lag, p) == [p0] + [bytes(w)] * ((1 << p) - 1), (lag, p)
    assert got == pc.expected_file(power, pc.ONE, prepared=True)
    top = pc.level(got, 12, power + 1)
    assert len(top) == 2 << power and bytes(64) not in top


def test_contributions_compose():
    new = nzcb.ptau_new(3)
    twice = nzcb.ptau_contribute(nzcb.ptau_contribute(new, secrets=A, device=HOST), secrets=B, device=HOST)
    assert twice == nzcb.ptau_contribute(new, secrets=pc.compose(A, B), device=HOST)
    assert twice == pc.expected_file(3, pc.compose(A, B))


def test_drawn_secrets_differ_and_entropy_is_accepted():
    new = nzcb.ptau_new(1)
    a = nzcb.ptau_contribute(new, device=HOST)
    b = nzcb.ptau_contribute(new, entropy="some text", device=HOST)
    assert len({a, b, new}) == 3 and len(a) == len(b) == len(new)
    assert nzcb.ptau_check(a, device=nzcb.KEY_HOST)["status"] == "OK"


def test_stale_and_unknown_sections_are_dropped():
    prepared = pc.expected_file(2, A, prepared=True)
    assert nzcb.ptau_contribute(prepared, secrets=B, device=HOST) == pc.expected_file(2, pc.compose(A, B))


@pytest.mark.parametrize("secrets", [(0, 1, 1), (1, pc.R, 1), (1, 1, pc.R + 1), (1, 1, (1 << 256) - 1)])
def test_bad_secret(secrets):
    with pytest.raises(nzcb.NzcbError) as e:
        nzcb.ptau_contribute(nzcb.ptau_new(1), secrets=secrets, device=HOST)
    assert e.value.name == "ARG"


@pytest.mark.parametrize("power", [0, 25, -1])
def test_power_out_of_range(power):
    with pytest.raises(nzcb.NzcbError) as e:
        nzcb.ptau_new(power)
    assert e.value.name == "ARG"
    if power >= 0:
        bad = pc.patch_point(nzcb.ptau_new(1), 1, 0, pc.header(power))
        for op in (lambda d: nzcb.ptau_contribute(d, secrets=A, device=HOST),
                   lambda d: nzcb.ptau_prepare_phase2(d, device=HOST)):
            with pytest.raises(nzcb.NzcbError) as e:
                op(bad)
            assert e.value.name == "ARG"


@pytest.mark.parametrize("kind", ["range", "curve", "zero"])
@pytest.mark.parametrize("sid, index", [(2, 0), (2, 14), (3, 5), (4, 7), (5, 1), (6, 0)])
def test_spoiled_point_is_named(sid, index, kind):
    good = pc.expected_file(3, A)
    with pytest.raises(nzcb.NzcbError) as e:
        nzcb.ptau_contribute(pc.spoiled(good, sid, index, kind), secrets=B, device=HOST)
    assert e.value.name == "FORMAT"
    assert f"section {sid} point {index} " in str(e.value)


def test_lowest_section_and_index_win():
    bad = pc.expected_file(3, A)
    for sid, index, kind in ((5, 0, "zero"), (3, 6, "curve"), (3, 2, "range"), (3, 4, "zero")):
        bad = pc.spoiled(bad, sid, index, kind)
    with pytest.raises(nzcb.NzcbError) as e:
        nzcb.ptau_contribute(bad, secrets=B, device=HOST)
    assert "section 3 point 2 " in str(e.value) and "(3 defective" in str(e.value)


@pytest.mark.parametrize("sid", range(1, 8))
def test_missing_or_short_section(sid):
    good = pc.expected_file(2, A)
    for bad in (pc.without_section(good, sid), pc.with_short_section(good, sid), good[:-1], good[:11], b""):
        for op in (lambda d: nzcb.ptau_contribute(d, secrets=B, device=HOST),
                   lambda d: nzcb.ptau_prepare_phase2(d, device=HOST)):
            with pytest.raises(nzcb.NzcbError) as e:
                op(bad)
            assert e.value.name == "FORMAT"


def test_existing_check_accepts_the_contributed_file():
    power = 4
    got = nzcb.ptau_contribute(nzcb.ptau_new(power), secrets=A, device=HOST)
    assert nzcb.ptau_check(got, device=nzcb.KEY_HOST)["status"] == "OK"
    assert pc.points(got, 2)[:4] == [pc.gen_mul(False, pow(A[0], i, pc.R)) for i in range(4)]
    assert pc.points(got, 3)[:2] == [bn.g2_to_lem(bn.G2_GEN), bn.g2_to_lem(bn.g2_mul(bn.G2_GEN, A[0]))]


def test_file_forms(tmp_path):
    p0, p1, p2 = (str(tmp_path / f"pot_{k}.ptau") for k in range(3))
    assert nzcb.ptau_new(2, p0) == p0
    assert nzcb.ptau_contribute(p0, p1, secrets=A, device=HOST) == p1
    assert nzcb.ptau_prepare_phase2(p1, p2, device=HOST) == p2
    with open(p2, "rb") as f:
        assert f.read() == pc.expected_file(2, A, prepared=True)
    assert nzcb.ptau_prepare_phase2(p1, device=HOST) == pc.expected_file(2, A, prepared=True)
    with pytest.raises(nzcb.NzcbError) as e:
        nzcb.ptau_contribute(p1, p1, secrets=A, device=HOST)
    assert e.value.name == "ARG"
    bad = str(tmp_path / "bad.ptau")
    with open(bad, "wb") as f:
        f.write(pc.spoiled(pc.expected_file(2, A), 4, 1, "curve"))
    with pytest.raises(nzcb.NzcbError):
        nzcb.ptau_contribute(bad, str(tmp_path / "never.ptau"), secrets=B, device=HOST)
    assert not os.path.exists(tmp_path / "never.ptau")  # a failed operation leaves no partial file
