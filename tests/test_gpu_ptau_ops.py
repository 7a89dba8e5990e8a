"""The powers-of-tau operations on device 0: the kernels of csrc/ptau_ops.hip (point test, scale,
the elliptic-curve inverse transform over G1 and over G2) against the restatement of
tests/ptau_ops_cases.py, against the host path byte for byte, against the group law in Python,
and against two independent kernels of the library (csrc/lagrange.hip, csrc/synth.hip)."""
import functools

import pytest

import nzcb
import ptau_ops_cases as pc
from oracle import binfmt, r1cs, synth

pytestmark = pytest.mark.gpu

HOST = nzcb.PTAU_HOST
A, B = pc.SECRETS_A, pc.SECRETS_B


@pytest.mark.parametrize("power", [1, 2, 4, 5])
def test_contribute_and_prepare_against_the_restatement(power):
    got = nzcb.ptau_contribute(nzcb.ptau_new(power), secrets=A, device=0)
    assert got == pc.expected_file(power, A)
    assert nzcb.ptau_prepare_phase2(got, device=0) == pc.expected_file(power, A, prepared=True)


@functools.lru_cache(maxsize=None)
def prepared_9() -> bytes:
    """Power 9 through both operations on the device: 512 G2 points (two blocks of lanes) and
    stages on both sides of the 64-group ordering switch."""
    return nzcb.ptau_prepare_phase2(nzcb.ptau_contribute(nzcb.ptau_new(9), secrets=A, device=0), device=0)


def test_device_bytes_equal_host_bytes_at_power_9():
    new = nzcb.ptau_new(9)
    host = nzcb.ptau_contribute(new, secrets=A, device=HOST)
    dev = nzcb.ptau_contribute(new, secrets=A, device=0)
    assert pc.sections(dev) == pc.sections(host)
    assert pc.sections(prepared_9()) == pc.sections(nzcb.ptau_prepare_phase2(host, device=HOST))


@pytest.mark.parametrize("batch_top", [0, 3, 7, 25])
def test_levels_alone_and_side_by_side_give_the_same_bytes(batch_top):
    """The levels up to batch_top share their launches, each larger one runs alone (as every level
    above 16 does by default): level ranges that begin at 0, below a wave and on a wave."""
    cont = nzcb.ptau_contribute(nzcb.ptau_new(9), secrets=A, device=0)
    prev = nzcb.ptau_batch_top(batch_top)
    try:
        got = nzcb.ptau_prepare_phase2(cont, device=0)
    finally:
        nzcb.ptau_batch_top(prev)
    assert got == prepared_9()


@pytest.mark.parametrize("src, lag", [(2, 12), (3, 13), (4, 14), (5, 15)])
def test_every_level_sums_to_its_first_point(src, lag):
    """sum_k out_p[k] = sum_i P_i (1/n) sum_k w^(-ik) = P_0, with Python's point additions."""
    data = prepared_9()
    p0, g2 = pc.points(data, src)[0], src == 3
    for p in range(9 + (2 if lag == 12 else 1)):
        assert pc.point_sum(pc.level(data, lag, p), g2) == p0, p


def test_section_12_equals_the_prover_lagrange_kernel():
    """Every level p >= 1 of section 12 at power 12 against Engine.lagrange_basis (csrc/lagrange.hip)
    over the same points; the top level reads the 2^13 - 1 points padded with infinity."""
    power = 12
    cont = nzcb.ptau_contribute(nzcb.ptau_new(power), secrets=A, device=0)
    got = nzcb.ptau_prepare_phase2(cont, device=0)
    n_top = 2 << power
    src = pc.sections(cont)[2] + bytes(64 * 3)  # 2^13 - 1 points, then infinity up to n + 2
    eng = nzcb.Engine(0, max_log_ntt=-1, max_msm_points=0)
    dp, do = nzcb.dev_alloc(len(src)), nzcb.dev_alloc(64 * (n_top + 2))
    try:
        nzcb.h2d(dp, src)
        for p in range(1, power + 2):
            n = 1 << p
            eng.lagrange_basis(dp, n_top + 2, p, do)
            assert b"".join(pc.level(got, 12, p)) == nzcb.d2h(do, 64 * n), p
    finally:
        nzcb.dev_free(dp)
        nzcb.dev_free(do)
        eng.close()
    # and the scale kernel against the fixed-base kernel of csrc/synth.hip
    tau_only = nzcb.ptau_contribute(nzcb.ptau_new(power), secrets=(A[0], 1, 1), device=0)
    synth_file = nzcb.ptau_synth(power, A[0])
    assert pc.sections(tau_only)[2] == pc.sections(synth_file)[2]
    assert pc.sections(tau_only)[3][:256] == pc.sections(synth_file)[3]


def test_contributions_compose_at_power_10():
    new = nzcb.ptau_new(10)
    twice = nzcb.ptau_contribute(nzcb.ptau_contribute(new, secrets=A, device=0), secrets=B, device=0)
    assert twice == nzcb.ptau_contribute(new, secrets=pc.compose(A, B), device=0)


def test_prepare_of_new_is_degenerate_on_the_device():
    power = 6
    new = nzcb.ptau_new(power)
    got = nzcb.ptau_prepare_phase2(new, device=0)
    for src, lag in ((2, 12), (3, 13), (4, 14), (5, 15)):
        p0, w = pc.points(new, src)[0], pc.point_bytes(src)
        for p in range(power + 1):
            assert pc.level(got, lag, p) == [p0] + [bytes(w)] * ((1 << p) - 1), (lag, p)
    top = pc.level(got, 12, power + 1)
    assert bytes(64) not in top and pc.point_sum(top, False) == pc.points(new, 2)[0]
    assert got == nzcb.ptau_prepare_phase2(new, device=HOST)


@pytest.mark.parametrize("sid, index, kind", [(2, 510, "curve"), (3, 255, "range"), (4, 0, "zero"), (5, 77, "curve"),
                                              (6, 0, "curve")])
def test_spoiled_point_is_named(sid, index, kind):
    good = nzcb.ptau_contribute(nzcb.ptau_new(8), secrets=A, device=0)
    bad = pc.spoiled(good, sid, index, kind)
    if (sid, index) < (5, 200):
        bad = pc.spoiled(bad, 5, 200, "zero")  # a later defect does not take the name
    with pytest.raises(nzcb.NzcbError) as e:
        nzcb.ptau_contribute(bad, secrets=B, device=0)
    assert e.value.name == "FORMAT" and f"section {sid} point {index} " in str(e.value)


def test_end_to_end_at_power_8(tmp_path):
    """new, two contributions (the second with drawn secrets, through files), the existing check,
    prepare, a PLONK setup with the result, the key check, a proof and its verification."""
    p0, p1, p2, p3 = (str(tmp_path / f"pot8_{k}.ptau") for k in range(4))
    nzcb.ptau_new(8, p0)
    nzcb.ptau_contribute(p0, p1, secrets=A, device=0)
    nzcb.ptau_contribute(p1, p2, entropy="second contribution", device=0)
    assert nzcb.ptau_check(p2)["status"] == "OK"
    nzcb.ptau_prepare_phase2(p2, p3, device=0)
    with open(p3, "rb") as f:
        final = f.read()
    assert sorted(pc.sections(final)) == [1, 2, 3, 4, 5, 6, 7, 12, 13, 14, 15]
    assert nzcb.ptau_check(final)["status"] == "OK"
    data, w = r1cs.random_r1cs(21, n_out=3, n_pub_in=2, n_prv_in=4, n_steps=40)
    zkey = nzcb.plonk_setup(data, final)
    assert nzcb.zkey_check(zkey)["ok"]
    bl = b"".join(x.to_bytes(32, "little") for x in synth.fixed_blindings())
    ctx = nzcb.ProverContext(zkey)
    try:
        proof, pub = ctx.prove_raw(binfmt.write_wtns(w), bl)
        assert nzcb.verify(ctx.vk, proof, pub)
    finally:
        ctx.close()
