"""Groth16 key generation on device 0: the kernels of csrc/groth16.hip (point test, chunk sums,
folds, store, scale over G1 and G2) against the restatement of tests/groth16_cases.py and
against the host path byte for byte. The checks themselves are in tests/groth16_checks.py, shared
with the host path's tests."""
import os

import pytest

import groth16_cases as gc
import groth16_checks as ck
import nzcb

pytestmark = pytest.mark.gpu

HOST = nzcb.GROTH16_HOST
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


@pytest.mark.parametrize("seed, power", [(21, 7), (22, 7), (21, 6)])
def test_random_circuit_equals_the_restatement(seed, power):
    """power 6 = cirPower: T is the level built from 2n - 1 points and the point at infinity."""
    ck.check_random_circuit(0, seed, power)


def test_edge_circuit_equals_the_restatement():
    ck.check_edge_circuit(0)


@pytest.mark.parametrize("chunk, fan_in", [(4, 2), (5, 3), (64, 64), (0, 0)])
def test_schedule_does_not_change_the_bytes(chunk, fan_in):
    """Rows of 1 to about 230 chunks, one fold level up to eight, chunk edges at every offset."""
    ck.check_schedule(0, chunk, fan_in)


@pytest.mark.parametrize("g2", [False, True])
def test_rows_alone(g2):
    ck.check_rows(0, g2)


def test_degenerate_file():
    ck.check_degenerate_file(0)


def test_device_bytes_equal_host_bytes():
    r1cs = gc.edge_circuit(300)
    ptau = ck.prepared(9, 0)
    dev = nzcb.groth16_setup(r1cs, ptau, device=0)
    t = nzcb.groth16_timings()
    assert t["kernels_ms"] > 0 and t["rows_g1_ms"] > 0 and t["rows_g2_ms"] > 0
    assert dev == nzcb.groth16_setup(r1cs, ptau, device=HOST)
    assert nzcb.groth16_contribute(dev, secret=gc.D1, device=0) == nzcb.groth16_contribute(dev, secret=gc.D1,
                                                                                         device=HOST)
    assert nzcb.groth16_timings()["kernels_ms"] == 0


def test_contribute():
    ck.check_contribute(0)


@pytest.mark.parametrize("kind", ["range", "curve", "zero"])
def test_contribute_names_a_spoiled_point(kind):
    ck.check_contribute_names_a_spoiled_point(0, kind)


def test_pairing_equation_after_a_drawn_contribution():
    ck.check_pairing_equation(0)


def test_errors():
    with open(os.path.join(GOLD, "p5.zkey"), "rb") as f:
        zkey = f.read()
    ck.check_errors(0, zkey)
    with pytest.raises(nzcb.NzcbError) as e:
        nzcb.ProverContext(gc.expected_zkey(gc.random_circuit(21)[0], 7, ck.A), device=0)
    assert str(e.value) == "zkey file is not plonk"


def test_file_forms(tmp_path):
    ck.check_file_forms(0, tmp_path)
