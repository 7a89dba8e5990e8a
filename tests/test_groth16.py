"""Groth16 key generation on the host path (nzcb.GROTH16_HOST) against the restatement of
tests/groth16_cases.py: nzcb.groth16_setup and groth16_contribute whole files byte for byte, the
edge circuit, the schedule knob, the kernel family's host form on bare arrays, the degenerate
powers-of-tau file, the pairing equation with a Python prover, and every error the operations
name. The checks themselves are in tests/groth16_checks.py, shared with the device's tests."""
import os

import pytest

import groth16_checks as ck
import nzcb

HOST = nzcb.GROTH16_HOST
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


@pytest.mark.parametrize("seed, power", [(21, 7), (22, 7), (21, 6)])
def test_random_circuit_equals_the_restatement(seed, power):
    """power 6 = cirPower: T is the level built from 2n - 1 points and the point at infinity."""
    ck.check_random_circuit(HOST, seed, power)


def test_edge_circuit_equals_the_restatement():
    ck.check_edge_circuit(HOST)


@pytest.mark.parametrize("chunk, fan_in", [(4, 2), (5, 3), (64, 64), (0, 0)])
def test_schedule_does_not_change_the_bytes(chunk, fan_in):
    ck.check_schedule(HOST, chunk, fan_in)


@pytest.mark.parametrize("g2", [False, True])
def test_rows_alone(g2):
    ck.check_rows(HOST, g2)


def test_degenerate_file():
    ck.check_degenerate_file(HOST)


def test_contribute():
    ck.check_contribute(HOST)


@pytest.mark.parametrize("kind", ["range", "curve", "zero"])
def test_contribute_names_a_spoiled_point(kind):
    ck.check_contribute_names_a_spoiled_point(HOST, kind)


def test_pairing_equation_after_a_drawn_contribution():
    ck.check_pairing_equation(HOST)


def test_errors():
    with open(os.path.join(GOLD, "p5.zkey"), "rb") as f:
        ck.check_errors(HOST, f.read())


def test_file_forms(tmp_path):
    ck.check_file_forms(HOST, tmp_path)


def test_schedule_knob_bounds():
    prev = nzcb.groth16_schedule(0, 0)
    assert nzcb.groth16_schedule(0, 0) == (32, 8)
    for chunk, fan_in in ((1025, 8), (32, 1), (32, 1025)):
        with pytest.raises(nzcb.NzcbError):
            nzcb.groth16_schedule(chunk, fan_in)
    assert nzcb.groth16_schedule(*prev) == (32, 8)
