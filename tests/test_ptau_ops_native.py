"""The bounds and the arithmetic of csrc/ptau_ops.h, the source the kernels and the host path of
the powers-of-tau operations share: tests/native/ptau_ops_host.cpp is a stand-alone program
(clang++ of the ROCm toolchain, built with -fsanitize=address,undefined, every sanitizer report
fatal) that opens each file from a heap allocation of exactly its length. Files cut at every
section edge +-1 and at 20 seeded offsets, and files with flipped bits, must run clean; the
point findings, the new file and scalar multiples over Fq and Fq2 must be the restatement's
(tests/ptau_ops_cases.py). Runs on the CPU only; the program is never loaded into Python."""
import os
import random
import shutil
import subprocess

import pytest

import ptau_ops_cases as pc
from oracle import bn254 as bn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CXX = shutil.which("clang++") or "/opt/rocm/lib/llvm/bin/clang++"


@pytest.fixture(scope="module")
def host_bin(tmp_path_factory):
    if not os.path.exists(CXX):
        pytest.skip("no clang++")
    out = str(tmp_path_factory.mktemp("ptau_ops") / "ptau_ops_host")
    subprocess.run([CXX, "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    os.path.join(ROOT, "tests", "native", "ptau_ops_host.cpp"), "-o", out], check=True)
    return out


def run(host_bin, lines):
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    p = subprocess.run([host_bin], input="".join(ln + "\n" for ln in lines), capture_output=True, text=True,
                       timeout=300, env=env)
    assert p.returncode == 0, p.stderr[-4000:]
    assert p.stderr == ""
    return p.stdout.splitlines()


def test_truncated_files_run_clean(host_bin):
    rng = random.Random(1)
    for data in (pc.expected_file(2, pc.SECRETS_A), pc.expected_file(1, pc.SECRETS_A, prepared=True)):
        cuts = {c + d for c in pc.section_edges(data) for d in (-1, 0, 1)} | {rng.randrange(len(data)) for _ in range(20)}
        cuts = sorted(c for c in cuts if 0 <= c < len(data))
        out = run(host_bin, [f"ptau {data.hex()} {','.join(map(str, cuts))}"])
        assert out == ["ERR 2"] * len(cuts)  # a file cut short is malformed wherever the cut falls


def test_point_findings_equal_the_restatement(host_bin):
    good = pc.expected_file(2, pc.SECRETS_A)
    bad = good
    for sid, index, kind in ((2, 0, "range"), (2, 6, "zero"), (3, 3, "curve"), (4, 1, "zero"), (5, 2, "range"),
                             (6, 0, "curve")):
        bad = pc.spoiled(bad, sid, index, kind)
    out = run(host_bin, [f"ptau {good.hex()} -", f"ptau {bad.hex()} -", f"ptau {pc.without_section(good, 4).hex()} -",
                         f"ptau {pc.with_short_section(good, 3).hex()} -"])
    assert out == ["OK 2 0000000 0000 0000 0000 0", "OK 2 2000003 0003 0300 0020 3", "ERR 2", "ERR 2"]


def test_new_and_scalar_multiples_equal_the_restatement(host_bin):
    k = pc.SECRETS_B[1]
    g1, g2 = bn.g1_mul(bn.G1_GEN, 77), bn.g2_mul(bn.G2_GEN, 77)
    out = run(host_bin, ["new 1", "new 3", "new 0", "new 25",
                         f"mul g1 {bn.g1_to_lem(g1).hex()} {bn.to_le(k).hex()}",
                         f"mul g2 {bn.g2_to_lem(g2).hex()} {bn.to_le(k).hex()}",
                         f"mul g2 {bn.g2_to_lem(g2).hex()} {bn.to_le(pc.R - 1).hex()}",
                         f"mul g1 {bytes(64).hex()} {bn.to_le(k).hex()}"])
    assert out == ["OK " + pc.expected_file(1).hex(), "OK " + pc.expected_file(3).hex(), "ERR 1", "ERR 1",
                   "OK " + bn.g1_to_lem(bn.g1_mul(g1, k)).hex(), "OK " + bn.g2_to_lem(bn.g2_mul(g2, k)).hex(),
                   "OK " + bn.g2_to_lem(bn.g2_neg(g2)).hex(), "OK " + bytes(64).hex()]


def test_mutated_bytes_run_clean(host_bin):
    """Bit flips in the section table and in the sections: any verdict, no sanitizer report."""
    rng = random.Random(3)
    data = pc.expected_file(2, pc.SECRETS_A)
    edges = pc.section_edges(data)
    lines = []
    for k in range(24):
        at = (edges[k % len(edges)] + rng.randrange(12)) % len(data) if k < 16 else rng.randrange(len(data))
        lines.append(f"ptau {(data[:at] + bytes([data[at] ^ (1 << rng.randrange(8))]) + data[at + 1:]).hex()} -")
    for field in (4, 8, 12 + 4, 12 + 11):  # version, section count, a section's size (low and high byte)
        lines.append(f"ptau {(data[:field] + bytes([0xff]) + data[field + 1:]).hex()} -")
    out = run(host_bin, lines)
    assert len(out) == len(lines) and all(ln.startswith(("OK ", "ERR 1", "ERR 2")) for ln in out)
