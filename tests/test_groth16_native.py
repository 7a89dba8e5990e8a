"""The bounds and the arithmetic of csrc/groth16.h, the source the kernels and the host path of
the Groth16 key generation share: tests/native/groth16_host.cpp is a stand-alone program (clang++
of the ROCm toolchain, built with -fsanitize=address,undefined, every sanitizer report fatal) that
opens each input from a heap allocation of exactly its length. r1cs, prepared powers-of-tau and
Groth16 zkey inputs cut at every section edge +-1 and at 20 seeded offsets, and inputs with
flipped bits, must run clean; a small setup and contribute must be the restatement's
(tests/groth16_cases.py). Runs on the CPU only; the program is never loaded into Python."""
import json
import os
import random
import shutil
import subprocess

import pytest

import groth16_cases as gc
import ptau_ops_cases as pc
from oracle import bn254 as bn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CXX = shutil.which("clang++") or "/opt/rocm/lib/llvm/bin/clang++"
A = pc.SECRETS_A


@pytest.fixture(scope="module")
def host_bin(tmp_path_factory):
    if not os.path.exists(CXX):
        pytest.skip("no clang++")
    out = str(tmp_path_factory.mktemp("groth16") / "groth16_host")
    subprocess.run([CXX, "-O1", "-g", "-std=c++17", "-pthread", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", os.path.join(ROOT, "tests", "native", "groth16_host.cpp"), "-o", out],
                   check=True)
    return out


def run(host_bin, lines):
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    p = subprocess.run([host_bin], input="".join(ln + "\n" for ln in lines), capture_output=True, text=True,
                       timeout=600, env=env)
    assert p.returncode == 0, p.stderr[-4000:]
    assert p.stderr == ""
    return p.stdout.splitlines()


def cuts_of(data: bytes, magic: bytes, seed: int) -> list:
    rng = random.Random(seed)
    cuts = {c + d for c in gc.section_edges(data, magic) for d in (-1, 0, 1)} | {rng.randrange(len(data)) for _ in range(20)}
    return sorted(c for c in cuts if 0 <= c < len(data))


TINY = gc.edge_circuit(3)  # 3 constraints, nPublic 3: cirPower 3


def test_small_setup_and_contribute_equal_the_restatement(host_bin):
    r1cs = gc.edge_circuit()
    ptau, key = pc.expected_file(5, A, prepared=True), gc.expected_zkey(r1cs, 5, A)
    out = run(host_bin, [f"setup {r1cs.hex()} {ptau.hex()} -", f"contribute {key.hex()} {bn.to_le(gc.D1).hex()} -",
                         f"vk {key.hex()} - -", f"contribute {key.hex()} {bn.to_le(gc.R).hex()} -",
                         f"vk {pc.expected_file(1).hex()} - -"])
    assert out[0] == "OK " + key.hex()
    assert out[1] == "OK " + gc.expected_zkey(r1cs, 5, A, gc.D1).hex()
    assert json.loads(out[2][3:]) == gc.expected_vk(key)
    assert out[3:] == ["ERR 1", "ERR 2"]


def test_truncated_inputs_run_clean(host_bin):
    ptau, key = pc.expected_file(3, A, prepared=True), gc.expected_zkey(TINY, 3, A)
    rc, pcuts, kc = cuts_of(TINY, b"r1cs", 1), cuts_of(ptau, b"ptau", 2), cuts_of(key, b"zkey", 3)
    join = lambda cuts: ",".join(map(str, cuts))
    out = run(host_bin, [f"setup {TINY.hex()} {ptau.hex()} {join(rc)}", f"setupp {TINY.hex()} {ptau.hex()} {join(pcuts)}",
                         f"contribute {key.hex()} {bn.to_le(gc.D1).hex()} {join(kc)}", f"vk {key.hex()} - {join(kc)}"])
    # a file cut short is malformed wherever the cut falls
    assert out == ["ERR 2"] * (len(rc) + len(pcuts) + 2 * len(kc))


def test_mutated_bytes_run_clean(host_bin):
    """Bit flips in the section tables and in the sections: any verdict, no sanitizer report."""
    rng = random.Random(5)
    ptau, key = pc.expected_file(3, A, prepared=True), gc.expected_zkey(TINY, 3, A)
    lines = []
    for kind, data, magic, rest in (("setup", TINY, b"r1cs", ptau.hex()), ("setupp", ptau, b"ptau", None),
                                    ("contribute", key, b"zkey", bn.to_le(gc.D1).hex()), ("vk", key, b"zkey", "-")):
        edges = gc.section_edges(data, magic)
        for k in range(24):
            at = (edges[k % len(edges)] + rng.randrange(12)) % len(data) if k < 16 else rng.randrange(len(data))
            flipped = data[:at] + bytes([data[at] ^ (1 << rng.randrange(8))]) + data[at + 1:]
            lines.append(f"setupp {TINY.hex()} {flipped.hex()} -" if kind == "setupp" else
                         f"{kind} {flipped.hex()} {rest} -")
    out = run(host_bin, lines)
    assert len(out) == len(lines) and all(ln.startswith(("OK ", "ERR 1", "ERR 2", "ERR 4")) for ln in out)
