"""The bounds of csrc/key_check.h's readers, the source the kernels and the host path share:
tests/native/key_check_host.cpp is a stand-alone program (clang++ of the ROCm toolchain, built
with -fsanitize=address,undefined, every sanitizer report fatal) that examines each file from a
heap allocation of exactly its length. Truncated and mutated ptau and zkey bytes (cut at every
section boundary +-1 and at 20 seeded offsets) must run clean, and the point findings it prints
must be the restatement's (tests/key_check_cases.py). Runs on the CPU only; the program is never
loaded into Python."""
import os
import random
import shutil
import subprocess

import pytest

import key_check_cases as kc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CXX = shutil.which("clang++") or "/opt/rocm/lib/llvm/bin/clang++"
DIGIT = {"OK": "0", "RANGE": "2", "CURVE": "3"}  # include/nzcb.h NZCB_KEY_*


@pytest.fixture(scope="module")
def host_bin(tmp_path_factory):
    if not os.path.exists(CXX):
        pytest.skip("no clang++")
    out = str(tmp_path_factory.mktemp("key_check") / "key_check_host")
    subprocess.run([CXX, "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    os.path.join(ROOT, "tests", "native", "key_check_host.cpp"), "-o", out], check=True)
    return out


def run(host_bin, lines):
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    p = subprocess.run([host_bin], input="".join(ln + "\n" for ln in lines), capture_output=True, text=True,
                       timeout=300, env=env)
    assert p.returncode == 0, p.stderr[-4000:]
    assert p.stderr == ""
    return p.stdout.splitlines()


def cuts_of(data: bytes, magic: bytes, seed: int) -> list:
    rng = random.Random(seed)
    cuts = {c + d for c in kc.section_edges(data, magic) for d in (-1, 0, 1)} | {rng.randrange(len(data)) for _ in range(20)}
    return sorted(c for c in cuts if 0 <= c < len(data))


def point_digits(pts: list) -> str:
    """The restatement's judgement of every stored point, one digit each."""
    out = ""
    for b in pts:
        f = kc.expected_finding([b], kc.G2_ONE, 1)
        out += DIGIT[f["status"] if f["status"] in DIGIT else "OK"]
    return out


def test_truncated_files_run_clean(host_bin):
    ptau = kc.make_ptau(3, kc.raw_points(kc.TAU, 15))
    zkey = kc.golden_zkey("p5")
    pc, zc = cuts_of(ptau, b"ptau", 1), cuts_of(zkey, b"zkey", 2)
    out = run(host_bin, [f"ptau {ptau.hex()} {','.join(map(str, pc))}", f"zkey {zkey.hex()} {','.join(map(str, zc))}"])
    assert len(out) == len(pc) + len(zc)
    assert out == ["ERR 2"] * len(out)  # a file cut short is malformed wherever the cut falls


def test_point_findings_equal_the_restatement(host_bin):
    pts = kc.raw_points(kc.TAU, 15)
    kc.spoil_range(pts, 0)
    kc.spoil_y(pts, 7)
    kc.spoil_zero(pts, 8)
    kc.spoil_other_point(pts, 13)
    kc.spoil_range(pts, 14)
    z = kc.golden_zkey("p5")
    n = kc.zkey_n(z)
    zpts = [z[kc.ptau_offset(z, i):][:64] for i in range(n + 6)]
    kc.spoil_y(zpts, 5)
    kc.spoil_range(zpts, n + 5)
    zbad = kc.patch(kc.patch(z, kc.ptau_offset(z, 0), b"".join(zpts)), kc.part_offset(z, "S1") + 32 * 7, kc.bn.to_le(kc.R))
    zbad = kc.patch(zbad, kc.part_offset(z, "L2") + 32 * (5 * n - 1), b"\xff" * 32)
    out = run(host_bin, [f"ptau {kc.make_ptau(3, pts).hex()} -", f"ptau {kc.make_ptau(3, kc.raw_points(kc.TAU, 15)).hex()} -",
                         f"zkey {zbad.hex()} -", f"zkey {z.hex()} -",
                         f"ptau {kc.make_ptau(3, pts[:9]).hex()} -", f"ptau {kc.make_ptau(3, pts, sections=(1, 2)).hex()} -"])
    assert out == [f"OK 3 {point_digits(pts)}", "OK 3 " + "0" * 15, f"OK {point_digits(zpts)} 2", "OK " + "0" * (n + 6) + " 0",
                   "ERR 2", "ERR 2"]
    assert point_digits(pts) == "200000033000002"


def test_mutated_bytes_run_clean(host_bin):
    """Bit flips in the section table and in the sections: any verdict, no sanitizer report."""
    rng = random.Random(3)
    lines = []
    for data, magic in ((kc.make_ptau(3, kc.raw_points(kc.TAU, 15)), "ptau"), (kc.golden_zkey("p5"), "zkey")):
        edges = kc.section_edges(data, magic.encode())
        for k in range(24):
            at = (edges[k % len(edges)] + rng.randrange(12)) % len(data) if k < 16 else rng.randrange(len(data))
            lines.append(f"{magic} {kc.patch(data, at, bytes([data[at] ^ (1 << rng.randrange(8))])).hex()} -")
        for field in (4, 8, 12 + 4, 12 + 11):  # version, section count, a section's size (low and high byte)
            lines.append(f"{magic} {kc.patch(data, field, bytes([0xff])).hex()} -")
    out = run(host_bin, lines)
    assert len(out) == len(lines) and all(ln.startswith(("OK ", "ERR 2")) for ln in out)
