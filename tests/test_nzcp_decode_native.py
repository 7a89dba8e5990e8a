"""The bounds check of csrc/nzcp_decode.h, the decoder source the kernel and the host path share:
tests/native/nzcp_decode_host.cpp is a stand-alone program (clang++ of the ROCm toolchain, built
with -fsanitize=address,undefined, every sanitizer report fatal) that decodes each URI from a heap
allocation of exactly its length. Sets B and C (tests/nzcp_decode_cases.py: malformed, truncated
and mutated passes) and A must run clean, and the records and input blocks it prints must be the
restatement's. Runs on the CPU only; the program is never loaded into Python."""
import hashlib
import os
import shutil
import subprocess

import pytest

import nzcp_decode_cases as C

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CXX = shutil.which("clang++") or "/opt/rocm/lib/llvm/bin/clang++"


@pytest.fixture(scope="module")
def host_bin(tmp_path_factory):
    if not os.path.exists(CXX):
        pytest.skip("no clang++")
    out = str(tmp_path_factory.mktemp("nzcp_decode") / "nzcp_decode_host")
    subprocess.run([CXX, "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    os.path.join(ROOT, "tests", "native", "nzcp_decode_host.cpp"), "-o", out], check=True)
    return out


@pytest.mark.parametrize("which", ["A", "B", "C"])
def test_sanitized_host_build_runs_clean_and_equals_the_restatement(host_bin, which):
    uris = C.uris_of(which)
    text = "".join((u.hex() or "-") + "\n" for u in uris)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    p = subprocess.run([host_bin], input=text, capture_output=True, text=True, timeout=300, env=env)
    assert p.returncode == 0, p.stderr[-4000:]
    assert p.stderr == ""
    lines = p.stdout.splitlines()
    assert len(lines) == len(uris)
    for i, (line, uri) in enumerate(zip(lines, uris)):
        rec_hex, block_digest = line.split()
        want, block = C.restate(uri, C.LIVE, bytes(range(1, 21)))
        got = C.fields(bytes.fromhex(rec_hex))
        for k in got:
            assert got[k] == want[k], (which, i, k)
        assert block_digest == hashlib.sha256(block).hexdigest(), (which, i)
