"""csrc/capi_guard.h, the host-only header every C-ABI entry point goes through:
tests/native/capi_guard_host.cpp is a stand-alone program (clang++ of the ROCm toolchain, built with
-fsanitize=address,undefined, every sanitizer report fatal, leaks included) that checks guarded
(success clears err.code and keeps err.msg; Error and other exceptions; truncation; a NULL err),
guarded_new (nothing leaks when the builder throws) and MappedFile (missing, empty and 3-byte
files). Runs on the CPU only; the program is never loaded into Python."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CXX = shutil.which("clang++") or "/opt/rocm/lib/llvm/bin/clang++"


@pytest.fixture(scope="module")
def host_bin(tmp_path_factory):
    if not os.path.exists(CXX):
        pytest.skip("no clang++")
    out = str(tmp_path_factory.mktemp("capi_guard") / "capi_guard_host")
    subprocess.run([CXX, "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    os.path.join(ROOT, "tests", "native", "capi_guard_host.cpp"), "-o", out], check=True)
    return out


def test_sanitized_guard_program_runs_clean(host_bin, tmp_path):
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    p = subprocess.run([host_bin, str(tmp_path)], capture_output=True, text=True, timeout=60, env=env)
    assert p.returncode == 0, (p.stdout + p.stderr)[-4000:]
    assert p.stderr == ""
    assert p.stdout == "ok\n"
