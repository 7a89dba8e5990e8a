"""csrc/msm_seg.h: the sizes MsmScratch::init allocates for the segment plan of the dense
fixed-base MSMs (segments, whole segments, buckets cut into pieces, their carries and pieces)
hold for brute-force plans (tests/native/msm_seg_host.cpp, built for the host with address and
undefined-behaviour checks)."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CXX = shutil.which("clang++") or "/opt/rocm/lib/llvm/bin/clang++"


def test_segment_plan_bounds(tmp_path):
    if not os.path.exists(CXX):
        pytest.skip("no clang++")
    out = str(tmp_path / "msm_seg_host")
    subprocess.run([CXX, "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    os.path.join(ROOT, "tests", "native", "msm_seg_host.cpp"), "-o", out], check=True)
    p = subprocess.run([out], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stdout + p.stderr
    assert p.stdout.startswith("ok ") and int(p.stdout.split()[1]) > 40000
