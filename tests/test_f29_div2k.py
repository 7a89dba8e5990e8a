"""csrc/f29.h div2k29 (x 2^-K mod r by one word step of a Montgomery reduction: the inverse
NTT's 1/N) built for the host (tests/native/f29_div2k_host.cpp) against exact integers. The
same vectors run on the GPU in tests/test_gpu_ntt_twist.py."""
import os
import random
import shutil
import subprocess

import pytest

from oracle.bn254 import R_MOD as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CXX = shutil.which("clang++") or "/opt/rocm/lib/llvm/bin/clang++"
M = (1 << 29) - 1
KS = (1, 5, 8, 21, 23, 24, 28)
XMAX = 12 * R // 5  # inputs are below 2.4 r


def limbs(x):
    return [(x >> (29 * i)) & M for i in range(9)]


def val(l):
    return sum(v << (29 * i) for i, v in enumerate(l))


def div2k_vectors(k, count=1000):
    """`count` random values below 2.4 r and the edges: 0, 1, r - 1, r, 2r, low K bits all
    ones / all zero, and the largest value below 2.4 r (the top limb at its bound)."""
    rng = random.Random(0xD2 + k)
    low = (1 << k) - 1
    x = rng.randrange(XMAX)
    edges = [0, 1, R - 1, R, 2 * R, x | low, x & ~low, low, XMAX - 1, (XMAX - 1) | low, (XMAX - 1) & ~low]
    return edges + [rng.randrange(XMAX) for _ in range(count)]


def check_div2k(k, x, got):
    """congruent to x 2^-K mod r, below x / 2^K + r, every limb below 2^29"""
    assert max(got) <= M, (k, x)
    v = val(got)
    assert v % R == x * pow(2, -k, R) % R, (k, x)
    assert (v - R) << k < x, (k, x)   # v < x / 2^K + r, exactly


@pytest.fixture(scope="module")
def host_bin(tmp_path_factory):
    if not os.path.exists(CXX):
        pytest.skip("no clang++")
    out = str(tmp_path_factory.mktemp("f29d") / "f29_div2k_host")
    subprocess.run([CXX, "-O1", "-std=c++17", os.path.join(ROOT, "tests", "native", "f29_div2k_host.cpp"), "-o", out],
                   check=True)
    return out


def test_div2k29_host(host_bin):
    lines, items = [], []
    for k in KS:
        for x in div2k_vectors(k):
            lines.append("%d %s" % (k, " ".join("%x" % v for v in limbs(x))))
            items.append((k, x))
    p = subprocess.run([host_bin], input="\n".join(lines) + "\n", capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stderr
    got = [[int(t, 16) for t in ln.split()] for ln in p.stdout.splitlines()]
    assert len(got) == len(items)
    for (k, x), g in zip(items, got):
        check_div2k(k, x, g)
