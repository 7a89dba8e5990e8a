"""The constant factors folded into tables (csrc/ntt.hip, csrc/f29.h): the forward transform
on a coset through per-coset twiddles (NttIo::tw, ntt_coset_twiddles) against exact
arithmetic, and div2k29 (the inverse transform's 1/N as a shift) on the GPU.

Bit-exact: every output is a unique field element."""
import random

import pytest

from oracle import bn254 as bn
from oracle.bn254 import R_MOD
from test_f29_div2k import KS, check_div2k, div2k_vectors, limbs

pytestmark = pytest.mark.gpu

FOLDS = (0, 2, 3, 6)


def _lem(vals):
    return b"".join(bn.to_lem(v, R_MOD) for v in vals)


def _from_lem(data):
    return [bn.from_lem(data[i:i + 32], R_MOD) for i in range(0, len(data), 32)]


def _cosets(log_n, rng):
    """1, the prover's c_j = g w4^j (g = 5, w4 the 4n-th root) for this size, one random element"""
    w4 = bn.FR_W[log_n + 2]
    return [1] + [5 * pow(w4, j, R_MOD) % R_MOD for j in range(3)] + [rng.randrange(1, R_MOD)]


@pytest.mark.parametrize("k", KS)
def test_div2k29_device_exact(k):
    """div2k29(x, K) as the device compiles it (nzcb_debug_f29 op 7): congruent to x 2^-K mod r,
    below x / 2^K + r, limbs below 2^29, over 1000 random x < 2.4 r and the edges."""
    import nzcb
    xs = div2k_vectors(k)
    words = []
    for x in xs:
        words += limbs(x) + [k]
    out = nzcb.f29_check(7, words)
    assert len(out) == 9 * len(xs)
    for i, x in enumerate(xs):
        check_div2k(k, x, out[9 * i:9 * i + 9])


@pytest.mark.parametrize("log_n", [1, 2, 3, 7, 8, 9, 10, 13, 14])
def test_ntt_coset_twiddles(engine, log_n):
    """out[i] = A(c w^i) for a polynomial of n + fold coefficients, against the oracle's FFT of
    (a_k + a_(k+n) c^n) c^k. The sizes are one pass of L stages (odd and even counts), and a
    pass of 8 with a second pass of 1, 2, 5 and 6 stages (the odd radix-2 stage in a later
    pass); the fold lengths are those that fit below n."""
    rng = random.Random(0x7157 + log_n)
    n = 1 << log_n
    for c in _cosets(log_n, rng):
        cn = pow(c, n, R_MOD)
        cp = [1] * n
        for k in range(1, n):
            cp[k] = cp[k - 1] * c % R_MOD
        for fold in FOLDS:
            if fold > n:
                continue
            a = [rng.randrange(R_MOD) for _ in range(n + fold)]
            got = _from_lem(engine.ntt_coset(_lem(a), log_n, _lem([c])))
            tw = [(a[k] + (a[k + n] * cn if k < fold else 0)) * cp[k] % R_MOD for k in range(n)]
            assert got == bn.fft(tw), (c, fold)


def test_ntt_coset_twiddles_three_passes():
    """2^17 (three passes): output 0 is the sum of the inputs' twisted images, and Horner at
    four random output indices."""
    import nzcb
    log_n, fold = 17, 6
    n = 1 << log_n
    rng = random.Random(0x717)
    eng = nzcb.Engine(0, max_log_ntt=log_n, max_msm_points=0)
    try:
        w = bn.FR_W[log_n]
        for c in (5 * bn.FR_W[log_n + 2] % R_MOD, rng.randrange(1, R_MOD)):
            a = [rng.randrange(R_MOD) for _ in range(n + fold)]
            got = _from_lem(eng.ntt_coset(_lem(a), log_n, _lem([c])))
            assert got[0] == bn.eval_pol(a, c)
            for i in [rng.randrange(1, n) for _ in range(4)]:
                assert got[i] == bn.eval_pol(a, c * pow(w, i, R_MOD) % R_MOD), i
    finally:
        eng.close()
