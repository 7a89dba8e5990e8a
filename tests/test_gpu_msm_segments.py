"""Dense fixed-base MSMs by whole-bucket segments (msm.hip msm_seg_*_kernel,
msm_accumulate29_seg_kernel; NZCB_ACC_SEGMENTS): both sides of the switch give the oracle's
point, byte for byte, and the segment plan tiles the buckets, longest first, the same way in
every run.

The switch is read once per process, so each side runs in a fresh child (this file, run as a
script, is the child): it does every MSM of the module and reports results and plans, which
the tests then compare. Bases are an arithmetic progression P + i S, so the oracle's MSM is
(sum s_i) P + (sum i s_i) S: two scalar multiplications of oracle/bn254.py whatever the size.
"""
import os
import pickle
import random
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if __name__ == "__main__":
    sys.path[:0] = [os.path.join(ROOT, "nzcb-circom_amd"), ROOT]

from oracle import bn254 as bn  # noqa: E402
from oracle.bn254 import R_MOD  # noqa: E402

pytestmark = pytest.mark.gpu

WINDOWS = (16, 20)
KINV = pow(2, -256, R_MOD)
N_BIG = 13000
SEED = 20251
# the cap the library is built with (csrc/msm_seg.h kSegMax); the child reports the real one and
# test_edge_lengths checks that the edge case was built for it
SEG_MAX = 256


def _line(seed):
    rng = random.Random(seed)
    return (bn.g1_mul(bn.G1_GEN, rng.randrange(1, R_MOD)), bn.g1_mul(bn.G1_GEN, rng.randrange(1, R_MOD)))


def _progression(n, seed):
    p, step = _line(seed)
    pts = []
    for _ in range(n):
        pts.append(p)
        p = bn.g1_add(p, step)
    return pts


def _want_line(seed, sc):
    """sum sc_i (P + i S) by two scalar multiplications."""
    p, step = _line(seed)
    return bn.g1_add(bn.g1_mul(p, sum(sc) % R_MOD), bn.g1_mul(step, sum(i * s for i, s in enumerate(sc)) % R_MOD))


def _pm1(n, c, rng):
    """Scalars whose signed c-bit digits are all +1 or -1 (the top one +1): every entry of every
    window lands in bucket 0. Below 2^240, so min(s, r - s) = s and, as a raw integer of the
    folded table, s is below r."""
    nw = 240 // c
    return [sum(rng.choice((1, -1)) << (c * w) for w in range(nw - 1)) + (1 << (c * (nw - 1))) for _ in range(n)]


def _cases():
    """name -> (points or None for the shared progression, {window: scalars})."""
    rng = random.Random(77)
    both = lambda sc: {c: sc for c in WINDOWS}  # noqa: E731
    v = rng.randrange(R_MOD)
    pool = [rng.randrange(R_MOD) for _ in range(10)]
    g = bn.g1_mul(bn.G1_GEN, 4321)
    k = SEG_MAX
    # one window-0 digit each: buckets of k - 1, k and k + 1 entries, then 70 buckets of one entry
    # (74 segments: a second wave of 10)
    edge = [5] * (k - 1) + [6] * k + [7] * (k + 1) + list(range(100, 170))
    return {
        "rand": (None, both([rng.randrange(R_MOD) for _ in range(3000)])),
        "pm1": (None, {c: _pm1(3000, c, rng) for c in WINDOWS}),
        "pm1_big": (None, {c: _pm1(N_BIG, c, rng) for c in WINDOWS}),  # one bucket of > 2^16 entries: three pieces
        "repeat": (None, both([v] * 3000)),
        "ten": (None, both([pool[i % 10] for i in range(N_BIG)])),
        "ends": (None, both([0, 1, R_MOD - 1])),
        "double": ([g, g], both([9, 9])),
        "cancel": ([g, bn.g1_neg(g)], both([9, 9])),
        "inf_bases": ([g, None, bn.g1_neg(g), g, None, g], both([5, 6, 5, 7 << 200, 9, R_MOD - 5])),
        "edge": (None, both(edge)),
    }


PLANS = ("rand", "repeat", "edge")  # cases whose plan the child reads back (default window, twice)


def _child(inp, outp):
    import nzcb
    with open(inp, "rb") as f:
        job = pickle.load(f)
    eng = nzcb.Engine(0, max_log_ntt=4, max_msm_points=1 << 14)
    res, plans = {}, {}
    for name, (bases, per_window) in job.items():
        n_table = len(bases) // 64
        db = nzcb.dev_alloc(len(bases))
        nzcb.h2d(db, bases)
        for c, scal in per_window.items():
            n = len(scal) // 32
            ds = nzcb.dev_alloc(len(scal))
            nzcb.h2d(ds, scal)
            # the scalars as they stand: normal form on the plain table, raw integers on the folded one
            res[name, c, "plain"] = eng.msm_fixed_dev(db, n_table, ds, n, False, window=c)
            res[name, c, "fold"] = eng.msm_fixed_dev(db, n_table, ds, n, True, window=c, fold=True)
            if name in PLANS and c == 20:
                runs = [eng.msm_plan(db, n_table, ds, n, False, window=c) for _ in range(2)]
                plans[name] = [(out, plan) for out, plan in runs]
            nzcb.dev_free(ds)
        nzcb.dev_free(db)
    eng.close()
    with open(outp, "wb") as f:
        pickle.dump({"res": res, "plans": plans}, f)


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    """{switch value: the child's results}, and the oracle's points."""
    import nzcb
    if nzcb.device_count() < 1:
        pytest.fail("GPU test requested but no HIP device is visible")
    d = tmp_path_factory.mktemp("segs")
    line = b"".join(bn.g1_to_lem(p) for p in _progression(N_BIG, SEED))
    job, want = {}, {}
    for name, (pts, per_window) in _cases().items():
        bases = line if pts is None else b"".join(bn.g1_to_lem(p) for p in pts)
        job[name] = (bases, {c: b"".join(bn.to_le(s) for s in sc) for c, sc in per_window.items()})
        for c, sc in per_window.items():
            folded = [s * KINV % R_MOD for s in sc]
            if pts is None:
                want[name, c, "plain"], want[name, c, "fold"] = _want_line(SEED, sc), _want_line(SEED, folded)
            else:
                want[name, c, "plain"], want[name, c, "fold"] = bn.msm(pts, sc), bn.msm(pts, folded)
    inp = d / "job.pkl"
    with open(inp, "wb") as f:
        pickle.dump(job, f)
    out = {}
    for sw in ("0", "1"):
        outp = d / f"out{sw}.pkl"
        p = subprocess.run([sys.executable, os.path.abspath(__file__), str(inp), str(outp)], capture_output=True,
                           text=True, timeout=200, env=dict(os.environ, NZCB_ACC_SEGMENTS=sw))
        assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-3000:]
        with open(outp, "rb") as f:
            out[sw] = pickle.load(f)
    return out, want


def _affine(b):
    x, y = bn.from_le(b[:32]), bn.from_le(b[32:])
    return None if x == 0 and y == 0 else (x, y)


@pytest.mark.parametrize("mode", ["plain", "fold"])
@pytest.mark.parametrize("window", WINDOWS)
@pytest.mark.parametrize("name", ["rand", "pm1", "pm1_big", "repeat", "ten", "ends", "double", "cancel",
                                  "inf_bases", "edge"])
def test_switch_sides_agree_with_oracle(runs, name, window, mode):
    """Chunks (NZCB_ACC_SEGMENTS=0) and segments (1): the same 64 bytes, the oracle's point."""
    out, want = runs
    a, b = out["0"]["res"][name, window, mode], out["1"]["res"][name, window, mode]
    assert a == b
    assert _affine(b) == want[name, window, mode]


def test_switch_selects_the_plan(runs):
    """The segment side ran by segments, the chunk side has no plan."""
    out, _ = runs
    for name in PLANS:
        assert all(plan is None for _, plan in out["0"]["plans"][name])
        assert all(plan is not None for _, plan in out["1"]["plans"][name])


@pytest.mark.parametrize("name", ["rand", "repeat", "edge"])
def test_plan_invariants(runs, name):
    """From the offsets read back: the segments tile every non-empty bucket exactly once (the
    first at the bucket's start, each later one seg_max further), no length above seg_max,
    lengths do not increase, equal lengths in bucket order, and a second run gives the same plan
    and the same point."""
    import numpy as np
    out, want = runs
    (r1, p1), (r2, p2) = out["1"]["plans"][name]
    assert r1 == r2 and _affine(r1) == want[name, 20, "plain"]
    assert p1 == p2
    cap = p1["seg_max"]
    off = np.array(p1["offsets"], dtype=np.int64)
    start, ln, bucket = (np.array(p1[k], dtype=np.int64) for k in ("start", "len", "bucket"))
    assert len(off) == (1 << 19) + 1 and off[0] == 0
    sizes = np.diff(off)
    assert len(start) == int(np.sum((sizes + cap - 1) // cap))  # ceil(size / cap) segments per bucket
    assert ln.min() >= 1 and ln.max() <= cap
    assert np.all(np.diff(ln) <= 0)
    # inside their bucket, at a multiple of cap from its start, as long as the cap and the bucket allow
    rel = start - off[bucket]
    assert np.all(rel >= 0) and np.all(rel % cap == 0)
    assert np.all(ln == np.minimum(cap, off[bucket + 1] - start))
    # exactly once: in stream order the segments follow each other from 0 to the entry count
    order = np.argsort(start, kind="stable")
    assert start[order][0] == 0 and np.all(start[order][1:] == (start + ln)[order][:-1])
    assert (start + ln)[order][-1] == off[-1]
    # stable: by bucket within a length, by position within a bucket
    key = np.lexsort((start, bucket, -ln))
    assert np.all(key == np.arange(len(start)))


def test_edge_lengths(runs):
    """Buckets of seg_max - 1, seg_max and seg_max + 1 entries in one MSM: a whole segment that
    is a bucket, one that is a piece, a rest of one entry; 74 segments, so the second wave has
    ten lanes."""
    out, _ = runs
    _, plan = out["1"]["plans"]["edge"][0]
    cap = plan["seg_max"]
    assert cap == SEG_MAX  # _cases builds the edge scalars for this cap
    assert plan["len"] == [cap, cap, cap - 1] + [1] * 71
    assert plan["bucket"][:3] == [5, 6, 4] and plan["bucket"][3] == 6
    assert plan["bucket"][4:] == list(range(99, 169))
    assert len(plan["len"]) % 64 == 10


if __name__ == "__main__":
    _child(sys.argv[1], sys.argv[2])
