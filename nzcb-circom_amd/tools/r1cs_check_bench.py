#!/usr/bin/env python3
"""The witness check on the nzcp_live r1cs over GPU-resident witnesses, in one process on device 0.

Witnesses of live-shaped passes are made in HBM by the GPU witness VM (WitnessProgram.run_dev,
timed as the yardstick: what a check costs next to making the witness), then, after a warm-up
call: R1cs.check_dev at count = 1, 8, 64 and 512 (median of 5 wall times, with the kernels'
HIP-event times of nzcb_debug_r1cs_check_timings), the long-row threshold candidates and the
witness-tile sizes at count = 64, the host path's single-thread time for one witness, and the
kernels' register use from -Rpass-analysis=kernel-resource-usage. Every timed result is
compared with the first (all witnesses satisfied). Writes profiles/r1cs_check.txt (or --out).

  python tools/r1cs_check_bench.py [--out FILE] [--resources FILE] [--counts 1,8,64,512]

--resources: the compiler's remark text captured earlier (hipcc ... --cuda-device-only
-Rpass-analysis=kernel-resource-usage -c csrc/r1cs_check.hip 2> FILE) instead of compiling here.
"""
import argparse
import os
import re
import statistics
import subprocess
import sys
import time

PKG = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ROOT = os.path.dirname(PKG)
sys.path[:0] = [ROOT, PKG]
import bench  # noqa: E402
import nzcb  # noqa: E402
from nzcb import nzcplive  # noqa: E402

THRESHOLDS = (8, 16, 32, 64, 256, 1 << 20)   # 2^20: no row is long (nzcp_live's longest has 836 terms)
TILES = (1, 2, 4)


def resources(path):
    if path:
        text = open(path).read()
    else:
        cmd = [os.environ.get("HIPCC", "/opt/rocm/bin/hipcc"), "-O3", "-std=c++17", "--offload-arch=gfx950",
               "--cuda-device-only", "-Rpass-analysis=kernel-resource-usage", "-c",
               os.path.join(PKG, "csrc", "r1cs_check.hip"), "-o", os.devnull]
        text = subprocess.run(cmd, capture_output=True, text=True, check=True).stderr
    rows = []
    for line in text.splitlines():
        m = re.search(r"remark:\s+(Function Name|VGPRs|AGPRs|ScratchSize \[bytes/lane\]|Occupancy \[waves/SIMD\]"
                      r"|VGPRs Spill|LDS Size \[bytes/block\]): (\S+)", line)
        if not m:
            continue
        if m.group(1) == "Function Name":
            name = re.search(r"(k_r1cs_[a-z_]+?)(?:ILi(\d)E)?E", m.group(2))
            rows.append([f"{name.group(1)}<{name.group(2)}>" if name and name.group(2) else
                         name.group(1) if name else m.group(2)])
        else:
            rows[-1].append(f"{m.group(1)} {m.group(2)}")
    return ["  " + r[0] + ": " + ", ".join(r[1:]) for r in rows]


def timed(fn, reps):
    walls = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        walls.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(walls), min(walls), max(walls)


def timed_check(r, d_wit, count, stride, reps=5):
    """median wall ms, min, max and the median kernel ms (rows, long rows, collect)"""
    walls, kernels = [], []
    for _ in range(reps):
        t0 = time.perf_counter()
        res = r.check_dev(d_wit, count, stride)
        walls.append((time.perf_counter() - t0) * 1e3)
        kernels.append(nzcb.R1cs.timings())
        assert all(x["n_bad"] == 0 for x in res), "a witness of the batch fails the r1cs"
    return (statistics.median(walls), min(walls), max(walls),
            [statistics.median(k[i] for k in kernels) for i in range(3)])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r1cs_check.txt"))
    ap.add_argument("--resources", default=None)
    ap.add_argument("--counts", default="1,8,64,512")
    args = ap.parse_args()
    counts = [int(x) for x in args.counts.split(",")]
    r1cs, prog, _ = nzcplive.build()
    wp = nzcb.WitnessProgram(prog)
    stride = 32 * wp.n_wires
    top = max(counts + [64])
    inputs = bench.pass_inputs(range(top))
    d_in, d_wit = nzcb.dev_alloc(len(inputs)), nzcb.dev_alloc(top * stride)
    nzcb.h2d(d_in, inputs)
    t0 = time.perf_counter()
    r = nzcb.R1cs(r1cs, device=0)
    create_ms = (time.perf_counter() - t0) * 1e3
    info = r.info
    out = [f"r1cs_check_bench: {nzcb.version()}",
           f"nzcp_live r1cs: {info['n_constraints']} constraints, {info['n_wires']} wires, {info['n_terms']} terms, "
           f"{info['n_long_rows']} rows of {info['long_row_threshold']} or more terms",
           f"nzcb_r1cs_create (parse {len(r1cs) >> 20} MiB, upload): {create_ms:.0f} ms", ""]
    assert not any(wp.run_dev(d_in, 1, d_wit, stride))          # warm-up: HIP start-up, code load
    r.check_dev(d_wit, 1, stride)
    for n in counts:
        vm, vlo, vhi = timed(lambda: wp.run_dev(d_in, n, d_wit, stride), 3)
        med, lo, hi, k = timed_check(r, d_wit, n, stride)
        out.append(f"check_dev, count {n}: median {med:.3f} ms of 5 (min {lo:.3f}, max {hi:.3f}), "
                   f"{med / n:.4f} ms per witness")
        out.append(f"    kernels (HIP events): lane-per-row {k[0]:.3f} ms, wave-per-row {k[1]:.3f} ms, "
                   f"collect {k[2]:.3f} ms; {sum(k) / n:.4f} ms per witness")
        out.append(f"    WitnessProgram.run_dev, the same count: median {vm:.3f} ms of 3 (min {vlo:.3f}, max {vhi:.3f}), "
                   f"{vm / n:.4f} ms per witness; check / run_dev = {med / vm:.3f}")
    if top > 64:
        assert not any(wp.run_dev(d_in, 64, d_wit, stride))
    out += ["", "long-row threshold at count 64 (kernel ms, median of 5; the results are equal):"]
    for t in THRESHOLDS:
        rt = nzcb.R1cs(r1cs, device=0, long_row_threshold=t)
        rt.check_dev(d_wit, 64, stride)
        med, lo, hi, k = timed_check(rt, d_wit, 64, stride)
        out.append(f"    threshold {t:>7d}: {rt.info['n_long_rows']:6d} long rows, lane-per-row {k[0]:8.3f}, "
                   f"wave-per-row {k[1]:7.3f}, both {k[0] + k[1]:8.3f}; call {med:.3f} ms")
        rt.close()
    for n in sorted({64, top}):
        if n != 64:
            assert not any(wp.run_dev(d_in, n, d_wit, stride))
        out += ["", f"witness tile at count {n} (witnesses evaluated per row by one lane or wave; kernel ms, "
                    "median of 5):"]
        for tile in TILES:
            rt = nzcb.R1cs(r1cs, device=0, witness_tile=tile)
            rt.check_dev(d_wit, n, stride)
            med, lo, hi, k = timed_check(rt, d_wit, n, stride)
            out.append(f"    tile {tile}: lane-per-row {k[0]:8.3f}, wave-per-row {k[1]:7.3f}, both {k[0] + k[1]:8.3f}; "
                       f"call {med:.3f} ms")
            rt.close()
    one = nzcb.d2h(d_wit, stride)
    host = nzcb.R1cs(r1cs, device=nzcb.R1CS_HOST)
    t0 = time.perf_counter()
    res = host.check(one, count=1)
    host_ms = (time.perf_counter() - t0) * 1e3
    assert res[0]["n_bad"] == 0
    host.close()
    out += ["", f"host path (NZCB_R1CS_HOST), one witness, one thread: {host_ms:.1f} ms"]
    out += ["", "kernel resource usage (gfx950, -Rpass-analysis=kernel-resource-usage):"] + resources(args.resources)
    r.close()
    wp.close()
    nzcb.dev_free(d_in)
    nzcb.dev_free(d_wit)
    text = "\n".join(out) + "\n"
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)
    print(text, end="")
    return 0


if __name__ == "__main__":
    sys.exit(main())
