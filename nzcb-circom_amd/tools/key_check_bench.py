#!/usr/bin/env python3
"""The key material check at the sizes the prover is used at, in one process on device 0.

A power-21 powers-of-tau file (nzcb_ptau_synth) and the nzcp_live zkey made from it
(nzcb_plonk_setup, n = 2^21; its wall time is the yardstick: regenerating the key is the only
other way to validate one, and it needs the r1cs). After a warm-up call: nzcb.ptau_check of
all 2^22 - 1 points and nzcb.zkey_check of the key, median of 5 wall times with the phases of
nzcb_debug_key_check_timings (kernels by HIP events: points, weights, transforms, compares; the
MSMs and commitments by wall time with their host part; the pairing checks on the host), the
host path at power 12 for a per-point figure, and the kernels' register use from
-Rpass-analysis=kernel-resource-usage. Each file is then checked once more with defects planted at
its far end and on a chunk edge, which must be found where they were put. Writes profiles/key_check.txt (or --out).

  python tools/key_check_bench.py [--out FILE] [--resources FILE] [--power 21] [--reps 5]

--power: the ptau's power; the zkey part runs only at 21 (the nzcp_live circuit's domain).
--resources: the compiler's remark text captured earlier (hipcc ... --cuda-device-only
-Rpass-analysis=kernel-resource-usage -c csrc/key_check.hip 2> FILE) instead of compiling here.
"""
import argparse
import os
import re
import statistics
import struct
import subprocess
import sys
import time

PKG = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ROOT = os.path.dirname(PKG)
sys.path[:0] = [ROOT, PKG]
import nzcb  # noqa: E402
from nzcb import nzcplive  # noqa: E402

TAU = 0x6E7A6362746175
PHASES = ("points kernel", "weights kernel", "two MSMs (wall)", "copies and rest of the device pass (wall)",
          "pairing checks (host)", "call", "transforms", "compare kernel", "commitments' MSMs (wall)")


def resources(path):
    if path:
        text = open(path).read()
    else:
        cmd = [os.environ.get("HIPCC", "/opt/rocm/bin/hipcc"), "-O3", "-std=c++17", "--offload-arch=gfx950",
               "--cuda-device-only", "-Rpass-analysis=kernel-resource-usage", "-c",
               os.path.join(PKG, "csrc", "key_check.hip"), "-o", os.devnull]
        text = subprocess.run(cmd, capture_output=True, text=True, check=True).stderr
    rows = []
    for line in text.splitlines():
        m = re.search(r"remark:\s+(Function Name|VGPRs|AGPRs|ScratchSize \[bytes/lane\]|Occupancy \[waves/SIMD\]"
                      r"|VGPRs Spill|LDS Size \[bytes/block\]): (\S+)", line)
        if not m:
            continue
        if m.group(1) == "Function Name":
            name = re.search(r"(k_(?:srs|fr)_[a-z]+)", m.group(2))
            rows.append([name.group(1) if name else m.group(2)])
        elif rows:
            rows[-1].append(f"{m.group(1)} {m.group(2)}")
    return ["  " + r[0] + ": " + ", ".join(r[1:]) for r in rows]


def timed(fn, reps, ok):
    """median, min, max wall ms and the median of every phase over `reps` calls that must be ok"""
    walls, phases = [], []
    for _ in range(reps):
        t0 = time.perf_counter()
        res = fn()
        walls.append((time.perf_counter() - t0) * 1e3)
        phases.append(nzcb.Engine.key_check_timings())
        assert ok(res), res
    return (statistics.median(walls), min(walls), max(walls),
            [statistics.median(p[i] for p in phases) for i in range(len(phases[0]))])


def report(out, what, reps, med, lo, hi, ph, which):
    out.append(f"{what}: median {med:.1f} ms of {reps} (min {lo:.1f}, max {hi:.1f})")
    for i in which:
        out.append(f"    {PHASES[i]}: {ph[i]:.2f} ms")


def section(data, sid):
    """(offset, size) of section `sid` of an iden3 binary file"""
    nsec = struct.unpack_from("<I", data, 8)[0]
    off = 12
    for _ in range(nsec):
        t, size = struct.unpack_from("<IQ", data, off)
        off += 12
        if t == sid:
            return off, size
        off += size
    raise KeyError(sid)


def say(msg):
    print(f"[key_check_bench] {msg}", file=sys.stderr, flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "key_check.txt"))
    ap.add_argument("--resources", default=None)
    ap.add_argument("--power", type=int, default=21)
    ap.add_argument("--reps", type=int, default=5)
    args = ap.parse_args()
    out = [f"key_check_bench: {nzcb.version()}", ""]

    # warm-up: HIP start-up, code load
    small = nzcb.ptau_synth(8, TAU)
    assert nzcb.ptau_check(small, device=0)["status"] == "OK"

    t0 = time.perf_counter()
    ptau = nzcb.ptau_synth(args.power, TAU)
    out.append(f"nzcb_ptau_synth, power {args.power}: {(time.perf_counter() - t0) * 1e3:.0f} ms, {len(ptau) >> 20} MiB")
    m = (2 << args.power) - 1
    say(out[-1])
    nzcb.ptau_check(ptau, device=0)
    med, lo, hi, ph = timed(lambda: nzcb.ptau_check(ptau, device=0), args.reps, lambda f: f["status"] == "OK")
    report(out, f"ptau_check, all {m} points", args.reps, med, lo, hi, ph, (0, 1, 2, 3, 4))
    out.append(f"    {med * 1e3 / m:.3f} us per point")
    ptau_ms = med
    say(f"ptau_check: {med:.1f} ms")
    # planted defects: a flipped bit on the second chunk's first point, the last point a copy of its neighbour
    spoiled = bytearray(ptau)
    g1, _ = section(ptau, 2)
    edge = min(1 << 20, m - 2)
    spoiled[g1 + 64 * (m - 1):g1 + 64 * m] = ptau[g1 + 64 * (m - 2):g1 + 64 * (m - 1)]
    f = nzcb.ptau_check(spoiled, device=0)
    assert (f["status"], f["index"]) == ("SEQUENCE", m - 1), f
    out.append(f"    last point replaced by its neighbour: {f['status']} at {f['index']}, {f['pairing_checks']} pairing "
               f"checks, {nzcb.Engine.key_check_timings()[5]:.1f} ms")
    spoiled[g1 + 64 * edge + 3] ^= 0x40
    f = nzcb.ptau_check(spoiled, device=0)
    assert (f["status"], f["index"], f["n_bad"]) == ("CURVE", edge, 1), f
    out.append(f"    and a bit of point {edge} flipped: {f['status']} at {f['index']}, {f['n_bad']} defective")
    del spoiled

    if args.power == 21:
        r1cs, _, _ = nzcplive.build()
        t0 = time.perf_counter()
        ptr, size = nzcb.plonk_setup_raw(r1cs, ptau, device=0)
        setup_ms = (time.perf_counter() - t0) * 1e3
        zkey = nzcb._take(ptr, size)  # outside the timed call: a 3.9 GB host copy
        nzcb.free_ptr(ptr)
        say(f"plonk_setup: {setup_ms:.0f} ms")
        out += ["", f"nzcb_plonk_setup of the nzcp_live key (the yardstick): {setup_ms:.0f} ms wall, {len(zkey) >> 20} MiB"]
        nzcb.zkey_check(zkey, device=0)
        med, lo, hi, ph = timed(lambda: nzcb.zkey_check(zkey, device=0), args.reps, lambda r: r["ok"])
        report(out, "zkey_check of that key (n = 2^21, 11 parts)", args.reps, med, lo, hi, ph, (0, 1, 2, 3, 4, 6, 7, 8))
        out.append(f"    zkey_check / plonk_setup = {med / setup_ms:.3f}; ptau_check + zkey_check = {ptau_ms + med:.0f} ms")
        zbad = bytearray(zkey)
        del zkey
        lag, size = section(zbad, 13)
        zbad[lag + size - 32] ^= 1          # the last evaluation of the last Lagrange polynomial
        s14, _ = section(zbad, 14)
        n = 1 << 21
        zbad[s14 + 64 * (n + 5):s14 + 64 * (n + 6)] = zbad[s14 + 64 * (n + 4):s14 + 64 * (n + 5)]
        r = nzcb.zkey_check(zbad, device=0)
        last = list(r["parts"])[-1]
        bad = {k: v["status"] for k, v in r["parts"].items() if v["status"] != "OK"}
        assert not r["ok"] and bad == {last: "EVALS"} and r["parts"][last]["index"] == 4 * n - 1, r
        assert (r["srs"]["status"], r["srs"]["index"]) == ("SEQUENCE", n + 5), r["srs"]
        out.append(f"    last evaluation of {last} flipped, last PTau point replaced by its neighbour: {last} EVALS at "
                   f"{r['parts'][last]['index']}, PTau SEQUENCE at {r['srs']['index']} ({r['srs']['pairing_checks']} "
                   f"pairing checks), no commitment checked: {not any(p['commit_checked'] for p in r['parts'].values())}")
        del zbad

    host_ptau = nzcb.ptau_synth(12, TAU)
    t0 = time.perf_counter()
    f = nzcb.ptau_check(host_ptau, device=nzcb.KEY_HOST)
    host_ms = (time.perf_counter() - t0) * 1e3
    assert f["status"] == "OK"
    out += ["", f"host path (NZCB_KEY_HOST), power 12, {f['checked']} points, one thread: {host_ms:.0f} ms, "
                f"{host_ms * 1e3 / f['checked']:.1f} us per point"]
    out += ["", "kernel resource usage (gfx950, -Rpass-analysis=kernel-resource-usage):"] + resources(args.resources)
    text = "\n".join(out) + "\n"
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write(text)
    print(text, end="")
    return 0


if __name__ == "__main__":
    sys.exit(main())
