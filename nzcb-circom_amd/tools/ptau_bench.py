#!/usr/bin/env python3
"""The powers-of-tau operations (snarkjs's `phase1` recipe) at three sizes, in one process on
device 0.

Per power: nzcb_ptau_new_file, nzcb_ptau_contribute_file with drawn secrets and
nzcb_ptau_prepare_phase2_file, file to file in a temporary directory (a prepared power-21 file is
2.25 GiB), wall time and the kernels' time by HIP events (nzcb_debug_ptau_timings), one run each
after a warm-up at power 8; the existing nzcb_ptau_check must accept the contributed file. Beside
them the host path (NZCB_PTAU_HOST) at power 12, nzcb_ptau_synth at the largest power from the
same run (the yardstick for contribute's tauG1 share: one fixed-base multiplication per point),
and the kernels' register use from -Rpass-analysis=kernel-resource-usage. Writes
profiles/ptau_ops.txt (or --out).

  python tools/ptau_bench.py [--out FILE] [--resources FILE] [--powers 12,16,21]

--resources: the compiler's remark text captured earlier (hipcc ... --cuda-device-only
-Rpass-analysis=kernel-resource-usage -c csrc/ptau_ops.hip 2> FILE) instead of compiling here.
"""
import argparse
import os
import re
import subprocess
import sys
import tempfile
import time

PKG = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ROOT = os.path.dirname(PKG)
sys.path[:0] = [ROOT, PKG]
import nzcb  # noqa: E402

TAU = 0x6E7A6362746175


def resources(path):
    if path:
        text = open(path).read()
    else:
        cmd = [os.environ.get("HIPCC", "/opt/rocm/bin/hipcc"), "-O3", "-std=c++17", "--offload-arch=gfx950",
               "--cuda-device-only", "-Rpass-analysis=kernel-resource-usage", "-c",
               os.path.join(PKG, "csrc", "ptau_ops.hip"), "-o", os.devnull]
        text = subprocess.run(cmd, capture_output=True, text=True, check=True).stderr
    rows = []
    for line in text.splitlines():
        m = re.search(r"remark:\s+(Function Name|VGPRs|AGPRs|ScratchSize \[bytes/lane\]|Occupancy \[waves/SIMD\]"
                      r"|VGPRs Spill|LDS Size \[bytes/block\]): (\S+)", line)
        if not m:
            continue
        if m.group(1) == "Function Name":
            name = re.search(r"\d+(k_(?:pt|intt)_[a-z]+)(.*)", m.group(2))
            group = "" if not name or "twiddles" in name.group(1) else ("<Fq2>" if "Fq2E" in name.group(2)[:24] else "<Fq>")
            rows.append([(name.group(1) + group) if name else m.group(2)])
        elif rows:
            rows[-1].append(f"{m.group(1)} {m.group(2)}")
    return ["  " + r[0] + ": " + ", ".join(r[1:]) for r in rows]


def say(msg):
    print(f"[ptau_bench] {msg}", file=sys.stderr, flush=True)


def timed(fn):
    t0 = time.perf_counter()
    fn()
    wall = (time.perf_counter() - t0) * 1e3
    return wall, nzcb.ptau_timings()[0]


def recipe(power, device, d, out):
    p0, p1, p2 = (os.path.join(d, f"pot{power}_{k}.ptau") for k in range(3))
    t0 = time.perf_counter()
    nzcb.ptau_new(power, p0)
    out.append(f"  new:            {(time.perf_counter() - t0) * 1e3:9.1f} ms wall (host), {os.path.getsize(p0) >> 10} KiB")
    wall, kern = timed(lambda: nzcb.ptau_contribute(p0, p1, entropy="ptau_bench", device=device))
    out.append(f"  contribute:     {wall:9.1f} ms wall, kernels {kern:9.1f} ms ({5 << power} scalar multiplications)")
    say(out[-1])
    if device >= 0:
        f = nzcb.ptau_check(p1, device=device)
        assert f["status"] == "OK", f
    wall, kern = timed(lambda: nzcb.ptau_prepare_phase2(p1, p2, device=device))
    out.append(f"  prepare phase2: {wall:9.1f} ms wall, kernels {kern:9.1f} ms, {os.path.getsize(p2) >> 10} KiB")
    say(out[-1])
    for p in (p0, p1, p2):
        os.remove(p)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ptau_ops.txt"))
    ap.add_argument("--resources", default=None)
    ap.add_argument("--powers", default="12,16,21")
    args = ap.parse_args()
    powers = [int(p) for p in args.powers.split(",")]
    out = [f"ptau_bench: {nzcb.version()}", ""]
    with tempfile.TemporaryDirectory() as d:
        recipe(8, 0, d, [])  # warm-up: HIP start-up, code load
        for power in powers:
            out.append(f"power {power}, device 0:")
            recipe(power, 0, d, out)
        out += ["", "power 12, host path (NZCB_PTAU_HOST, up to 16 threads):"]
        recipe(12, nzcb.PTAU_HOST, d, out)
    t0 = time.perf_counter()
    synth = nzcb.ptau_synth(max(powers), TAU)
    out += ["", f"nzcb_ptau_synth, power {max(powers)} (tauG1 by the fixed-base kernel, two G2 points on the host): "
                f"{(time.perf_counter() - t0) * 1e3:.0f} ms wall, {len(synth) >> 20} MiB"]
    out += ["", "kernel resource usage (gfx950, -Rpass-analysis=kernel-resource-usage):"] + resources(args.resources)
    text = "\n".join(out) + "\n"
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write(text)
    print(text, end="")
    return 0


if __name__ == "__main__":
    sys.exit(main())
