#!/usr/bin/env python3
"""Batch verification against the single-proof verifier, in one process on device 0.

Proofs of the golden n = 2^8 circuit under distinct blindings (GPU prover), then, after a
warm-up call: nzcb.verify_batch at 64 and 512 items (median of 5, with the phases of
nzcb_debug_verify_batch_timings: host scalar preparation, the group sums and their two kernels
by HIP events, the pairing check), the same 64 items through the nzcb_verify loop (the
yardstick) and through the batch verifier's host path, and the kernels' register use from
-Rpass-analysis=kernel-resource-usage. Writes profiles/verify_batch.txt (or --out).

  python tools/verify_batch_bench.py [--out FILE] [--resources FILE]

--resources: the compiler's remark text captured earlier (hipcc ... --cuda-device-only
-Rpass-analysis=kernel-resource-usage -c csrc/verify_batch.hip 2> FILE) instead of compiling here.
"""
import argparse
import hashlib
import os
import re
import statistics
import subprocess
import sys
import time

PKG = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ROOT = os.path.dirname(PKG)
sys.path.insert(0, PKG)
import nzcb  # noqa: E402

R = 21888242871839275222246405745257275088548364400416034343698204186575808495617
PHASES = ("host scalars", "group sums (wall)", "term-mul kernel", "group-sum kernel", "pairing checks")


def blinding(k: int) -> bytes:
    return b"".join((int.from_bytes(hashlib.sha256(f"vb-bench {k} {j}".encode()).digest(), "big") % R)
                    .to_bytes(32, "little") for j in range(11))


def resources(path):
    if path:
        text = open(path).read()
    else:
        cmd = [os.environ.get("HIPCC", "/opt/rocm/bin/hipcc"), "-O3", "-std=c++17", "--offload-arch=gfx950",
               "--cuda-device-only", "-Rpass-analysis=kernel-resource-usage", "-c",
               os.path.join(PKG, "csrc", "verify_batch.hip"), "-o", os.devnull]
        text = subprocess.run(cmd, capture_output=True, text=True, check=True).stderr
    rows, name = [], None
    for line in text.splitlines():
        m = re.search(r"remark:\s+(Function Name|VGPRs|AGPRs|ScratchSize \[bytes/lane\]|Occupancy \[waves/SIMD\]"
                      r"|VGPRs Spill|LDS Size \[bytes/block\]): (\S+)", line)
        if not m:
            continue
        if m.group(1) == "Function Name":
            name = re.search(r"k_g1_[a-z_]+?(?=E)", m.group(2))
            name = name.group(0) if name else m.group(2)
            rows.append([name])
        else:
            rows[-1].append(f"{m.group(1)} {m.group(2)}")
    return ["  " + r[0] + ": " + ", ".join(r[1:]) for r in rows]


def timed_batch(vk, proofs, pubs, device, reps):
    walls, phases, checks = [], [], 0
    for _ in range(reps):
        t0 = time.perf_counter()
        ok = nzcb.verify_batch(vk, proofs, pubs, device=device)
        walls.append((time.perf_counter() - t0) * 1e3)
        assert all(ok), "a proof of the batch was rejected"
        t = nzcb.Engine.verify_batch_timings()
        phases.append(t[:5])
        checks = int(t[5])
    med = [statistics.median(p[k] for p in phases) for k in range(5)]
    return statistics.median(walls), min(walls), max(walls), med, checks


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "verify_batch.txt"))
    ap.add_argument("--resources", default=None)
    args = ap.parse_args()
    gold = os.path.join(ROOT, "tests", "golden")
    zkey = open(os.path.join(gold, "p8.zkey"), "rb").read()
    wtns = open(os.path.join(gold, "p8.wtns"), "rb").read()
    ctx = nzcb.ProverContext(zkey, device=0)
    t0 = time.perf_counter()
    items = [ctx.prove_raw(wtns, blinding(k)) for k in range(512)]
    prove_ms = (time.perf_counter() - t0) * 1e3
    ctx.close()
    vk = nzcb.vk_from_zkey(zkey)
    proofs, pubs = [p for p, _ in items], [u for _, u in items]
    out = [f"verify_batch_bench: {nzcb.version()}",
           f"512 proofs of the golden n = 2^8 circuit, distinct blindings: {prove_ms:.0f} ms on one lane", ""]
    nzcb.verify_batch(vk, proofs[:8], pubs[:8], device=0)  # warm-up: HIP start-up, code load
    for n in (64, 512):
        med, lo, hi, ph, checks = timed_batch(vk, proofs[:n], pubs[:n], 0, 5)
        out.append(f"verify_batch, {n} items, device 0: median {med:.2f} ms of 5 (min {lo:.2f}, max {hi:.2f}), "
                   f"{checks} pairing check(s), {med / n:.3f} ms per proof")
        out += [f"    {name:<20s} {v:9.3f} ms" for name, v in zip(PHASES, ph)]
        out.append(f"    {'other (Python, copies)':<20s} {med - ph[0] - ph[1] - ph[4]:7.3f} ms")
        if n == 64:
            gpu64 = med
    t0 = time.perf_counter()
    ok = [nzcb.verify(vk, p, u) for p, u in zip(proofs[:64], pubs[:64])]
    loop = (time.perf_counter() - t0) * 1e3
    assert all(ok)
    out.append(f"nzcb_verify loop, the same 64 items, host: {loop:.1f} ms ({loop / 64:.2f} ms per proof)")
    med, lo, hi, ph, checks = timed_batch(vk, proofs[:64], pubs[:64], nzcb.VERIFY_HOST, 1)
    out.append(f"verify_batch, 64 items, NZCB_VERIFY_HOST: {med:.1f} ms (group sums {ph[1]:.1f} ms, "
               f"pairing check {ph[4]:.1f} ms)")
    out.append(f"ratio, nzcb_verify loop / verify_batch on device 0 at 64 items: {loop / gpu64:.1f}")
    out.append("PASS: the batch of 64 on the GPU is faster than the loop" if gpu64 < loop else
               "FAIL: the batch of 64 on the GPU is not faster than the loop")
    out += ["", "kernel resource usage (gfx950, -Rpass-analysis=kernel-resource-usage):"] + resources(args.resources)
    text = "\n".join(out) + "\n"
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)
    print(text, end="")
    return 0 if gpu64 < loop else 1


if __name__ == "__main__":
    sys.exit(main())
