#!/usr/bin/env python3
"""Batch ECDSA P-256 verification (nzcb.P256Key) in one process on device 0.

128 distinct valid signatures under one key are made with the exact-integer oracle of
tests/p256_cases.py and tiled to the batch sizes. After a warm-up call, for each window width
(4 and 8): the table build (kernel, HIP events, and the nzcb_p256_key_create call), then
verify_dev over HBM-resident digests and signatures at count = 1, 64, 512, 4096 and 65536 (one wave
per SIMD of an MI355X; median of 5
wall times with the kernel's HIP-event time of nzcb_debug_p256_timings); every status is checked.
Then the host path for 64, Node's crypto.verify (OpenSSL, one host core) over the same 512
signatures for scale, the share of the kernel that is the inversion of s (operation counts, and
the two window widths' kernel times solved for it), and the kernels' register use from
-Rpass-analysis=kernel-resource-usage. Writes profiles/p256_verify.txt (or --out).

  python tools/p256_verify_bench.py [--out FILE] [--resources FILE] [--counts 1,64,512,4096,65536]

--resources: the compiler's remark text captured earlier (hipcc ... --cuda-device-only
-Rpass-analysis=kernel-resource-usage -c csrc/p256_verify.hip 2> FILE) instead of compiling here.
"""
import argparse
import hashlib
import json
import os
import random
import re
import shutil
import statistics
import subprocess
import sys
import tempfile
import time

PKG = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ROOT = os.path.dirname(PKG)
sys.path[:0] = [ROOT, PKG, os.path.join(ROOT, "tests")]
import nzcb  # noqa: E402
import p256_cases as C  # noqa: E402

WINDOWS = (4, 8)
POOL = 128
MIXED_ADD_PRODUCTS = 11   # csrc/p256.h jac_add_affine: 3 squarings and 8 products in F_p

NODE_SCRIPT = """
const crypto = require('crypto');
const d = JSON.parse(require('fs').readFileSync(process.argv[1], 'utf8'));
const der = Buffer.concat([Buffer.from('3059301306072a8648ce3d020106082a8648ce3d03010703420004', 'hex'),
  Buffer.from(d.key, 'hex')]);
const key = crypto.createPublicKey({ key: der, format: 'der', type: 'spki' });
const msgs = d.msgs.map((m) => Buffer.from(m, 'hex'));
const sigs = d.sigs.map((s) => Buffer.from(s, 'hex'));
const run = () => {
  let ok = 0;
  for (let i = 0; i < d.count; i++) {
    if (crypto.verify('sha256', msgs[i % msgs.length], { key, dsaEncoding: 'ieee-p1363' }, sigs[i % sigs.length])) ok++;
  }
  return ok;
};
run();
const times = [];
let ok = 0;
for (let r = 0; r < 5; r++) {
  const t0 = process.hrtime.bigint();
  ok = run();
  times.push(Number(process.hrtime.bigint() - t0) / 1e6);
}
times.sort((a, b) => a - b);
console.log(JSON.stringify({ ok, median: times[2], min: times[0], max: times[4], node: process.version,
  openssl: process.versions.openssl }));
"""


def resources(path):
    if path:
        text = open(path).read()
    else:
        cmd = [os.environ.get("HIPCC", "/opt/rocm/bin/hipcc"), "-O3", "-std=c++17", "--offload-arch=gfx950",
               "--cuda-device-only", "-Rpass-analysis=kernel-resource-usage", "-c",
               os.path.join(PKG, "csrc", "p256_verify.hip"), "-o", os.devnull]
        text = subprocess.run(cmd, capture_output=True, text=True, check=True).stderr
    rows = []
    for line in text.splitlines():
        m = re.search(r"remark:\s+(Function Name|VGPRs|AGPRs|ScratchSize \[bytes/lane\]|Occupancy \[waves/SIMD\]"
                      r"|VGPRs Spill|LDS Size \[bytes/block\]): (\S+)", line)
        if not m:
            continue
        if m.group(1) == "Function Name":
            name = re.search(r"(k_p256_[a-z0-9]+)E", m.group(2))
            rows.append([name.group(1) if name else m.group(2)])
        elif rows:
            rows[-1].append(f"{m.group(1)} {m.group(2)}")
    return ["  " + r[0] + ": " + ", ".join(r[1:]) for r in rows]


def signatures():
    """(Q, messages, digests, signatures): POOL valid signatures under one seeded key."""
    rng = random.Random(0xB256)
    d = rng.randrange(1, C.N)
    msgs = [f"p256 verify bench {i}".encode() for i in range(POOL)]
    hashes = [hashlib.sha256(m).digest() for m in msgs]
    return C.mul(d, C.G), msgs, hashes, [C.sign(d, z, rng.randrange(1, C.N)) for z in hashes]


def timed_verify(key, d_h, d_s, count, reps=5):
    walls, kernels = [], []
    for _ in range(reps):
        t0 = time.perf_counter()
        st = key.verify_dev(d_h, 32, d_s, 64, count)
        walls.append((time.perf_counter() - t0) * 1e3)
        kernels.append(nzcb.P256Key.timings()[1])
        assert st == [C.OK] * count, "a signature of the batch does not verify"
    return statistics.median(walls), min(walls), max(walls), statistics.median(kernels)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "p256_verify.txt"))
    ap.add_argument("--resources", default=None)
    ap.add_argument("--counts", default="1,64,512,4096,65536")
    args = ap.parse_args()
    counts = [int(x) for x in args.counts.split(",")]
    top = max(counts + [512])
    q, msgs, hashes, sigs = signatures()
    tiled_h = b"".join(hashes[i % POOL] for i in range(top))
    tiled_s = b"".join(sigs[i % POOL] for i in range(top))
    d_h, d_s = nzcb.dev_alloc(len(tiled_h)), nzcb.dev_alloc(len(tiled_s))
    nzcb.h2d(d_h, tiled_h)
    nzcb.h2d(d_s, tiled_s)
    out = [f"p256_verify_bench: {nzcb.version()}",
           f"{POOL} distinct valid signatures under one key, tiled to the batch; digests and signatures in HBM", ""]
    warm = nzcb.P256Key(C.xy(q), device=0)            # warm-up: HIP start-up, code load
    warm.verify_dev(d_h, 32, d_s, 64, 1)
    warm.close()
    kernel_at = {}
    for w in WINDOWS:
        builds, calls = [], []
        for _ in range(5):
            t0 = time.perf_counter()
            key = nzcb.P256Key(C.xy(q), device=0, window=w)
            calls.append((time.perf_counter() - t0) * 1e3)
            builds.append(nzcb.P256Key.timings()[0])
            key.close()
        key = nzcb.P256Key(C.xy(q), device=0, window=w)
        windows = (256 + w - 1) // w
        out.append(f"window {w}: {windows} additions per base, tables 2 x {(windows << w) * 64 >> 10} KiB; table build "
                   f"kernel {statistics.median(builds):.3f} ms, nzcb_p256_key_create {statistics.median(calls):.3f} ms "
                   "(medians of 5)")
        for n in counts:
            med, lo, hi, k = timed_verify(key, d_h, d_s, n)
            kernel_at[(w, n)] = k
            out.append(f"    verify_dev, count {n:5d}: kernel {k:8.3f} ms ({k / n * 1e3:9.2f} us per signature, "
                       f"{n / k:8.1f} signatures/ms); call median {med:.3f} ms of 5 (min {lo:.3f}, max {hi:.3f})")
        key.close()
    # the host path, at both widths
    out.append("")
    for w in WINDOWS:
        t0 = time.perf_counter()
        host = nzcb.P256Key(C.xy(q), device=nzcb.P256_HOST, window=w)
        build_ms = (time.perf_counter() - t0) * 1e3
        t0 = time.perf_counter()
        st = host.verify(hashes[:64], sigs[:64])
        host_ms = (time.perf_counter() - t0) * 1e3
        host.close()
        assert st == [C.OK] * 64
        out.append(f"host path (NZCB_P256_HOST), window {w}, one thread: tables {build_ms:.1f} ms, 64 signatures "
                   f"{host_ms:.1f} ms ({host_ms / 64 * 1e3:.0f} us per signature)")
    # OpenSSL through Node, for scale
    out.append("")
    if shutil.which("node"):
        with tempfile.NamedTemporaryFile("w", suffix=".json", delete=False) as f:
            json.dump({"key": C.xy(q).hex(), "msgs": [m.hex() for m in msgs], "sigs": [s.hex() for s in sigs],
                       "count": 512}, f)
        try:
            p = subprocess.run(["node", "-e", NODE_SCRIPT, f.name], capture_output=True, text=True, check=True)
        finally:
            os.unlink(f.name)
        d = json.loads(p.stdout)
        assert d["ok"] == 512, "OpenSSL rejects a signature of the pool"
        out.append(f"Node {d['node']} crypto.verify (OpenSSL {d['openssl']}, one host core, SHA-256 included), the same "
                   f"512: median {d['median']:.1f} ms of 5 (min {d['min']:.1f}, max {d['max']:.1f}), "
                   f"{d['median'] / 512 * 1e3:.0f} us per signature")
    else:
        out.append("node is not installed: no OpenSSL figure")
    # the inversion's share
    inv = 256 + bin(C.N - 2).count("1")
    out += ["", f"products per signature (operation counts): 1 / s by Fermat in F_n = 256 squarings + "
                f"{bin(C.N - 2).count('1')} products = {inv}, with to_mont, u1 and u2: {inv + 3};"]
    for w in WINDOWS:
        windows = (256 + w - 1) // w
        adds = 2 * windows * (1 - 2.0 ** -w)
        fp = adds * MIXED_ADD_PRODUCTS + 3
        out.append(f"    window {w}: {adds:.1f} mixed additions (zero windows skipped) x {MIXED_ADD_PRODUCTS} + 3 = "
                   f"{fp:.0f} in F_p; the inversion is {inv / (inv + 3 + fp) * 100:.0f} % of the products")
    n = 64
    if (4, n) in kernel_at and (8, n) in kernel_at:
        # one wave per workgroup and fewer waves than SIMDs: the kernel's time is one wave's latency
        a4 = 2 * 64 * (1 - 2.0 ** -4)
        a8 = 2 * 32 * (1 - 2.0 ** -8)
        per_add = (kernel_at[(4, n)] - kernel_at[(8, n)]) / (a4 - a8)
        rest = kernel_at[(8, n)] - a8 * per_add
        out.append(f"    measured at count {n} (one wave, its latency): kernel(4) - kernel(8) over {a4 - a8:.1f} additions "
                   f"gives {per_add * 1e3:.1f} us per mixed addition; what is not table additions (mostly 1 / s) is "
                   f"{rest:.3f} ms = {rest / kernel_at[(8, n)] * 100:.0f} % of the window-8 kernel, "
                   f"{rest / kernel_at[(4, n)] * 100:.0f} % of the window-4 kernel")
    ref = 512 if (4, 512) in kernel_at and (8, 512) in kernel_at else n
    if (4, ref) in kernel_at and (8, ref) in kernel_at:
        best = min(WINDOWS, key=lambda w: kernel_at[(w, ref)])
        other = 4 if best == 8 else 8
        out += ["", f"default window: {best} is the faster at every count here (count {ref}: "
                    f"{kernel_at[(best, ref)]:.3f} ms against {kernel_at[(other, ref)]:.3f} ms at window {other}); "
                    "the table build is paid once per key object"
                if all(kernel_at[(best, c)] < kernel_at[(other, c)] for c in counts) else
                f"default window: {best} is the faster at count {ref} ({kernel_at[(best, ref)]:.3f} ms against "
                f"{kernel_at[(other, ref)]:.3f} ms at window {other}), not at every count"]
    out += ["", "kernel resource usage (gfx950, -Rpass-analysis=kernel-resource-usage):"] + resources(args.resources)
    nzcb.dev_free(d_h)
    nzcb.dev_free(d_s)
    text = "\n".join(out) + "\n"
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)
    print(text, end="")
    return 0


if __name__ == "__main__":
    sys.exit(main())
