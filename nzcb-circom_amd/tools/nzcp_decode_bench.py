#!/usr/bin/env python3
"""Pass decode (nzcb.nzcp_decode, csrc/nzcp_decode.hip) in one process on device 0.

128 distinct MoH-shaped passes (names of varying length, each signed under one seeded key with the
exact-integer oracle of tests/p256_cases.py) are tiled to the batch sizes. After a warm-up call, at
count = 1, 64, 512, 4096 and 65536:

* nzcb_nzcp_decode over host buffers, records only: the kernel (HIP events) and the call (URI bytes
  up, kernel, records down), medians of 5, from nzcb_debug_nzcp_decode_timings;
* the same with the live circuit's input blocks (95 KB per pass written by the kernel and copied
  down), up to --inputs-max passes (the host copy of 65,536 blocks would be 6.2 GB);
* the host path (NZCB_NZCP_HOST), one core;
* the per-pass host loop that verify_passes runs in front of the signature kernel (decode_pass,
  protected_header, cbor_decode, sig_structure, hashlib.sha256), and nzcp.input_signals, one core;
* end to end: P256Key.verify_uris against P256Key.verify_passes, same URIs, same box. With
  --parent-lib the verify_passes side also runs in a child process on that library (the parent
  commit's build), so the comparison is against the parent's code, not only its Python.

Every record and verdict is checked. Writes profiles/nzcp_decode.txt (or --out).

  python tools/nzcp_decode_bench.py [--out FILE] [--resources FILE] [--parent-lib libnzcb.so]
                                    [--counts 1,64,512,4096,65536] [--inputs-max 4096]

--resources: the compiler's remark text captured earlier (hipcc ... --cuda-device-only
-Rpass-analysis=kernel-resource-usage -c csrc/nzcp_decode.hip 2> FILE) instead of compiling here.
"""
import argparse
import hashlib
import json
import os
import random
import re
import statistics
import subprocess
import sys
import time

PKG = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ROOT = os.path.dirname(PKG)
sys.path[:0] = [ROOT, PKG, os.path.join(ROOT, "tests")]
import nzcb  # noqa: E402
import p256_cases as P  # noqa: E402
from nzcb import nzcp  # noqa: E402

POOL = 128


def resources(path):
    if path:
        text = open(path).read()
    else:
        cmd = [os.environ.get("HIPCC", "/opt/rocm/bin/hipcc"), "-O3", "-std=c++17", "--offload-arch=gfx950",
               "--cuda-device-only", "-Rpass-analysis=kernel-resource-usage", "-c",
               os.path.join(PKG, "csrc", "nzcp_decode.hip"), "-o", os.devnull]
        text = subprocess.run(cmd, capture_output=True, text=True, check=True).stderr
    rows = []
    for line in text.splitlines():
        m = re.search(r"remark:\s+(Function Name|TotalSGPRs|VGPRs|AGPRs|ScratchSize \[bytes/lane\]"
                      r"|Occupancy \[waves/SIMD\]|SGPRs Spill|VGPRs Spill|LDS Size \[bytes/block\]): (\S+)", line)
        if not m:
            continue
        if m.group(1) == "Function Name":
            name = re.search(r"(k_nzcp_[a-z0-9_]+?)E", m.group(2))
            rows.append([name.group(1) if name else m.group(2)])
        elif rows:
            rows[-1].append(f"{m.group(1)} {m.group(2)}")
    return ["  " + r[0] + ": " + ", ".join(r[1:]) for r in rows]


def pool():
    """(public key Q, POOL pass URIs valid under it)."""
    import base64
    rng = random.Random(0x4E5A4350)
    d = rng.randrange(1, P.N)
    protected = nzcp.cbor_encode({4: nzcp.LIVE_KID, 1: -7})
    uris = []
    for i in range(POOL):
        subject = nzcp.credential_subject("G" * (1 + i % 9), "F" * (1 + i % 13), f"19{60 + i % 40}-04-16")
        payload = nzcp.cbor_encode(nzcp.claims(iss=nzcp.LIVE_ISS, subject=subject, jti=rng.randbytes(16)))
        z = hashlib.sha256(nzcp.sig_structure(protected, payload)).digest()
        cose = nzcp.cbor_encode(nzcp.Tag(18, [protected, {}, payload, P.sign(d, z, rng.randrange(1, P.N))]))
        uris.append("NZCP:/1/" + base64.b32encode(cose).decode().rstrip("="))
    return P.mul(d, P.G), uris


def tiled(uris, count):
    return [uris[i % len(uris)] for i in range(count)]


def med(xs):
    return statistics.median(xs), min(xs), max(xs)


def host_loop(uris):
    """What verify_passes does per pass before anything goes to the GPU."""
    for uri in uris:
        protected, payload, _sig = nzcp.decode_pass(uri)
        nzcp.protected_header(uri)
        nzcp.cbor_decode(payload)
        hashlib.sha256(nzcp.sig_structure(protected, payload)).digest()


def time_verify_passes(key, uris, reps):
    walls = []
    for _ in range(reps):
        t0 = time.perf_counter()
        got = key.verify_passes(uris)
        walls.append((time.perf_counter() - t0) * 1e3)
        assert all(g["valid"] for g in got), "a pass of the pool does not verify"
    return walls


def child(args):
    """verify_passes on whatever library NZCB_LIB names: one JSON line {count: [wall ms, ...]}."""
    q, uris = pool()
    key = nzcb.P256Key(P.xy(q), device=0)
    key.verify_passes(uris[:1])
    out = {}
    for n in [int(x) for x in args.counts.split(",")]:
        out[n] = time_verify_passes(key, tiled(uris, n), 5 if n <= 4096 else 2)
    key.close()
    print(json.dumps({"version": nzcb.version(), "lib": nzcb.LIB_PATH, "walls": out}))
    return 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "nzcp_decode.txt"))
    ap.add_argument("--resources", default=None)
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--counts", default="1,64,512,4096,65536")
    ap.add_argument("--inputs-max", type=int, default=4096)
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.child:
        return child(args)
    counts = [int(x) for x in args.counts.split(",")]
    q, uris = pool()
    size = nzcb.ctypes.sizeof(nzcb.NzcpPass)
    block = nzcb.nzcp_input_signals(nzcb.NZCP_LIVE) * 32
    want = {u: (hashlib.sha256(nzcp.to_be_signed(u)).digest(), len(nzcp.to_be_signed(u))) for u in uris}
    lens = sorted(len(u) for u in uris)
    out = [f"nzcp_decode_bench: {nzcb.version()}",
           f"{POOL} distinct MoH-shaped passes signed under one key, tiled to the batch; URIs of {lens[0]} to "
           f"{lens[-1]} bytes, ToBeSigned of {min(v[1] for v in want.values())} to "
           f"{max(v[1] for v in want.values())} bytes (live circuit: 351); one workgroup of 64 lanes per pass", ""]
    nzcb.nzcp_decode(uris[:1], device=0)     # warm-up: HIP start-up, code load

    def check(raw, batch):
        recs = [nzcb.NzcpPass.from_buffer_copy(raw[i * size:(i + 1) * size]) for i in range(0, len(batch), 61)]
        for r, u in zip(recs, batch[::61]):
            assert r.status == 0 and bytes(r.tbs_sha256) == want[u][0], "a record is wrong"

    out.append("nzcb_nzcp_decode on device 0, host buffers in and out (medians of 5; kernel by HIP events):")
    for with_inputs in (False, True):
        for n in counts:
            if with_inputs and n > args.inputs_max:
                out.append(f"    count {n:5d}, live inputs: not measured (the input blocks alone are "
                           f"{n * block / 2 ** 30:.1f} GiB)")
                continue
            print(f"decode, count {n}, inputs {with_inputs}", file=sys.stderr, flush=True)
            batch = tiled(uris, n)
            blob, offs = nzcb.pack_uris(batch)
            kernels, calls = [], []
            for _ in range(5):
                raw, inputs, _ = nzcb.nzcp_decode_raw(blob, nzcb.NZCP_LIVE if with_inputs else None, None, 0,
                                                      offsets=list(offs))
                k, c = nzcb.nzcp_decode_timings()
                kernels.append(k)
                calls.append(c)
                check(raw, batch)
                if with_inputs:
                    assert len(inputs) == block * n and inputs[32 * 2808] == want[batch[0]][1] & 0xFF
            k, c = med(kernels), med(calls)
            what = (f"records + live inputs ({n * block / 2 ** 20:8.1f} MiB)" if with_inputs else "records only")
            out.append(f"    count {n:5d}, {what}: kernel {k[0]:8.3f} ms ({k[0] / n * 1e3:8.2f} us per pass, "
                       f"{n / k[0]:9.1f} passes/ms"
                       + (f", {n * block / k[0] / 1e6:6.1f} GB/s written" if with_inputs else "")
                       + f"); call {c[0]:9.3f} ms (min {c[1]:.3f}, max {c[2]:.3f})")
        out.append("")
    # the host path of the library, one core
    for n, prm, what in ((4096, None, "records only"), (512, nzcb.NZCP_LIVE, "records + live inputs")):
        batch = tiled(uris, n)
        blob, offs = nzcb.pack_uris(batch)
        calls = []
        for _ in range(5):
            raw, _, _ = nzcb.nzcp_decode_raw(blob, prm, None, nzcb.NZCP_HOST, offsets=list(offs))
            calls.append(nzcb.nzcp_decode_timings()[1])
            check(raw, batch)
        c = med(calls)
        out.append(f"host path (NZCB_NZCP_HOST), one thread, {n} passes, {what}: {c[0]:.3f} ms "
                   f"({c[0] / n * 1e3:.2f} us per pass; min {c[1]:.3f}, max {c[2]:.3f})")
    # the interpreter loops the device route replaces
    batch = tiled(uris, 512)
    walls = []
    for _ in range(5):
        t0 = time.perf_counter()
        host_loop(batch)
        walls.append((time.perf_counter() - t0) * 1e3)
    w = med(walls)
    out.append(f"Python per-pass loop in front of the signature kernel (decode_pass, protected_header, cbor_decode, "
               f"sig_structure, sha256), one core, 512 passes: {w[0]:.1f} ms ({w[0] / 512 * 1e3:.0f} us per pass; min "
               f"{w[1]:.1f}, max {w[2]:.1f})")
    walls = []
    tbs = [nzcp.to_be_signed(u) for u in uris[:16]]
    for _ in range(5):
        t0 = time.perf_counter()
        for t in tbs:
            nzcp.input_signals(nzcp.circuit_input(t, bytes(20), nzcp.LIVE_TOBESIGNED_MAX))
        walls.append((time.perf_counter() - t0) * 1e3)
    w = med(walls)
    out += [f"Python nzcp.input_signals(nzcp.circuit_input(...)), one core, 16 passes: {w[0]:.1f} ms "
            f"({w[0] / 16 * 1e3:.0f} us per pass; min {w[1]:.1f}, max {w[2]:.1f})", ""]
    # end to end
    key = nzcb.P256Key(P.xy(q), device=0)
    key.verify_uris(uris[:1])
    key.verify_passes(uris[:1])
    parent = None
    if args.parent_lib:
        env = dict(os.environ, NZCB_LIB=os.path.abspath(args.parent_lib))
        p = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", "--counts", args.counts],
                           capture_output=True, text=True, env=env, check=True)
        parent = json.loads(p.stdout.splitlines()[-1])
        out.append(f"end to end, wall ms, same URIs; verify_passes also in a child process on the parent commit's "
                   f"library ({parent['version']}):")
    else:
        out.append("end to end, wall ms, same URIs (no --parent-lib: verify_passes on this library only; its code "
                   "path, Python and nzcb_p256_verify, is the parent commit's):")
    for n in counts:
        batch = tiled(uris, n)
        reps = 5 if n <= 4096 else 2
        print(f"end to end, count {n}", file=sys.stderr, flush=True)
        new, old = [], []
        for _ in range(reps):      # alternating
            t0 = time.perf_counter()
            got = key.verify_uris(batch)
            new.append((time.perf_counter() - t0) * 1e3)
            assert all(g["valid"] for g in got), "a pass of the pool does not verify"
            old += time_verify_passes(key, batch, 1)
        a, b = med(new), med(old)
        line = (f"    count {n:5d}: verify_uris {a[0]:10.2f} (min {a[1]:.2f}, max {a[2]:.2f}); verify_passes "
                f"{b[0]:10.2f} (min {b[1]:.2f}, max {b[2]:.2f})")
        if parent:
            c = med(parent["walls"][str(n)])
            line += f"; parent library {c[0]:10.2f} (min {c[1]:.2f}, max {c[2]:.2f})"
            b = c if c[0] < b[0] else b
        line += f"; median of {reps}; ratio {b[0] / a[0]:.1f}x" + ("" if a[0] < b[0] else "  <- the device route does NOT win here")
        out.append(line)
    key.close()
    out += ["", "kernel resource usage (gfx950, -Rpass-analysis=kernel-resource-usage):"] + resources(args.resources)
    text = "\n".join(out) + "\n"
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)
    print(text, end="")
    return 0


if __name__ == "__main__":
    sys.exit(main())
