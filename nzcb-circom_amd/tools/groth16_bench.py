#!/usr/bin/env python3
"""Groth16 setup and zkey contribute (snarkjs's `phase2` recipe) at small sizes and for the
nzcp_live r1cs, in one process on device 0 and on the host path.

The powers-of-tau file of each size is made with this library's own new -> contribute (secrets
the tool chooses, so the trapdoor is known) -> prepare phase2, file to file in a temporary
directory. Per size: nzcb_groth16_setup_file and nzcb_groth16_contribute_file, the median wall
time of `--reps` runs (the host path at full size: one run) after a warm-up at a small size, the kernels' time by HIP events and the
term and chunk counts (nzcb_debug_groth16_timings), on device 0 and with NZCB_GROTH16_HOST; the
bytes of the two paths must be equal. The small sizes are seeded synthetic circuits with circom's
mix of coefficients; the full size is the r1cs tools/r1cs_check_bench.py builds (nzcb.nzcplive),
cirPower 20, on a power-20 file. At full size 64 seeded rows of the key (the longest ones among
them) are compared with a restatement from the trapdoor: the row's scalar summed in Fr over
L_c(tau) = w^c (tau^n - 1) / (n (tau - w^c)), then one multiplication of the generator
(oracle/bn254.py). Also the kernels' register use from -Rpass-analysis=kernel-resource-usage.
Writes profiles/groth16_setup.txt (or --out).

  python tools/groth16_bench.py [--out FILE] [--resources FILE] [--powers 12,16] [--reps 3] [--no-live]
"""
import argparse
import os
import random
import re
import statistics
import struct
import subprocess
import sys
import tempfile
import time

PKG = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ROOT = os.path.dirname(PKG)
sys.path[:0] = [ROOT, PKG]
import nzcb  # noqa: E402
from nzcb import nzcplive  # noqa: E402
from oracle import bn254 as bn  # noqa: E402

R = bn.R_MOD
SECRETS = (0x6E7A63625F746175, 0x616C7068615F6E7A6362, 0x626574615F6E7A6362)  # tau, alpha, beta
DELTA = 0x6E7A63625F64656C7461


def say(msg):
    print(f"[groth16_bench] {msg}", file=sys.stderr, flush=True)


def resources(path):
    if path:
        text = open(path).read()
    else:
        cmd = [os.environ.get("HIPCC", "/opt/rocm/bin/hipcc"), "-O3", "-std=c++17", "--offload-arch=gfx950",
               "--cuda-device-only", "-Rpass-analysis=kernel-resource-usage", "-c",
               os.path.join(PKG, "csrc", "groth16.hip"), "-o", os.devnull]
        text = subprocess.run(cmd, capture_output=True, text=True, check=True).stderr
    rows = []
    for line in text.splitlines():
        m = re.search(r"remark:\s+(Function Name|VGPRs|AGPRs|ScratchSize \[bytes/lane\]|Occupancy \[waves/SIMD\]"
                      r"|VGPRs Spill|LDS Size \[bytes/block\]): (\S+)", line)
        if not m:
            continue
        if m.group(1) == "Function Name":
            name = re.search(r"\d+(k_g16_[a-z]+)(.*)", m.group(2))
            rows.append([(name.group(1) + ("<Fq2>" if "Fq2E" in name.group(2)[:24] else "<Fq>")) if name
                         else m.group(2)])
        elif rows:
            rows[-1].append(f"{m.group(1)} {m.group(2)}")
    return ["  " + r[0] + ": " + ", ".join(r[1:]) for r in rows]


def synthetic_r1cs(m: int, seed: int) -> bytes:
    """m constraints over m + 8 wires (2 outputs, 2 public inputs): A of 1-3 terms, B of 1-2, C of
    1-2, wire 0 in a third of them; coefficients mostly 1 and -1, some small powers of two, one in
    sixteen random."""
    rng = random.Random(seed)
    n_wires = m + 8
    le = lambda v: (v % R).to_bytes(32, "little")
    one, minus = le(1), le(-1)

    def coef():
        k = rng.randrange(16)
        return one if k < 8 else minus if k < 12 else le(1 << rng.randrange(1, 9)) if k < 15 else le(rng.randrange(R))

    body = bytearray()
    for i in range(m):
        for hi in (3, 2, 2):
            wires = [rng.randrange(1, n_wires) for _ in range(rng.randrange(1, hi + 1))]
            if rng.randrange(3) == 0:
                wires.append(0)
            body += struct.pack("<I", len(wires))
            for w in wires:
                body += struct.pack("<I", w) + coef()
    hdr = struct.pack("<I", 32) + R.to_bytes(32, "little") + struct.pack("<IIIIQI", n_wires, 2, 2, 4, n_wires, m)
    out = bytearray(b"r1cs") + struct.pack("<II", 1, 2)
    for sid, payload in ((1, hdr), (2, bytes(body))):
        out += struct.pack("<IQ", sid, len(payload)) + payload
    return bytes(out)


def make_ptau(power: int, d: str) -> str:
    p0, p1, p2 = (os.path.join(d, f"pot{power}_{k}.ptau") for k in range(3))
    nzcb.ptau_new(power, p0)
    nzcb.ptau_contribute(p0, p1, secrets=SECRETS, device=0)
    os.remove(p0)
    nzcb.ptau_prepare_phase2(p1, p2, device=0)
    os.remove(p1)
    return p2


def timed(fn, reps):
    walls, stats = [], []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        walls.append((time.perf_counter() - t0) * 1e3)
        stats.append(nzcb.groth16_timings())
    mid = sorted(range(reps), key=lambda i: walls[i])[reps // 2]
    return statistics.median(walls), min(walls), max(walls), stats[mid]


def measure(label, r1cs_path, ptau_path, d, dev_reps, host_reps, out):
    """setup and contribute on the device and on the host; returns the device's fresh key's path"""
    keys = {}
    for name, device, reps in (("device 0", 0, dev_reps),
                               ("host path (NZCB_GROTH16_HOST, up to 16 threads)", nzcb.GROTH16_HOST, host_reps)):
        z0, z1 = (os.path.join(d, f"{label}_{device}_{k}.zkey") for k in range(2))
        med, lo, hi, t = timed(lambda: nzcb.groth16_setup(r1cs_path, ptau_path, z0, device=device), reps)
        if device == 0:
            out.append(f"  terms: A {t['terms_A']:.0f}, B1 {t['terms_B1']:.0f}, B2 {t['terms_B2']:.0f}, K {t['terms_K']:.0f}; "
                       f"chunks: G1 run {t['chunks_g1']:.0f}, G2 run {t['chunks_g2']:.0f}; "
                       f"zkey {os.path.getsize(z0) >> 10} KiB")
        out.append(f"  {name}:")
        out.append(f"    setup:      median {med:9.1f} ms wall of {reps} (min {lo:.1f}, max {hi:.1f}); kernels {t['kernels_ms']:8.1f} ms "
                   f"(G1 rows {t['rows_g1_ms']:.1f}, G2 rows {t['rows_g2_ms']:.1f}, point tests {t['tests_ms']:.1f}); "
                   f"host lists and schedule {t['plan_ms']:.1f} ms")
        say(out[-1])
        med, lo, hi, t = timed(lambda: nzcb.groth16_contribute(z0, z1, secret=DELTA, device=device), reps)
        out.append(f"    contribute: median {med:9.1f} ms wall of {reps} (min {lo:.1f}, max {hi:.1f}); kernels {t['kernels_ms']:8.1f} ms "
                   f"(scaling {t['scale_ms']:.1f}, point tests {t['tests_ms']:.1f})")
        say(out[-1])
        keys[device] = (z0, z1)
    for a, b in zip(keys[0], keys[nzcb.GROTH16_HOST]):
        with open(a, "rb") as fa, open(b, "rb") as fb:
            while True:
                x, y = fa.read(1 << 24), fb.read(1 << 24)
                assert x == y, "device and host bytes differ"
                if not x:
                    break
    out.append("  device bytes == host bytes (setup and contribute)")
    for p in keys[nzcb.GROTH16_HOST] + keys[0][1:]:
        os.remove(p)
    return keys[0][0]


# ---------------------------------------------------------------- the restatement at full size
def read_sections(path, magic):
    with open(path, "rb") as f:
        head = f.read(12)
        assert head[:4] == magic
        n_sec = struct.unpack_from("<I", head, 8)[0]
        sec, off = {}, 12
        for _ in range(n_sec):
            f.seek(off)
            sid, size = struct.unpack("<IQ", f.read(12))
            sec[sid] = (off + 12, size)
            off += 12 + size
    return sec


def r1cs_layout(r1cs: bytes):
    """(offset of the constraints, n_wires, n_out, n_pub_in, m)"""
    sec = {}
    off = 12
    for _ in range(struct.unpack_from("<I", r1cs, 8)[0]):
        sid, size = struct.unpack_from("<IQ", r1cs, off)
        sec[sid] = off + 12
        off += 12 + size
    n_wires, n_out, n_pub_in, _, _, m = struct.unpack_from("<IIIIQI", r1cs, sec[1] + 36)
    return sec[2], n_wires, n_out, n_pub_in, m


def check_rows(r1cs: bytes, zkey_path: str, power: int, count: int, out):
    """`count` seeded rows of the fresh key against scalars summed from the trapdoor."""
    tau, alpha, beta = SECRETS
    o, n_wires, n_out, n_pub_in, m = r1cs_layout(r1cs)
    n_pub = n_out + n_pub_in
    cp = max(1, (m + n_pub).bit_length())
    n = 1 << cp
    rng = random.Random(64)
    picks = {("A", 0), ("B1", 0), ("B2", 0), ("K", 0), ("K", n_pub), ("K", n_pub + 1), ("A", n_wires - 1)}
    while len(picks) < count - 8:
        picks.add((rng.choice(("A", "B1", "B2", "K")), rng.randrange(n_wires)))
    wires = {s for _, s in picks}
    rows = {p: [] for p in picks}   # (constraint, coefficient, which Lagrange family)
    unpack_u32 = struct.Struct("<I").unpack_from
    for c in range(m):
        for lc in range(3):
            nt, = unpack_u32(r1cs, o)
            o += 4
            for _ in range(nt):
                s, = unpack_u32(r1cs, o)
                if s in wires:
                    v = int.from_bytes(r1cs[o + 4:o + 36], "little")
                    if lc == 0:
                        for key, fam in ((("A", s), 1), (("K", s), beta)):
                            if key in rows:
                                rows[key].append((c, v * fam))
                    elif lc == 1:
                        for key, fam in ((("B1", s), 1), (("B2", s), 1), (("K", s), alpha)):
                            if key in rows:
                                rows[key].append((c, v * fam))
                    elif ("K", s) in rows:
                        rows[("K", s)].append((c, v))
                o += 36
    for (g, s), terms in rows.items():
        if s <= n_pub and g in ("A", "K"):
            terms.append((m + s, 1 if g == "A" else beta))
    # L_c(tau) for every constraint that occurs, with one inversion
    w = bn.FR_W[cp]
    cs = sorted({c for terms in rows.values() for c, _ in terms})
    wc = [pow(w, c, R) for c in cs]
    dens = [(tau - x) % R for x in wc]
    pref = [1]
    for x in dens:
        pref.append(pref[-1] * x % R)
    inv = bn.fr_inv(pref[-1])
    zn = (pow(tau, n, R) - 1) * bn.fr_inv(n) % R
    lag = {}
    for i in range(len(cs) - 1, -1, -1):
        lag[cs[i]] = wc[i] * zn % R * (inv * pref[i] % R) % R
        inv = inv * dens[i] % R
    zsec = read_sections(zkey_path, b"zkey")
    longest = 0
    with open(zkey_path, "rb") as f:
        def point(sid, index, width):
            f.seek(zsec[sid][0] + width * index)
            return f.read(width)
        for (g, s), terms in sorted(rows.items()):
            scalar = sum(v * lag[c] for c, v in terms) % R
            longest = max(longest, len(terms))
            if g == "B2":
                assert point(7, s, 128) == bn.g2_to_lem(bn.g2_mul(bn.G2_GEN, scalar) if scalar else None), (g, s)
                continue
            sid, index = {"A": (5, s), "B1": (6, s)}.get(g) or ((3, s) if s <= n_pub else (8, s - n_pub - 1))
            assert point(sid, index, 64) == bn.g1_to_lem(bn.g1_mul(bn.G1_GEN, scalar)), (g, s)
        # H[i] = T[2 i + 1]: level cirPower + 1 of section 12, built from 2n - 1 points and the point
        # at infinity when cirPower is the file's power
        w2 = bn.FR_W[cp + 1]
        t2n = pow(tau, 2 * n, R)
        for i in [0, n - 1] + [rng.randrange(n) for _ in range(6)]:
            x = pow(w2, 2 * i + 1, R)
            scalar = x * (t2n - 1) % R * bn.fr_inv(2 * n * (tau - x) % R) % R
            if cp == power:
                scalar = (scalar - bn.fr_inv(2 * n) * x % R * pow(tau, 2 * n - 1, R)) % R
            assert point(9, i, 64) == bn.g1_to_lem(bn.g1_mul(bn.G1_GEN, scalar)), ("H", i)
    out.append(f"  {len(rows) + 8} seeded rows (A, B1, B2, IC, C and H; the longest has {longest} terms) equal the "
               "restatement from the trapdoor")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "groth16_setup.txt"))
    ap.add_argument("--resources", default=None)
    ap.add_argument("--powers", default="12,16")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--no-live", action="store_true")
    args = ap.parse_args()
    if nzcb.device_count() < 1:
        raise SystemExit("groth16_bench: no HIP device")
    powers = [int(p) for p in args.powers.split(",") if p]
    out = [f"groth16_bench: {nzcb.version()}", "ptau: new -> contribute -> prepare phase2 of this library on device 0; "
           "times are medians of whole file-to-file calls", ""]
    with tempfile.TemporaryDirectory() as d:
        def circuit_file(name, data):
            path = os.path.join(d, name + ".r1cs")
            with open(path, "wb") as f:
                f.write(data)
            return path
        measure("warm", circuit_file("warm", synthetic_r1cs(200, 1)), make_ptau(8, d), d, 1, 1, [])  # HIP start-up, code load
        for power in powers:
            m = (1 << power) - 8
            out.append(f"synthetic circuit, {m} constraints, {m + 8} wires, cirPower {power}, ptau power {power}:")
            ptau = make_ptau(power, d)
            os.remove(measure(f"p{power}", circuit_file(f"p{power}", synthetic_r1cs(m, power)), ptau, d, args.reps, args.reps, out))
            os.remove(ptau)
            out.append("")
        if not args.no_live:
            r1cs, _, _ = nzcplive.build()
            _, n_wires, _, _, m = r1cs_layout(r1cs)
            out.append(f"nzcp_live r1cs ({len(r1cs) >> 20} MiB): {m} constraints, {n_wires} wires, cirPower 20, ptau power 20:")
            t0 = time.perf_counter()
            ptau = make_ptau(20, d)
            out.append(f"  (the prepared ptau: {(time.perf_counter() - t0):.1f} s, {os.path.getsize(ptau) >> 20} MiB)")
            fresh = measure("live", circuit_file("live", r1cs), ptau, d, args.reps, 1, out)
            t0 = time.perf_counter()
            check_rows(r1cs, fresh, 20, 64, out)
            say(f"row check {(time.perf_counter() - t0):.1f} s")
            out.append("")
    out += ["kernel resource usage (gfx950, -Rpass-analysis=kernel-resource-usage):"] + resources(args.resources)
    text = "\n".join(out) + "\n"
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write(text)
    print(text, end="")
    return 0


if __name__ == "__main__":
    sys.exit(main())
