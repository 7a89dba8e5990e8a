"""Shared cases of the key material check's tests (tests/test_key_check.py on the host path,
tests/test_gpu_key_check.py on the device): powers-of-tau point lists with a known tau, the
finding and the two weighted sums they must give in exact integers, and ways to spoil ptau and
zkey bytes."""
import functools
import math
import os
import random
import struct

from oracle import binfmt, bn254 as bn, keccak, pairing

P, R = bn.P_MOD, bn.R_MOD
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")

SEED = bytes((7 * i + 3) & 0xFF for i in range(32))
TAU = 0x6E7A63625F746175  # the trapdoor of the tests' files
TAU2 = 0x5EC0D7A0  # "another ceremony"
BAD_INDICES = (0, 1, 7, 8, -2, -1)  # with chunk_points = 8 on both sides of a chunk edge


# ---------------------------------------------------------------- points and encodings
@functools.lru_cache(maxsize=None)
def powers(tau: int, m: int, first=bn.G1_GEN):
    """[tau^i] first for i < m, affine."""
    out, t = [], 1
    for _ in range(m):
        out.append(bn.g1_mul(first, t))
        t = t * tau % R
    return tuple(out)


def raw_points(tau: int, m: int) -> list:
    """The m stored points, 64 bytes each (x || y, LE Montgomery)."""
    return [bn.g1_to_lem(p) for p in powers(tau, m)]


def g2_of(tau: int) -> bytes:
    return bn.g2_to_lem(bn.g2_mul(bn.G2_GEN, tau))


G2_ONE = bn.g2_to_lem(bn.G2_GEN)


def _fq2_sqrt(a):
    """A square root in Fq2 = Fq[u]/(u^2 + 1), q = 3 mod 4, or None."""
    if a == (0, 0):
        return a
    a1 = pairing.fq2_pow(a, (P - 3) // 4)
    x0 = bn.fq2_mul(a1, a)
    alpha = bn.fq2_mul(a1, x0)
    if alpha == (P - 1, 0):
        x = bn.fq2_mul((0, 1), x0)
    else:
        b = pairing.fq2_pow(bn.fq2_add((1, 0), alpha), (P - 1) // 2)
        x = bn.fq2_mul(b, x0)
    return x if bn.fq2_mul(x, x) == a else None


@functools.lru_cache(maxsize=None)
def g2_outside_subgroup() -> bytes:
    """A point of the twist that [r] does not send to infinity: a seeded search for x in Fq2 with
    a square x^3 + b' (the twist's cofactor is 2q - r, so nearly every such point will do)."""
    rng = random.Random(0x62D2)
    while True:
        x = (rng.randrange(P), rng.randrange(P))
        y = _fq2_sqrt(bn.fq2_add(bn.fq2_mul(bn.fq2_mul(x, x), x), bn.G2_B))
        if y is None:
            continue
        pt = (x, y)
        assert bn.g2_is_on_curve(pt)
        if _g2_mul(pt, R) is not None:
            return bn.g2_to_lem(pt)


def _g2_mul(pt, k: int):
    """k * pt without reducing k mod r (bn.g2_mul is for points of the subgroup)."""
    acc = None
    for bit in bin(k)[2:]:
        if acc is not None:
            acc = bn.g2_double(acc)
        if bit == "1":
            acc = pt if acc is None else bn.g2_add(acc, pt)
    return acc


def g2_off_twist() -> bytes:
    (x0, x1), (y0, y1) = bn.g2_mul(bn.G2_GEN, TAU)
    return bn.g2_to_lem(((x0, x1), ((y0 + 1) % P, y1)))


# ---------------------------------------------------------------- defects of one point list
def spoil_range(pts: list, k: int):
    pts[k] = bn.to_le(P) + bn.to_le((1 << 256) - 1)


def spoil_y(pts: list, k: int):
    x, y = bn.g1_from_lem(pts[k])
    pts[k] = bn.g1_to_lem((x, (y + 1) % P))


def spoil_zero(pts: list, k: int):
    pts[k] = bytes(64)


def spoil_other_point(pts: list, k: int):
    pts[k] = bn.g1_to_lem(bn.g1_mul(bn.G1_GEN, 0xBADC0FFEE + k))


def spoil_swap(pts: list, k: int):
    pts[k], pts[k + 1] = pts[k + 1], pts[k]


def spoil_tail(pts: list, k: int):
    """From k on the powers of another tau, continuing from the last good point."""
    first = bn.g1_from_lem(pts[k - 1]) if k else bn.G1_GEN
    tail = powers(TAU2, len(pts) - k + 1, first)
    pts[k:] = [bn.g1_to_lem(p) for p in tail[1:]] if k else [bn.g1_to_lem(p) for p in tail[:-1]]


# ---------------------------------------------------------------- expectations in exact integers
def weight(seed: bytes, i: int) -> int:
    rho = int.from_bytes(keccak.keccak256(seed + struct.pack("<I", i)), "big") & ((1 << 128) - 1)
    return rho or 1


def expected_lr(pts: list, seed: bytes) -> bytes:
    """L || R over the whole range: affine, 32-byte LE normal form, zeros for infinity."""
    aff = [bn.g1_from_lem(b) for b in pts]
    rho = [weight(seed, i) for i in range(len(aff) - 1)]

    def enc(pt):
        return bytes(64) if pt is None else bn.to_le(pt[0]) + bn.to_le(pt[1])
    return enc(bn.msm(aff[:-1], rho)) + enc(bn.msm(aff[1:], rho))


def _stored(b: bytes):
    return [bn.from_le(b[i:i + 32]) for i in range(0, len(b), 32)]


def _g2_defective(g2: bytes) -> bool:
    if any(v >= P for v in _stored(g2)):
        return True
    pt = bn.g2_from_lem(g2)
    return pt is None or not bn.g2_is_on_curve(pt) or _g2_mul(pt, R) is not None


def expected_finding(pts: list, g2: bytes, tau_of_g2: int, g2_first: bytes = G2_ONE) -> dict:
    """status, index, n_bad and checked of the check's steps, in their order. tau_of_g2: the
    discrete logarithm of a well-formed g2. pairing_checks is bounded by checks_ok()."""
    m = len(pts)
    out = {"status": "OK", "index": 0, "n_bad": 0, "checked": m}
    if _g2_defective(g2):
        return dict(out, status="G2", checked=0)
    bad = []
    for i, b in enumerate(pts):
        x, y = bn.g1_from_lem(b) or (0, 0)
        if any(v >= P for v in _stored(b)):
            bad.append((i, "RANGE"))
        elif (x, y) == (0, 0) or (y * y - x * x * x - 3) % P:
            bad.append((i, "CURVE"))
    if bad:
        return dict(out, status=bad[0][1], index=bad[0][0], n_bad=len(bad))
    aff = [bn.g1_from_lem(b) for b in pts]
    if aff[0] != bn.G1_GEN or g2_first != G2_ONE:
        return dict(out, status="GENERATOR")
    for i in range(1, m):
        if aff[i] != bn.g1_mul(aff[i - 1], tau_of_g2):
            return dict(out, status="SEQUENCE", index=i)
    return out


def checks_ok(finding: dict, m: int) -> bool:
    """The pairing checks a finding may have cost: one on the clean path, at most
    2 + ceil(log2 m) on a failing sequence, none when an earlier step ended the check."""
    n = finding["pairing_checks"]
    if finding["status"] == "OK":
        return n == (1 if m >= 2 else 0)
    if finding["status"] == "SEQUENCE":
        return 2 <= n <= 2 + math.ceil(math.log2(m)) or (m == 2 and n == 1)
    return n == 0


def strip(finding: dict) -> dict:
    return {k: v for k, v in finding.items() if k != "pairing_checks"}


# ---------------------------------------------------------------- ptau files
def make_ptau(power: int, pts: list, g2_points=None, sections=(1, 2, 3)) -> bytes:
    """A powers-of-tau file of `power` holding the stored points `pts` and tauG2 = g2_points."""
    g2_points = [G2_ONE, g2_of(TAU)] if g2_points is None else g2_points
    body = {1: struct.pack("<I", 32) + bn.to_le(P) + struct.pack("<II", power, power), 2: b"".join(pts),
            3: b"".join(g2_points)}
    return binfmt.write_binfile(b"ptau", 1, [(s, body[s]) for s in sections])


def section_span(data: bytes, magic: bytes, sid: int):
    """(offset, size) of a file's section."""
    return binfmt.read_binfile(data, magic)[1][sid][0]


def section_edges(data: bytes, magic: bytes) -> list:
    """Every offset at which a section's header or payload begins or ends."""
    edges = {12, len(data)}
    for spans in binfmt.read_binfile(data, magic)[1].values():
        for off, size in spans:
            edges |= {off - 12, off, off + size}
    return sorted(edges)


# ---------------------------------------------------------------- zkey files
@functools.lru_cache(maxsize=None)
def golden_zkey(name: str) -> bytes:
    with open(os.path.join(GOLD, f"{name}.zkey"), "rb") as f:
        return f.read()


PART_SECTION = {"Qm": (7, 0), "Ql": (8, 0), "Qr": (9, 0), "Qo": (10, 0), "Qc": (11, 0), "S1": (12, 0), "S2": (12, 1),
                "S3": (12, 2)}
HEADER_POINTS = ("Qm", "Ql", "Qr", "Qo", "Qc", "S1", "S2", "S3")


def zkey_n(data: bytes) -> int:
    off, _ = section_span(data, b"zkey", 2)
    return struct.unpack_from("<I", data, off + 4 + 32 + 4 + 32 + 8)[0]


def part_offset(data: bytes, part: str) -> int:
    """Offset of a part's n coefficients (its 4n evaluations follow); "L<j>" for Lagrange j."""
    n = zkey_n(data)
    sid, k = (13, int(part[1:])) if part.startswith("L") else PART_SECTION[part]
    return section_span(data, b"zkey", sid)[0] + k * 5 * n * 32


def header_offset(data: bytes, field: str) -> int:
    """Offset of k1, k2, a commitment or X_2 in the plonk header."""
    base = section_span(data, b"zkey", 2)[0] + 4 + 32 + 4 + 32 + 20
    if field in ("k1", "k2"):
        return base + 32 * ("k1", "k2").index(field)
    if field == "X_2":
        return base + 64 + 64 * 8
    return base + 64 + 64 * HEADER_POINTS.index(field)


def ptau_offset(data: bytes, i: int) -> int:
    return section_span(data, b"zkey", 14)[0] + 64 * i


def read_fr(data: bytes, off: int, count: int) -> list:
    return [bn.from_lem(data[off + 32 * i:off + 32 * i + 32], R) for i in range(count)]


def patch(data: bytes, off: int, new: bytes) -> bytes:
    return data[:off] + new + data[off + len(new):]


def fr_bytes(vals) -> bytes:
    return b"".join(bn.to_lem(v, R) for v in vals)


def with_coefficient(data: bytes, part: str, k: int, delta: int = 1, recompute: bool = True) -> bytes:
    """Coefficient k of a part changed; with `recompute` its 4n evaluations follow (bn.fft of
    the padded coefficients), so only what is derived from the coefficients elsewhere is left
    inconsistent."""
    n = zkey_n(data)
    off = part_offset(data, part)
    coef = read_fr(data, off, n)
    coef[k] = (coef[k] + delta) % R
    out = patch(data, off, fr_bytes(coef))
    if recompute:
        out = patch(out, off + 32 * n, fr_bytes(bn.fft(coef + [0] * (3 * n))))
    return out


def all_ok_except(result: dict, **expected) -> list:
    """The findings of a zkey_check result that are not what `expected` says (OK when it says
    nothing): header, srs and every part by name."""
    wrong = []
    flat = dict(result["parts"], header=result["header"], srs=result["srs"])
    for name, f in flat.items():
        want = expected.get(name, "OK")
        if f["status"] != want:
            wrong.append((name, f["status"], want))
    if result["ok"] != (not expected):
        wrong.append(("ok", result["ok"], not expected))
    return wrong


@functools.lru_cache(maxsize=None)
def zkey_mutations():
    """(name, bytes, findings that must not be OK, extra assertions on the result)."""
    z = golden_zkey("p5")
    n = zkey_n(z)
    out = []
    off = part_offset(z, "Ql") + 32 * (5 * n - 1)
    out.append(("last-eval-of-Ql", patch(z, off, bytes([z[off] ^ 1]) + z[off + 1:off + 32]), {"Ql": "EVALS"},
                lambda r: (r["parts"]["Ql"]["index"], r["parts"]["Ql"]["n_bad"]) == (4 * n - 1, 1)))
    out.append(("coefficient-0-of-S2", with_coefficient(z, "S2", 0, recompute=False), {"S2": "EVALS"},
                lambda r: (r["parts"]["S2"]["index"], r["parts"]["S2"]["n_bad"]) == (0, 4 * n)))
    out.append(("Qo-coefficient-consistent", with_coefficient(z, "Qo", 3), {"Qo": "COMMIT"},
                lambda r: r["parts"]["Qo"]["commit_checked"]))
    qc = bn.g1_from_lem(z[header_offset(z, "Qc"):][:64])
    out.append(("header-Qc-doubled", patch(z, header_offset(z, "Qc"), bn.g1_to_lem(bn.g1_mul(qc, 2))),
                {"Qc": "COMMIT"}, None))
    out.append(("lagrange-consistent", with_coefficient(z, "L1", 2), {"L1": "LAGRANGE"},
                lambda r: r["parts"]["L1"]["n_bad"] == n))
    off = part_offset(z, "S1") + 32 * (n + 5)
    out.append(("value-is-r", patch(z, off, bn.to_le(R)), {"S1": "NONCANONICAL"},
                lambda r: (r["parts"]["S1"]["index"], r["parts"]["S1"]["n_bad"]) == (n + 5, 1)))
    other = bn.g1_to_lem(bn.g1_mul(bn.G1_GEN, 0xC0FFEE))
    out.append(("ptau-point-5", patch(z, ptau_offset(z, 5), other), {"srs": "SEQUENCE"},
                lambda r: r["srs"]["index"] == 5 and not any(p["commit_checked"] for p in r["parts"].values())))
    out.append(("X_2-of-another-tau", patch(z, header_offset(z, "X_2"), g2_of(TAU2)), {"srs": "SEQUENCE"},
                lambda r: r["srs"]["index"] == 1))
    k1 = read_fr(z, header_offset(z, "k1"), 1)[0]
    w = bn.FR_W[n.bit_length() - 1]
    out.append(("k2-in-k1-coset", patch(z, header_offset(z, "k2"), fr_bytes([k1 * w % R])),
                {"header": "COSETS"}, None))
    out.append(("k1-is-one", patch(z, header_offset(z, "k1"), fr_bytes([1])), {"header": "COSETS"}, None))
    return out


# ---------------------------------------------------------------- one SRS case, on either path
def check_srs(nzcb, device: int, pts: list, g2: bytes, tau_of_g2: int, chunk_points: int = 0):
    """Runs the engine entry and holds its finding against the exact-integer expectation, and
    L || R against the Python sums whenever the check got as far as the sequence step. Returns
    (finding, lr) for comparisons between the paths."""
    finding, lr = nzcb.Engine.srs_check(b"".join(pts), g2, device=device, seed=SEED, chunk_points=chunk_points)
    want = expected_finding(pts, g2, tau_of_g2)
    assert strip(finding) == want
    assert checks_ok(finding, len(pts)), finding
    if want["status"] in ("OK", "SEQUENCE") and len(pts) >= 2:
        assert lr == expected_lr(pts, SEED)
    else:
        assert lr == bytes(128)
    return finding, lr
