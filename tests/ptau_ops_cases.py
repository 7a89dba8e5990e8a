"""Expected bytes of the powers-of-tau operations (nzcb.ptau_new, ptau_contribute,
ptau_prepare_phase2) for tests/test_ptau_ops.py on the host path and tests/test_gpu_ptau_ops.py
on the device: a restatement from oracle/bn254.py. With the trapdoors known every point of a
file is [scalar] generator, and a Lagrange point is [c L_k(tau)] with L_k(tau) evaluated in Fr
(bn.ifft of the scalars c tau^i). Python's G2 multiplication is slow: keep G2 expectations to
power <= 5 and G1 ones to power <= 8."""
import functools
import struct

from oracle import binfmt, bn254 as bn

P, R = bn.P_MOD, bn.R_MOD

# (tau, alpha, beta) of two contributions, and what contributing both amounts to
SECRETS_A = (0x6E7A63625F746175, 0x616C7068615F6E7A6362, 0x626574615F6E7A6362)
SECRETS_B = (R - 5, 0x1234567890ABCDEF1234567890ABCDEF, 3)
ONE = (1, 1, 1)
G2_SECTIONS = (3, 6, 13)


def compose(a, b):
    """The secrets one contribution would need to do what a then b do: the component-wise product."""
    return tuple(x * y % R for x, y in zip(a, b))


# ---------------------------------------------------------------- [s] generator
@functools.lru_cache(maxsize=None)
def _doubles(g2: bool):
    pts, pt = [], bn.G2_GEN if g2 else bn.G1_GEN
    for _ in range(254):
        pts.append(pt)
        pt = bn.g2_double(pt) if g2 else bn.g1_add(pt, pt)
    return tuple(pts)


@functools.lru_cache(maxsize=None)
def gen_mul(g2: bool, s: int) -> bytes:
    """The stored bytes of [s] G1 or [s] G2: a sum over the generator's doublings."""
    s %= R
    if not g2:
        return bn.g1_to_lem(bn.g1_mul(bn.G1_GEN, s))
    acc = None
    for i, pt in enumerate(_doubles(True)):
        if (s >> i) & 1:
            acc = bn.g2_add(acc, pt)
    return bn.g2_to_lem(acc)


# ---------------------------------------------------------------- scalars of the sections
@functools.lru_cache(maxsize=None)
def section_scalars(power: int, secrets: tuple) -> dict:
    """Section id -> the scalar of each of its points, for sections 2-6 and 12-15."""
    tau, alpha, beta = secrets
    n = 1 << power
    pw = [pow(tau, i, R) for i in range(2 * n - 1)]
    src = {2: pw, 3: pw[:n], 4: [alpha * t % R for t in pw[:n]], 5: [beta * t % R for t in pw[:n]], 6: [beta]}
    out = dict(src)
    for sid, lag in ((2, 12), (3, 13), (4, 14), (5, 15)):
        levels = []
        for p in range(power + 1):
            levels += bn.ifft(src[sid][:1 << p])
        if sid == 2:
            levels += bn.ifft(pw + [0])  # level power + 1: the 2n - 1 points, then the point at infinity
        out[lag] = levels
    return out


def header(power: int) -> bytes:
    return struct.pack("<I", 32) + bn.to_le(P) + struct.pack("<II", power, power)


@functools.lru_cache(maxsize=None)
def expected_file(power: int, secrets: tuple = ONE, prepared: bool = False) -> bytes:
    """new(power) after contributions whose composition is `secrets`, prepared or not."""
    sc = section_scalars(power, secrets)
    ids = (2, 3, 4, 5, 6) + ((12, 13, 14, 15) if prepared else ())
    body = {sid: b"".join(gen_mul(sid in G2_SECTIONS, s) for s in sc[sid]) for sid in ids}
    body[1] = header(power)
    body[7] = struct.pack("<I", 0)
    return binfmt.write_binfile(b"ptau", 1, [(sid, body[sid]) for sid in (1, 2, 3, 4, 5, 6, 7) + ids[5:]])


# ---------------------------------------------------------------- reading and spoiling files
def sections(data: bytes) -> dict:
    """Section id -> payload bytes."""
    return {sid: data[off:off + size] for sid, ((off, size),) in binfmt.read_binfile(data, b"ptau")[1].items()}


def point_bytes(sid: int) -> int:
    return 128 if sid in G2_SECTIONS else 64


def points(data: bytes, sid: int) -> list:
    body, w = sections(data)[sid], point_bytes(sid)
    return [body[i:i + w] for i in range(0, len(body), w)]


def patch_point(data: bytes, sid: int, index: int, new: bytes) -> bytes:
    (off, _), = binfmt.read_binfile(data, b"ptau")[1][sid]
    at = off + point_bytes(sid) * index
    return data[:at] + new + data[at + len(new):]


def spoiled(data: bytes, sid: int, index: int, kind: str) -> bytes:
    """Point `index` of section `sid` made defective: "range" (a stored word = q), "curve" (y + 1)
    or "zero" ((0, 0))."""
    w = point_bytes(sid)
    old = points(data, sid)[index]
    if kind == "zero":
        new = bytes(w)
    elif kind == "range":
        new = old[:w - 32] + bn.to_le(P)
    elif sid in G2_SECTIONS:
        x, (y0, y1) = bn.g2_from_lem(old)
        new = bn.g2_to_lem((x, ((y0 + 1) % P, y1)))
    else:
        x, y = bn.g1_from_lem(old)
        new = bn.g1_to_lem((x, (y + 1) % P))
    return patch_point(data, sid, index, new)


def without_section(data: bytes, sid: int) -> bytes:
    return binfmt.write_binfile(b"ptau", 1, [(s, b) for s, b in sorted(sections(data).items()) if s != sid])


def with_short_section(data: bytes, sid: int, drop: int = 1) -> bytes:
    return binfmt.write_binfile(b"ptau", 1, [(s, b[:-drop] if s == sid else b) for s, b in sorted(sections(data).items())])


def section_edges(data: bytes) -> list:
    """Every offset at which a section's table entry or payload begins or ends."""
    edges = {12, len(data)}
    for spans in binfmt.read_binfile(data, b"ptau")[1].values():
        for off, size in spans:
            edges |= {off - 12, off, off + size}
    return sorted(edges)


# ---------------------------------------------------------------- group sums in Python
def point_sum(pts: list, g2: bool) -> bytes:
    acc = None
    for b in pts:
        if g2:
            acc = bn.g2_add(acc, bn.g2_from_lem(b))
        else:
            acc = bn.g1_add(acc, bn.g1_from_lem(b))
    return bn.g2_to_lem(acc) if g2 else bn.g1_to_lem(acc)


def level(data: bytes, sid: int, p: int) -> list:
    """The 2^p points of level p of a Lagrange section."""
    return points(data, sid)[(1 << p) - 1:(2 << p) - 1]
