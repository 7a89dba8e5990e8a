"""An exact-integer P-256 / ECDSA oracle (Python integers, affine coordinates) and the case
builders shared by tests/test_p256_verify.py (host path), tests/test_gpu_p256_verify.py (device 0)
and tests/test_node_p256.py. The oracle costs milliseconds per verification, so the pool of
distinct signatures stays at 128 and larger batches tile it."""
import functools
import hashlib
import random

P = 0xffffffff00000001000000000000000000000000ffffffffffffffffffffffff
N = 0xffffffff00000000ffffffffffffffffbce6faada7179e84f3b9cac2fc632551
B = 0x5ac635d8aa3a93e7b3ebbd55769886bc651d06b0cc53b0f63bce3c3e27d2604b
G = (0x6b17d1f2e12c4247f8bce6e563a440f277037d812deb33a0f4a13945d898c296,
     0x4fe342e2fe1a7f9b8ee7eb4a7c0f9e162bce33576b315ececbb6406837bf51f5)
OK, INVALID, RANGE = 0, 1, 2  # include/nzcb.h NZCB_SIG_*
BAD_KEY_TEXT = "public key is not a point on P-256"


# ---------------------------------------------------------------- the oracle
def on_curve(pt) -> bool:
    x, y = pt
    return (y * y - (x * x * x - 3 * x + B)) % P == 0


def add(a, b):
    """a + b; None is the point at infinity."""
    if a is None:
        return b
    if b is None:
        return a
    if a[0] == b[0]:
        if (a[1] + b[1]) % P == 0:
            return None
        lam = (3 * a[0] * a[0] - 3) * pow(2 * a[1], -1, P) % P
    else:
        lam = (b[1] - a[1]) * pow(b[0] - a[0], -1, P) % P
    x = (lam * lam - a[0] - b[0]) % P
    return x, (lam * (a[0] - x) - a[1]) % P


def neg(a):
    return None if a is None else (a[0], -a[1] % P)


def mul(k: int, a):
    r = None
    for bit in bin(k % N)[2:] if k % N else "":
        r = add(r, r)
        if bit == "1":
            r = add(r, a)
    return r


def mul2(u1: int, u2: int, q):
    return add(mul(u1, G), mul(u2, q))


def verify(q, z: bytes, sig: bytes) -> int:
    """ECDSA (FIPS 186-4 6.4.2 / SEC 1 4.1.4) over a 32-byte digest; no low-s rule."""
    r, s = int.from_bytes(sig[:32], "big"), int.from_bytes(sig[32:], "big")
    if not (1 <= r < N and 1 <= s < N):
        return RANGE
    w = pow(s, -1, N)
    pt = mul2(int.from_bytes(z, "big") * w % N, r * w % N, q)
    return OK if pt is not None and pt[0] % N == r else INVALID


def sign(d: int, z: bytes, k: int) -> bytes:
    r = mul(k, G)[0] % N
    s = pow(k, -1, N) * (int.from_bytes(z, "big") + r * d) % N
    assert r and s
    return be(r) + be(s)


def be(x: int) -> bytes:
    return x.to_bytes(32, "big")


def xy(q) -> bytes:
    return be(q[0]) + be(q[1])


def lift_x(x: int):
    """The curve point with this x and the even y, or None (p = 3 mod 4)."""
    rhs = (x * x * x - 3 * x + B) % P
    y = pow(rhs, (P + 1) // 4, P)
    if y * y % P != rhs:
        return None
    return x, (y if y % 2 == 0 else P - y)


# ---------------------------------------------------------------- field cases
FIELD_OPS = ("add", "sub", "mul", "sqr", "inv")


def field_expected(op: str, m: int, a: int, b: int) -> int:
    return {"add": (a + b) % m, "sub": (a - b) % m, "mul": a * b % m, "sqr": a * a % m,
            "inv": pow(a, m - 2, m)}[op]


def field_edges(m: int) -> list:
    return [0, 1, 2, m - 1, m - 2, 1 << 255, (1 << 256) - m, (m - 1) // 2, (m + 1) // 2]


@functools.lru_cache(maxsize=None)
def field_pairs(m: int):
    """The edge set crossed with itself, then 4096 seeded random pairs (so that every lane of
    several waves computes), as two lists."""
    e = field_edges(m)
    rng = random.Random(m & 0xffffffff)
    pairs = [(a, b) for a in e for b in e] + [(rng.randrange(m), rng.randrange(m)) for _ in range(4096)]
    return [a for a, _ in pairs], [b for _, b in pairs]


# ---------------------------------------------------------------- mul2 cases
def window_scalars() -> list:
    """All-zero and all-ones windows at widths 4 and 8, a zero top and a zero bottom window."""
    return [int(h * (64 // len(h)), 16) for h in ("0f", "f0", "00ff", "ff00", "0000ffff", "ffff0000")] + [
        (1 << 248) - 1, (1 << 252) - 1, ((1 << 256) - 1) ^ 0xff, ((1 << 256) - 1) ^ 0xf, 1 << 248, 1 << 252,
        0xff << 120, 0xf << 124, (1 << 256) - 1]


@functools.lru_cache(maxsize=None)
def mul2_keys():
    """(name, d, Q = d G) for Q = G, -G, 2G and a seeded random Q."""
    d = random.Random(2561).randrange(1, N)
    return [("G", 1, G), ("-G", N - 1, neg(G)), ("2G", 2, mul(2, G)), ("random", d, mul(d, G))]


@functools.lru_cache(maxsize=None)
def mul2_case(name: str):
    """(Q, u1 list, u2 list, expected points) for one of mul2_keys()."""
    _, d, q = next(k for k in mul2_keys() if k[0] == name)
    rng = random.Random(d & 0xffff)
    edge = [0, 1, 2, 3, N - 1, N - 2, 1 << 255, (N - 1) // 2, (N + 1) // 2]
    pairs = [(a, b) for a in edge for b in edge]
    pairs += [(rng.randrange(N), rng.randrange(N)) for _ in range(6)]
    for u2 in (1, 2, rng.randrange(1, N)):
        pairs.append((u2 * d % N, u2))       # u1 G = u2 Q: the last addition is a doubling
        pairs.append((-u2 * d % N, u2))      # u1 G = -u2 Q: the point at infinity
    ws = window_scalars()
    pairs += [(w, ws[(i + 1) % len(ws)]) for i, w in enumerate(ws)]
    pairs += [(w, 0) for w in ws[:4]] + [(0, w) for w in ws[:4]]
    # the oracle's scalar multiples, each computed once
    g1, g2 = {}, {}
    for a, b in pairs:
        if a not in g1:
            g1[a] = mul(a, G)
        if b not in g2:
            g2[b] = mul(b, q)
    return q, [a for a, _ in pairs], [b for _, b in pairs], [add(g1[a], g2[b]) for a, b in pairs]


# ---------------------------------------------------------------- signatures
def digest(tag) -> bytes:
    return hashlib.sha256(repr(tag).encode()).digest()


@functools.lru_cache(maxsize=None)
def pool():
    """(Q, items): 128 distinct (hash, sig, expected status) under one key: valid signatures,
    their s -> n - s twins, corrupted ones and out-of-range ones, statuses from the oracle."""
    rng = random.Random(0x5256)
    d = rng.randrange(1, N)
    q = mul(d, G)
    z = digest("range")
    sig = sign(d, z, rng.randrange(1, N))
    r, s = sig[:32], sig[32:]
    items = [(z, bad) for bad in (be(0) + s, r + be(0), be(N) + s, r + be(N), r + be((1 << 256) - 1),
                                  be((1 << 256) - 1) + s, be(N + 1) + s, be(0) + be(0))]
    for zz in (be(0), be(N), be((1 << 256) - 1), be(N - 1), be(1)):   # z = 0, z >= n
        items.append((zz, sign(d, zz, rng.randrange(1, N))))
        items.append((zz, sig))
    for i in range(64):
        z = digest(("pool", i))
        sig = sign(d, z, rng.randrange(1, N))
        items.append((z, sig))
        if i % 4 == 0:   # the high-s twin is as valid
            items.append((z, sig[:32] + be(N - int.from_bytes(sig[32:], "big"))))
        if i % 2 == 0:   # one bit of r, s or the digest flipped
            j = rng.randrange(96 * 8)
            blob = bytearray(z + sig)
            blob[j // 8] ^= 1 << (j % 8)
            items.append((bytes(blob[:32]), bytes(blob[32:])))
        if i % 3 == 0:   # another digest
            items.append((digest(("other", i)), sig))
    items = items[:128]
    assert len(set(items)) == len(items) == 128
    return q, [(z, sg, verify(q, z, sg)) for z, sg in items]


def batch(count: int, seed: int = 1):
    """`count` pool items in a seeded shuffle (the pool tiled when count exceeds it)."""
    _, items = pool()
    idx = [i % len(items) for i in range(count)]
    random.Random(seed * 1000 + count).shuffle(idx)
    return [items[i] for i in idx]


@functools.lru_cache(maxsize=None)
def constructed():
    """Signatures built without discrete logarithms; name -> (Q, hash, sig, the status stated in
    the issue). The oracle agrees with every one (asserted here)."""
    rng = random.Random(0xC0)
    out = {}
    # R.x >= n: the curve point with the smallest such x has x = n + 3, so r = 3
    x0 = next(x for x in range(N, N + 64) if lift_x(x))
    assert x0 == N + 3 and x0 < P
    r0 = lift_x(x0)
    u1, u2 = rng.randrange(1, N), rng.randrange(1, N)
    q = mul(pow(u2, -1, N), add(r0, neg(mul(u1, G))))
    r = x0 - N
    s = r * pow(u2, -1, N) % N
    z = u1 * s % N
    out["rx_ge_n"] = (q, be(z), be(r) + be(s), OK)
    out["rx_ge_n_unreduced_r"] = (q, be(z), be(r + N) + be(s), RANGE)
    # Q = d G, R = k G, u1 = k / 2, u2 = k / (2 d): u1 G = u2 Q, the sum is a doubling
    d, k = rng.randrange(2, N), rng.randrange(2, N)
    q = mul(d, G)
    u1, u2 = k * pow(2, -1, N) % N, k * pow(2 * d, -1, N) % N
    r = mul(k, G)[0] % N
    s = r * pow(u2, -1, N) % N
    out["doubling"] = (q, be(u1 * s % N), be(r) + be(s), OK)
    # z = -r d: u1 G + u2 Q is the point at infinity
    r, s = rng.randrange(1, N), rng.randrange(1, N)
    out["infinity"] = (q, be(-r * d % N), be(r) + be(s), INVALID)
    for name, (qq, zz, sg, want) in out.items():
        assert on_curve(qq) and verify(qq, zz, sg) == want, name
    return out


def bad_keys() -> dict:
    """name -> 64 bytes that are no P-256 public key."""
    x = next(x for x in range(5, 64) if lift_x(x) is None)   # x^3 - 3x + b is a non-residue: the twist
    rhs = (x * x * x - 3 * x + B) % P
    # a point of the quadratic twist v y^2 = x^3 - 3x + b for the non-residue v = -1 (p = 3 mod 4)
    ty = pow(-rhs % P, (P + 1) // 4, P)
    assert ty * ty % P == -rhs % P
    return {"zero": bytes(64), "x_is_p": be(P) + be(G[1]), "y_off_by_one": be(G[0]) + be(G[1] + 1),
            "y_is_p": be(G[0]) + be(P), "twist": be(x) + be(ty)}


# ---------------------------------------------------------------- the example pass
EXAMPLE_Z = "271ce33d"   # SHA-256 of the example pass's 314-byte Sig_structure begins and ends so
EXAMPLE_Z_END = "8c11f3ee"


def example_tampered_tbs(tbs: bytes) -> bytes:
    """The example ToBeSigned with the last byte of nbf (CWT claim 5, before exp) changed."""
    from nzcb import nzcp
    needle = b"\x05\x1a" + nzcp.EXAMPLE_NBF.to_bytes(4, "big")
    at = tbs.index(needle) + len(needle) - 1
    return tbs[:at] + bytes([tbs[at] ^ 1]) + tbs[at + 1:]


# ---------------------------------------------------------------- checks shared by the host and GPU tests
def example_key(device: int, **kw):
    import nzcb
    from nzcb import nzcp
    return nzcb.P256Key(nzcp.EXAMPLE_PUBLIC_KEY, device=device, **kw)


def example_hash_sig():
    from nzcb import nzcp
    protected, payload, sig = nzcp.decode_pass(nzcp.EXAMPLE_PASS_URI)
    z = hashlib.sha256(nzcp.sig_structure(protected, payload)).digest()
    assert z.hex().startswith(EXAMPLE_Z) and z.hex().endswith(EXAMPLE_Z_END)
    return z, sig


def check_field(device: int, field: str, op: str):
    import nzcb
    m = {"p": P, "n": N}[field]
    a, b = field_pairs(m)
    got = nzcb.p256_field(op, field, a, b, device=device)
    want = [field_expected(op, m, x, y) for x, y in zip(a, b)]
    bad = [i for i in range(len(a)) if got[i] != want[i]]
    assert not bad, (field, op, len(bad), hex(a[bad[0]]), hex(b[bad[0]]), hex(got[bad[0]]), hex(want[bad[0]]))
    return got


def check_mul2(device: int, name: str, window: int):
    import nzcb
    q, u1, u2, want = mul2_case(name)
    key = nzcb.P256Key(xy(q), device=device, window=window)
    try:
        got = key.mul2(u1, u2)
    finally:
        key.close()
    bad = [i for i in range(len(u1)) if got[i] != want[i]]
    assert not bad, (name, window, len(bad), hex(u1[bad[0]]), hex(u2[bad[0]]))
    assert None in want   # the point at infinity is among the cases
    return got


def statuses(device: int, q, items, **kw):
    import nzcb
    key = nzcb.P256Key(xy(q), device=device, **kw)
    try:
        return key.verify([z for z, *_ in items], [s for _, s, *_ in items])
    finally:
        key.close()
