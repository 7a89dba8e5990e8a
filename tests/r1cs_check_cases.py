"""Shared builders for the witness-check tests (tests/test_r1cs_check.py on the host path,
tests/test_gpu_r1cs_check.py on the device): case r1cs files written with
oracle.r1cs.write_r1cs, witnesses that satisfy them by construction, mutated copies, and the
reference verdicts from the exact-integer check (oracle.wvm.r1cs_unsatisfied over
oracle.r1cs.read_r1cs), never from the code under test.

A case is (name, r1cs bytes, [witness as a list of ints, ...])."""
import random

from oracle import r1cs as orc
from oracle import wvm
from oracle.bn254 import R_MOD as R, fr_inv

_PARSED = {}


def expected(r1cs: bytes, wit, cap: int = 8) -> dict:
    """What R1cs.check must return for one witness."""
    if r1cs not in _PARSED:
        _PARSED[r1cs] = orc.read_r1cs(r1cs)
    bad = wvm.r1cs_unsatisfied(_PARSED[r1cs], wit, limit=1 << 62)
    return {"n_bad": len(bad), "first_bad": bad[0] if bad else None, "bad": bad[:cap]}


def pack(wits, stride=None) -> bytes:
    """32-byte LE values, witness i at byte i * stride (default packed); the gaps are 0xEE."""
    if not wits:
        return b""
    n = len(wits[0])
    stride = stride or 32 * n
    out = bytearray(b"\xee" * (stride * (len(wits) - 1) + 32 * n))
    for i, w in enumerate(wits):
        out[i * stride:i * stride + 32 * n] = b"".join(v.to_bytes(32, "little") for v in w)
    return bytes(out)


def bump(wit, wire, by=1):
    w = list(wit)
    w[wire] = (w[wire] + by) % R
    return w


def random_cases():
    """oracle.r1cs.random_r1cs for 6 seeds: the satisfied witness and 8 copies with one wire
    changed each (wire 0 among them for some seeds)."""
    out = []
    for seed in range(1, 7):
        data, w = orc.random_r1cs(seed, n_steps=40 + 9 * seed)
        rng = random.Random(1000 + seed)
        wires = rng.sample(range(len(w)), 8)
        out.append((f"random{seed}", data, [w] + [bump(w, k, rng.randrange(1, R)) for k in wires]))
    return out


EDGE_COEFS = (1, R - 1, R - 2, 4, 1 << 253, 0x2B5E1A7C9D3F4E6A8B0C2D4E6F8091A2B3C4D5E6F708192A3B4C5D6E7F8091A2 % R)


def edge_case():
    """Hand-built: empty sides, terms on wire 0, the coefficient kinds, a repeated wire, the
    values 0, 1 and r - 1, (r - 1)(r - 1) = 1 and witness values >= r. Returns the case and the
    set of constraints that use the constant wire (each of them fails when wire 0 is 2)."""
    x4 = 0x1234567890ABCDEF1234567890ABCDEF1234567890ABCDEF1234567890ABCDEF % R
    big = (1 << 256) - 1
    w = [1, 0, 1, R - 1, x4, R, R + 5, big, big % R]   # wires 1..8: 0, 1, r-1, x4, r, r+5, 2^256-1, its residue
    X0, X1, XM, X4, XR, XR5, XBIG, Z = 1, 2, 3, 4, 5, 6, 7, 8
    cons = [
        ([], [(X4, 1)], []),                                  # empty A
        ([(X4, 3)], [], [(X0, 7)]),                           # empty B
        ([(X0, 1)], [(X4, 1)], []),                           # empty C
        ([], [], []),                                         # all empty
        ([(0, 5)], [(0, 1)], [(0, 5)]),                       # the constant alone
        ([(0, 2), (X1, 3)], [(0, 1)], [(0, 5)]),
        ([(X4, 2), (X4, 3)], [(0, 1)], [(X4, 5)]),            # a repeated wire adds up
        ([(X4, 2), (X4, R - 2)], [(X4, 1)], []),              # ... to zero
        ([(XM, 1)], [(XM, 1)], [(X1, 1)]),                    # (r-1)(r-1) = 1
        ([(XM, R - 1)], [(X1, 1)], [(X1, 1)]),                # (r-1)(r-1) = 1 through the coefficient
        ([(XR, 1)], [(X4, 1)], []),                           # r counts as 0, on the +1 path
        ([(XR, R - 1)], [(X4, 1)], []),                       # on the r-1 path
        ([(XR, 9)], [(X4, 1)], []),                           # through a product
        ([(XR5, 1)], [(X1, 1)], [(0, 5)]),                    # r + 5 counts as 5
        ([(XR5, 3)], [(X1, 1)], [(0, 15)]),
        ([(XR5, R - 1)], [(X1, 1)], [(0, R - 5)]),
        ([(XBIG, 1)], [(0, 1)], [(Z, 1)]),                    # 2^256 - 1 counts modulo r
        ([(XBIG, R - 1)], [(0, 1)], [(Z, R - 1)]),
        ([(XBIG, 7)], [(0, 1)], [(Z, 7)]),
        ([(X4, 1)], [(XBIG, 1)], [(Z, x4)]),
    ]
    for c in EDGE_COEFS:                                      # c * x4 = y_c, one wire per coefficient
        w.append(c * x4 % R)
        cons.append(([(X4, c)], [(0, 1)], [(len(w) - 1, 1)]))
    data = orc.write_r1cs(len(w), 1, 1, 2, cons)
    uses_one = {k for k, lcs in enumerate(cons) if any(s == 0 for lc in lcs for s, _ in lc)}
    w0_is_2 = [2] + w[1:]
    wits = [w, w0_is_2] + [bump(w, k) for k in range(1, len(w))] + [bump(w, XBIG, R - 7)]
    return ("edge", data, wits), uses_one


SIZES = (0, 1, 63, 64, 65, 129)


def size_case(n: int):
    """n constraints x_k * x_k = y_k (wire 1 + k times itself = wire 1 + n + k): the satisfied
    witness, only the first constraint failing, only the last, and all of them."""
    rng = random.Random(77 + n)
    xs = [rng.randrange(R) for _ in range(n)]
    w = [1] + xs + [x * x % R for x in xs]
    cons = [([(1 + k, 1)], [(1 + k, 1)], [(1 + n + k, 1)]) for k in range(n)]
    data = orc.write_r1cs(len(w), 0, 0, n, cons)
    wits = [w]
    if n:
        every = [1] + xs + [(y + 1) % R for y in w[1 + n:]]
        wits += [bump(w, 1 + n), bump(w, 2 * n), every]
    return (f"size{n}", data, wits)


def long_row_lengths(T: int):
    """Total terms of the rows of long_rows_case: around the threshold, nzcp_live's longest
    row, and 64 k + 1 (one lane walks one term more than the others)."""
    return [T - 1, T, T + 1, 836, 64 * 5 + 1]


def long_rows_case(T: int):
    """One row per length of long_row_lengths(T), (1)(1) = C with C of length - 2 terms over
    wires of its own, then a row whose C side alone has 64 * 2 + 1 terms, and a row with 70
    terms in A and 70 in B. Coefficients mix +1, r - 1 and full-width ones. Witnesses: the
    satisfied one, then per row a copy that fails that row only, through the last term of its
    last non-empty side. Returns the case and the rows' total lengths."""
    rng = random.Random(4242 + T)
    w = [1]
    cons, last_wires, lengths = [], [], []

    def coef():
        return rng.choice((1, R - 1, rng.randrange(2, R - 1)))

    def side(n_terms):
        """n_terms terms on fresh wires with random values; returns (lc, value)."""
        lc = []
        for _ in range(n_terms):
            w.append(rng.randrange(R))
            lc.append((len(w) - 1, coef()))
        return lc, sum(c * w[s] for s, c in lc) % R

    def close(lc, value, target):
        """One more term on a fresh wire that makes the side sum to target."""
        c = coef()
        w.append((target - value) * fr_inv(c) % R)
        return lc + [(len(w) - 1, c)]

    for total in long_row_lengths(T) + [64 * 2 + 1 + 2]:
        lc, v = side(max(total - 3, 0))
        cons.append(([(0, 1)], [(0, 1)], close(lc, v, 1)))
        last_wires.append(len(w) - 1)
        lengths.append(len(lc) + 3)
    a, va = side(70)
    b, vb = side(70)
    cons.append((a, b, close([], 0, va * vb % R)))
    last_wires.append(len(w) - 1)
    lengths.append(141)
    data = orc.write_r1cs(len(w), 0, 0, len(w) - 1, cons)
    return (f"long{T}", data, [w] + [bump(w, k) for k in last_wires]), lengths


def malformed_files():
    """(a good one-constraint r1cs, its header section, its constraint section, [(bytes, the
    reader's text)]): constraint data cut short, a signal out of range, an unreduced coefficient."""
    import struct
    from oracle.binfmt import write_binfile
    from oracle.bn254 import to_le
    good = orc.write_r1cs(3, 1, 1, 0, [([(1, 1)], [(1, 1)], [(2, 1)])])
    hdr = struct.pack("<I", 32) + to_le(R) + struct.pack("<IIIIQI", 3, 1, 1, 0, 3, 1)
    body = struct.pack("<II", 1, 1) + to_le(1) + struct.pack("<II", 1, 1)
    truncated = write_binfile(b"r1cs", 1, [(1, hdr), (2, body + to_le(1)[:20])])
    out_of_range = orc.write_r1cs(3, 1, 1, 0, [([(1, 1)], [(3, 1)], [(2, 1)])])
    unreduced = good.replace(struct.pack("<I", 2) + to_le(1), struct.pack("<I", 2) + to_le(R + 1), 1)
    assert unreduced != good
    return good, hdr, body, [(truncated, "r1cs: truncated"), (out_of_range, "r1cs: signal out of range"),
                             (unreduced, "r1cs: coefficient not reduced")]


def wtns_file(wit) -> bytes:
    """snarkjs .wtns (version 2) of a witness."""
    from nzcb import nzcplive
    return nzcplive.wtns_file(pack([wit]))


def wrapper_case(n: int = 3):
    """nzcpgen's QuinSelector wrapper main: the accepted witness (index 1) and the negative
    KAT's witness carried past the failure (index = choices). Returns (Circuit, r1cs bytes,
    good witness, carried witness)."""
    from nzcb import nzcpgen
    c = nzcpgen.wrapper_circuit(f"quinSelector{n}_test")
    prog = c.write_program()
    good, fail = wvm.evaluate(prog, list(range(1, n + 1)) + [1])
    assert fail is None
    carried, fail = wvm.evaluate(prog, list(range(1, n + 1)) + [n])
    assert fail is not None
    return c, c.write_r1cs(), good, carried


def violated(c, wit, ks):
    """The failing constraints among ks, over Circuit.constraints (exact integers)."""
    bad = []
    for k in ks:
        A, B, Cc = c.constraints[k]
        a = sum(v * wit[i] for i, v in A.items()) % R
        b = sum(v * wit[i] for i, v in B.items()) % R
        cc = sum(v * wit[i] for i, v in Cc.items()) % R
        if (a * b - cc) % R:
            bad.append(k)
    return bad


def wire_index(c):
    """wire -> the constraints that mention it."""
    idx = {}
    for k, cons in enumerate(c.constraints):
        for part in cons:
            for wire in part:
                idx.setdefault(wire, set()).add(k)
    return idx


def check_all(r1cs_obj, case, cap: int = 8, batch: bool = True):
    """Run every witness of the case (one call, or one call per witness) on r1cs_obj."""
    _, _, wits = case
    if batch:
        return r1cs_obj.check(pack(wits), count=len(wits), bad_cap=cap)
    return [r1cs_obj.check(pack([w]), count=1, bad_cap=cap)[0] for w in wits]
