"""Expected bytes of the Groth16 key generation (nzcb.groth16_setup, groth16_contribute,
groth16_vk) for tests/test_groth16.py on the host path and tests/test_gpu_groth16.py on the
device: a restatement from oracle/bn254.py that uses no library code. With the trapdoor of the
powers-of-tau file known, every point of the key is [one scalar] generator: the scalar of a row
is summed in Fr from the r1cs coefficients and L_c(tau) (ptau_ops_cases.section_scalars, never
the file's Lagrange sections), then multiplied into the generator once. Also here: the edge
circuit, a Groth16 prover for tiny circuits over a key's own points, and the verification
equation over oracle.pairing."""
import functools
import random
import struct

import ptau_ops_cases as pc
from oracle import binfmt, bn254 as bn, pairing
from oracle.r1cs import random_r1cs, read_r1cs, write_r1cs

P, R = bn.P_MOD, bn.R_MOD
D1, D2 = 0x6E7A63625F64656C7461, R - 0x1234567  # contribution secrets

G2_SECTIONS = (7,)


def cir_power(m: int, n_public: int) -> int:
    return max(1, (m + n_public).bit_length())


def n_public_of(c: dict) -> int:
    return c["nOutputs"] + c["nPubInputs"]


# ---------------------------------------------------------------- circuits
@functools.lru_cache(maxsize=None)
def random_circuit(seed: int):
    """(r1cs bytes, witness): 40 constraints, 47 wires, nPublic 5, cirPower 6."""
    return random_r1cs(seed, n_out=3, n_pub_in=2, n_prv_in=4, n_steps=40)


EDGE_COEFS = [0, 1, R - 1, 2, R - 2, (R - 1) // 2, (R + 1) // 2, (1 << 253) + 1,
              random.Random(16).randrange(R), random.Random(17).randrange(R)]


@functools.lru_cache(maxsize=None)
def edge_circuit(n_cons: int = 14) -> bytes:
    """12 wires (1 output, 2 public inputs), `n_cons` constraints. Constraint i uses coefficient
    EDGE_COEFS[i mod 10] = k: A = k w4 + (i + 1) w0 + w5 - 2 w5 (a wire listed twice), B = w0 +
    k w6 + 2 w(1 + i mod 3) (wire 7 is in no B), C = k w8 + 7 w0 + 3 w7. Wire 0 is in A, B and C
    of every constraint, but for the empty linear combinations: A of constraints 10, 21, ... and C
    of constraints 12, 25, ... Wires 9-11 are in no constraint at all."""
    cons = []
    for i in range(n_cons):
        k = EDGE_COEFS[i % len(EDGE_COEFS)]
        a = [] if i % 11 == 10 else [(4, k), (0, i + 1), (5, 1), (5, R - 2)]
        b = [(0, 1), (6, k), (1 + i % 3, 2)]
        c = [] if i % 13 == 12 else [(8, k), (0, 7), (7, 3)]
        cons.append((a, b, c))
    return write_r1cs(12, 1, 2, 8, cons)


# ---------------------------------------------------------------- the key's scalars
def key_scalars(r1cs: bytes, power: int, secrets: tuple, d: int = 1) -> dict:
    """The scalar of every point of the key: "A", "B" (B1 and B2), "K" (IC then C), "H", and the
    header's alpha, beta, delta. d: the product of the contributions."""
    c = read_r1cs(r1cs)
    m, n_vars, n_pub = len(c["constraints"]), c["nWires"], n_public_of(c)
    cp = cir_power(m, n_pub)
    assert cp <= power
    n = 1 << cp
    sc = pc.section_scalars(power, secrets)
    level = lambda sid, p: sc[sid][(1 << p) - 1:(2 << p) - 1]
    l12, l14, l15, t = level(12, cp), level(14, cp), level(15, cp), level(12, cp + 1)
    a_s, b_s, k_s = [0] * n_vars, [0] * n_vars, [0] * n_vars
    for ci, (la, lb, lc) in enumerate(c["constraints"]):
        for s, v in la:
            a_s[s] += v * l12[ci]
            k_s[s] += v * l15[ci]
        for s, v in lb:
            b_s[s] += v * l12[ci]
            k_s[s] += v * l14[ci]
        for s, v in lc:
            k_s[s] += v * l12[ci]
    for s in range(n_pub + 1):
        a_s[s] += l12[m + s]
        k_s[s] += l15[m + s]
    di = bn.fr_inv(d)
    k_s = [x % R if s <= n_pub else x * di % R for s, x in enumerate(k_s)]
    return {"nVars": n_vars, "nPublic": n_pub, "m": m, "n": n, "constraints": c["constraints"],
            "A": [x % R for x in a_s], "B": [x % R for x in b_s], "K": k_s,
            "H": [t[2 * i + 1] * di % R for i in range(n)],
            "alpha": secrets[1] % R, "beta": secrets[2] % R, "delta": d % R}


def coefs_section(ks: dict) -> bytes:
    """Section 4: A's then B's terms per constraint, then the public rows; values "Montgomery twice"."""
    out, count = bytearray(), 0
    r2 = (1 << 512) % R
    for ci, (la, lb, _) in enumerate(ks["constraints"]):
        for matrix, lc in ((0, la), (1, lb)):
            for s, v in lc:
                out += struct.pack("<III", matrix, ci, s) + bn.to_le(v * r2 % R)
                count += 1
    for s in range(ks["nPublic"] + 1):
        out += struct.pack("<III", 0, ks["m"] + s, s) + bn.to_le(r2)
        count += 1
    return struct.pack("<I", count) + bytes(out)


def expected_zkey(r1cs: bytes, power: int, secrets: tuple, d: int = 1) -> bytes:
    ks = key_scalars(r1cs, power, secrets, d)
    g1 = lambda s: pc.gen_mul(False, s)
    g2 = lambda s: pc.gen_mul(True, s)
    n_pub = ks["nPublic"]
    hdr = struct.pack("<I", 32) + bn.to_le(P) + struct.pack("<I", 32) + bn.to_le(R)
    hdr += struct.pack("<III", ks["nVars"], n_pub, ks["n"])
    hdr += g1(ks["alpha"]) + g1(ks["beta"]) + g2(ks["beta"]) + g2(1) + g1(ks["delta"]) + g2(ks["delta"])
    body = [(1, struct.pack("<I", 1)), (2, hdr), (3, b"".join(g1(s) for s in ks["K"][:n_pub + 1])),
            (4, coefs_section(ks)), (5, b"".join(g1(s) for s in ks["A"])), (6, b"".join(g1(s) for s in ks["B"])),
            (7, b"".join(g2(s) for s in ks["B"])), (8, b"".join(g1(s) for s in ks["K"][n_pub + 1:])),
            (9, b"".join(g1(s) for s in ks["H"])), (10, bytes(64) + struct.pack("<I", 0))]
    return binfmt.write_binfile(b"zkey", 1, body)


# ---------------------------------------------------------------- reading and spoiling keys
OFF_DELTA1, OFF_DELTA2 = 468, 532  # in section 2


def sections(data: bytes) -> dict:
    return {sid: data[off:off + size] for sid, ((off, size),) in binfmt.read_binfile(data, b"zkey")[1].items()}


def point_bytes(sid: int) -> int:
    return 128 if sid in G2_SECTIONS else 64


def points(data: bytes, sid: int) -> list:
    body, w = sections(data)[sid], point_bytes(sid)
    return [body[i:i + w] for i in range(0, len(body), w)]


def header(data: bytes) -> dict:
    h = sections(data)[2]
    n_vars, n_pub, n = struct.unpack_from("<III", h, 72)
    return {"nVars": n_vars, "nPublic": n_pub, "n": n, "alpha1": h[84:148], "beta1": h[148:212], "beta2": h[212:340],
            "gamma2": h[340:468], "delta1": h[468:532], "delta2": h[532:660]}


def spoiled(data: bytes, sid: int, index: int, kind: str) -> bytes:
    """Point `index` of a G1 section of a key made defective, as ptau_ops_cases.spoiled does it."""
    (off, _), = binfmt.read_binfile(data, b"zkey")[1][sid]
    at = off + 64 * index
    old = data[at:at + 64]
    if kind == "zero":
        new = bytes(64)
    elif kind == "range":
        new = old[:32] + bn.to_le(P)
    else:
        x, y = bn.g1_from_lem(old)
        new = bn.g1_to_lem((x, (y + 1) % P))
    return data[:at] + new + data[at + 64:]


def section_edges(data: bytes, magic: bytes) -> list:
    edges = {12, len(data)}
    for spans in binfmt.read_binfile(data, magic)[1].values():
        for off, size in spans:
            edges |= {off - 12, off, off + size}
    return sorted(edges)


def expected_vk(data: bytes) -> dict:
    h = header(data)
    g1 = lambda b: ["0", "1", "0"] if b == bytes(64) else [str(v) for v in bn.g1_from_lem(b)] + ["1"]

    def g2(b):
        (x0, x1), (y0, y1) = bn.g2_from_lem(b)
        return [[str(x0), str(x1)], [str(y0), str(y1)], ["1", "0"]]
    return {"protocol": "groth16", "curve": "bn128", "nPublic": h["nPublic"], "vk_alpha_1": g1(h["alpha1"]),
            "vk_beta_2": g2(h["beta2"]), "vk_gamma_2": g2(h["gamma2"]), "vk_delta_2": g2(h["delta2"]),
            "IC": [g1(b) for b in points(data, 3)]}


# ---------------------------------------------------------------- a prover and the verifier
def _g1_lincomb(pts: list, scalars: list):
    acc = None
    for b, s in zip(pts, scalars):
        if s % R and b != bytes(64):
            acc = bn.g1_add(acc, bn.g1_mul(bn.g1_from_lem(b), s))
    return acc


def _g2_lincomb(pts: list, scalars: list):
    acc = None
    for b, s in zip(pts, scalars):
        if s % R and b != bytes(128):
            acc = bn.g2_add(acc, bn.g2_mul(bn.g2_from_lem(b), s))
    return acc


def quotient_evals(r1cs: bytes, witness: list, n: int) -> list:
    """h_i = (A B - C) at the odd 2n-th roots of unity, A, B, C the polynomials through the
    constraints' values on the n-th roots (the public rows: A = w_s, B = 0)."""
    c = read_r1cs(r1cs)
    m, n_pub = len(c["constraints"]), n_public_of(c)
    val = lambda lc: sum(v * witness[s] for s, v in lc) % R
    a, b, cc = [0] * n, [0] * n, [0] * n
    for ci, (la, lb, lc) in enumerate(c["constraints"]):
        a[ci], b[ci], cc[ci] = val(la), val(lb), val(lc)
        assert a[ci] * b[ci] % R == cc[ci]
    for s in range(n_pub + 1):
        a[m + s] = witness[s]
    ext = lambda ev: bn.fft(bn.ifft(ev) + [0] * n)
    ea, eb, ec = ext(a), ext(b), ext(cc)
    return [(ea[2 * i + 1] * eb[2 * i + 1] - ec[2 * i + 1]) % R for i in range(n)]


def prove(zkey: bytes, r1cs: bytes, witness: list, r: int = 0x1234567, s: int = 0x89ABCDEF1):
    """(pi_A, pi_B, pi_C) over the key's own points, r, s != 0 so B1, beta1 and delta1 matter."""
    h = header(zkey)
    n_pub = h["nPublic"]
    w = [x % R for x in witness]
    alpha1, beta1, delta1 = (bn.g1_from_lem(h[k]) for k in ("alpha1", "beta1", "delta1"))
    beta2, delta2 = bn.g2_from_lem(h["beta2"]), bn.g2_from_lem(h["delta2"])
    pi_a = bn.g1_add(bn.g1_add(alpha1, _g1_lincomb(points(zkey, 5), w)), bn.g1_mul(delta1, r))
    pi_b = bn.g2_add(bn.g2_add(beta2, _g2_lincomb(points(zkey, 7), w)), bn.g2_mul(delta2, s))
    pi_b1 = bn.g1_add(bn.g1_add(beta1, _g1_lincomb(points(zkey, 6), w)), bn.g1_mul(delta1, s))
    pi_c = bn.g1_add(_g1_lincomb(points(zkey, 8), w[n_pub + 1:]),
                     _g1_lincomb(points(zkey, 9), quotient_evals(r1cs, w, h["n"])))
    pi_c = bn.g1_add(pi_c, bn.g1_mul(pi_a, s))
    pi_c = bn.g1_add(pi_c, bn.g1_mul(pi_b1, r))
    pi_c = bn.g1_add(pi_c, bn.g1_mul(delta1, -r * s % R))
    return pi_a, pi_b, pi_c


def verify(vk: dict, public: list, proof) -> bool:
    """e(A, B) = e(alpha1, beta2) e(sum pub_i IC_i, gamma2) e(C, delta2), on a groth16_vk dict."""
    g1 = lambda v: None if v[2] == "0" else (int(v[0]), int(v[1]))
    g2 = lambda v: ((int(v[0][0]), int(v[0][1])), (int(v[1][0]), int(v[1][1])))
    pi_a, pi_b, pi_c = proof
    vkx = g1(vk["IC"][0])
    for x, ic in zip(public, vk["IC"][1:]):
        vkx = bn.g1_add(vkx, bn.g1_mul(g1(ic), x % R))
    return pairing.pairing_check([(bn.g1_neg(pi_a), pi_b), (g1(vk["vk_alpha_1"]), g2(vk["vk_beta_2"])),
                                  (vkx, g2(vk["vk_gamma_2"])), (pi_c, g2(vk["vk_delta_2"]))])
