"""Shared cases of the batch-verifier tests (tests/test_verify_batch.py on the host path,
tests/test_gpu_verify_batch.py on the device): term lists for the G1 group routine with their
oracle answers, and ways to spoil a proof."""
import random

from oracle import bn254 as bn, plonk

R = bn.R_MOD
G = bn.G1_GEN
NEG_G = bn.g1_neg(G)
EDGE_SCALARS = (0, 1, 2, R - 1, 1 << 253)


def pt_bytes(pt) -> bytes:
    return bytes(64) if pt is None else bn.to_le(pt[0]) + bn.to_le(pt[1])


def pack(groups):
    """groups: list of lists of (point, scalar) -> (points, scalars, group_end)."""
    pts, scs, ends = b"", b"", []
    n = 0
    for g in groups:
        for p, k in g:
            pts += pt_bytes(p)
            scs += bn.to_le(k)
        n += len(g)
        ends.append(n)
    return pts, scs, ends


def oracle_sums(groups):
    out = []
    for g in groups:
        acc = None
        for p, k in g:
            acc = bn.g1_add(acc, bn.g1_mul(p, k))
        out.append(pt_bytes(acc))
    return out


def edge_groups():
    """Issue cases: scalars 0, 1, 2, r-1, 2^253 and seeded random ones on G, -G and infinity
    (one group per term), P + P, P + (-P) by r-1, an empty group, and a mixed group."""
    rng = random.Random(0x6C696E63)
    scalars = list(EDGE_SCALARS) + [rng.randrange(R) for _ in range(3)]
    groups = [[(b, k)] for b in (G, NEG_G, None) for k in scalars]
    p = bn.g1_mul(G, 0xD1CE)
    groups += [[(p, 1), (p, 1)], [(p, 1), (p, R - 1)], [], [(p, 5), (bn.g1_neg(p), 5)],
               [(G, 3), (None, 7), (p, R - 1), (NEG_G, 1 << 253), (p, 0)], []]
    return groups


def random_groups(n_terms, sizes, seed):
    """n_terms seeded random terms over a few bases, cut into groups of the sizes in `sizes`
    in turn (the last group takes what is left)."""
    rng = random.Random(seed)
    bases = [bn.g1_mul(G, rng.randrange(1, R)) for _ in range(5)] + [None]
    terms = [(bases[rng.randrange(len(bases))], rng.randrange(R)) for _ in range(n_terms)]
    groups, i, k = [], 0, 0
    while i < n_terms:
        s = min(sizes[k % len(sizes)], n_terms - i)
        groups.append(terms[i:i + s])
        i += s
        k += 1
    return groups


def pub_bytes(pub) -> bytes:
    return b"".join(int(x).to_bytes(32, "little") for x in pub)


def tamper(proof: bytes, pub: bytes, kind: str):
    """A spoiled copy of (proof, pub): 'eval' an evaluation + 1, 'point' T2 + G, 'pub' a public
    signal + 1 (all well formed: only the pairing tells), 'offcurve' a point off the curve,
    'big' an evaluation >= r (both rejected before the sums)."""
    p = plonk.proof_from_bytes(proof)
    if kind == "eval":
        p["eval_zw"] = (p["eval_zw"] + 1) % R
    elif kind == "point":
        p["T2"] = bn.g1_add(p["T2"], G)
    elif kind == "pub":
        return proof, bn.to_le((bn.from_le(pub[:32]) + 1) % R) + pub[32:]
    elif kind == "offcurve":
        b = bytearray(proof)
        b[64] ^= 1  # B.x
        return bytes(b), pub
    elif kind == "big":
        b = bytearray(proof)
        b[576:608] = (R + 1).to_bytes(32, "little")  # eval_a
        return bytes(b), pub
    else:
        raise ValueError(kind)
    return plonk.proof_to_bytes(p), pub
