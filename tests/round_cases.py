"""References for the prover's round 2-5 kernels (include/nzcb_internal.h nzcb_debug_grand_product,
nzcb_debug_div_pol1, nzcb_debug_eval_many, nzcb_debug_quotient): plain Python integers mod r,
no library code, no tiles, no Montgomery form. tests/test_round_cases.py holds them against
oracle/plonk.py on real proofs; tests/test_gpu_round_kernels.py holds the kernels against them.

The kernels load raw 32-byte Montgomery words m (the value is m 2^-256 mod r), so the edge
patterns below are raw words: ``lem`` / ``unlem`` move between a word string and values.
"""
import random

R = 21888242871839275222246405745257275088548364400416034343698204186575808495617
RINV = pow(1 << 256, -1, R)      # 2^-256 mod r
TWO_ADICITY = 28                 # r - 1 = 2^28 * odd
GEN = 5                          # a generator of F_r^* (ffjavascript's nqr); also the quotient's coset shift g

TILE = 1024                      # elements per workgroup of the tile scans (kTileN = kT * kPer)
EVAL_BLOCK = 4096                # coefficients per workgroup of the evaluation (kT * kEvalChunk2)


# ---------------------------------------------------------------------------
# words <-> values
# ---------------------------------------------------------------------------
def word_of(v: int) -> int:
    """The raw Montgomery word of the value v."""
    return (v << 256) % R


def value_of(m: int) -> int:
    return m * RINV % R


def raw_bytes(words) -> bytes:
    """Raw words as the entries take them (32-byte LE each)."""
    return b"".join(m.to_bytes(32, "little") for m in words)


def raw_words(data: bytes):
    return [int.from_bytes(data[i:i + 32], "little") for i in range(0, len(data), 32)]


def lem(values) -> bytes:
    return raw_bytes([(v << 256) % R for v in values])


def unlem(data: bytes):
    return [m * RINV % R for m in raw_words(data)]


def root_of_unity(order: int) -> int:
    """A primitive root of unity of `order` (a power of two up to 2^28)."""
    assert order & (order - 1) == 0 and order <= 1 << TWO_ADICITY
    w = pow(GEN, (R - 1) // order, R)
    assert order == 1 or pow(w, order // 2, R) != 1
    return w


# ---------------------------------------------------------------------------
# value patterns (raw Montgomery words m < r)
# ---------------------------------------------------------------------------
def max_limb_word() -> int:
    """The largest m < r whose eight low 29-bit limbs are all 2^29 - 1."""
    low = (1 << 232) - 1
    m = ((R - 1) >> 232 << 232) | low
    if m >= R:
        m -= 1 << 232
    assert m < R and m & low == low and m + (1 << 232) >= R
    return m


def word_patterns():
    ps = [0, 1, R - 1, max_limb_word()]
    for k in range(1, 9):
        ps += [1 << (29 * k), (1 << (29 * k)) - 1]
    ps += [(R - 1) // 2, (R + 1) // 2]
    assert all(0 <= m < R for m in ps) and len(set(ps)) == len(ps)
    return ps


def challenge_words():
    """Raw words for beta, gamma, alpha: the patterns, and the canonical values r - 1, 1, 2^253."""
    return word_patterns() + [word_of(R - 1), word_of(1), word_of(1 << 253)]


def random_words(rng: random.Random, count: int):
    return [rng.randrange(R) for _ in range(count)]


# ---------------------------------------------------------------------------
# round 2: the grand product
# ---------------------------------------------------------------------------
def grand_product(a, b, c, s1, s2, s3, x, beta, gamma, k1, k2):
    """N_i = (a_i + beta x_i + gamma)(b_i + k1 beta x_i + gamma)(c_i + k2 beta x_i + gamma), D_i the
    same with sigma_k in place of k x; z_i = prod_{k<i} N_k prod_{k>=i} D_k / prod D.
    Returns (z, prod N, prod D); z is None when prod D = 0 (no defined answer)."""
    n = len(x)
    num, den = [0] * n, [0] * n
    for i in range(n):
        bx = beta * x[i] % R
        num[i] = (a[i] + bx + gamma) * (b[i] + k1 * bx + gamma) % R * (c[i] + k2 * bx + gamma) % R
        den[i] = (a[i] + beta * s1[i] + gamma) * (b[i] + beta * s2[i] + gamma) % R * (c[i] + beta * s3[i] + gamma) % R
    suf = [1] * (n + 1)                       # suf[i] = prod_{k>=i} D_k
    for i in range(n - 1, -1, -1):
        suf[i] = suf[i + 1] * den[i] % R
    prod_d = suf[0]
    z, pre = None, 1                          # pre = prod_{k<i} N_k
    if prod_d:
        inv = pow(prod_d, -1, R)
        z = [0] * n
        for i in range(n):
            z[i] = pre * suf[i] % R * inv % R
            pre = pre * num[i] % R
    else:
        for i in range(n):
            pre = pre * num[i] % R
    return z, pre, prod_d


# ---------------------------------------------------------------------------
# round 5: divPol1
# ---------------------------------------------------------------------------
def div_pol1(p, d, p0_adjust=0):
    """oracle.plonk._div_pol1's recurrence: q[m-1] = 0, q[m-2] = p[m-1], q[i] = p[i+1] + d q[i+1].
    Returns (q, divides) with divides iff p[0] - p0_adjust == -d q[0]."""
    m = len(p)
    q = [0] * m
    q[m - 2] = p[m - 1] % R
    for i in range(m - 3, -1, -1):
        q[i] = (p[i + 1] + d * q[i + 1]) % R
    return q, (p[0] - p0_adjust) % R == (-d * q[0]) % R


def times_linear(q, d):
    """(X - d) Q."""
    p = [0] * (len(q) + 1)
    for i, c in enumerate(q):
        p[i + 1] = c
    for i, c in enumerate(q):
        p[i] = (p[i] - d * c) % R
    return p


# ---------------------------------------------------------------------------
# round 4: evaluation
# ---------------------------------------------------------------------------
def horner(p, x):
    acc = 0
    for c in reversed(p):
        acc = (acc * x + c) % R
    return acc


# ---------------------------------------------------------------------------
# round 3: the quotient's numerator, point by point
# ---------------------------------------------------------------------------
def quotient_num(a, b, c, z, zw, qm, ql, qr, qo, qc, s1, s2, s3, ls, apub, x, beta, gamma, alpha, k1, k2):
    """N = qm a b + ql a + qr b + qo c + qc - sum_j L_j apub_j
         + alpha [(a + beta x + gamma)(b + k1 beta x + gamma)(c + k2 beta x + gamma) z
                  - (a + beta s1 + gamma)(b + beta s2 + gamma)(c + beta s3 + gamma) z_w]
         + alpha^2 (z - 1) L_0
    at one point x. ls: L_0.. at the point (at least L_0), apub: the public inputs."""
    gate = (qm * a * b + ql * a + qr * b + qo * c + qc) % R
    for lj, pj in zip(ls, apub):
        gate -= lj * pj
    bx = beta * x % R
    num = (a + bx + gamma) * (b + k1 * bx + gamma) % R * (c + k2 * bx + gamma) % R * z % R
    den = (a + beta * s1 + gamma) * (b + beta * s2 + gamma) % R * (c + beta * s3 + gamma) % R * zw % R
    return (gate + alpha * (num - den) + alpha * alpha % R * (z - 1) % R * ls[0]) % R


def quotient_points(power: int, three: bool):
    """The kernels' point order: [(x, index of z(w x))] over P = 3n (three) or 4n points, on the
    coset g <w4> of the 4n-th roots of unity."""
    n = 1 << power
    w4 = root_of_unity(4 * n)
    pw = [1] * (4 * n)
    for i in range(1, 4 * n):
        pw[i] = pw[i - 1] * w4 % R
    if three:
        return [(GEN * pw[4 * m + j] % R, j * n + (m + 1) % n) for j in range(3) for m in range(n)]
    return [(GEN * pw[i] % R, (i + 4) % (4 * n)) for i in range(4 * n)]


def quotient(power, three, abcz, q, s, ls, apub, beta, gamma, alpha, k1, k2, pts=None):
    """What the kernel stores over columns of values (abcz: 4, q: 5, s: 3, ls: max(npub, 1)
    columns of P values): N(x) for three, N(x) / (x^n - 1) for the 4n form."""
    n = 1 << power
    pts = pts or quotient_points(power, three)
    out = []
    for i, (x, izw) in enumerate(pts):
        v = quotient_num(abcz[0][i], abcz[1][i], abcz[2][i], abcz[3][i], abcz[3][izw], q[0][i], q[1][i], q[2][i],
                         q[3][i], q[4][i], s[0][i], s[1][i], s[2][i], [col[i] for col in ls], apub, x, beta, gamma,
                         alpha, k1, k2)
        if not three:
            v = v * pow(pow(x, n, R) - 1, -1, R) % R
        out.append(v)
    return out


# ---------------------------------------------------------------------------
# the bound chains of csrc/prover.hip's comments, at the patterns
# ---------------------------------------------------------------------------
def limbs29(m: int):
    """The 9x29 split of a 256-bit word (csrc/f29.h split29): eight 29-bit limbs and the rest."""
    return [(m >> (29 * k)) & ((1 << 29) - 1) for k in range(8)] + [m >> 232]


def perm_column_bound_reached():
    """k_perm_tile's comment bounds a limb of x + 3 b w + g by 5 2^29, with b w a Shoup product's
    normalized limbs (< 2^29 each below the top one). With x and gamma at the all-max-limbs word
    their eight low limbs are 2^29 - 1 each, so a low limb of the factor is 2 (2^29 - 1) + 3 l for
    the Shoup product's limb l, which the caller does not choose. Returns the largest share of
    the 5 2^29 bound the inputs alone pin: 2 (2^29 - 1) / (5 2^29) < 1, i.e. the bound itself is
    NOT claimed as reached."""
    lo = limbs29(max_limb_word())[:8]
    assert all(v == (1 << 29) - 1 for v in lo)
    return 2 * ((1 << 29) - 1) / (5 * (1 << 29))
