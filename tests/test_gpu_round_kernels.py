"""The prover's round 2-5 kernels alone (include/nzcb_internal.h nzcb_debug_grand_product,
nzcb_debug_div_pol1, nzcb_debug_eval_many, nzcb_debug_quotient) against tests/round_cases.py's
plain-integer references, bit for bit, at the sizes where the tile scans change shape and with
the raw Montgomery words the kernels load at their extremes.

Shapes are written in terms of the scans' tile (T = 1024 elements per workgroup) and the
evaluation block (EB = 4096 coefficients per workgroup); the comparisons are exact, so a build
with another tile (-DNZ_KPER=2) must pass unchanged.

Limits: the intermediate products of these kernels cannot be steered from outside. The patterns
put the *inputs* (the words a kernel loads) at their extremes, a few thousand random points cover
the interior, and no bound of the kernels' comments is claimed as reached unless round_cases.py
computes that it is (round_cases.perm_column_bound_reached: the inputs alone pin 2/5 of
k_perm_tile's column bound)."""
import functools
import random

import pytest

import nzcb
import round_cases as rc

pytestmark = pytest.mark.gpu

R = rc.R
T = rc.TILE
EB = rc.EVAL_BLOCK
PATS = rc.word_patterns()
INV2 = pow(2, -1, R)


def W(m: int) -> bytes:
    return m.to_bytes(32, "little")


def VW(v: int) -> bytes:
    """The raw word of a value."""
    return W(rc.word_of(v))


def _same(got: bytes, want: bytes, what: str):
    if got == want:
        return
    assert len(got) == len(want), f"{what}: {len(got)} bytes for {len(want)}"
    bad = [i for i in range(len(want) // 32) if got[32 * i:32 * i + 32] != want[32 * i:32 * i + 32]]
    i = bad[0]
    raise AssertionError(f"{what}: {len(bad)} of {len(want) // 32} elements differ, first at {i} (tile {i // T}, "
                         f"block {i // EB}): got {got[32 * i:32 * i + 32].hex()} want {want[32 * i:32 * i + 32].hex()}")


def _rand_raw(rng: random.Random, count: int) -> bytes:
    """count random raw words below 2^253 < r, as bytes (the large cases: no per-word draw)."""
    ba = bytearray(rng.randbytes(32 * count))
    ba[31::32] = ba[31::32].translate(bytes(b & 0x1f for b in range(256)))
    return bytes(ba)


def _values(raw: bytes):
    return rc.unlem(raw)


# ---------------------------------------------------------------------------
# round 2: k_perm_tile, k_perm_factors, k_apply_tiles
# ---------------------------------------------------------------------------
def _gp_check(cols, beta_w, gamma_w, k1, k2, generics, what, want_zero_num=False, large=False):
    """cols: a, b, c, s1, s2, s3, x as raw-word byte strings of n words each; beta_w, gamma_w raw
    words; k1, k2 values. One reference, one run per entry of `generics`.

    large: every factor a + beta x + gamma is linear in (a, b, c, s1..s3, x, gamma) together, z_i
    holds as many factors above as below and the totals are compared by cross-multiplication, so
    a common factor on those inputs changes nothing that is checked: the 10^6-element case hands
    the reference the raw words themselves (the common factor is 2^256) and saves 7 n conversions."""
    if large:
        z, pn, pd = rc.grand_product(*[rc.raw_words(c) for c in cols], rc.value_of(beta_w), gamma_w, k1, k2)
    else:
        z, pn, pd = rc.grand_product(*[_values(c) for c in cols], rc.value_of(beta_w), rc.value_of(gamma_w), k1, k2)
    want = rc.lem(z) if z is not None else None
    for generic in generics:
        tag = f"{what}, {'generic k' if generic or (k1, k2) != (2, 3) else 'k = 2, 3'}"
        got, tot = nzcb.debug_grand_product(cols[0] + cols[1] + cols[2], cols[3] + cols[4] + cols[5], cols[6],
                                            W(beta_w), W(gamma_w), VW(k1), VW(k2), generic)
        t0, t1 = rc.unlem(tot)
        # the kernels' totals carry a common power of two (2^-15 per element, csrc/prover.hip)
        assert t0 * pd % R == t1 * pn % R, f"k_perm_factors totals ({tag})"
        if want is None:        # prod D = 0: no defined z (the all-zero pattern); the totals still say so
            assert t1 == 0, f"k_perm_factors totals[1] with prod D = 0 ({tag})"
            continue
        assert t1 != 0, f"k_perm_factors totals[1] ({tag})"
        if want_zero_num:
            assert t0 == 0 != t1, f"k_perm_factors totals with a zero numerator ({tag})"
        _same(got, want, f"grand product z ({tag})")


@functools.lru_cache(maxsize=2)
def _gp_random_cols(n: int):
    rng = random.Random(0x9e3779b9 ^ n)
    if n > 4 * T:
        return tuple(_rand_raw(rng, n) for _ in range(7))
    return tuple(rc.raw_bytes(rc.random_words(rng, n)) for _ in range(7))


GP_SIZES = [1, 2, 5, T - 1, T, T + 1, 2 * T + 3, 65 * T + 7, 1025 * T + 1]


@pytest.mark.parametrize("kmode", ["k23", "generic"])
@pytest.mark.parametrize("n", GP_SIZES)
def test_grand_product_sizes(n, kmode):
    """Random words at every tile count where k_perm_factors' scan changes shape: one tile, a
    ragged second, several waves of tiles with one tile per thread (65 T + 7) and two tiles per
    thread with a ragged tail (1025 T + 1). k23 runs k1, k2 = 2, 3 by additions and by the
    generic products against one reference; generic runs k1 = r - 1 and a random k2."""
    rng = random.Random(n * 31 + len(kmode))
    cols = _gp_random_cols(n)
    beta_w, gamma_w = rng.randrange(R), rng.randrange(R)
    if kmode == "k23":
        _gp_check(cols, beta_w, gamma_w, 2, 3, (False, True), f"n = {n}", large=n > 4 * T)
    else:
        _gp_check(cols, beta_w, gamma_w, R - 1, rng.randrange(R), (False,), f"n = {n}", large=n > 4 * T)


@pytest.mark.parametrize("n", [5, 2 * T + 3])
def test_grand_product_all_columns_at_a_pattern(n):
    """Every column, x and gamma at each raw-word pattern at once (all-max limbs in x and gamma is
    the nearest a caller can push k_perm_tile's 5 2^29 column bound: round_cases
    .perm_column_bound_reached). The all-zero pattern has prod D = 0: only its totals are checked."""
    rng = random.Random(n)
    for p in PATS:
        col = W(p) * n
        for k1, k2, generics in ((2, 3, (False, True)), (R - 1, rng.randrange(R), (False,))):
            _gp_check((col,) * 7, rng.randrange(R), p, k1, k2, generics, f"n = {n}, pattern {p:#x}")


def test_grand_product_beta_patterns():
    n = 300
    rng = random.Random(300)
    cols = _gp_random_cols(n)
    for bw in rc.challenge_words():
        _gp_check(cols, bw, rng.randrange(R), 2, 3, (False, True), f"beta word {bw:#x}")
        _gp_check(cols, bw, rng.randrange(R), R - 1, rng.randrange(R), (False,), f"beta word {bw:#x}")
    for gw in rc.challenge_words():
        _gp_check(cols, rng.randrange(R), gw, 2, 3, (False, True), f"gamma word {gw:#x}")


def test_grand_product_zero_witness_columns():
    n = 2 * T + 3
    cols = _gp_random_cols(n)
    zero = bytes(32 * n)
    rng = random.Random(7)
    _gp_check((zero, zero, zero) + cols[3:], rng.randrange(R), rng.randrange(R), 2, 3, (False, True), "a = b = c = 0")
    _gp_check((zero, zero, zero) + cols[3:], rng.randrange(R), rng.randrange(R), R - 1, 12345, (False,),
              "a = b = c = 0")


@pytest.mark.parametrize("at", [T - 1, T])
def test_grand_product_zero_numerator_factor(at):
    """a_i = -beta x_i - gamma at the last element of tile 0 / the first of tile 1: z is 0 past
    it and totals[0] = 0 != totals[1]."""
    n = 2 * T + 3
    cols = list(_gp_random_cols(n))
    rng = random.Random(at)
    beta_w, gamma_w = rng.randrange(R), rng.randrange(R)
    x_at = rc.value_of(int.from_bytes(cols[6][32 * at:32 * at + 32], "little"))
    a_at = (-rc.value_of(beta_w) * x_at - rc.value_of(gamma_w)) % R
    cols[0] = cols[0][:32 * at] + VW(a_at) + cols[0][32 * at + 32:]
    _gp_check(tuple(cols), beta_w, gamma_w, 2, 3, (False, True), f"zero factor at {at}", want_zero_num=True)
    z, _, _ = rc.grand_product(*[_values(c) for c in cols], rc.value_of(beta_w), rc.value_of(gamma_w), 2, 3)
    assert all(v == 0 for v in z[at + 1:]) and all(v != 0 for v in z[:at + 1])


# ---------------------------------------------------------------------------
# round 5: lin_tables, k_lin_tile, k_tile_heads, k_div_check
# ---------------------------------------------------------------------------
def _div_ds():
    rng = random.Random(5)
    return {"0": 0, "1": 1, "r-1": R - 1, "2": 2, "random": rng.randrange(R), "root4": rc.root_of_unity(4),
            "root1024": rc.root_of_unity(1024), "root4096": rc.root_of_unity(4096)}


DIV_DS = _div_ds()
DIV_SIZES = [2, 3, 5, T - 1, T, T + 1, T + 2, 2 * T + 1, 65 * T + 9, 1025 * T + 2]


@functools.lru_cache(maxsize=2)
def _div_quotient(m: int):
    """A random quotient Q of m - 1 coefficients: (values, the bytes the entry must return)."""
    raw = _rand_raw(random.Random(m), m - 1)
    return _values(raw), raw + bytes(32)


@pytest.mark.parametrize("dname", list(DIV_DS))
@pytest.mark.parametrize("m", DIV_SIZES)
def test_div_pol1_sizes(m, dname):
    """P = (X - d) Q: the exact quotient and divides = 1; P[0] + 1 and P[m-1] + 1 must report
    divides = 0 (as the recurrence says: d = 0 still divides after P[m-1] + 1) with the quotient
    still the recurrence's; a p0_adjust that repairs the remainder reports divides = 1. Tile
    counts 1, 2, 3, 66 (one tile per thread of k_tile_heads, several waves) and 1026 (two per
    thread, ragged); the roots of unity make the kernels' power tables cycle or all ones."""
    d = DIV_DS[dname]
    qv, qbytes = _div_quotient(m)
    p = rc.times_linear(qv, d)
    pb = rc.lem(p)
    what = f"divPol1 m = {m}, d = {dname}"
    got, ok = nzcb.debug_div_pol1(pb, VW(d))
    _same(got, qbytes, what)
    assert ok, f"k_div_check: {what} divides"
    # a remainder in P[0]: same quotient, the check fires; p0_adjust repairs it
    p0 = VW((p[0] + 1) % R)
    got, ok = nzcb.debug_div_pol1(p0 + pb[32:], VW(d))
    _same(got, qbytes, what + ", P[0] + 1")
    assert not ok, f"k_div_check: {what}, P[0] + 1 must not divide"
    got, ok = nzcb.debug_div_pol1(p0 + pb[32:], VW(d), VW(1))
    _same(got, qbytes, what + ", P[0] + 1 repaired")
    assert ok, f"k_div_check: {what}, p0_adjust = 1 repairs P[0] + 1"
    # a remainder from the top coefficient: the recurrence's quotient and verdict
    p2 = p[:-1] + [(p[-1] + 1) % R]
    q2, ok2 = rc.div_pol1(p2, d)
    assert ok2 == (d == 0)
    got, ok = nzcb.debug_div_pol1(pb[:-32] + VW(p2[-1]), VW(d))
    _same(got, rc.lem(q2), what + ", P[m-1] + 1")
    assert ok == ok2, f"k_div_check: {what}, P[m-1] + 1"


@pytest.mark.parametrize("dname", list(DIV_DS))
def test_div_pol1_coefficient_patterns(dname):
    d = DIV_DS[dname]
    m = T + 2
    mixed = [PATS[i % len(PATS)] for i in range(m)]
    for words in [[p] * m for p in PATS] + [mixed]:
        q, ok = rc.div_pol1([rc.value_of(w) for w in words], d)
        got, gok = nzcb.debug_div_pol1(rc.raw_bytes(words), VW(d))
        _same(got, rc.lem(q), f"divPol1 m = {m}, d = {dname}, coefficient words {words[0]:#x}..")
        assert gok == ok, f"k_div_check: d = {dname}, coefficient words {words[0]:#x}.."


# ---------------------------------------------------------------------------
# round 4: k_eval_pows, k_eval_multi, k_eval_sum
# ---------------------------------------------------------------------------
def _eval_xs():
    rng = random.Random(4)
    return [0, 1, R - 1, rng.randrange(R), rc.root_of_unity(256), rc.root_of_unity(4096)]


EVAL_XS = _eval_xs()
EVAL_LENS = [1, 255, 256, 257, EB - 1, EB, EB + 1, 17 * EB + 5, 257 * EB + 5]


@functools.lru_cache(maxsize=16)
def _eval_poly(length: int, seed: int = 0):
    rng = random.Random(length * 7 + seed)
    raw = _rand_raw(rng, length) if length > 2 * EB else rc.raw_bytes(rc.random_words(rng, length))
    return raw, _values(raw)


@pytest.mark.parametrize("length", EVAL_LENS)
def test_eval_one(length):
    """np = 1 against Horner: one coefficient, around the 256 coefficients of one Horner step,
    around one block, 18 blocks, and 258 blocks, where k_eval_sum's threads take a second
    partial sum each."""
    raw, vals = _eval_poly(length)
    for x in EVAL_XS:
        got = nzcb.debug_eval_many([raw], VW(x))
        _same(got, VW(rc.horner(vals, x)), f"k_eval_multi<1>, len = {length}, x = {x:#x}")


def _eval7(lens, xs, what):
    polys = [_eval_poly(ln, seed=j) for j, ln in enumerate(lens)]
    got = nzcb.debug_eval_many([p[0] for p in polys], b"".join(VW(x) for x in xs))
    want = b"".join(VW(rc.horner(p[1], x)) for p, x in zip(polys, xs))
    for j in range(7):
        _same(got[32 * j:32 * j + 32], want[32 * j:32 * j + 32], f"k_eval_multi<7> {what}, polynomial {j}")


@pytest.mark.parametrize("power", [10, 12])
def test_eval_seven_prover_shape(power):
    n = 1 << power
    w = rc.root_of_unity(n)
    lens = (n + 2, n + 2, n + 2, n, n, 3 * n + 6, n + 3)
    for x in EVAL_XS:
        _eval7(lens, [x] * 6 + [x * w % R], f"n = 2^{power}, x = {x:#x}")


def test_eval_seven_uneven_lengths():
    """Some polynomials end whole blocks before the longest; one point for all, then a
    different point per polynomial."""
    lens = (1, EB, EB + 1, 3, 2 * EB, 2 * EB + 1, 256)
    for i, x in enumerate(EVAL_XS):
        _eval7(lens, [x] * 7, f"uneven, x = {x:#x}")
        _eval7(lens, [EVAL_XS[(i + j) % len(EVAL_XS)] for j in range(7)], f"uneven, points rotated by {i}")


@pytest.mark.parametrize("word", [R - 1, rc.max_limb_word()], ids=["r-1", "maxlimbs"])
def test_eval_extreme_coefficients(word):
    n = EB + 1
    raw, v = W(word) * n, [rc.value_of(word)] * n
    for x in EVAL_XS:
        _same(nzcb.debug_eval_many([raw], VW(x)), VW(rc.horner(v, x)), f"k_eval_multi<1>, words {word:#x}, x = {x:#x}")
    short = [(W(word) * ln, [rc.value_of(word)] * ln) for ln in (n, n, n, 5, 256, 257, 2 * EB)]
    for x in EVAL_XS:
        got = nzcb.debug_eval_many([p[0] for p in short], VW(x) * 7)
        for j, p in enumerate(short):
            _same(got[32 * j:32 * j + 32], VW(rc.horner(p[1], x)),
                  f"k_eval_multi<7>, words {word:#x}, x = {x:#x}, polynomial {j}")


# ---------------------------------------------------------------------------
# round 3: k_quotient_coset29<three>, k_beta_xlo, k_quotient_coset
# ---------------------------------------------------------------------------
Q_SCALE = (10, 5, 5, 5, 0)     # the context's exponent pre-scaling of qm, ql, qr, qo, qc; L_j: 5


def _unscale(col, e):
    """The entry's input whose pre-scaled word (x 2^e) is the given one."""
    f = pow(INV2, e, R)
    return [m * f % R for m in col]


def _quot_check(power, three, npub, abcz, q, s, ls, apub, ch, k1, k2, what, scaled=True):
    """Columns of raw words. scaled: q and ls are the words the kernel is to load after the
    entry's pre-scaling (the entry gets them unscaled); else they are the entry's inputs."""
    if scaled:
        q = [_unscale(c, e) for c, e in zip(q, Q_SCALE)]
        ls = [_unscale(c, 5) for c in ls]
    val = lambda cols: [[rc.value_of(m) for m in c] for c in cols]
    beta, gamma, alpha = (rc.value_of(m) for m in ch)
    want = rc.quotient(power, three, val(abcz), val(q), val(s), val(ls), [rc.value_of(m) for m in apub], beta, gamma,
                       alpha, k1, k2)
    flat = lambda cols: b"".join(rc.raw_bytes(c) for c in cols)
    got = nzcb.debug_quotient(power, three, npub, flat(abcz), flat(q), flat(s), flat(ls), rc.raw_bytes(apub), W(ch[0]),
                              W(ch[1]), W(ch[2]), VW(k1), VW(k2))
    kern = "k_quotient_coset29<true>" if three else "k_quotient_coset29<false>" if npub <= 8 else "k_quotient_coset"
    _same(got, rc.lem(want), f"{kern}, power {power}, npub {npub}, {what}")


def _quot_random(rng, pts, nl, npub):
    cols = lambda k: [rc.random_words(rng, pts) for _ in range(k)]
    return cols(4), cols(5), cols(3), cols(nl), rc.random_words(rng, npub)


@pytest.mark.parametrize("generic", [False, True], ids=["k23", "generic"])
@pytest.mark.parametrize("npub", [0, 1, 4, 5, 8])
@pytest.mark.parametrize("three", [False, True], ids=["four", "three"])
@pytest.mark.parametrize("power", [2, 3])
def test_quotient_input_patterns(power, three, npub, generic):
    """Every point's loaded words at the patterns: all columns of a point at one pattern, then
    each column at a different one; the public inputs at patterns too. The challenges are
    random here (test_quotient_challenge_patterns)."""
    rng = random.Random(power * 1000 + three * 100 + npub * 2 + generic)
    pts = (3 if three else 4) << power
    nl = max(npub, 1)
    k1, k2 = (R - 1, rng.randrange(R)) if generic else (2, 3)
    for off in range(0, len(PATS), pts):
        for rot in (0, 1):
            col = lambda c: [PATS[(i + off + rot * c) % len(PATS)] for i in range(pts)]
            abcz = [col(c) for c in range(4)]
            q = [col(4 + c) for c in range(5)]
            s = [col(9 + c) for c in range(3)]
            ls = [col(12 + c) for c in range(nl)]
            apub = [PATS[(j + off + rot) % len(PATS)] for j in range(npub)]
            ch = rc.random_words(rng, 3)
            _quot_check(power, three, npub, abcz, q, s, ls, apub, ch, k1, k2,
                        f"patterns from {off}, {'rotated' if rot else 'aligned'}")


@pytest.mark.parametrize("which", [0, 1, 2], ids=["beta", "gamma", "alpha"])
def test_quotient_challenge_patterns(which):
    rng = random.Random(which)
    configs = [(p, t, npub, g) for p in (2, 3) for t in (False, True) for npub in (0, 1, 4, 5, 8) for g in (False, True)]
    for i, w in enumerate(rc.challenge_words()):
        for power, three, npub, generic in (configs[(2 * i) % len(configs)], configs[(2 * i + 21) % len(configs)]):
            pts = (3 if three else 4) << power
            abcz, q, s, ls, apub = _quot_random(rng, pts, max(npub, 1), npub)
            ch = rc.random_words(rng, 3)
            ch[which] = w
            k1, k2 = (R - 1, rng.randrange(R)) if generic else (2, 3)
            _quot_check(power, three, npub, abcz, q, s, ls, apub, ch, k1, k2,
                        f"{'beta gamma alpha'.split()[which]} word {w:#x}, {'generic' if generic else 'k23'}",
                        scaled=False)


@pytest.mark.parametrize("three,npub", [(False, 3), (True, 3), (False, 9)], ids=["four", "three", "four-8x32"])
def test_quotient_power_11(three, npub):
    """Random words at the first size where the point tables' high index passes 0 (4n > 4096);
    npub = 9 runs the 8x32 kernel against the same reference."""
    rng = random.Random(11 + npub + three)
    pts = (3 if three else 4) << 11
    abcz, q, s, ls, apub = _quot_random(rng, pts, npub, npub)
    for k1, k2 in ((2, 3), (R - 1, rng.randrange(R))):
        _quot_check(11, three, npub, abcz, q, s, ls, apub, rc.random_words(rng, 3), k1, k2, f"random, k1 = {k1:#x}",
                    scaled=False)


def test_argument_errors():
    """three = 1 past 8 public inputs is not a path the context runs; words at or above r are
    refused by every entry."""
    rng = random.Random(1)
    pts = 3 << 2
    abcz, q, s, ls, apub = _quot_random(rng, pts, 9, 9)
    flat = lambda cols: b"".join(rc.raw_bytes(c) for c in cols)
    one = VW(1)
    with pytest.raises(nzcb.NzcbError) as e:
        nzcb.debug_quotient(2, True, 9, flat(abcz), flat(q), flat(s), flat(ls), rc.raw_bytes(apub), one, one, one,
                            VW(2), VW(3))
    assert e.value.name == "ARG"
    big = W(R)
    with pytest.raises(nzcb.NzcbError) as e:
        nzcb.debug_quotient(2, True, 1, flat(abcz), flat(q), flat(s), flat(ls[:1]), big, one, one, one, VW(2), VW(3))
    assert e.value.name == "ARG"
    with pytest.raises(nzcb.NzcbError) as e:
        nzcb.debug_grand_product(one * 3, one * 3, one, big, one, VW(2), VW(3))
    assert e.value.name == "ARG"
    with pytest.raises(nzcb.NzcbError) as e:
        nzcb.debug_div_pol1(one + big, one)
    assert e.value.name == "ARG"
    with pytest.raises(nzcb.NzcbError) as e:
        nzcb.debug_eval_many([one + big], one)
    assert e.value.name == "ARG"
    with pytest.raises(nzcb.NzcbError) as e:
        nzcb.debug_eval_many([one, one], one * 2)      # np = 2: not an instantiation
    assert e.value.name == "ARG"
