"""tests/round_cases.py's references agree with oracle/plonk.py on real proofs: Z on H, both
divPol1 outputs, the seven evaluations and T on the 4n domain. This anchors the references the
round-kernel tests (tests/test_gpu_round_kernels.py) compare against to the oracle, not to the
kernels, and runs without a GPU."""
import json
import os

import pytest

import round_cases as rc
from oracle import binfmt, plonk, synth
from oracle.bn254 import FR_W, R_MOD

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def _p5():
    with open(os.path.join(GOLD, "p5.json")) as f:
        meta = json.load(f)
    with open(os.path.join(GOLD, "p5.zkey"), "rb") as f:
        zk = binfmt.read_zkey(f.read())
    c = synth.synth_circuit(meta["power"], meta["n_public"], meta["n_inputs"], seed=meta["seed"])
    return zk, c["witness"]


def _synth6():
    c = synth.synth_circuit(6, 3, 5, seed=23)
    return plonk.setup(c, 1234577), c["witness"]


@pytest.fixture(scope="module", params=["p5", "synth6"])
def proved(request):
    zk, wit = _p5() if request.param == "p5" else _synth6()
    tr = {}
    proof, _ = plonk.prove(zk, wit, synth.fixed_blindings(), trace=tr)
    return zk, proof, tr


def test_constants():
    assert rc.R == R_MOD
    assert rc.root_of_unity(1 << 7) == FR_W[7]
    assert rc.value_of(rc.word_of(12345)) == 12345
    assert rc.unlem(rc.lem([0, 1, rc.R - 1])) == [0, 1, rc.R - 1]
    ps = rc.word_patterns()
    assert len(ps) == 22 and rc.limbs29(rc.max_limb_word())[:8] == [(1 << 29) - 1] * 8
    assert 0 < rc.perm_column_bound_reached() < 1


def test_grand_product_is_the_oracles_z(proved):
    zk, _, tr = proved
    n = zk["domainSize"]
    w = FR_W[zk["power"]]
    x = [pow(w, i, rc.R) for i in range(n)]
    s = [zk["sigma"][k][1][::4] for k in range(3)]
    z, pn, pd = rc.grand_product(tr["A"], tr["B"], tr["C"], s[0], s[1], s[2], x, tr["beta"], tr["gamma"], zk["k1"],
                                 zk["k2"])
    assert z == tr["Z"]
    assert pn == pd != 0          # the copy constraints hold


def test_grand_product_ignores_a_common_factor():
    """What the 10^6-element kernel test relies on when it hands the reference raw Montgomery
    words: a common factor on the columns and gamma leaves z unchanged and scales both totals
    alike."""
    import random
    rng = random.Random(3)
    n, lam = 37, rng.randrange(1, rc.R)
    cols = [rc.random_words(rng, n) for _ in range(7)]
    beta, gamma = rng.randrange(rc.R), rng.randrange(rc.R)
    z, pn, pd = rc.grand_product(*cols, beta, gamma, 2, 3)
    z2, pn2, pd2 = rc.grand_product(*[[v * lam % rc.R for v in c] for c in cols], beta, gamma * lam % rc.R, 2, 3)
    assert z2 == z and pn2 * pd % rc.R == pd2 * pn % rc.R and pd2 == pd * pow(lam, 3 * n, rc.R) % rc.R


def test_div_pol1_is_the_oracles(proved):
    zk, proof, tr = proved
    w = FR_W[zk["power"]]
    q, ok = rc.div_pol1(tr["wxi_num"], tr["xi"])
    assert ok and q == tr["pol_wxi"]
    q, ok = rc.div_pol1(tr["wxiw_num"], tr["xi"] * w % rc.R)
    assert ok and q == tr["pol_wxiw"]
    # the prover's own form of the second one: the evaluation as p0_adjust
    q2, ok = rc.div_pol1(tr["pol_z"], tr["xi"] * w % rc.R, proof["eval_zw"])
    assert ok and q2 == q
    assert not rc.div_pol1(tr["pol_z"], tr["xi"] * w % rc.R, proof["eval_zw"] + 1)[1]
    assert rc.div_pol1(rc.times_linear(tr["pol_wxi"][:-1], tr["xi"]), tr["xi"])[0] == tr["pol_wxi"]
    with pytest.raises(plonk.ProverError):
        plonk._div_pol1([tr["wxi_num"][0] + 1] + tr["wxi_num"][1:], tr["xi"])
    assert not rc.div_pol1([tr["wxi_num"][0] + 1] + tr["wxi_num"][1:], tr["xi"])[1]


def test_horner_is_the_oracles_evaluations(proved):
    zk, proof, tr = proved
    xi, w = tr["xi"], FR_W[zk["power"]]
    polys = {"a": tr["pol_a"], "b": tr["pol_b"], "c": tr["pol_c"], "s1": zk["sigma"][0][0], "s2": zk["sigma"][1][0],
             "r": tr["pol_r"]}
    for k, p in polys.items():
        assert rc.horner(p, xi) == proof["eval_" + k]
    assert rc.horner(tr["pol_t"], xi) == tr["eval_t"]
    assert rc.horner(tr["pol_z"], xi * w % rc.R) == proof["eval_zw"]


def test_quotient_num_is_the_oracles_t(proved):
    """The oracle evaluates T on the plain 4n domain (x_i = w4^i) over the unblinded columns;
    the same per-point formula there is its T[i]."""
    zk, _, tr = proved
    n = zk["domainSize"]
    w4 = FR_W[zk["power"] + 2]
    pts = [(pow(w4, i, rc.R), (i + 4) % (4 * n)) for i in range(4 * n)]
    abcz = [tr["A4"], tr["B4"], tr["C4"], tr["Z4"]]
    q = [zk[k][1] for k in ("qm", "ql", "qr", "qo", "qc")]
    s = [zk["sigma"][k][1] for k in range(3)]
    ls = [zk["lagrange"][j][1] for j in range(len(zk["lagrange"]))]
    apub = tr["A"][:zk["nPublic"]]
    got = rc.quotient(zk["power"], True, abcz, q, s, ls, apub, tr["beta"], tr["gamma"], tr["alpha"], zk["k1"],
                      zk["k2"], pts=pts)          # three = True: N itself, no division
    assert got == tr["T"]
