"""The checks tests/test_groth16.py runs on the host path (nzcb.GROTH16_HOST) and
tests/test_gpu_groth16.py on device 0: nzcb.groth16_setup, groth16_contribute, groth16_vk and
groth16_rows against the restatement of tests/groth16_cases.py. Prepared powers-of-tau files come
from the library's own new -> contribute -> prepare phase2 on the same device, cached."""
import functools
import os
import random

import pytest

import groth16_cases as gc
import nzcb
import ptau_ops_cases as pc
from oracle import bn254 as bn

A = pc.SECRETS_A
R = bn.R_MOD


@functools.lru_cache(maxsize=None)
def prepared(power: int, device: int, secrets=A) -> bytes:
    new = nzcb.ptau_new(power)
    if secrets is not None:
        new = nzcb.ptau_contribute(new, secrets=secrets, device=device)
    return nzcb.ptau_prepare_phase2(new, device=device)


@functools.lru_cache(maxsize=None)
def wide_edge_key() -> bytes:
    """The edge circuit widened to 300 constraints (cirPower 9): the restatement's bytes."""
    return gc.expected_zkey(gc.edge_circuit(300), 9, A)


def same_sections(got: bytes, want: bytes):
    gs, ws = gc.sections(got), gc.sections(want)
    assert list(gs) == list(ws)
    for sid in ws:
        assert gs[sid] == ws[sid], f"section {sid}"
    assert got == want


# ---------------------------------------------------------------- 1, 2, 5: whole keys
def check_random_circuit(device, seed, power):
    r1cs, _ = gc.random_circuit(seed)
    same_sections(nzcb.groth16_setup(r1cs, prepared(power, device), device=device), gc.expected_zkey(r1cs, power, A))


def check_edge_circuit(device):
    r1cs = gc.edge_circuit()
    got = nzcb.groth16_setup(r1cs, prepared(5, device), device=device)
    same_sections(got, gc.expected_zkey(r1cs, 5, A))
    b1, b2 = gc.points(got, 6), gc.points(got, 7)
    for wire in (4, 5, 7, 8, 9, 10, 11):  # in no B
        assert b1[wire] == bytes(64) and b2[wire] == bytes(128)
    assert gc.points(got, 5)[9] == bytes(64)  # in no constraint at all
    n_coefs = int.from_bytes(gc.sections(got)[4][:4], "little")
    assert n_coefs == sum(len(a) + len(b) for a, b, _ in gc.read_r1cs(r1cs)["constraints"]) + 4


def check_degenerate_file(device):
    """new -> prepare phase2 without a contribution: tau = alpha = beta = 1, so every level is the
    generator followed by points at infinity, L12, L14 and L15 are the same points (doublings
    and cancellations between the three parts of K) and public rows pick up nothing."""
    r1cs, _ = gc.random_circuit(21)
    got = nzcb.groth16_setup(r1cs, prepared(6, device, None), device=device)
    same_sections(got, gc.expected_zkey(r1cs, 6, pc.ONE))


# ---------------------------------------------------------------- 3: the schedule
def check_schedule(device, chunk, fan_in):
    prev = nzcb.groth16_schedule(chunk, fan_in)
    try:
        got = nzcb.groth16_setup(gc.edge_circuit(300), prepared(9, device), device=device)
        chunks = nzcb.groth16_timings()["chunks_g1"]
    finally:
        nzcb.groth16_schedule(*prev)
    assert nzcb.groth16_schedule(*prev) == prev
    same_sections(got, wide_edge_key())
    if chunk == 4:  # K of wire 0 has about 900 terms
        assert chunks > 1000


# ---------------------------------------------------------------- 4: the kernel entry alone
def _rows_case(g2: bool):
    rng = random.Random(4 + g2)
    gen = bn.G2_GEN if g2 else bn.G1_GEN
    mul = bn.g2_mul if g2 else bn.g1_mul
    add = bn.g2_add if g2 else bn.g1_add
    lem = bn.g2_to_lem if g2 else bn.g1_to_lem
    base = [mul(gen, rng.randrange(1, R)) for _ in range(7)] + [None]  # point 7: (0, 0)
    pts = b"".join(lem(p) for p in base)
    chunk = nzcb.groth16_schedule(0, 0)[0]
    nzcb.groth16_schedule(0, 0)
    k = rng.randrange(1, R)
    rows = [[(3, rng.randrange(R))]]                                     # one row of one term
    rows += [[(i % 7, (i * 0x9E3779B97F4A7C15 + 1) % R if i % 3 else 1)] for i in range(65)]  # one past a wave
    for ln in (chunk - 1, chunk, chunk + 1):                             # around a chunk's edge
        rows.append([(rng.randrange(7), rng.choice([1, 1, R - 1, 2, rng.randrange(R)])) for _ in range(ln)])
    rows.append([(2, k), (2, R - k)])                                    # infinity
    rows.append([(5, 1), (5, 1)])                                        # a doubling
    rows.append([(7, 5)])                                                # only (0, 0)
    rows.append([])                                                      # empty
    rows.append([(7, 1), (1, 0), (6, (R - 1) // 2), (6, (R + 1) // 2), (0, (1 << 253) + 1)])
    want = []
    for row in rows:
        acc = None
        for i, c in row:
            if base[i] is not None and c % R:
                acc = add(acc, mul(base[i], c))
        want.append(lem(acc))
    return pts, rows, want


def check_rows(device, g2):
    pts, rows, want = _rows_case(g2)
    row_off = [0]
    for row in rows:
        row_off.append(row_off[-1] + len(row))
    idx = [i for row in rows for i, _ in row]
    coefs = [c for row in rows for _, c in row]
    got = nzcb.groth16_rows(pts, row_off, idx, coefs, g2=g2, device=device)
    w = 128 if g2 else 64
    assert want[-5:-1] == [bytes(w), want[-4], bytes(w), bytes(w)] and want[-4] != bytes(w)
    for r, (g, x) in enumerate(zip(got, want)):
        assert g == x, f"row {r}"
    for bad in (dict(idx=[8] + idx[1:]), dict(coefs=[R] + coefs[1:]), dict(row_off=[0, 2, 1] + row_off[3:])):
        with pytest.raises(nzcb.NzcbError) as e:
            nzcb.groth16_rows(pts, bad.get("row_off", row_off), bad.get("idx", idx), bad.get("coefs", coefs), g2=g2,
                              device=device)
        assert e.value.name == "ARG"


# ---------------------------------------------------------------- 7: contribute
def check_contribute(device):
    r1cs, _ = gc.random_circuit(21)
    fresh = gc.expected_zkey(r1cs, 7, A)
    got = nzcb.groth16_contribute(fresh, secret=gc.D1, device=device)
    same_sections(got, gc.expected_zkey(r1cs, 7, A, gc.D1))
    gs, fs = gc.sections(got), gc.sections(fresh)
    for sid in (1, 3, 4, 5, 6, 7, 10):
        assert gs[sid] == fs[sid]
    assert gs[8] != fs[8] and gs[9] != fs[9]
    twice = nzcb.groth16_contribute(got, secret=gc.D2, device=device)
    assert twice == nzcb.groth16_contribute(fresh, secret=gc.D1 * gc.D2 % R, device=device)
    for secret in (0, R, (1 << 256) - 1):
        with pytest.raises(nzcb.NzcbError) as e:
            nzcb.groth16_contribute(fresh, secret=secret, device=device)
        assert e.value.name == "ARG"


def check_contribute_names_a_spoiled_point(device, kind):
    r1cs, _ = gc.random_circuit(21)
    fresh = gc.expected_zkey(r1cs, 7, A)
    n = gc.header(fresh)["n"]
    for sid, index, later in ((8, 3, (8, 9)), (9, n - 1, None)):
        bad = gc.spoiled(fresh, sid, index, kind)
        if later:  # a later defect does not take the name
            bad = gc.spoiled(gc.spoiled(bad, later[0], later[1], "curve"), 9, 0, "range")
        if kind == "zero":  # (0, 0) is the point at infinity in C and H
            assert len(nzcb.groth16_contribute(gc.spoiled(fresh, sid, index, kind), secret=gc.D1,
                                               device=device)) == len(fresh)
            continue
        with pytest.raises(nzcb.NzcbError) as e:
            nzcb.groth16_contribute(bad, secret=gc.D1, device=device)
        assert e.value.name == "FORMAT" and f"section {sid} point {index} " in str(e.value)
    for off in (gc.OFF_DELTA1, gc.OFF_DELTA2):
        (at, _), = gc.binfmt.read_binfile(fresh, b"zkey")[1][2]
        bad = fresh[:at + off] + bytes(64) + fresh[at + off + 64:]
        with pytest.raises(nzcb.NzcbError) as e:
            nzcb.groth16_contribute(bad, secret=gc.D1, device=device)
        assert e.value.name == "FORMAT" and "delta" in str(e.value)


# ---------------------------------------------------------------- 7, 8: a drawn secret, the pairing equation
def check_pairing_equation(device):
    r1cs, w = gc.random_circuit(21)
    fresh = nzcb.groth16_setup(r1cs, prepared(7, device), device=device)
    key = nzcb.groth16_contribute(fresh, entropy="some text", device=device)  # a drawn secret
    again = nzcb.groth16_contribute(fresh, device=device)
    assert len({key, again, fresh}) == 3 and len(key) == len(again) == len(fresh)
    vk = nzcb.groth16_vk(key)
    assert vk == gc.expected_vk(key) and list(vk) == list(gc.expected_vk(key))
    proof = gc.prove(key, r1cs, w)
    public = w[1:6]
    assert gc.verify(vk, public, proof)
    assert not gc.verify(vk, public[:2] + [public[2] + 1] + public[3:], proof)
    assert not gc.verify(dict(vk, vk_delta_2=nzcb.groth16_vk(fresh)["vk_delta_2"]), public, proof)


# ---------------------------------------------------------------- 9: errors
def check_errors(device, plonk_zkey):
    r1cs, _ = gc.random_circuit(21)
    good = prepared(7, device)
    key = gc.expected_zkey(r1cs, 7, A)

    def fails(name, text, fn, *args, **kw):
        with pytest.raises(nzcb.NzcbError) as e:
            fn(*args, **kw)
        assert e.value.name == name and text in str(e.value), str(e.value)

    unprepared = nzcb.ptau_contribute(nzcb.ptau_new(7), secrets=A, device=device)
    fails("FORMAT", "ptau: not prepared for phase 2 (section 12 is missing)", nzcb.groth16_setup, r1cs, unprepared,
          device=device)
    fails("FORMAT", "(section 14 is missing)", nzcb.groth16_setup, r1cs, pc.without_section(good, 14), device=device)
    fails("FORMAT", "section 13 is shorter", nzcb.groth16_setup, r1cs, pc.with_short_section(good, 13), device=device)
    fails("ARG", "circuit too big for this power of tau ceremony. 40*2 > 2**5", nzcb.groth16_setup, r1cs,
          prepared(5, device), device=device)
    other = r1cs.replace(bn.to_le(R), bn.to_le(bn.P_MOD), 1)
    fails("CURVE", "", nzcb.groth16_setup, other, good, device=device)
    fails("FORMAT", "zkey file is not groth16", nzcb.groth16_contribute, plonk_zkey, secret=gc.D1, device=device)
    fails("FORMAT", "zkey file is not groth16", nzcb.groth16_vk, plonk_zkey)
    fails("FORMAT", "", nzcb.groth16_vk, key[:700])
    fails("NOT_PLONK", "zkey file is not plonk", nzcb.vk_from_zkey, key)
    # cirPower 6 in a power-7 file: level 6 begins at point 63, T (level 7 of section 12) at 127
    for sid, index, kind in ((13, 63 + 17, "curve"), (12, 127 + 2 * 64 - 1, "range"), (12, 63, "curve"),
                             (15, 63 + 40, "range"), (4, 0, "zero"), (6, 0, "curve")):
        fails("FORMAT", f"ptau: section {sid} point {index} ", nzcb.groth16_setup, r1cs,
              pc.spoiled(good, sid, index, kind), device=device)
    # the lowest section and index win
    bad = pc.spoiled(pc.spoiled(pc.spoiled(good, 14, 70, "curve"), 13, 100, "range"), 13, 90, "curve")
    fails("FORMAT", "ptau: section 13 point 90 ", nzcb.groth16_setup, r1cs, bad, device=device)
    # levels and sections the setup does not read are not tested
    unread = good
    for sid, index in ((13, 127 + 5), (12, 10), (14, 62), (15, 127), (2, 3), (3, 1), (4, 1), (5, 127)):
        unread = pc.spoiled(unread, sid, index, "curve")
    assert nzcb.groth16_setup(r1cs, unread, device=device) == key


def check_file_forms(device, tmp_path):
    r1cs, _ = gc.random_circuit(21)
    rp, pp, z0, z1 = (str(tmp_path / n) for n in ("c.r1cs", "pot.ptau", "c_0000.zkey", "c_0001.zkey"))
    with open(rp, "wb") as f:
        f.write(r1cs)
    with open(pp, "wb") as f:
        f.write(prepared(7, device))
    assert nzcb.groth16_setup(rp, pp, z0, device=device) == z0
    assert nzcb.groth16_contribute(z0, z1, secret=gc.D1, device=device) == z1
    with open(z1, "rb") as f:
        assert f.read() == gc.expected_zkey(r1cs, 7, A, gc.D1)
    assert nzcb.groth16_vk(z1) == gc.expected_vk(gc.expected_zkey(r1cs, 7, A, gc.D1))
    assert nzcb.groth16_setup(rp, prepared(7, device), device=device) == gc.expected_zkey(r1cs, 7, A)
    for fn, args in ((nzcb.groth16_setup, (rp, pp, pp)), (nzcb.groth16_setup, (rp, pp, rp)),
                     (nzcb.groth16_contribute, (z0, z0))):
        with pytest.raises(nzcb.NzcbError) as e:
            fn(*args, device=device)
        assert e.value.name == "ARG"
    with open(pp, "rb") as f:
        assert f.read() == prepared(7, device)
    bad = str(tmp_path / "bad.zkey")
    with open(bad, "wb") as f:
        f.write(gc.spoiled(gc.expected_zkey(r1cs, 7, A), 9, 5, "curve"))
    with pytest.raises(nzcb.NzcbError):
        nzcb.groth16_contribute(bad, str(tmp_path / "never.zkey"), secret=gc.D1, device=device)
    assert not os.path.exists(tmp_path / "never.zkey")  # a failed operation leaves no partial file
