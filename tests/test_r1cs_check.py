"""The witness check on the host path (nzcb.R1cs with device = R1CS_HOST, no GPU needed):
n_bad, first_bad and the list of every case against the exact-integer reference
(r1cs_check_cases.expected), the sizes and batch forms, the long-row split, the errors with
their texts, .wtns input and a wrapper circuit of the nzcp gadgets. The same cases run on the
device in tests/test_gpu_r1cs_check.py."""
import struct

import pytest

import nzcb
import r1cs_check_cases as C
from oracle import r1cs as orc
from oracle.binfmt import write_binfile
from oracle.bn254 import P_MOD, R_MOD as R, to_le

HOST = nzcb.R1CS_HOST


def _obj(data, **kw):
    return nzcb.R1cs(data, device=HOST, **kw)


def _assert_case(case, cap=8, **kw):
    name, data, wits = case
    r = _obj(data, **kw)
    try:
        got = C.check_all(r, case, cap)
        single = C.check_all(r, case, cap, batch=False)
    finally:
        r.close()
    want = [C.expected(data, w, cap) for w in wits]
    assert got == want, name
    assert single == want, name
    return want


# ---------------------------------------------------------------- random r1cs
@pytest.mark.parametrize("case", C.random_cases(), ids=lambda c: c[0])
def test_random_r1cs_matches_reference(case):
    want = _assert_case(case)
    assert want[0]["n_bad"] == 0 and want[0]["first_bad"] is None and want[0]["bad"] == []
    assert any(w["n_bad"] for w in want[1:])


def test_threshold_and_tile_do_not_change_results():
    case = C.random_cases()[2]
    want = _assert_case(case)
    for kw in (dict(long_row_threshold=1), dict(long_row_threshold=3, witness_tile=1), dict(witness_tile=2)):
        assert _assert_case(case, **kw) == want


# ---------------------------------------------------------------- edge r1cs
def test_edge_r1cs():
    case, uses_one = C.edge_case()
    want = _assert_case(case, cap=64)
    assert want[0]["n_bad"] == 0                                  # satisfied, values >= r included
    assert set(want[1]["bad"]) == uses_one and want[1]["n_bad"] == len(uses_one)   # wire 0 = 2
    assert all(w["n_bad"] for w in want[2:])


# ---------------------------------------------------------------- sizes
@pytest.mark.parametrize("n", C.SIZES)
def test_sizes(n):
    case = C.size_case(n)
    want = _assert_case(case, cap=200)
    r = _obj(case[1])
    assert r.info["n_constraints"] == n and r.info["n_terms"] == 3 * n and r.info["n_wires"] == 2 * n + 1
    r.close()
    if n:
        assert [w["bad"] for w in want] == [[], [0], [n - 1], list(range(n))]
        assert [w["first_bad"] for w in want] == [None, 0, n - 1, 0]


def test_count_zero_and_batch_with_stride_and_caps():
    name, data, wits = C.size_case(65)
    two = C.bump(C.bump(wits[0], 66 + 7), 66 + 40)
    batch = [wits[3], wits[0], two, wits[2], wits[1]]
    r = _obj(data)
    try:
        assert r.check(b"", count=0) == []
        stride = 32 * len(wits[0]) + 48
        for cap in (0, 1, 8, 64, 65, 100):
            got = r.check(C.pack(batch, stride), count=5, bad_cap=cap, stride=stride)
            assert got == [C.expected(data, w, cap) for w in batch], cap
        assert [g["n_bad"] for g in got] == [65, 0, 2, 1, 1]
        # the verdicts do not depend on the order or the size of the batch
        rev = r.check(C.pack(batch[::-1], stride), count=5, bad_cap=8, stride=stride)
        assert rev[::-1] == r.check(C.pack(batch), bad_cap=8)
    finally:
        r.close()


# ---------------------------------------------------------------- long rows
def test_long_rows():
    r = _obj(C.size_case(1)[1])
    T = r.info["long_row_threshold"]
    r.close()
    assert 4 <= T <= 836
    case, lengths = C.long_rows_case(T)
    want = _assert_case(case)
    assert want[0]["n_bad"] == 0
    assert [w["bad"] for w in want[1:]] == [[k] for k in range(len(lengths))]   # each through its last term only
    r = _obj(case[1])
    assert r.info["n_long_rows"] == sum(n >= T for n in lengths)
    assert r.info["n_terms"] == sum(lengths)
    r.close()
    r = _obj(case[1], long_row_threshold=322)
    assert r.info["long_row_threshold"] == 322 and r.info["n_long_rows"] == sum(n >= 322 for n in lengths)
    r.close()


# ---------------------------------------------------------------- errors
def _err(fn, code, text):
    with pytest.raises(nzcb.NzcbError) as e:
        fn()
    assert e.value.name == code and str(e.value) == text, (e.value.name, str(e.value))
    return str(e.value)


def test_errors():
    name, data, wits = C.size_case(3)
    r = _obj(data)
    try:
        _err(lambda: r.check(C.pack([wits[0] + [5]]), count=1), "WITNESS_LEN",
             "Invalid witness length. Circuit: 7, witness: 8")
        _err(lambda: r.check(C.pack([wits[0][:-1]]), count=1), "WITNESS_LEN",
             "Invalid witness length. Circuit: 7, witness: 6")
        _err(lambda: r.check(C.wtns_file(wits[0] + [5])), "WITNESS_LEN",
             "Invalid witness length. Circuit: 7, witness: 8")
    finally:
        r.close()
    # a prime that is not BN254's r (BN254's base field prime)
    other = data.replace(to_le(R), to_le(P_MOD), 1)
    assert other != data
    _err(lambda: _obj(other), "CURVE", "r1cs: curve not supported (the prime is not BN254's r)")
    # malformed files, in the setup reader's words (tests/test_gpu_r1cs_check.py compares the two)
    good, hdr, body, malformed = C.malformed_files()
    _obj(good).close()
    for bad, text in malformed:
        _err(lambda: _obj(bad), "FORMAT", text)
    _err(lambda: _obj(b"nope" + good[4:]), "FORMAT", "r1cs: invalid file format")
    # a header that promises more constraints than the section holds
    lying = write_binfile(b"r1cs", 1, [(1, hdr[:-4] + struct.pack("<I", 1 << 30)), (2, body)])
    _err(lambda: _obj(lying), "FORMAT", "r1cs: truncated")


def test_unknown_sections_are_ignored_and_file_input(tmp_path):
    name, data, wits = C.size_case(3)
    parsed = orc.read_r1cs(data)
    hdr = struct.pack("<I", 32) + to_le(R) + struct.pack("<IIIIQI", 7, 0, 0, 3, 7, 3)
    body = b"".join(struct.pack("<I", len(lc)) + b"".join(struct.pack("<I", s) + to_le(c) for s, c in lc)
                    for cons in parsed["constraints"] for lc in cons)
    extra = write_binfile(b"r1cs", 1, [(9, b"custom gates"), (1, hdr), (77, b"x" * 40), (2, body)])
    path = tmp_path / "c.r1cs"
    path.write_bytes(extra)
    for src in (extra, str(path)):
        r = _obj(src)
        try:
            assert r.check(C.pack(wits)) == [C.expected(data, w) for w in wits]
        finally:
            r.close()
    _err(lambda: _obj(str(tmp_path / "missing.r1cs")), "ARG", f"cannot open {tmp_path / 'missing.r1cs'}")


# ---------------------------------------------------------------- .wtns input
def test_wtns_input_equals_raw_values():
    name, data, wits = C.random_cases()[0]
    r = _obj(data)
    try:
        for w in wits[:4]:
            assert r.check(C.wtns_file(w)) == r.check(C.pack([w])) == [C.expected(data, w)]
    finally:
        r.close()


# ---------------------------------------------------------------- wrapper circuit
def test_wrapper_circuit_and_negative_kat():
    c, data, good, carried = C.wrapper_case(3)
    ks = range(len(c.constraints))
    want_bad = C.violated(c, carried, ks)
    assert C.violated(c, good, ks) == [] and want_bad
    r = _obj(data)
    try:
        assert r.info["n_constraints"] == len(c.constraints) and r.info["n_wires"] == c.n_wires
        got = r.check(C.pack([good, carried]), bad_cap=len(c.constraints))
    finally:
        r.close()
    assert got[0] == {"n_bad": 0, "first_bad": None, "bad": []}
    assert got[1] == {"n_bad": len(want_bad), "first_bad": want_bad[0], "bad": want_bad}
