"""ECDSA P-256 verification on the host path (nzcb.P256Key with device = P256_HOST, no GPU
needed): csrc/p256.h's two fields and the table scalar multiplication against exact integers, the
NZCP example pass under the specification's example key, constructed signatures (R.x >= n, a
final doubling, R at infinity), range and bad-key handling, and batches against the oracle of
tests/p256_cases.py. The same cases run on the device in tests/test_gpu_p256_verify.py."""
import base64
import ctypes
import hashlib

import pytest

import nzcb
import p256_cases as C
from nzcb import nzcp

HOST = nzcb.P256_HOST


# ---------------------------------------------------------------- fields
@pytest.mark.parametrize("op", C.FIELD_OPS)
@pytest.mark.parametrize("field", ["p", "n"])
def test_field_matches_integers(field, op):
    C.check_field(HOST, field, op)


def test_field_probe_rejects_unreduced_operands():
    with pytest.raises(nzcb.NzcbError, match="below the modulus"):
        nzcb.p256_field("add", "n", [C.N], [1], device=HOST)
    assert nzcb.p256_field("add", "p", [C.N], [1], device=HOST) == [C.N + 1]


# ---------------------------------------------------------------- u1 G + u2 Q
@pytest.mark.parametrize("window", [4, 8])
@pytest.mark.parametrize("name", [k[0] for k in C.mul2_keys()])
def test_mul2_matches_oracle(name, window):
    C.check_mul2(HOST, name, window)


# ---------------------------------------------------------------- known answer
def test_example_pass_is_valid():
    z, sig = C.example_hash_sig()
    key = C.example_key(HOST)
    assert key.verify([z], [sig]) == [C.OK]
    (res,) = key.verify_passes([nzcp.EXAMPLE_PASS_URI])
    assert res == {"valid": True, "status": C.OK, "reason": None, "alg": -7, "kid": nzcp.EXAMPLE_KID,
                   "iss": nzcp.EXAMPLE_ISS, "nbf": nzcp.EXAMPLE_NBF, "exp": nzcp.EXAMPLE_EXP}
    key.close()


def test_example_pass_tampered_is_invalid():
    z, sig = C.example_hash_sig()
    key = C.example_key(HOST)
    tbs = nzcp.to_be_signed(nzcp.EXAMPLE_PASS_URI)
    assert key.verify([hashlib.sha256(tbs).digest()], [sig]) == [C.OK]
    assert key.verify([hashlib.sha256(C.example_tampered_tbs(tbs)).digest()], [sig]) == [C.INVALID]
    for bit in (0, 255, 256, 511):
        bad = bytearray(sig)
        bad[bit // 8] ^= 0x80 >> (bit % 8)
        assert key.verify([z], [bytes(bad)]) == [C.INVALID], bit
    key.close()


def test_verify_passes_reports_what_it_does_not_verify():
    protected, payload, sig = nzcp.decode_pass(nzcp.EXAMPLE_PASS_URI)

    def uri(prot, sg):
        cose = nzcp.cbor_encode(nzcp.Tag(18, [prot, {}, payload, sg]))
        return "NZCP:/1/" + base64.b32encode(cose).decode().rstrip("=")

    key = C.example_key(HOST)
    es384 = nzcp.cbor_encode({4: nzcp.EXAMPLE_KID, 1: -35})
    got = key.verify_passes([uri(protected, sig), uri(es384, sig), uri(protected, sig[:63]), "NZCP:/1/AAAA",
                             nzcp.EXAMPLE_PASS_URI])
    key.close()
    assert [g["valid"] for g in got] == [True, False, False, False, True]
    assert got[1]["status"] is None and "alg" in got[1]["reason"] and got[1]["alg"] == -35
    assert got[2]["status"] is None and got[2]["reason"] == "signature is not 64 bytes"
    assert got[3]["status"] is None and got[3]["reason"].startswith("malformed pass")


# ---------------------------------------------------------------- constructed signatures
@pytest.mark.parametrize("name", ["rx_ge_n", "rx_ge_n_unreduced_r", "doubling", "infinity"])
@pytest.mark.parametrize("window", [4, 8])
def test_constructed_signatures(name, window):
    q, z, sig, want = C.constructed()[name]
    assert C.statuses(HOST, q, [(z, sig)], window=window) == [want]


def test_range_and_extreme_hashes():
    q, items = C.pool()
    special = items[:18]   # r, s out of range; z = 0, n, 2^256 - 1, n - 1, 1
    assert [w for *_, w in special[:8]] == [C.RANGE] * 8
    assert [w for *_, w in special[8::2]] == [C.OK] * 5
    assert C.statuses(HOST, q, special) == [w for *_, w in special]


def test_high_s_twin_stays_valid():
    q, items = C.pool()
    z, sig, want = next(it for it in items[18:] if it[2] == C.OK)
    twin = sig[:32] + C.be(C.N - int.from_bytes(sig[32:], "big"))
    assert C.verify(q, z, twin) == C.OK
    assert C.statuses(HOST, q, [(z, sig), (z, twin)]) == [C.OK, C.OK]


@pytest.mark.parametrize("name", list(C.bad_keys()))
def test_bad_keys_raise(name):
    with pytest.raises(nzcb.NzcbError, match=C.BAD_KEY_TEXT) as e:
        nzcb.P256Key(C.bad_keys()[name], device=HOST)
    assert e.value.name == "ARG"


# ---------------------------------------------------------------- batches
@pytest.mark.parametrize("count", [0, 1, 63, 64, 65, 1000])
def test_batches_match_oracle(count):
    q, _ = C.pool()
    items = C.batch(count)
    want = [w for *_, w in items]
    assert C.statuses(HOST, q, items) == want
    if count > 1:   # another order, and every item alone or in a smaller batch
        again = C.batch(count, seed=2)
        assert C.statuses(HOST, q, again) == [w for *_, w in again]
        assert C.statuses(HOST, q, items[:7]) == want[:7]


def test_pool_mixes_all_statuses_and_windows_agree():
    q, items = C.pool()
    want = [w for *_, w in items]
    assert {C.OK, C.INVALID, C.RANGE} == set(want)
    assert C.statuses(HOST, q, items, window=4) == want
    assert C.statuses(HOST, q, items, window=8) == want
    with pytest.raises(nzcb.NzcbError, match="window width"):
        nzcb.P256Key(C.xy(q), device=HOST, window=5)


def test_strides():
    q, _ = C.pool()
    items = C.batch(9)
    want = [w for *_, w in items]
    key = nzcb.P256Key(C.xy(q), device=HOST)
    rec = ctypes.sizeof(nzcb.NzcpRecord)
    off = nzcb.NzcpRecord.tbs_sha256.offset
    recs = b"".join(bytes([0xEE]) * off + z + bytes([0xEE]) * (rec - off - 32) for z, *_ in items)
    sigs = b"".join(s for _, s, _ in items)
    wide = b"".join(s + bytes(8) for _, s, _ in items)
    assert key.verify(b"".join(z for z, *_ in items), sigs) == want          # 32 and 64
    assert key.verify(recs[off:], sigs, hash_stride=rec) == want            # the record stride
    assert key.verify(recs[off:], wide, hash_stride=rec, sig_stride=72) == want
    key.close()


def test_wrong_lengths_raise():
    q, items = C.pool()
    z, sig, _ = items[20]
    key = nzcb.P256Key(C.xy(q), device=HOST)
    for hashes, sigs in (([z[:31]], [sig]), ([z], [sig[:63]]), ([z, z], [sig]), (z + b"\0", sig), (z, sig + b"\0"),
                         (b"", sig)):
        with pytest.raises(ValueError):
            key.verify(hashes, sigs)
    with pytest.raises(ValueError):
        nzcb.P256Key(bytes(63), device=HOST)
    with pytest.raises(nzcb.NzcbError, match="host key object"):
        key.verify_dev(4096, 32, 8192, 64, 1)
    key.close()
