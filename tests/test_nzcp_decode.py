"""Pass decode on the host path (nzcb.nzcp_decode with device = NZCP_HOST, no GPU needed): the
records and input blocks of case sets A, B and C (tests/nzcp_decode_cases.py) equal the pure-Python
restatement field for field; on A they also equal nzcb.nzcp's own decoders, hashlib and
nzcp.input_signals; set B's statuses are the ones written down with the cases. verify_uris on a
host key against verify_passes, batch independence, bad offsets and the record's layout. The same
cases run on the device in tests/test_gpu_nzcp_decode.py."""
import base64
import ctypes
import hashlib

import pytest

import nzcb
import nzcp_decode_cases as C
import p256_cases
from nzcb import nzcp

HOST = nzcb.NZCP_HOST
LIVE_PRM, EXAMPLE_PRM = nzcb.NZCP_LIVE, nzcb.NZCP_EXAMPLE


def decode(uris, params=LIVE_PRM, device=HOST, want_tbs=0):
    data = b"".join(C.data_for(i) for i in range(len(uris)))
    return nzcb.nzcp_decode_raw(list(uris), params, data, device, want_tbs)


def check_against_restatement(which, params=LIVE_PRM, device=HOST):
    uris = C.uris_of(which)
    want = C.expected(which, params["max_tbs_bytes"])
    recs, inputs, tbs = decode(uris, params, device, want_tbs=C.nzcp.LIVE_TOBESIGNED_MAX + 1)
    block = len(want[0][1])
    stride = C.nzcp.LIVE_TOBESIGNED_MAX + 1
    assert len(inputs) == block * len(uris)
    for i, (raw, (rec, blk)) in enumerate(zip(C.split(recs, len(uris)), want)):
        got = C.fields(raw)
        for k in got:
            assert got[k] == rec[k], (which, i, k, uris[i][:40])
        assert inputs[i * block:(i + 1) * block] == blk, (which, i)
        assert tbs[i * stride:(i + 1) * stride] == rec["tbs"][:stride].ljust(stride, b"\0"), (which, i)
    return recs, inputs


@pytest.mark.parametrize("which", ["A", "B", "C"])
def test_records_and_inputs_equal_the_restatement(which):
    check_against_restatement(which)


def test_set_a_against_the_example_circuit():
    check_against_restatement("A", EXAMPLE_PRM)
    fits = {n: r["fits"] for (n, _), (r, _) in zip(C.set_a(), C.expected("A", C.EXAMPLE))}
    assert (fits["tbs 314"], fits["tbs 315"], fits["example"]) == (1, 0, 1)
    fits = {n: r["fits"] for (n, _), (r, _) in zip(C.set_a(), C.expected("A", C.LIVE))}
    assert (fits["tbs 351"], fits["tbs 352"]) == (1, 0)


def test_set_a_is_well_formed_and_equals_the_host_decoders():
    """nzcp.decode_pass accepts every pass of A, and where the decoder took the pass (all but the
    2,049-byte URI) its record says what nzcp's decoders, hashlib and input_signals say."""
    names = [n for n, _ in C.set_a()]
    uris = C.uris_of("A")
    recs, inputs, _ = decode(uris)
    block = nzcb.nzcp_input_signals(LIVE_PRM) * 32
    for i, (name, uri, raw) in enumerate(zip(names, uris, C.split(recs, len(uris)))):
        protected, payload, sig = nzcp.decode_pass(uri.decode())      # raises if it does not accept
        hdr = nzcp.protected_header(uri.decode())
        claims, _ = nzcp.cbor_decode(payload)
        got = nzcb.nzcp_passes_from_bytes(raw, 1)[0]
        if name == "uri 2049":
            assert (got["status"], got["detail"]) == (C.LENGTH, 2049)
            continue
        assert got["status"] == 0, name
        tbs = nzcp.sig_structure(protected, payload)
        assert got["alg"] == hdr.get(1) and got["kid_len"] == len(hdr[4]) and got["kid"] == hdr[4][:32], name
        assert got["iss"] == claims[1][:64] and got["iss_len"] == len(claims[1].encode()), name
        assert (got["nbf"], got["exp"], got["cti"]) == (claims.get(5), claims.get(4), claims.get(7)), name
        assert got["sig"] == sig and got["sig_len"] == 64, name
        cose = C.cose_of(uri)
        assert cose[got["protected_off"]:][:got["protected_len"]] == protected, name
        assert cose[got["payload_off"]:][:got["payload_len"]] == payload, name
        assert nzcp.cbor_decode(cose)[1] == got["cose_len"], name
        assert got["tbs_len"] == len(tbs) and got["tbs_sha256"] == hashlib.sha256(tbs).digest(), name
        assert got["fits"] == (len(tbs) <= C.LIVE), name
        blk = inputs[i * block:(i + 1) * block]
        if got["fits"]:
            assert blk == nzcp.input_signals(nzcp.circuit_input(tbs, C.data_for(i), C.LIVE)), name
        else:
            assert blk == bytes(block), name
    assert sum(r["fits"] for r, _ in C.expected("A")) >= 20


def test_the_example_pass():
    (got,) = nzcb.nzcp_decode([nzcp.EXAMPLE_PASS_URI], device=HOST)
    assert len(nzcp.EXAMPLE_PASS_URI) == 600 and got["cose_len"] == 370 and got["tbs_len"] == 314
    assert got["tbs_sha256"].hex().startswith("271ce33d") and got["tbs_sha256"].hex().endswith("11f3ee")
    assert (got["status"], got["status_name"], got["version"], got["alg"]) == (0, "OK", 1, -7)
    assert (got["kid"], got["iss"], got["nbf"], got["exp"]) == (nzcp.EXAMPLE_KID, nzcp.EXAMPLE_ISS, nzcp.EXAMPLE_NBF,
                                                                nzcp.EXAMPLE_EXP)
    assert got["cti"] == nzcp.EXAMPLE_JTI and got["fits"] == 0
    recs, inputs = nzcb.nzcp_decode([nzcp.EXAMPLE_PASS_URI], EXAMPLE_PRM, [bytes(range(1, 21))], device=HOST)
    tbs = nzcp.to_be_signed(nzcp.EXAMPLE_PASS_URI)
    assert recs[0]["fits"] == 1
    assert inputs == nzcp.input_signals(nzcp.circuit_input(tbs, bytes(range(1, 21)), nzcp.EXAMPLE_TOBESIGNED_MAX))


def test_set_b_statuses_are_the_ones_written_down():
    for (name, uri, status, detail, present), (rec, _) in zip(C.set_b(), C.expected("B")):
        assert rec["status"] == status, name
        if detail is not None:
            assert rec["detail"] == detail, name
        if present is not None:
            assert rec["present"] == present, name
        if status:   # a failed pass keeps status, detail and version only
            assert all(not rec[k] for k in C.INT_FIELDS[3:]) and not any(rec["tbs_sha256"]), name
    assert {s for _, _, s, *_ in C.set_b()} == set(range(9))
    by_name = {n: r for (n, *_), (r, _) in zip(C.set_b(), C.expected("B"))}
    assert by_name["alg 2^40"]["alg"] == 2 ** 31 - 1 and by_name["alg -2^40"]["alg"] == -2 ** 31
    assert by_name["alg -2^31"]["alg"] == -2 ** 31
    assert by_name["sig 63"]["sig_len"] == 63 and by_name["sig 65"]["sig_len"] == 65
    assert not any(by_name["sig 63"]["sig"]) and not any(by_name["sig 65"]["sig"])
    long = by_name["exp 2^64-1, long iss and cti"]
    assert (long["exp"], long["iss_len"], long["cti_len"], long["nbf"]) == (2 ** 64 - 1, 65, 40, 0)
    assert long["iss"] == b"i" * 64 and long["cti"] == bytes(range(32))


def test_set_c_reaches_every_parser_status():
    statuses = [r["status"] for r, _ in C.expected("C")]
    assert len(statuses) == 2000
    assert set(statuses) >= {C.OK, C.TRUNCATED, C.CBOR, C.NOT_COSE, C.HEADER, C.CLAIMS}


def test_results_do_not_depend_on_the_batch():
    uris = (C.uris_of("A") + C.uris_of("B"))
    whole, _, _ = decode(uris, None)
    size = ctypes.sizeof(nzcb.NzcpPass)
    back, _, _ = nzcb.nzcp_decode_raw(list(reversed(uris)), device=HOST)
    assert C.split(back, len(uris)) == list(reversed(C.split(whole, len(uris))))
    for i in (0, 5, len(uris) - 1):
        alone, _, _ = nzcb.nzcp_decode_raw([uris[i]], device=HOST)
        assert alone == whole[i * size:(i + 1) * size]
    assert nzcb.nzcp_decode([], device=HOST) == []
    assert nzcb.nzcp_decode([], LIVE_PRM, device=HOST) == ([], b"")


def test_bad_arguments_raise():
    blob = nzcp.EXAMPLE_PASS_URI.encode()
    for offsets in ([0, 700, 600], [10, 0], [0, 2 ** 31 + 1]):
        with pytest.raises(nzcb.NzcbError) as e:
            nzcb.nzcp_decode_raw(blob, device=HOST, offsets=offsets)
        assert e.value.name == "ARG"
    recs, _, _ = nzcb.nzcp_decode_raw(blob, device=HOST, offsets=[0, 600, 600, 600])
    assert [C.fields(r)["status"] for r in C.split(recs, 3)] == [C.OK, C.PREFIX, C.PREFIX]
    with pytest.raises(nzcb.NzcbError, match="MaxToBeSignedBytes"):
        nzcb.nzcp_decode([blob], dict(LIVE_PRM, max_tbs_bytes=513), device=HOST)
    with pytest.raises(ValueError):
        nzcb.nzcp_decode([blob], LIVE_PRM, [bytes(19)], device=HOST)


def test_layout():
    lay = (ctypes.c_uint32 * 3)()
    nzcb.load().nzcb_nzcp_pass_layout(lay)
    assert list(lay) == [ctypes.sizeof(nzcb.NzcpPass), nzcb.NzcpPass.sig.offset, nzcb.NzcpPass.tbs_sha256.offset]
    assert lay[0] % 8 == 0 and lay[1] % 4 == 0 and lay[2] % 4 == 0
    assert nzcb.PASS_MAX_URI == C.MAX_URI and len(nzcb.PASS_STATUS_NAMES) == 9


def test_verify_uris_on_a_host_key_equals_verify_passes():
    """The five passes of test_verify_passes_reports_what_it_does_not_verify."""
    protected, payload, sig = nzcp.decode_pass(nzcp.EXAMPLE_PASS_URI)

    def uri(prot, sg):
        cose = nzcp.cbor_encode(nzcp.Tag(18, [prot, {}, payload, sg]))
        return "NZCP:/1/" + base64.b32encode(cose).decode().rstrip("=")

    es384 = nzcp.cbor_encode({4: nzcp.EXAMPLE_KID, 1: -35})
    uris = [uri(protected, sig), uri(es384, sig), uri(protected, sig[:63]), "NZCP:/1/AAAA", nzcp.EXAMPLE_PASS_URI]
    key = p256_cases.example_key(nzcb.P256_HOST)
    want, got = key.verify_passes(uris), key.verify_uris(uris)
    assert key.verify_uris([]) == []
    key.close()
    assert [g["valid"] for g in got] == [True, False, False, False, True]
    assert got[3]["reason"] == "malformed pass: NOT_COSE at 0" and want[3]["reason"].startswith("malformed pass")
    want[3]["reason"] = got[3]["reason"]
    assert got == want
