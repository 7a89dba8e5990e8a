"""Pass decode on the GPU (csrc/nzcp_decode.hip): the kernel's records, input blocks and ToBeSigned
bytes for case sets A, B and C (tests/nzcp_decode_cases.py) equal the host path's byte for byte
(which tests/test_nzcp_decode.py holds against the restatement), at batch sizes around the
workgroup width too; the pipeline URI bytes -> decode -> signature verdict in place -> witness on
one stream, with no digest or input built on the host; and verify_uris against verify_passes."""
import base64
import ctypes
import functools

import pytest

import nzcb
import nzcp_decode_cases as C
import p256_cases
from nzcb import nzcp
from test_node_p256 import _tamper

pytestmark = pytest.mark.gpu
TBS_STRIDE = 360


def both_paths(uris, params=nzcb.NZCP_LIVE):
    data = b"".join(C.data_for(i) for i in range(len(uris)))
    host = nzcb.nzcp_decode_raw(list(uris), params, data, nzcb.NZCP_HOST, TBS_STRIDE)
    dev = nzcb.nzcp_decode_raw(list(uris), params, data, 0, TBS_STRIDE)
    return host, dev


def assert_same(host, dev, count):
    for h, d, what in zip(host, dev, ("records", "inputs", "ToBeSigned")):
        if h != d:   # name the first pass that differs instead of printing megabytes
            size = len(h) // count
            bad = next(i for i in range(count) if h[i * size:(i + 1) * size] != d[i * size:(i + 1) * size])
            raise AssertionError(f"{what} of pass {bad} differ between the host and the device path")
        assert len(h) == len(d)


@pytest.mark.parametrize("which", ["A", "B", "C"])
def test_device_equals_host_path(which):
    uris = C.uris_of(which)
    host, dev = both_paths(uris)
    assert_same(host, dev, len(uris))
    want = [r["status"] for r, _ in C.expected(which)]
    assert [C.fields(r)["status"] for r in C.split(dev[0], len(uris))] == want


def test_device_equals_host_path_example_circuit_and_no_circuit():
    uris = C.uris_of("A")
    host, dev = both_paths(uris, nzcb.NZCP_EXAMPLE)
    assert_same(host, dev, len(uris))
    host, dev = both_paths(uris, None)
    assert dev[1] is None
    assert_same((host[0], host[2]), (dev[0], dev[2]), len(uris))
    fits = [C.fields(r)["fits"] for r in C.split(dev[0], len(uris))]
    assert fits == [0] * len(uris)


@functools.lru_cache(maxsize=None)
def mixed_pool():
    a, b, c = C.uris_of("A"), C.uris_of("B"), C.uris_of("C")
    return tuple(x for trio in zip(a * 9, b * 5, c) for x in trio)[:257]


@pytest.mark.parametrize("count", [0, 1, 63, 64, 65, 257])
def test_batch_counts(count):
    uris = mixed_pool()[:count]
    host, dev = both_paths(uris)
    assert len(dev[0]) == ctypes.sizeof(nzcb.NzcpPass) * count
    if count:
        assert_same(host, dev, count)
    if count > 1:    # the same passes in another order give the same records
        back = nzcb.nzcp_decode_raw(list(reversed(uris)), device=0)[0]
        plain = nzcb.nzcp_decode_raw(list(uris), device=0)[0]
        assert C.split(back, count) == list(reversed(C.split(plain, count)))


def test_bad_offsets_raise_on_the_device_path():
    blob = nzcp.EXAMPLE_PASS_URI.encode()
    for offsets in ([0, 700, 600], [0, 2 ** 31 + 1]):
        with pytest.raises(nzcb.NzcbError) as e:
            nzcb.nzcp_decode_raw(blob, device=0, offsets=offsets)
        assert e.value.name == "ARG"


def test_pipeline_without_a_host_digest():
    """URI bytes up; decode (live parameters, data 01..14), the signature verdicts read in place
    from the records, and the witness kernel on the decoder's input blocks, all on one stream."""
    live = next(u for n, u in C.set_a() if n == "live Jack").decode()
    uris = [nzcp.EXAMPLE_PASS_URI, _tamper(nzcp.EXAMPLE_PASS_URI), live]
    n = len(uris)
    blob, offs = nzcb.pack_uris(uris)
    data = bytes(range(1, 21)) * n
    size = ctypes.sizeof(nzcb.NzcpPass)
    wsize = ctypes.sizeof(nzcb.NzcpRecord)
    block = nzcb.nzcp_input_signals(nzcb.NZCP_LIVE) * 32
    sizes = (len(blob), 4 * (n + 1), len(data), size * n, block * n, wsize * n, block * n, wsize * n)
    bufs = [nzcb.dev_alloc(s) for s in sizes]
    d_uris, d_off, d_data, d_pass, d_inputs, d_wrec, d_host_inputs, d_host_wrec = bufs
    key = nzcb.P256Key(nzcp.EXAMPLE_PUBLIC_KEY, device=0)
    hip = nzcb.load()
    stream = ctypes.c_void_p()
    assert hip.hipStreamCreate(ctypes.byref(stream)) == 0
    try:
        nzcb.h2d(d_uris, blob)
        nzcb.h2d(d_off, bytes(offs))
        nzcb.h2d(d_data, data)
        nzcb.nzcp_decode_dev(d_uris, d_off, n, d_pass, nzcb.NZCP_LIVE, d_data, d_inputs, stream=stream)
        verdicts = key.verify_dev(d_pass + nzcb.NzcpPass.tbs_sha256.offset, size, d_pass + nzcb.NzcpPass.sig.offset,
                                  size, n, stream)
        nzcb.nzcp_witness_dev(d_inputs, n, nzcb.NZCP_LIVE, dev_records=d_wrec, stream=stream)
        assert hip.hipStreamSynchronize(stream) == 0
        passes = nzcb.nzcp_passes_from_bytes(nzcb.d2h(d_pass, size * n), n)
        wrecs = nzcb.nzcp_records_from_bytes(nzcb.d2h(d_wrec, wsize * n), n)
        # the same witness kernel over inputs built on the host
        tbs = [nzcp.to_be_signed(u) for u in uris]
        host_inputs = b"".join(nzcp.input_signals(nzcp.circuit_input(t, bytes(range(1, 21)), C.LIVE)) for t in tbs)
        assert nzcb.d2h(d_inputs, block * n) == host_inputs
        nzcb.h2d(d_host_inputs, host_inputs)
        nzcb.nzcp_witness_dev(d_host_inputs, n, nzcb.NZCP_LIVE, dev_records=d_host_wrec, stream=stream)
        assert hip.hipStreamSynchronize(stream) == 0
        want = nzcb.nzcp_records_from_bytes(nzcb.d2h(d_host_wrec, wsize * n), n)
    finally:
        assert hip.hipStreamDestroy(stream) == 0
        key.close()
        for p in bufs:
            nzcb.dev_free(p)
    assert [p["status"] for p in passes] == [0, 0, 0] and [p["fits"] for p in passes] == [1, 1, 1]
    assert verdicts == [nzcb.SIG_OK, nzcb.SIG_INVALID, nzcb.SIG_INVALID]
    assert wrecs == want
    assert wrecs[2]["status"] == 0 and any(wrecs[2]["out"])      # the live-shaped pass satisfies the live circuit
    assert wrecs[2]["tbs_sha256"] == passes[2]["tbs_sha256"]
    assert [w["out"] for w in wrecs] == [w["out"] for w in want]
    assert [w["tbs_sha256"] for w in wrecs] == [w["tbs_sha256"] for w in want]


def test_verify_uris_equals_verify_passes_on_a_mixed_batch():
    protected, payload, sig = nzcp.decode_pass(nzcp.EXAMPLE_PASS_URI)

    def uri(prot, sg):
        cose = nzcp.cbor_encode(nzcp.Tag(18, [prot, {}, payload, sg]))
        return "NZCP:/1/" + base64.b32encode(cose).decode().rstrip("=")

    es384 = nzcp.cbor_encode({4: nzcp.EXAMPLE_KID, 1: -35})
    uris = [uri(protected, sig), uri(es384, sig), uri(protected, sig[:63]), "NZCP:/1/AAAA", nzcp.EXAMPLE_PASS_URI,
            _tamper(nzcp.EXAMPLE_PASS_URI), uri(protected, bytes(64)), "not a pass"] * 9
    uris += [u.decode() for n, u in C.set_a() if n.startswith(("live", "tbs 3"))]   # MoH-shaped
    key = p256_cases.example_key(0)
    want, got = key.verify_passes(uris), key.verify_uris(uris)
    key.close()
    assert len(got) == len(uris) and sum(g["valid"] for g in got) == 18
    for w, g in zip(want, got):
        if w["reason"] and w["reason"].startswith("malformed pass"):
            assert g["reason"].startswith("malformed pass: ") and g["status"] is None and not g["valid"]
            g = dict(g, reason=w["reason"])
        assert g == w
    assert {g["status"] for g in got} == {None, nzcb.SIG_OK, nzcb.SIG_INVALID, nzcb.SIG_RANGE}
