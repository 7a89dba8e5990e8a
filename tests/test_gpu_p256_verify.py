"""ECDSA P-256 verification on the GPU (csrc/p256_verify.hip): the cases of
tests/test_p256_verify.py on device 0, against the oracle of tests/p256_cases.py and byte for
byte against the host path; device buffers read in place, the records nzcb_nzcp_witness_dev wrote
for the example pass, and a batch verified while a prover context works on the same device."""
import ctypes
import hashlib
import os

import pytest

import nzcb
import p256_cases as C
from nzcb import nzcp

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
HOST = nzcb.P256_HOST


# ---------------------------------------------------------------- fields
@pytest.mark.parametrize("op", C.FIELD_OPS)
@pytest.mark.parametrize("field", ["p", "n"])
def test_field_matches_integers_and_host(field, op):
    got = C.check_field(0, field, op)
    a, b = C.field_pairs({"p": C.P, "n": C.N}[field])
    assert got == nzcb.p256_field(op, field, a, b, device=HOST)


# ---------------------------------------------------------------- u1 G + u2 Q
@pytest.mark.parametrize("window", [4, 8])
@pytest.mark.parametrize("name", [k[0] for k in C.mul2_keys()])
def test_mul2_matches_oracle(name, window):
    C.check_mul2(0, name, window)


# ---------------------------------------------------------------- known answer
def test_example_pass_is_valid():
    z, sig = C.example_hash_sig()
    key = C.example_key(0)
    assert key.verify([z], [sig]) == [C.OK]
    (res,) = key.verify_passes([nzcp.EXAMPLE_PASS_URI])
    assert res["valid"] and res["status"] == C.OK and res["kid"] == nzcp.EXAMPLE_KID and res["alg"] == -7
    tbs = nzcp.to_be_signed(nzcp.EXAMPLE_PASS_URI)
    assert key.verify([hashlib.sha256(C.example_tampered_tbs(tbs)).digest()], [sig]) == [C.INVALID]
    for bit in (0, 255, 256, 511):
        bad = bytearray(sig)
        bad[bit // 8] ^= 0x80 >> (bit % 8)
        assert key.verify([z], [bytes(bad)]) == [C.INVALID], bit
    key.close()


def test_records_of_the_witness_kernel_verify_in_place():
    """The example pass, the pass with one payload byte changed, and the pass again with one
    signature bit flipped: the witness kernel hashes each ToBeSigned into its record in HBM and
    verify_records reads the digests there."""
    _, _, sig = nzcp.decode_pass(nzcp.EXAMPLE_PASS_URI)
    tbs = nzcp.to_be_signed(nzcp.EXAMPLE_PASS_URI)
    flipped = bytes([sig[0] ^ 1]) + sig[1:]
    passes = [(tbs, sig, C.OK), (C.example_tampered_tbs(tbs), sig, C.INVALID), (tbs, flipped, C.INVALID)]
    inputs = b"".join(nzcp.input_signals(nzcp.circuit_input(t, bytes(range(1, 21)), nzcp.EXAMPLE_TOBESIGNED_MAX))
                      for t, _, _ in passes)
    rec_size = ctypes.sizeof(nzcb.NzcpRecord)
    d_in, d_rec, d_sig = nzcb.dev_alloc(len(inputs)), nzcb.dev_alloc(rec_size * 3), nzcb.dev_alloc(64 * 3)
    key = C.example_key(0)
    try:
        nzcb.h2d(d_in, inputs)
        nzcb.h2d(d_sig, b"".join(s for _, s, _ in passes))
        nzcb.nzcp_witness_dev(d_in, 3, nzcb.NZCP_EXAMPLE, dev_records=d_rec)   # asynchronous, default stream
        # the copy waits for the witness kernel; the verification runs on a stream of its own,
        # which does not, so it starts after the records are complete
        recs = nzcb.nzcp_records_from_bytes(nzcb.d2h(d_rec, rec_size * 3), 3)
        got = key.verify_records(d_rec, d_sig, 3)
        # the other way to order them: witness kernel and verification on one HIP stream
        # (created through the library's own HIP runtime), over records wiped in between
        nzcb.h2d(d_rec, bytes(rec_size * 3))
        hip = nzcb.load()
        stream = ctypes.c_void_p()
        assert hip.hipStreamCreate(ctypes.byref(stream)) == 0
        try:
            nzcb.nzcp_witness_dev(d_in, 3, nzcb.NZCP_EXAMPLE, dev_records=d_rec, stream=stream)
            same_stream = key.verify_records(d_rec, d_sig, 3, stream=stream)
        finally:
            assert hip.hipStreamDestroy(stream) == 0
    finally:
        key.close()
        for p in (d_in, d_rec, d_sig):
            nzcb.dev_free(p)
    assert [r["status"] for r in recs] == [0, 0, 0]
    assert [r["tbs_sha256"] for r in recs] == [hashlib.sha256(t).digest() for t, _, _ in passes]
    assert got == [w for *_, w in passes]
    assert same_stream == got


# ---------------------------------------------------------------- constructed signatures
@pytest.mark.parametrize("name", ["rx_ge_n", "rx_ge_n_unreduced_r", "doubling", "infinity"])
@pytest.mark.parametrize("window", [4, 8])
def test_constructed_signatures(name, window):
    q, z, sig, want = C.constructed()[name]
    assert C.statuses(0, q, [(z, sig)], window=window) == [want]


def test_range_and_extreme_hashes():
    q, items = C.pool()
    special = items[:18]
    assert C.statuses(0, q, special) == [w for *_, w in special]


@pytest.mark.parametrize("name", list(C.bad_keys()))
def test_bad_keys_raise(name):
    with pytest.raises(nzcb.NzcbError, match=C.BAD_KEY_TEXT):
        nzcb.P256Key(C.bad_keys()[name], device=0)


# ---------------------------------------------------------------- batches
@pytest.mark.parametrize("count", [0, 1, 63, 64, 65, 1000])
def test_batches_match_oracle_and_host(count):
    q, _ = C.pool()
    items = C.batch(count)
    want = [w for *_, w in items]
    got = C.statuses(0, q, items)
    assert got == want
    assert got == C.statuses(HOST, q, items)
    if count > 1:
        again = C.batch(count, seed=2)
        assert C.statuses(0, q, again) == [w for *_, w in again]
        assert C.statuses(0, q, items[:7]) == want[:7]


def test_windows_agree():
    q, items = C.pool()
    want = [w for *_, w in items]
    assert C.statuses(0, q, items, window=4) == want
    assert C.statuses(0, q, items, window=8) == want


def test_strides_and_device_buffers():
    """Tight strides, the record stride and a wide signature stride, from host buffers and from
    HBM in place."""
    q, _ = C.pool()
    items = C.batch(131)
    want = [w for *_, w in items]
    n = len(items)
    rec = ctypes.sizeof(nzcb.NzcpRecord)
    off = nzcb.NzcpRecord.tbs_sha256.offset
    assert off % 4 == 0 and rec % 4 == 0
    tight = b"".join(z for z, *_ in items)
    recs = b"".join(bytes([0xEE]) * off + z + bytes([0xEE]) * (rec - off - 32) for z, *_ in items)
    sigs = b"".join(s for _, s, _ in items)
    wide = b"".join(s + bytes([0xDD]) * 8 for _, s, _ in items)
    key = nzcb.P256Key(C.xy(q), device=0)
    bufs = [nzcb.dev_alloc(len(b)) for b in (tight, recs, sigs, wide)]
    try:
        assert key.verify(tight, sigs) == want
        assert key.verify(recs[off:], wide, hash_stride=rec, sig_stride=72) == want
        for p, b in zip(bufs, (tight, recs, sigs, wide)):
            nzcb.h2d(p, b)
        d_tight, d_recs, d_sigs, d_wide = bufs
        assert key.verify_dev(d_tight, 32, d_sigs, 64, n) == want
        assert key.verify_dev(d_recs + off, rec, d_sigs, 64, n) == want
        assert key.verify_records(d_recs, d_sigs, n) == want
        assert key.verify_dev(d_recs + off, rec, d_wide, 72, n) == want
        assert key.verify_dev(d_tight, 32, d_sigs, 64, 0) == []
        with pytest.raises(nzcb.NzcbError, match="multiples of 4"):
            key.verify_dev(d_tight + 1, 32, d_sigs, 64, 1)
        with pytest.raises(nzcb.NzcbError, match="multiples of 4"):
            key.verify_dev(d_tight, 34, d_sigs, 64, 1)
    finally:
        key.close()
        for p in bufs:
            nzcb.dev_free(p)


def test_wrong_lengths_raise():
    q, items = C.pool()
    z, sig, _ = items[20]
    key = nzcb.P256Key(C.xy(q), device=0)
    for hashes, sigs in (([z[:31]], [sig]), ([z], [sig[:63]]), ([z, z], [sig]), (z + b"\0", sig)):
        with pytest.raises(ValueError):
            key.verify(hashes, sigs)
    key.close()


def test_timings_report_the_kernels():
    q, _ = C.pool()
    key = nzcb.P256Key(C.xy(q), device=0)
    build_ms = nzcb.P256Key.timings()[0]
    items = C.batch(64)
    key.verify([z for z, *_ in items], [s for _, s, _ in items])
    t = nzcb.P256Key.timings()
    key.close()
    assert build_ms > 0 and len(t) == 3 and 0 < t[1] <= t[2]


# ---------------------------------------------------------------- next to a prover
def test_verify_while_a_context_proves():
    """A call has its own stream and buffers: the statuses are the same while a prover context
    works on the same device from another thread, and the proofs made meanwhile verify."""
    import threading
    q, _ = C.pool()
    items = C.batch(200)
    want = [w for *_, w in items]
    hashes, sigs = [z for z, *_ in items], [s for _, s, _ in items]
    zkey = open(os.path.join(GOLD, "p5.zkey"), "rb").read()
    wtns = open(os.path.join(GOLD, "p5.wtns"), "rb").read()
    ctx = nzcb.ProverContext(zkey, device=0)
    key = nzcb.P256Key(C.xy(q), device=0)
    made, errors = [], []

    def prove():
        try:
            for k in range(12):
                blinding = b"".join(hashlib.sha256(f"p256 meanwhile {k} {j}".encode()).digest()[:31] + b"\0"
                                    for j in range(11))
                made.append(ctx.prove_raw(wtns, blinding))
        except Exception as e:  # noqa: BLE001 (reported by the assertion below)
            errors.append(e)

    t = threading.Thread(target=prove)
    t.start()
    try:
        got = [key.verify(hashes, sigs) for _ in range(3)]
    finally:
        t.join()
        ctx.close()
        key.close()
    assert errors == [] and len(made) == 12
    assert got == [want] * 3
    vk = nzcb.vk_from_zkey(zkey)
    assert nzcb.verify_batch(vk, [p for p, _ in made], [u for _, u in made], device=0) == [True] * 12
