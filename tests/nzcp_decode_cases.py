"""Shared by the pass-decode tests (tests/test_nzcp_decode.py on the host path, test_gpu_nzcp_decode.py
on the device, test_nzcp_decode_native.py under sanitizers, test_node_nzcp_decode.py through Node):

* ``restate``: a strict pure-Python restatement of the decode rules of include/nzcb.h
  (nzcb_nzcp_decode), returning the record as a dict of the struct's fields and the pass's block of
  input signals;
* case set A, well-formed passes built with nzcb.nzcp's encoders, every one accepted by
  nzcp.decode_pass; set B, one case per status and boundary, each with the status (and detail)
  written down by hand; set C, 2,000 seeded mutations of A's COSE bytes.

Everything is computed once per process and never modified."""
import base64
import ctypes
import functools
import hashlib
import random

import nzcb
from nzcb import nzcp
from nzcb.nzcp import Raw, Tag, cbor_encode, cbor_head

OK, LENGTH, PREFIX, BASE32, TRUNCATED, CBOR, NOT_COSE, HEADER, CLAIMS = range(9)
HAS_ALG, HAS_KID, HAS_ISS, HAS_NBF, HAS_EXP, HAS_CTI, HAS_SIG = 1, 2, 4, 8, 16, 32, 64
MAX_URI = 2048
DATA = bytes(range(1, 21))
LIVE, EXAMPLE = nzcp.LIVE_TOBESIGNED_MAX, nzcp.EXAMPLE_TOBESIGNED_MAX
_B32 = "ABCDEFGHIJKLMNOPQRSTUVWXYZ234567"
_ONE, _ZERO = (1).to_bytes(32, "little"), bytes(32)
INT_FIELDS = ("status", "detail", "version", "present", "alg", "kid_len", "iss_len", "cti_len", "sig_len",
              "cose_len", "protected_off", "protected_len", "payload_off", "payload_len", "tbs_len", "fits", "nbf",
              "exp")
BYTE_FIELDS = (("kid", 32), ("cti", 32), ("iss", 64), ("sig", 64), ("tbs_sha256", 32))


# ------------------------------------------------------------------ the restatement
class Fail(Exception):
    def __init__(self, status, detail=0):
        super().__init__(status, detail)
        self.status, self.detail = status, detail


def _head(buf, off, end):
    """(major, arg, offset after the head) of the head at `off` of the region ending at `end`."""
    if off >= end:
        raise Fail(TRUNCATED, off)
    major, info = buf[off] >> 5, buf[off] & 31
    nxt = off + 1
    if info >= 28:
        raise Fail(CBOR, off)
    arg = info
    if info >= 24:
        nb = 1 << (info - 24)
        if nb > end - nxt:
            raise Fail(TRUNCATED, off)
        arg = int.from_bytes(buf[nxt:nxt + nb], "big")
        nxt += nb
    if major in (2, 3, 4, 5) and arg > end - nxt:
        raise Fail(TRUNCATED, off)
    return major, arg, nxt


def _skip(buf, off, end):
    todo = 1
    while todo:
        major, arg, off = _head(buf, off, end)
        todo -= 1
        if major in (2, 3):
            off += arg
        elif major == 4:
            todo += arg
        elif major == 5:
            todo += 2 * arg
        elif major == 6:
            todo += 1
    return off


def _sat(major, arg):
    v = arg if major == 0 else -1 - arg
    return max(-(1 << 31), min((1 << 31) - 1, v))


def _map(buf, off, end, claims, not_map, rec):
    major, count, at = _head(buf, off, end)
    if major != 5:
        raise Fail(not_map, off)
    for _ in range(count):
        kmajor, key, after_key = _head(buf, at, end)
        if kmajor == 0:
            at = after_key
        else:
            key = None
            at = _skip(buf, at, end)
        vmajor, varg, body = _head(buf, at, end)
        known = {(False, 1): ("alg", HAS_ALG), (False, 4): ("kid", HAS_KID), (True, 1): ("iss", HAS_ISS),
                 (True, 4): ("exp", HAS_EXP), (True, 5): ("nbf", HAS_NBF), (True, 7): ("cti", HAS_CTI)}
        if (claims, key) in known:
            name, bit = known[(claims, key)]
            rec["present"] &= ~bit          # the last occurrence counts, whatever came before
            rec[name] = 0 if name in ("alg", "exp", "nbf") else b""
            if name != "alg" and name + "_len" in rec:
                rec[name + "_len"] = 0
            if name == "alg" and vmajor in (0, 1):
                rec["alg"], rec["present"] = _sat(vmajor, varg), rec["present"] | bit
            elif name in ("exp", "nbf") and vmajor == 0:
                rec[name], rec["present"] = varg, rec["present"] | bit
            elif name in ("kid", "cti") and vmajor == 2 or name == "iss" and vmajor == 3:
                rec[name], rec[name + "_len"] = bytes(buf[body:body + varg]), varg
                rec["present"] |= bit
        at = _skip(buf, at, end)


def _parse(cose, rec):
    n = len(cose)
    major, arg, at = _head(cose, 0, n)
    if major != 6 or arg != 18:
        raise Fail(NOT_COSE, 0)
    off = at
    major, arg, at = _head(cose, off, n)
    if major != 4 or arg != 4:
        raise Fail(NOT_COSE, off)
    off = at
    major, arg, at = _head(cose, off, n)
    if major != 2:
        raise Fail(NOT_COSE, off)
    rec["protected_off"], rec["protected_len"] = at, arg
    off = _skip(cose, at + arg, n)
    major, arg, at = _head(cose, off, n)
    if major != 2:
        raise Fail(NOT_COSE, off)
    rec["payload_off"], rec["payload_len"] = at, arg
    off = at + arg
    major, arg, at = _head(cose, off, n)
    if major == 2:
        rec["present"] |= HAS_SIG
        rec["sig_len"] = arg
        rec["sig"] = bytes(cose[at:at + 64]) if arg == 64 else b""
        off = at + arg
    else:
        off = _skip(cose, off, n)
    rec["cose_len"] = off
    _map(cose, rec["protected_off"], rec["protected_off"] + rec["protected_len"], False, HEADER, rec)
    _map(cose, rec["payload_off"], rec["payload_off"] + rec["payload_len"], True, CLAIMS, rec)


def _blank():
    rec = {k: 0 for k in INT_FIELDS}
    rec.update({k: b"" for k, _ in BYTE_FIELDS})
    return rec


def input_block(tbs: bytes, max_tbs: int, data20: bytes) -> bytes:
    """nzcp.input_signals(nzcp.circuit_input(tbs, data20, max_tbs)) without the big integers."""
    fitted = tbs + bytes(max_tbs - len(tbs))
    bits = [_ONE if (b >> (7 - j)) & 1 else _ZERO for b in fitted for j in range(8)]
    data = [_ONE if (data20[19 - j // 8] >> (j % 8)) & 1 else _ZERO for j in range(160)]
    return b"".join(bits) + len(tbs).to_bytes(32, "little") + b"".join(data)


def restate(uri: bytes, max_tbs: int = 0, data20: bytes = bytes(20)):
    """-> (record dict: INT_FIELDS as ints, BYTE_FIELDS zero-padded to their sizes, plus "tbs", the
    ToBeSigned bytes or b""; the input block, (8 max_tbs + 161) x 32 bytes, or b"" without max_tbs)."""
    rec = _blank()
    tbs = b""
    try:
        if len(uri) > MAX_URI:
            raise Fail(LENGTH, len(uri))
        digits = 0
        while uri[6 + digits:7 + digits].isdigit() and uri[6 + digits:7 + digits].isascii():
            digits += 1
        start = 7 + digits
        if uri[:6] != b"NZCP:/" or not 1 <= digits <= 9 or uri[start - 1:start] != b"/" or len(uri) <= start:
            raise Fail(PREFIX, 0)
        rec["version"] = int(uri[6:6 + digits])
        for i in range(start, len(uri)):
            if chr(uri[i]) not in _B32:
                raise Fail(BASE32, i)
        value = 0
        for c in uri[start:]:
            value = value << 5 | _B32.index(chr(c))
        nchars = len(uri) - start
        nbytes = 5 * nchars // 8
        cose = (value >> (5 * nchars - 8 * nbytes)).to_bytes(nbytes, "big")
        _parse(cose, rec)
        prot = cose[rec["protected_off"]:rec["protected_off"] + rec["protected_len"]]
        payload = cose[rec["payload_off"]:rec["payload_off"] + rec["payload_len"]]
        tbs = b"\x84\x6aSignature1" + cbor_head(2, len(prot)) + prot + b"\x40" + cbor_head(2, len(payload)) + payload
        rec["tbs_len"] = len(tbs)
        rec["tbs_sha256"] = hashlib.sha256(tbs).digest()
        rec["fits"] = int(bool(max_tbs) and len(tbs) <= max_tbs)
    except Fail as f:
        version = rec["version"]
        rec = _blank()
        rec.update(status=f.status, detail=f.detail, version=version)
        tbs = b""
    for name, size in BYTE_FIELDS:
        rec[name] = rec[name][:size].ljust(size, b"\0")
    rec["tbs"] = tbs
    block = b""
    if max_tbs:
        block = input_block(tbs, max_tbs, data20) if rec["fits"] else bytes((8 * max_tbs + 161) * 32)
    return rec, block


def fields(raw: bytes) -> dict:
    """One nzcb_nzcp_pass (its bytes) as the restatement's dict, without "tbs"."""
    r = nzcb.NzcpPass.from_buffer_copy(raw)
    d = {k: getattr(r, k) for k in INT_FIELDS}
    d.update({k: bytes(getattr(r, k)) for k, _ in BYTE_FIELDS})
    return d


def split(raw: bytes, count: int) -> list:
    size = ctypes.sizeof(nzcb.NzcpPass)
    assert len(raw) == size * count
    return [raw[i * size:(i + 1) * size] for i in range(count)]


def data_for(i: int) -> bytes:
    """The 20 pass-through bytes the tests give pass i of a batch."""
    return bytes((17 * i + 3 * j + 1) & 0xFF for j in range(20))


# ------------------------------------------------------------------ builders
def b32(cose: bytes) -> str:
    return base64.b32encode(cose).decode().rstrip("=")


def uri_of(cose: bytes, version: str = "1") -> bytes:
    return f"NZCP:/{version}/{b32(cose)}".encode()


def cose_of(uri: bytes) -> bytes:
    return nzcp.base32_decode(uri.decode().split("/", 2)[2])


def sig_for(seed) -> bytes:
    return random.Random(f"sig {seed}").randbytes(64)


def sign1(protected, payload, sig, unprotected=None, tag=b"\xd2", array=b"\x84") -> bytes:
    """tag(18) [protected, unprotected, payload, sig] with the given heads; items that are bytes are
    encoded as byte strings, Raw items are taken as they are."""
    items = [protected, {} if unprotected is None else unprotected, payload, sig]
    return tag + array + b"".join(cbor_encode(x) for x in items)


LIVE_PROTECTED = cbor_encode({4: nzcp.LIVE_KID, 1: -7})
EXAMPLE_COSE = cose_of(nzcp.EXAMPLE_PASS_URI.encode())


def sized_header(length: int) -> bytes:
    """{4: kid, 1: -7} of exactly `length` bytes (length >= 6, not 29 or 30)."""
    for kid_len in range(length):
        enc = cbor_encode({4: bytes((65 + i % 26) for i in range(kid_len)), 1: -7})
        if len(enc) == length:
            return enc
    raise ValueError(length)


def sized_claims(length: int) -> bytes:
    """{1: iss} of exactly `length` bytes."""
    for iss_len in range(length):
        enc = cbor_encode({1: "did:web:" + "x" * iss_len})
        if len(enc) == length:
            return enc
    raise ValueError(length)


def pass_with_tbs_len(target: int) -> bytes:
    """A COSE_Sign1 with the live header whose Sig_structure is `target` bytes long."""
    if target < 300:      # shorter than any MoH-shaped pass: claims of an issuer alone
        candidates = (sized_claims(n) for n in range(target - 40, target - 20))
    else:
        candidates = (cbor_encode(nzcp.claims(iss=nzcp.LIVE_ISS, subject=nzcp.credential_subject("G" * g, "S" * f)))
                      for g in (1, 2) for f in range(1, 80))
    for payload in candidates:
        if len(nzcp.sig_structure(LIVE_PROTECTED, payload)) == target:
            return sign1(LIVE_PROTECTED, payload, sig_for(target))
    raise ValueError(target)


@functools.lru_cache(maxsize=None)
def set_a() -> tuple:
    """(name, URI bytes): nzcp.decode_pass accepts every one. Only "uri 2049" is not decoded
    (LENGTH): the cap is this interface's, not the format's."""
    out = [("example", nzcp.EXAMPLE_PASS_URI.encode()),
           ("version 123456789", b"NZCP:/123456789/" + nzcp.EXAMPLE_PASS_URI.encode()[8:])]
    for given, family in (("A", "B"), ("Jack", "Sparrow"), ("Wilhelmina-Alexandra", "Featherstonehaugh-Cholmondeley"),
                          ("Māui", "Tūhoe")):
        payload = cbor_encode(nzcp.claims(iss=nzcp.LIVE_ISS, subject=nzcp.credential_subject(given, family)))
        out.append((f"live {given}", uri_of(sign1(LIVE_PROTECTED, payload, sig_for(given)))))
    for n in (23, 24, 255, 256):
        out.append((f"lengths {n}", uri_of(sign1(sized_header(n), sized_claims(n), sig_for(n)))))
    payload = cbor_encode(nzcp.claims())
    for name, tag, array in (("heads 1 byte", b"\xd8\x12", b"\x98\x04"), ("heads 2 bytes", b"\xd9\x00\x12", b"\x99\x00\x04"),
                             ("heads 4 and 8 bytes", b"\xda\x00\x00\x00\x12", b"\x9b" + (4).to_bytes(8, "big"))):
        out.append((name, uri_of(sign1(LIVE_PROTECTED, payload, sig_for(name), tag=tag, array=array))))
    nested = {1: [[1, [2, [3, []]]], "x"], "k": {5: [b"ab", [], {}]}, -3: Tag(7, [True, Raw(b"\xf6")])}
    out.append(("unprotected nested", uri_of(sign1(LIVE_PROTECTED, payload, sig_for("n"), unprotected=nested))))
    for t in (119, 120, 127, 128, 183, 184, 191, 192, 314, 315, 351, 352):   # 55, 56, 63, 0 mod 64; the two maxima
        out.append((f"tbs {t}", uri_of(pass_with_tbs_len(t))))
    for extra in range(1, 8):     # the example pass has 592 digits; unpadded base32 alone gives 0, 2, 4, 5, 7 mod 8
        out.append((f"digits {(592 + extra) % 8} mod 8", nzcp.EXAMPLE_PASS_URI.encode() + b"A" * extra))
    long = nzcp.EXAMPLE_PASS_URI.encode()
    out.append(("uri 2048", long + b"A" * (2048 - len(long))))
    out.append(("uri 2049", long + b"A" * (2049 - len(long))))
    out.append(("claims reordered", uri_of(sign1(LIVE_PROTECTED, cbor_encode(nzcp.claims(order=(7, "vc", 4, 5, 1))),
                                                 sig_for("r")))))
    out.append(("no exp", uri_of(sign1(LIVE_PROTECTED, cbor_encode(nzcp.claims(order=(1, 5, "vc", 7))), sig_for("e")))))
    twice = Raw(b"\xa4" + b"".join(cbor_encode(x) for x in (1, nzcp.LIVE_ISS, 4, 1700000000, 5, 1600000000, 4, 1800000000)))
    out.append(("claims key 4 twice", uri_of(sign1(LIVE_PROTECTED, cbor_encode(twice), sig_for("t")))))
    hdr_twice = Raw(b"\xa3" + b"".join(cbor_encode(x) for x in (4, b"first", 1, -7, 4, nzcp.LIVE_KID)))
    out.append(("header key 4 twice", uri_of(sign1(cbor_encode(hdr_twice), payload, sig_for("h")))))
    assert len({n for n, _ in out}) == len(out)
    return tuple(out)


def _with(protected=LIVE_PROTECTED, payload=None, sig=None, **kw) -> bytes:
    return uri_of(sign1(protected, cbor_encode(nzcp.claims()) if payload is None else payload,
                        sig_for("b") if sig is None else sig, **kw))


@functools.lru_cache(maxsize=None)
def set_b() -> tuple:
    """(name, URI bytes, status, detail or None = not pinned here, present bits or None)."""
    ex = nzcp.EXAMPLE_PASS_URI.encode()
    whole = sign1(LIVE_PROTECTED, cbor_encode(nzcp.claims()), sig_for("b"))
    sig_head = len(whole) - 66
    assert whole[sig_head:sig_head + 2] == b"\x58\x40"
    p0 = 3                                     # d2 84 4x | protected bytes: the offset of short protected strings
    everything = HAS_ALG | HAS_KID | HAS_ISS | HAS_NBF | HAS_EXP | HAS_CTI | HAS_SIG
    claims_bits = HAS_ISS | HAS_NBF | HAS_EXP | HAS_CTI
    b = [
        ("empty", b"", PREFIX, 0, None),
        ("prefix alone", b"NZCP:/1/", PREFIX, 0, None),
        ("no slash", b"NZCP:/1", PREFIX, 0, None),
        ("no version", b"NZCP://AAAA", PREFIX, 0, None),
        ("ten digits", b"NZCP:/1234567890/" + ex[8:], PREFIX, 0, None),
        ("lower-case scheme", b"nzcp:/1/" + ex[8:], PREFIX, 0, None),
        ("lower-case digit", ex[:100] + ex[100:101].lower() + ex[101:], BASE32, 100, None),
        ("padding", ex + b"=", BASE32, len(ex), None),
        ("high byte", ex[:50] + b"\xc3" + ex[51:], BASE32, 50, None),
        ("lowest of three", ex[:9] + b"1" + ex[10:70] + b"0" + ex[71:200] + b" " + ex[201:], BASE32, 9, None),
        ("bad last byte of 2048", ex + b"A" * (2047 - len(ex)) + b"8", BASE32, 2047, None),
        ("one digit", b"NZCP:/1/A", TRUNCATED, 0, None),
        ("one-byte cose", uri_of(b"\xd2"), TRUNCATED, 1, None),
        ("bstr 2^32-1", uri_of(b"\xd2\x84\x5a\xff\xff\xff\xff" + bytes(40)), TRUNCATED, 2, None),
        ("bstr 2^64-1", uri_of(b"\xd2\x84\x5b" + b"\xff" * 8 + bytes(40)), TRUNCATED, 2, None),
        ("array 2^64-1", uri_of(b"\xd2\x9b" + b"\xff" * 8 + bytes(40)), TRUNCATED, 1, None),
        ("unprotected array 2^64-1", _with(unprotected=Raw(b"\x9b" + b"\xff" * 8)), TRUNCATED, 3 + len(LIVE_PROTECTED), None),
        ("unprotected map 2^63", _with(unprotected=Raw(b"\xbb\x80" + bytes(7))), TRUNCATED, 3 + len(LIVE_PROTECTED), None),
        ("head cut at the last byte", uri_of(whole[:sig_head + 1]), TRUNCATED, sig_head, None),
        ("body cut", uri_of(whole[:-1]), TRUNCATED, sig_head, None),
        ("inner map beyond its string", _with(protected=b"\xa2\x01\x26"), TRUNCATED, p0 + 3, None),
        ("inner kid beyond its string", _with(protected=b"\xa1\x04\x58\x20ab"), TRUNCATED, p0 + 2, None),
        ("inner count beyond its string", _with(protected=b"\xb8\x40\x01\x26"), TRUNCATED, p0, None),
        ("info 28", _with(unprotected=Raw(b"\x1c")), CBOR, 3 + len(LIVE_PROTECTED), None),
        ("break byte", _with(unprotected=Raw(b"\xff")), CBOR, 3 + len(LIVE_PROTECTED), None),
        ("indefinite array", _with(unprotected=Raw(b"\x9f\x01\xff")), CBOR, 3 + len(LIVE_PROTECTED), None),
        ("info 31 in the claims", _with(payload=b"\xa1\x01\x7f"), CBOR, None, None),
        ("tag 17", _with(tag=b"\xd1"), NOT_COSE, 0, None),
        ("no tag", uri_of(whole[1:]), NOT_COSE, 0, None),
        ("array of 3", uri_of(b"\xd2\x83" + whole[2:sig_head]), NOT_COSE, 1, None),
        ("array of 5", uri_of(b"\xd2\x85" + whole[2:] + b"\x00"), NOT_COSE, 1, None),
        ("a map, not an array", uri_of(b"\xd2\xa2" + whole[2:]), NOT_COSE, 1, None),
        ("protected is text", _with(protected=Raw(b"\x63abc")), NOT_COSE, 2, None),
        ("payload is text", _with(payload=Raw(cbor_encode("payload"))), NOT_COSE, 4 + len(LIVE_PROTECTED), None),
        ("zeros", b"NZCP:/1/AAAA", NOT_COSE, 0, None),
        ("sig 63", _with(sig=bytes(range(63))), OK, 0, everything),
        ("sig 65", _with(sig=bytes(range(65))), OK, 0, everything),
        ("sig 0", _with(sig=b""), OK, 0, everything),
        ("sig is an array", _with(sig=Raw(cbor_encode([1, [2, b"x"]]))), OK, 0, everything & ~HAS_SIG),
        ("empty protected", _with(protected=b""), TRUNCATED, p0, None),
        ("protected is an integer", _with(protected=b"\x01"), HEADER, p0, None),
        ("protected is an array", _with(protected=b"\x82\x01\x26"), HEADER, p0, None),
        ("empty payload", _with(payload=b""), TRUNCATED, None, None),
        ("payload a0", _with(payload=b"\xa0"), OK, 0, HAS_ALG | HAS_KID | HAS_SIG),
        ("payload is an array", _with(payload=b"\x80"), CLAIMS, None, None),
        ("header a0", _with(protected=b"\xa0"), OK, 0, claims_bits | HAS_SIG),
        ("alg is text", _with(protected=cbor_encode({1: "ES256", 4: b"k"})), OK, 0, everything & ~HAS_ALG),
        ("kid is text", _with(protected=cbor_encode({1: -7, 4: "key-1"})), OK, 0, everything & ~HAS_KID),
        ("alg then alg as text", _with(protected=b"\xa2\x01\x26\x01\x61a"), OK, 0, claims_bits | HAS_SIG),
        ("alg 2^40", _with(protected=cbor_encode({1: 1 << 40})), OK, 0, claims_bits | HAS_SIG | HAS_ALG),
        ("alg -2^40", _with(protected=cbor_encode({1: -(1 << 40)})), OK, 0, claims_bits | HAS_SIG | HAS_ALG),
        ("alg -2^31", _with(protected=cbor_encode({1: -(1 << 31)})), OK, 0, claims_bits | HAS_SIG | HAS_ALG),
        ("odd header keys", _with(protected=cbor_encode({-1: 1, "1": 2, b"\x04": 3, Tag(1, 4): b"kid", 1: -7})), OK, 0,
         claims_bits | HAS_SIG | HAS_ALG),
        ("claims of other types", _with(payload=cbor_encode({1: b"iss", 4: -5, 5: "nbf", 7: "cti"})), OK, 0,
         HAS_ALG | HAS_KID | HAS_SIG),
        ("exp 2^64-1, long iss and cti", _with(payload=cbor_encode({4: (1 << 64) - 1, 1: "i" * 65, 7: bytes(range(40)), 5: 0})),
         OK, 0, everything),
        ("major 7 values", _with(unprotected=[False, True, Raw(b"\xf6"), Raw(b"\xf8\x20"), Raw(b"\xf9\x3c\x00"),
                                              Raw(b"\xfa" + bytes(4)), Raw(b"\xfb" + bytes(8)), Raw(b"\xf7")]), OK, 0, everything),
        ("major 7 payload cut", _with(sig=Raw(b"\xfb" + bytes(7))), TRUNCATED, None, None),
        ("depth 500", _with(unprotected=Raw(b"\x81" * 500 + b"\x00")), OK, 0, everything),
        ("depth 500, tags", _with(unprotected=Raw(b"\xc1" * 500 + b"\xa0")), OK, 0, everything),
        ("depth cut", _with(unprotected=Raw(b"\x81" * 1200)), None, None, None),   # 1,200 arrays: the URI is over 2,048
    ]
    out = []
    for name, uri, status, detail, present in b:
        if status is None:
            assert len(uri) > MAX_URI
            status, detail = LENGTH, len(uri)
        out.append((name, uri, status, detail, present))
    assert len({n for n, *_ in out}) == len(out)
    return tuple(out)


@functools.lru_cache(maxsize=None)
def set_c() -> tuple:
    """2,000 seeded mutations of set A's COSE bytes, as URI bytes."""
    rng = random.Random(0x4E5A4350)
    pool = [cose_of(u) for n, u in set_a() if not n.startswith("uri ")]
    widths = (0x18, 0x19, 0x1a, 0x1b, 0x1c, 0x1f, 0x17, 0x00)
    out = []
    for i in range(2000):
        c = bytearray(rng.choice(pool))
        kind = i % 4
        if kind == 0:                                   # one to three bit flips
            for _ in range(rng.randint(1, 3)):
                c[rng.randrange(len(c))] ^= 1 << rng.randrange(8)
        elif kind == 1:                                 # a truncation
            del c[rng.randrange(len(c)):]
        elif kind == 2:                                 # a head's width or length, early in the structure or anywhere
            at = rng.randrange(min(len(c), 40)) if rng.random() < 0.5 else rng.randrange(len(c))
            c[at] = (c[at] & 0xE0) | rng.choice(widths)
            if rng.random() < 0.5 and at + 1 < len(c):
                c[at + 1] = rng.choice((0x00, 0x01, 0x7f, 0x80, 0xff))
        else:                                           # a byte replaced, and perhaps a cut as well
            c[rng.randrange(min(len(c), 40) if rng.random() < 0.5 else len(c))] = rng.randrange(256)
            if rng.random() < 0.3:
                del c[rng.randrange(1, len(c) + 1):]
        out.append(uri_of(bytes(c)))
    return tuple(out)


@functools.lru_cache(maxsize=None)
def expected(which: str, max_tbs: int = LIVE) -> tuple:
    """The restatement over a set, pass i with data_for(i): ((record dict, input block), ...)."""
    uris = uris_of(which)
    return tuple(restate(u, max_tbs, data_for(i)) for i, u in enumerate(uris))


def uris_of(which: str) -> tuple:
    if which == "A":
        return tuple(u for _, u in set_a())
    if which == "B":
        return tuple(u for _, u, *_ in set_b())
    return set_c()
