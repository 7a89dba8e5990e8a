"""The device plumbing the self-contained entry points share (csrc/devcall.h): a device id that
does not exist is NZCB_ERR_ARG "no such device" in every family, the host ids still select the
host paths, and a call on another device leaves the calling thread on the device it came from.
Each family runs its smallest input: one proof, the smallest random r1cs, one signature, one URI."""
import ctypes
import json
import os
import threading

import pytest

import nzcb
import p256_cases as P
import r1cs_check_cases as RC
import verify_batch_cases as VC
from nzcb import nzcp

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
NO_DEVICE = 1 << 20
URI = nzcp.EXAMPLE_PASS_URI.encode()


@pytest.fixture(scope="module")
def proof():
    """(vk, proof, public signals) of the golden n = 2^5 circuit: the oracle's committed proof."""
    with open(os.path.join(GOLD, "p5.json")) as f:
        exp = json.load(f)["proofs"]["fixed"]
    with open(os.path.join(GOLD, "p5.zkey"), "rb") as f:
        vk = nzcb.vk_from_zkey(f.read())
    pub = b"".join(int(s).to_bytes(32, "little") for s in exp["publicSignals"])
    return vk, bytes.fromhex(exp["proof_bin"]), pub


@pytest.fixture(scope="module")
def r1cs():
    return RC.random_cases()[0]


@pytest.fixture(scope="module")
def lincomb():
    return VC.pack([[(VC.G, 1)]])  # one group of one term: 1 * G


class DevUris:
    """The example URI, its offsets and room for one record in HBM on `device`."""

    def __init__(self, device):
        blob, offs = nzcb.pack_uris([URI])
        self.size = ctypes.sizeof(nzcb.NzcpPass)
        self.bufs = []
        for n in (len(blob), 8, self.size):
            p = nzcb.load().nzcb_dev_alloc_on(device, n)
            assert p
            self.bufs.append(p)
        nzcb.h2d(self.bufs[0], blob)
        nzcb.h2d(self.bufs[1], bytes(offs))

    def decode(self, device):
        uris, offs, passes = self.bufs
        nzcb.nzcp_decode_dev(uris, offs, 1, passes, device=device)
        return nzcb.nzcp_passes_from_bytes(nzcb.d2h(passes, self.size), 1)

    def free(self):
        for p in self.bufs:
            nzcb.dev_free(p)


def _no_such_device(fn):
    with pytest.raises(nzcb.NzcbError) as e:
        fn()
    assert (e.value.name, str(e.value)) == ("ARG", "no such device")


def test_a_device_that_does_not_exist_is_an_argument_error(proof, lincomb):
    vk, prf, pub = proof
    _no_such_device(lambda: nzcb.verify_batch(vk, [prf], [pub], device=NO_DEVICE))
    _no_such_device(lambda: nzcb.Engine.g1_lincomb(*lincomb, device=NO_DEVICE))
    _no_such_device(lambda: nzcb.P256Key(nzcp.EXAMPLE_PUBLIC_KEY, device=NO_DEVICE))
    _no_such_device(lambda: nzcb.nzcp_decode([URI], device=NO_DEVICE))
    d = DevUris(0)
    try:
        _no_such_device(lambda: d.decode(NO_DEVICE))
        assert d.decode(0)[0]["status"] == 0
    finally:
        d.free()


def test_host_ids_select_the_host_paths(proof, lincomb, r1cs):
    vk, prf, pub = proof
    assert list(nzcb.verify_batch(vk, [prf], [pub], device=nzcb.VERIFY_HOST)) == [True]
    assert nzcb.Engine.g1_lincomb(*lincomb, device=nzcb.VERIFY_HOST) == [VC.pt_bytes(VC.G)]
    name, data, wits = r1cs
    r = nzcb.R1cs(data, device=nzcb.R1CS_HOST)
    try:
        assert r.check(RC.pack(wits[:1])) == [RC.expected(data, wits[0])]
    finally:
        r.close()
    z, sig = P.example_hash_sig()
    key = P.example_key(nzcb.P256_HOST)
    try:
        assert key.verify([z], [sig]) == [nzcb.SIG_OK]
    finally:
        key.close()
    assert nzcb.nzcp_decode([URI], device=nzcb.NZCP_HOST)[0]["status"] == 0


def _hip():
    """The HIP runtime libnzcb.so has loaded, by the path it was mapped from."""
    nzcb.load()
    with open("/proc/self/maps") as f:
        paths = {line.split()[-1] for line in f if "libamdhip64" in line}
    assert len(paths) == 1, paths
    return ctypes.CDLL(paths.pop())


def test_a_call_on_another_device_leaves_the_caller_on_its_own(proof, lincomb, r1cs):
    if nzcb.device_count() < 2:
        pytest.skip("one GPU: nothing to return from")
    hip = _hip()
    vk, prf, pub = proof
    name, data, wits = r1cs
    z, sig = P.example_hash_sig()
    seen = {}

    def current(tag):
        dev = ctypes.c_int(-1)
        assert hip.hipGetDevice(ctypes.byref(dev)) == 0
        seen[tag] = dev.value

    def calls():
        assert hip.hipSetDevice(0) == 0
        seen["verify"] = list(nzcb.verify_batch(vk, [prf], [pub], device=1))
        current("after verify_batch")
        seen["lincomb"] = nzcb.Engine.g1_lincomb(*lincomb, device=1)
        current("after g1_lincomb")
        r = nzcb.R1cs(data, device=1)
        current("after R1cs")
        seen["r1cs"] = r.check(RC.pack(wits[:1]))
        current("after R1cs.check")
        r.close()
        current("after R1cs.close")
        key = P.example_key(1)
        current("after P256Key")
        seen["p256"] = key.verify([z], [sig])
        current("after P256Key.verify")
        key.close()
        current("after P256Key.close")
        seen["decode"] = nzcb.nzcp_decode([URI], device=1)[0]["status"]
        current("after nzcp_decode")
        d = DevUris(1)
        try:
            seen["decode_dev"] = d.decode(1)[0]["status"]
            current("after nzcp_decode_dev")
        finally:
            d.free()

    failure = []

    def run():
        try:
            calls()
        except BaseException as e:  # noqa: BLE001 (re-raised in the test's thread)
            failure.append(e)

    t = threading.Thread(target=run)
    t.start()
    t.join()
    if failure:
        raise failure[0]
    assert {k: v for k, v in seen.items() if k.startswith("after ")} == {
        k: 0 for k in ("after verify_batch", "after g1_lincomb", "after R1cs", "after R1cs.check", "after R1cs.close",
                       "after P256Key", "after P256Key.verify", "after P256Key.close", "after nzcp_decode",
                       "after nzcp_decode_dev")}
    assert seen["verify"] == [True] and seen["lincomb"] == [VC.pt_bytes(VC.G)]
    assert seen["r1cs"] == [RC.expected(data, wits[0])] and seen["p256"] == [nzcb.SIG_OK]
    assert seen["decode"] == 0 and seen["decode_dev"] == 0
