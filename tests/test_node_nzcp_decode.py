"""Pass decode through Node.js (js/index.js nzcp.decodePasses and verifyPasses with decode:
'device'): set A's records and input signals against the Python binding's and against
nzcp.circuitInput, and the decoded verification route against the default one. The host path
(device -1) runs without a GPU; the same on device 0 is marked gpu."""
import base64
import hashlib
import json
import os
import shutil
import subprocess

import pytest

import nzcb
import nzcp_decode_cases as C
from nzcb import nzcp
from test_node_p256 import _tamper

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
JS = os.path.join(ROOT, "nzcb-circom_amd", "js")
ADDON = os.path.join(JS, "build", "nzcb.node")

needs_node = pytest.mark.skipif(shutil.which("node") is None or not os.path.exists(ADDON),
                                reason="node or the built addon is unavailable")
DEVICES = [pytest.param(-1, id="host"), pytest.param(0, id="gpu", marks=pytest.mark.gpu)]


def run_node(script: str, timeout=300):
    p = subprocess.run(["node", "-e", script], capture_output=True, text=True, timeout=timeout, cwd=JS)
    assert p.returncode == 0, p.stderr
    return p.stdout


DECODE_SCRIPT = """
const crypto = require('crypto');
const m = require('./');
const uris = URIS;
const data = uris.map((_, i) => Buffer.from(Array.from({ length: 20 }, (_, j) => (17 * i + 3 * j + 1) & 255)));
(async () => {
  const { records, inputs } = await m.nzcp.decodePasses(uris, { device: DEVICE, circuit: 'live', data });
  const plain = await m.nzcp.decodePasses(uris, { device: DEVICE });
  const block = inputs.length / uris.length;
  const sameAsCircuitInput = records.map((r, i) => {
    const mine = inputs.subarray(i * block, (i + 1) * block);
    if (!r.fits) return mine.every((b) => b === 0);
    const inp = m.nzcp.circuitInput(uris[i], data[i], 351);
    const want = inp.toBeSigned.concat([inp.toBeSignedLen], inp.data);
    if (want.length * 32 !== block) return false;
    return want.every((v, k) => mine.readUInt32LE(32 * k) === Number(v) &&
      mine.subarray(32 * k + 4, 32 * k + 32).every((b) => b === 0));
  });
  const hex = (r) => Object.assign({}, r, { cti: r.cti && r.cti.toString('hex'), sig: r.sig && r.sig.toString('hex') });
  console.log(JSON.stringify({
    records: records.map(hex),
    inputsSha256: crypto.createHash('sha256').update(inputs).digest('hex'),
    sameAsCircuitInput,
    plainHasInputs: plain.inputs !== undefined,
    plainFits: plain.records.map((r) => r.fits),
    plainSame: JSON.stringify(plain.records.map((r) => Object.assign(hex(r), { fits: null }))) ===
      JSON.stringify(records.map((r) => Object.assign(hex(r), { fits: null }))),
  }));
})().catch((e) => { console.error(e); process.exit(1); });
"""


@needs_node
@pytest.mark.parametrize("device", DEVICES)
def test_decode_passes_equals_python_and_circuit_input(device):
    uris = [u.decode() for u in C.uris_of("A")]
    d = json.loads(run_node(DECODE_SCRIPT.replace("URIS", json.dumps(uris)).replace("DEVICE", str(device))))
    data = [C.data_for(i) for i in range(len(uris))]
    want, inputs = nzcb.nzcp_decode(uris, nzcb.NZCP_LIVE, data, device=nzcb.NZCP_HOST)
    assert d["inputsSha256"] == hashlib.sha256(inputs).hexdigest()
    assert d["sameAsCircuitInput"] == [True] * len(uris)
    assert sum(r["fits"] for r in d["records"]) >= 20
    assert not d["plainHasInputs"] and d["plainSame"] and not any(d["plainFits"])
    names = {"status": "status", "statusName": "status_name", "detail": "detail", "version": "version", "alg": "alg",
             "kidLen": "kid_len", "iss": "iss", "issLen": "iss_len", "nbf": "nbf", "exp": "exp", "ctiLen": "cti_len",
             "sigLen": "sig_len", "coseLen": "cose_len", "protectedOff": "protected_off",
             "protectedLen": "protected_len", "payloadOff": "payload_off", "payloadLen": "payload_len",
             "toBeSignedLen": "tbs_len"}
    for got, w in zip(d["records"], want):
        for js, py in names.items():
            assert got[js] == w[py], (js, got, w)
        assert got["fits"] == bool(w["fits"])
        assert got["kid"] == (w["kid"].decode() if w["kid"] is not None else None)
        assert got["cti"] == (w["cti"].hex() if w["cti"] is not None else None)
        assert got["sig"] == (w["sig"].hex() if w["sig"] is not None else None)
        assert got["toBeSignedHash"] == w["tbs_sha256"].hex()


@needs_node
@pytest.mark.parametrize("device", DEVICES)
def test_verify_passes_decode_device_equals_the_default_route(device):
    protected, payload, sig = nzcp.decode_pass(nzcp.EXAMPLE_PASS_URI)

    def uri(prot, sg):
        cose = nzcp.cbor_encode(nzcp.Tag(18, [prot, {}, payload, sg]))
        return "NZCP:/1/" + base64.b32encode(cose).decode().rstrip("=")

    es384 = nzcp.cbor_encode({4: nzcp.EXAMPLE_KID, 1: -35})
    uris = [uri(protected, sig), uri(es384, sig), uri(protected, sig[:63]), "NZCP:/1/AAAA", nzcp.EXAMPLE_PASS_URI,
            _tamper(nzcp.EXAMPLE_PASS_URI), uri(protected, bytes(64)), "not a pass"]
    script = f"""
const m = require('./');
(async () => {{
  const uris = {json.dumps(uris)};
  const plain = await m.nzcp.verifyPasses(uris, {{key: 'example', device: {device}, now: 1700000000}});
  const decoded = await m.nzcp.verifyPasses(uris, {{key: 'example', device: {device}, now: 1700000000,
    decode: 'device'}});
  let bad = null;
  try {{ await m.nzcp.verifyPasses(uris, {{key: 'example', device: {device}, decode: 'host'}}); }}
  catch (e) {{ bad = e.message; }}
  console.log(JSON.stringify({{plain, decoded, bad}}));
}})().catch((e) => {{ console.error(e); process.exit(1); }});
"""
    d = json.loads(run_node(script))
    assert "options.decode" in d["bad"]
    assert [r["valid"] for r in d["decoded"]] == [True, False, False, False, True, False, False, False]
    assert [r["status"] for r in d["decoded"]] == [0, None, None, None, 0, 1, 2, None]
    assert d["decoded"][3]["reason"] == "malformed pass: NOT_COSE at 0"
    assert d["decoded"][7]["reason"] == "malformed pass: PREFIX at 0"
    for p, q in zip(d["plain"], d["decoded"]):
        if p["reason"] and p["reason"].startswith("malformed pass"):
            q = dict(q, reason=p["reason"])
        assert p == q
