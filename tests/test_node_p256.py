"""Pass-signature verification through Node.js (js/index.js nzcp.verifyPass / verifyPasses /
p256Verify and `cli.js nzcp verify`): the verdicts against OpenSSL's (Node's crypto.verify, the
one implementation here that this project did not write) on a key pair and signatures made at
test time, the NZCP example pass, and the CLI verb's lines and exit codes. The host path
(device -1) runs without a GPU; the same on device 0 is marked gpu."""
import json
import os
import shutil
import subprocess

import pytest

from nzcb import nzcp

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


def _tamper(uri: str) -> str:
    """Another base32 digit eight from the end: five bits of the signature's s."""
    return uri[:-8] + ("A" if uri[-8] != "A" else "B") + uri[-7:]


OPENSSL_SCRIPT = """
const crypto = require('crypto');
const m = require('./');
const N = BigInt('0xffffffff00000000ffffffffffffffffbce6faada7179e84f3b9cac2fc632551');
const be = (x) => Buffer.from(x.toString(16).padStart(64, '0'), 'hex');
(async () => {
  const { publicKey, privateKey } = crypto.generateKeyPairSync('ec', { namedCurve: 'prime256v1' });
  const spki = publicKey.export({ type: 'spki', format: 'der' });
  if (spki.length !== 91 || spki[26] !== 4) throw new Error('unexpected SPKI layout');
  const key = spki.subarray(27);
  const msgs = [];
  const sigs = [];
  for (let i = 0; i < 32; i++) {
    let msg = crypto.randomBytes(1 + 5 * i);
    let sig = crypto.sign('sha256', msg, { key: privateKey, dsaEncoding: 'ieee-p1363' });
    if (sig.length !== 64) throw new Error('not an r || s signature');
    const s = BigInt('0x' + sig.subarray(32).toString('hex'));
    switch (i % 8) {
      case 1: sig[i % 64] ^= 1 << (i % 8); break;                       // a bit of r or s
      case 2: msg = Buffer.concat([msg, Buffer.from([i])]); break;       // another message
      case 3: sig = Buffer.concat([sig.subarray(0, 32), be(N - s)]); break;   // the high-s / low-s twin
      case 5: sig = Buffer.concat([i & 8 ? be(BigInt(0)) : be(N), sig.subarray(32)]); break;   // r out of range
      case 6: sig = Buffer.concat([sig.subarray(0, 32), i & 8 ? be(BigInt(0)) : be(N)]); break; // s out of range
      default: break;
    }
    msgs.push(msg);
    sigs.push(sig);
  }
  const openssl = msgs.map((msg, i) => crypto.verify('sha256', msg, { key: publicKey, dsaEncoding: 'ieee-p1363' },
    sigs[i]));
  const hashes = msgs.map((msg) => crypto.createHash('sha256').update(msg).digest());
  const status = await m.nzcp.p256Verify(key, hashes, sigs, { device: DEVICE });
  const jwk = { x: key.subarray(0, 32).toString('base64'), y: key.subarray(32).toString('base64') };
  const again = await m.nzcp.p256Verify(jwk, hashes, sigs, { device: DEVICE });
  console.log(JSON.stringify({ openssl, status, again }));
})().catch((e) => { console.error(e); process.exit(1); });
"""


@needs_node
@pytest.mark.parametrize("device", DEVICES)
def test_verdicts_equal_openssl(device):
    d = json.loads(run_node(OPENSSL_SCRIPT.replace("DEVICE", str(device))))
    assert len(d["openssl"]) == 32
    assert [s == 0 for s in d["status"]] == d["openssl"]
    assert d["again"] == d["status"]
    # the mix is as built: untouched and twin signatures verify, the rest do not, range ones say so
    assert [i for i, ok in enumerate(d["openssl"]) if ok] == [i for i in range(32) if i % 8 in (0, 3, 4, 7)]
    assert [i for i, s in enumerate(d["status"]) if s == 2] == [i for i in range(32) if i % 8 in (5, 6)]


@needs_node
@pytest.mark.parametrize("device", DEVICES)
def test_verify_pass_on_the_example_pass(device):
    uri = nzcp.EXAMPLE_PASS_URI
    flipped = _tamper(uri)
    script = f"""
const m = require('./');
(async () => {{
  const one = await m.nzcp.verifyPass({json.dumps(uri)}, {{key: 'example', device: {device}, now: 1700000000}});
  const many = await m.nzcp.verifyPasses([{json.dumps(uri)}, {json.dumps(flipped)}, 'NZCP:/1/AAAA'],
    {{key: m.nzcp.EXAMPLE_PUBLIC_KEY, device: {device}}});
  const late = await m.nzcp.verifyPass({json.dumps(uri)}, {{key: 'example', device: {device}, now: 1951416330}});
  let noKey = null;
  try {{ await m.nzcp.verifyPass({json.dumps(uri)}, {{device: {device}}}); }} catch (e) {{ noKey = e.message; }}
  let badKey = null;
  try {{ await m.nzcp.verifyPass({json.dumps(uri)}, {{key: Buffer.alloc(64), device: {device}}}); }}
  catch (e) {{ badKey = e.message; }}
  console.log(JSON.stringify({{one, many, late, noKey, badKey}}));
}})().catch((e) => {{ console.error(e); process.exit(1); }});
"""
    d = json.loads(run_node(script))
    assert d["one"] == {"valid": True, "status": 0, "reason": None, "alg": -7, "kid": "key-1",
                        "iss": nzcp.EXAMPLE_ISS, "nbf": nzcp.EXAMPLE_NBF, "exp": nzcp.EXAMPLE_EXP,
                        "expired": False, "notYetValid": False}
    assert [r["valid"] for r in d["many"]] == [True, False, False]
    assert d["many"][1]["status"] == 1 and d["many"][1]["reason"] == "invalid signature"
    assert d["many"][2]["status"] is None and d["many"][2]["reason"].startswith("malformed pass")
    assert "expired" not in d["many"][0]
    assert d["late"]["valid"] and d["late"]["expired"] and not d["late"]["notYetValid"]
    assert "options.key" in d["noKey"]
    assert d["badKey"] == "public key is not a point on P-256"


@needs_node
@pytest.mark.parametrize("device", DEVICES)
def test_cli_nzcp_verify(device, tmp_path):
    uri = nzcp.EXAMPLE_PASS_URI
    tampered = _tamper(uri)
    good, mixed = tmp_path / "good.txt", tmp_path / "mixed.txt"
    good.write_text(uri + "\n\n" + uri + "\n")
    mixed.write_text(uri + "\n" + tampered + "\nnot a pass\n")
    env = dict(os.environ, NZCB_DEVICE=str(device))
    key = nzcp.EXAMPLE_PUBLIC_KEY

    def cli(*args):
        return subprocess.run(["node", "cli.js", "nzcp", "verify", *args], capture_output=True, text=True,
                              timeout=300, cwd=JS, env=env)

    p = cli(str(good))
    assert (p.returncode, p.stdout.splitlines()) == (0, ["OK", "OK"]), p.stderr
    p = cli(str(good), "example")
    assert (p.returncode, p.stdout.splitlines()) == (0, ["OK", "OK"]), p.stderr
    p = cli(str(good), key["x"], key["y"])
    assert (p.returncode, p.stdout.splitlines()) == (0, ["OK", "OK"]), p.stderr
    p = cli(str(mixed))
    lines = p.stdout.splitlines()
    assert p.returncode == 1 and lines[:2] == ["OK", "INVALID SIGNATURE"] and lines[2].startswith("malformed pass")
    p = cli(str(good), key["y"], key["x"])     # not a point: an error, not a verdict
    assert p.returncode == 1 and "public key is not a point on P-256" in p.stderr
    p = subprocess.run(["node", "cli.js", "nzcp"], capture_output=True, text=True, timeout=60, cwd=JS)
    assert p.returncode == 1 and "nzcp verify" in p.stderr
