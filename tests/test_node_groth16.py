"""Groth16 key generation through Node.js: the first three `phase2` command lines of snarkjs
(groth16 setup, zkey contribute, zkey export verificationkey) through cli.js on the random circuit
of tests/groth16_cases.py, the refusal of `zkey export solidityverifier`, and js/index.js zKey with
snarkjs's names and argument order. The host path (NZCB_DEVICE=-1) runs without a GPU."""
import json
import os
import shutil
import subprocess

import pytest

import groth16_cases as gc
import groth16_checks as ck
import nzcb

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
JS = os.path.join(ROOT, "nzcb-circom_amd", "js")
ADDON = os.path.join(JS, "build", "nzcb.node")
GOLD = os.path.join(ROOT, "tests", "golden")

pytestmark = pytest.mark.skipif(shutil.which("node") is None or not os.path.exists(ADDON),
                                reason="node or the built addon is unavailable")
DEVICES = [pytest.param(-1, id="host"), pytest.param(0, id="gpu", marks=pytest.mark.gpu)]
HOST = nzcb.GROTH16_HOST


def cli(device: int, *args):
    env = dict(os.environ, NZCB_DEVICE=str(device))
    p = subprocess.run(["node", "cli.js", *args], capture_output=True, text=True, timeout=300, cwd=JS, env=env)
    return p.returncode, p.stdout.splitlines(), p.stderr


def inputs(d, device):
    r1cs, _ = gc.random_circuit(21)
    rp, pp = str(d / "circuit.r1cs"), str(d / "pot7_final.ptau")
    with open(rp, "wb") as f:
        f.write(r1cs)
    with open(pp, "wb") as f:
        f.write(ck.prepared(7, device))
    return r1cs, rp, pp


@pytest.mark.parametrize("device", DEVICES)
def test_cli_phase2_recipe(tmp_path, device):
    """The recipe's lines with only the program name changed."""
    r1cs, rp, pp = inputs(tmp_path, device)
    z0, z1, vkp, sol = (str(tmp_path / n) for n in ("circuit_0000.zkey", "circuit_0001.zkey", "verification_key.json",
                                                   "verifier.sol"))
    rc, lines, err = cli(device, "groth16", "setup", rp, pp, z0)
    assert rc == 0 and len(lines) == 1 and "delta = 1" in lines[0] and "NO circuit hash" in lines[0], err
    with open(z0, "rb") as f:
        fresh = f.read()
    assert fresh == nzcb.groth16_setup(r1cs, ck.prepared(7, device), device=HOST)
    rc, lines, err = cli(device, "zkey", "contribute", z0, z1, "--name=1st Contributor Name", "-v", "-e=some entropy")
    assert rc == 0 and len(lines) == 1 and "NO contribution record" in lines[0] and "1st Contributor Name" in lines[0], err
    assert "not recorded" in lines[0]
    with open(z1, "rb") as f:
        key = f.read()
    assert key != fresh and len(key) == len(fresh)
    assert all(gc.sections(key)[sid] == gc.sections(fresh)[sid] for sid in (1, 3, 4, 5, 6, 7, 10))
    rc, _, err = cli(device, "zkey", "export", "verificationkey", z1, vkp)
    assert rc == 0, err
    with open(vkp) as f:
        vk = json.load(f)
    assert vk == nzcb.groth16_vk(key) and list(vk) == list(nzcb.groth16_vk(key))
    rc, _, err = cli(device, "zkey", "export", "solidityverifier", z1, sol)
    assert rc != 0 and "groth16: the Solidity verifier is not implemented" in err and not os.path.exists(sol)
    # a PLONK key still exports as before, and is no input to contribute
    rc, _, err = cli(device, "zkey", "export", "verificationkey", os.path.join(GOLD, "p5.zkey"), vkp)
    assert rc == 0, err
    with open(vkp) as f:
        assert json.load(f)["protocol"] == "plonk"
    rc, _, err = cli(device, "zkey", "contribute", os.path.join(GOLD, "p5.zkey"), str(tmp_path / "no.zkey"))
    assert rc == 1 and "zkey file is not groth16" in err and not os.path.exists(tmp_path / "no.zkey")
    rc, _, err = cli(device, "groth16", "prove", z1, "w.wtns", "proof.json", "public.json")
    assert rc == 1 and "usage" in err


def test_api_names(tmp_path):
    r1cs, rp, pp = inputs(tmp_path, HOST)
    script = """
const m = require('./');
(async () => {
  const lines = [];
  const logger = { info: (s) => lines.push(s) };
  const out = {};
  await m.zKey.newZKey(R1CS, PTAU, DIR + '/a0.zkey', logger, { device: -1 });
  await m.zKey.contribute(DIR + '/a0.zkey', DIR + '/a1.zkey', 'me', 'entropy', logger, { device: -1 });
  out.vk = await m.zKey.exportVerificationKey(DIR + '/a1.zkey');
  out.mem = await m.zKey.exportVerificationKey({ type: 'mem', data: require('fs').readFileSync(DIR + '/a1.zkey') });
  try { await m.zKey.contribute(DIR + '/a0.zkey', DIR + '/a0.zkey', 'me', ''); } catch (e) { out.same = e.message; }
  try { await m.zKey.exportSolidityVerifier(DIR + '/a1.zkey'); } catch (e) { out.sol = e.message; }
  out.lines = lines;
  console.log(JSON.stringify(out));
})().catch((e) => { console.error(e); process.exit(1); });
""".replace("DIR", json.dumps(str(tmp_path))).replace("R1CS", json.dumps(rp)).replace("PTAU", json.dumps(pp))
    p = subprocess.run(["node", "-e", script], capture_output=True, text=True, timeout=300, cwd=JS,
                       env=dict(os.environ, NZCB_DEVICE="-1"))
    assert p.returncode == 0, p.stderr
    got = json.loads(p.stdout)
    with open(tmp_path / "a0.zkey", "rb") as f:
        assert f.read() == gc.expected_zkey(r1cs, 7, ck.A)
    assert got["vk"] == nzcb.groth16_vk(str(tmp_path / "a1.zkey")) == got["mem"]
    assert "output path is an input" in got["same"] and got["sol"] == "groth16: the Solidity verifier is not implemented"
    assert len(got["lines"]) == 2 and "NO contribution record" in got["lines"][1] and '"me"' in got["lines"][1]
