"""The key material check through Node.js: js/index.js powersOfTau.check and zKey.check, and the
cli.js verbs `powersoftau check` and `zkey check` with their exit codes, on a power-3 ptau and
the golden p5 key, a good and a bad file each. The host path (device -1) runs without a GPU; the
same on device 0 is marked gpu."""
import json
import os
import shutil
import subprocess

import pytest

import key_check_cases as kc
import nzcb

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
JS = os.path.join(ROOT, "nzcb-circom_amd", "js")
ADDON = os.path.join(JS, "build", "nzcb.node")

pytestmark = pytest.mark.skipif(shutil.which("node") is None or not os.path.exists(ADDON),
                                reason="node or the built addon is unavailable")
DEVICES = [pytest.param(-1, id="host"), pytest.param(0, id="gpu", marks=pytest.mark.gpu)]


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    d = tmp_path_factory.mktemp("keys")
    pts = kc.raw_points(kc.TAU, 15)
    bad = list(pts)
    kc.spoil_other_point(bad, 9)
    z = kc.golden_zkey("p5")
    n = kc.zkey_n(z)
    off = kc.part_offset(z, "Ql") + 32 * (5 * n - 1)
    out = {"good.ptau": kc.make_ptau(3, pts), "bad.ptau": kc.make_ptau(3, bad), "good.zkey": z,
           "bad.zkey": kc.patch(z, off, bytes([z[off] ^ 1]))}
    for name, data in out.items():
        (d / name).write_bytes(data)
    return {name: str(d / name) for name in out}


def cli(device: int, *args):
    env = dict(os.environ, NZCB_DEVICE=str(device))
    p = subprocess.run(["node", "cli.js", *args], capture_output=True, text=True, timeout=300, cwd=JS, env=env)
    return p.returncode, p.stdout.splitlines(), p.stderr


@pytest.mark.parametrize("device", DEVICES)
def test_cli_powersoftau_check(files, device):
    rc, lines, err = cli(device, "powersoftau", "check", files["good.ptau"])
    assert (rc, lines) == (0, ["tauG1: OK (15 checked)"]), err
    rc, lines, err = cli(device, "powersoftau", "check", files["bad.ptau"])
    assert (rc, lines) == (1, ["tauG1: SEQUENCE at 9"]), err
    rc, lines, err = cli(device, "powersoftau", "check", files["bad.ptau"], "1")  # 2^1 + 6 points: before the defect
    assert (rc, lines) == (0, ["tauG1: OK (8 checked)"]), err
    rc, lines, err = cli(device, "powersoftau", "check", files["good.zkey"])
    assert rc == 1 and lines == [] and "invalid file format" in err


@pytest.mark.parametrize("device", DEVICES)
def test_cli_zkey_check(files, device):
    n = kc.zkey_n(kc.golden_zkey("p5"))
    rc, lines, err = cli(device, "zkey", "check", files["good.zkey"])
    assert rc == 0 and len(lines) == 13 and all(": OK (" in ln for ln in lines), err
    assert lines[1] == f"PTau: OK ({n + 6} checked)" and lines[3] == f"Ql: OK ({5 * n} checked)"
    rc, lines, err = cli(device, "zkey", "check", files["bad.zkey"])
    assert rc == 1 and lines[3] == f"Ql: EVALS at {4 * n - 1}, 1 defective", err
    assert all(": OK (" in ln for k, ln in enumerate(lines) if k != 3) and len(lines) == 13


@pytest.mark.parametrize("device", DEVICES)
def test_api_matches_the_python_binding(files, device):
    script = """
const m = require('./');
(async () => {
  const lines = [];
  const logger = { info: (s) => lines.push(s) };
  const bad = await m.powersOfTau.check(FILES['bad.ptau'], logger, { device: DEVICE });
  const good = await m.powersOfTau.check(require('fs').readFileSync(FILES['good.ptau']), null, { device: DEVICE, power: 3 });
  const zk = await m.zKey.check(FILES['bad.zkey'], logger, { device: DEVICE });
  console.log(JSON.stringify({ bad, good, zk, lines: lines.length }));
})().catch((e) => { console.error(e); process.exit(1); });
""".replace("FILES", json.dumps(files)).replace("DEVICE", str(device))
    p = subprocess.run(["node", "-e", script], capture_output=True, text=True, timeout=300, cwd=JS)
    assert p.returncode == 0, p.stderr
    got = json.loads(p.stdout)

    def as_js(f):
        d = {"status": f["status"], "index": f["index"], "nBad": f["n_bad"], "checked": f["checked"]}
        if "commit_checked" in f:
            d["commitChecked"] = f["commit_checked"]
        return d

    def no_checks(f):
        return {k: v for k, v in f.items() if k != "pairingChecks"}

    want = nzcb.ptau_check(files["bad.ptau"], device=device, seed=kc.SEED)
    assert no_checks(got["bad"]) == as_js(want) and got["bad"]["pairingChecks"] >= 2
    assert got["good"] == dict(as_js(nzcb.ptau_check(files["good.ptau"], count=14, device=device)), pairingChecks=1)
    want = nzcb.zkey_check(files["bad.zkey"], device=device)
    assert got["zk"]["ok"] is False and got["lines"] == 14
    assert {k: v for k, v in got["zk"]["parts"].items()} == {k: as_js(v) for k, v in want["parts"].items()}
    assert no_checks(got["zk"]["srs"]) == as_js(want["srs"]) and no_checks(got["zk"]["header"]) == as_js(want["header"])
