"""The witness check on the device (csrc/r1cs_check.hip: the lane-per-row and wave-per-row
kernels and the bitmap collection) against the host path, which tests/test_r1cs_check.py pins
to the exact-integer reference: every case list field for field, batched and one witness at a
time; witnesses checked in place where the GPU witness VM wrote them; the single-wire soundness
probe on nzcp_live against the constraints computed in Python; a check while a context proves;
the Node.js calls and CLI verbs."""
import json
import os
import random
import shutil
import struct
import subprocess

import pytest

import nzcb
import nzcp_cases as NC
import r1cs_check_cases as C
from oracle.binfmt import write_binfile
from oracle.bn254 import P_MOD, R_MOD as R, to_le

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
JS = os.path.join(ROOT, "nzcb-circom_amd", "js")
GOLD = os.path.join(ROOT, "tests", "golden")
HOST = nzcb.R1CS_HOST


def _both(case, cap=8, one_by_one=False, **kw):
    """The case on the host and on device 0; asserts equality and returns the results."""
    name, data, wits = case
    host, dev = nzcb.R1cs(data, device=HOST), nzcb.R1cs(data, device=0, **kw)
    try:
        assert dev.info == dict(host.info, **{k: dev.info[k] for k in ("long_row_threshold", "n_long_rows")})
        want = C.check_all(host, case, cap)
        assert C.check_all(dev, case, cap) == want, name
        if one_by_one:
            assert C.check_all(dev, case, cap, batch=False) == want, name
    finally:
        host.close()
        dev.close()
    return want


# ---------------------------------------------------------------- host equality
@pytest.mark.parametrize("case", C.random_cases(), ids=lambda c: c[0])
def test_random_r1cs_equal_host(case):
    want = _both(case)
    assert want[0]["n_bad"] == 0 and any(w["n_bad"] for w in want[1:])


def test_edge_r1cs_equals_host():
    case, uses_one = C.edge_case()
    want = _both(case, cap=64, one_by_one=True)
    assert want[0]["n_bad"] == 0 and set(want[1]["bad"]) == uses_one


@pytest.mark.parametrize("n", C.SIZES)
def test_sizes_equal_host(n):
    want = _both(C.size_case(n), cap=200, one_by_one=True)
    if n:
        assert [w["bad"] for w in want] == [[], [0], [n - 1], list(range(n))]


def test_count_zero_batch_stride_and_caps_equal_host():
    name, data, wits = C.size_case(65)
    two = C.bump(C.bump(wits[0], 66 + 7), 66 + 40)
    batch = [wits[3], wits[0], two, wits[2], wits[1]]
    stride = 32 * len(wits[0]) + 48
    host, dev = nzcb.R1cs(data, device=HOST), nzcb.R1cs(data, device=0)
    try:
        assert dev.check(b"", count=0) == []
        for cap in (0, 1, 8, 64, 65, 100):
            got = dev.check(C.pack(batch, stride), count=5, bad_cap=cap, stride=stride)
            assert got == host.check(C.pack(batch, stride), count=5, bad_cap=cap, stride=stride), cap
        assert [g["n_bad"] for g in got] == [65, 0, 2, 1, 1]
        # every tile size and remainder: 1 to 9 witnesses, in both orders
        many = (batch + batch[::-1])[:9]
        want = host.check(C.pack(many))
        for k in range(1, 10):
            assert dev.check(C.pack(many[:k])) == want[:k], k
        assert dev.check(C.pack(many[::-1]))[::-1] == want
    finally:
        host.close()
        dev.close()


def test_long_rows_equal_host():
    r = nzcb.R1cs(C.size_case(1)[1], device=0)
    T = r.info["long_row_threshold"]
    r.close()
    case, lengths = C.long_rows_case(T)
    want = _both(case, one_by_one=True)
    assert want[0]["n_bad"] == 0
    assert [w["bad"] for w in want[1:]] == [[k] for k in range(len(lengths))]
    r = nzcb.R1cs(case[1], device=0)
    assert r.info["n_long_rows"] == sum(n >= T for n in lengths)
    r.close()


@pytest.mark.parametrize("kw", [dict(long_row_threshold=1), dict(long_row_threshold=3, witness_tile=1),
                                dict(long_row_threshold=1 << 20), dict(witness_tile=2), dict(witness_tile=4)],
                         ids=lambda kw: "-".join(f"{k[0]}{v}" for k, v in kw.items()))
def test_threshold_and_tile_do_not_change_results(kw):
    """Every row on the wave path, every row on the lane path, and each tile size."""
    _both(C.random_cases()[3], **kw)
    _both(C.long_rows_case(64)[0], **kw)
    _both(C.edge_case()[0], cap=64, **kw)


def test_wtns_input_on_device():
    name, data, wits = C.random_cases()[0]
    host, dev = nzcb.R1cs(data, device=HOST), nzcb.R1cs(data, device=0)
    try:
        for w in wits[:4]:
            assert dev.check(C.wtns_file(w)) == dev.check(C.pack([w])) == host.check(C.pack([w]))
    finally:
        host.close()
        dev.close()


def test_wrapper_circuit_on_device():
    c, data, good, carried = C.wrapper_case(3)
    want_bad = C.violated(c, carried, range(len(c.constraints)))
    got = _both(("quinSelector3", data, [good, carried]), cap=len(c.constraints))
    assert got[0]["n_bad"] == 0
    assert got[1] == {"n_bad": len(want_bad), "first_bad": want_bad[0], "bad": want_bad}


# ---------------------------------------------------------------- errors
def _err(fn, code, text):
    with pytest.raises(nzcb.NzcbError) as e:
        fn()
    assert (e.value.name, str(e.value)) == (code, text)


def test_errors_on_device_and_the_setup_readers_texts():
    name, data, wits = C.size_case(3)
    r = nzcb.R1cs(data, device=0)
    try:
        _err(lambda: r.check(C.pack([wits[0] + [5]]), count=1), "WITNESS_LEN",
             "Invalid witness length. Circuit: 7, witness: 8")
        buf = nzcb.dev_alloc(32 * 8)
        try:
            _err(lambda: r.check_dev(buf + 4, 1, 32 * 7), "ARG",
                 "device witnesses and their stride must be 16-byte aligned")
        finally:
            nzcb.dev_free(buf)
    finally:
        r.close()
    _err(lambda: nzcb.R1cs(data.replace(to_le(R), to_le(P_MOD), 1), device=0), "CURVE",
         "r1cs: curve not supported (the prime is not BN254's r)")
    _err(lambda: nzcb.R1cs(data, device=1 << 20), "ARG", "no such device")
    # the format messages shared with nzcb_plonk_setup, on the same bytes
    ptau = write_binfile(b"ptau", 1, [(1, struct.pack("<I", 32) + to_le(P_MOD) + struct.pack("<II", 3, 3)),
                                      (2, bytes(64)), (3, bytes(256))])
    good, hdr, body, malformed = C.malformed_files()
    for bad, text in malformed:
        _err(lambda: nzcb.R1cs(bad, device=0), "FORMAT", text)
        _err(lambda: nzcb.plonk_setup(bad, ptau, device=0), "FORMAT", text)


# ---------------------------------------------------------------- GPU witnesses, in place
@pytest.fixture(scope="module")
def example_program():
    from nzcb import nzcpgen, nzcplive
    r1cs, prog, _ = nzcplive.build(nzcpgen.EXAMPLE)
    return r1cs, prog


def test_check_in_place_of_gpu_witnesses(example_program):
    """WitnessProgram.run_dev writes the example pass and 3 input-mutated copies into one
    buffer (padded stride); check_dev reads that buffer where it is."""
    from nzcb import nzcp
    r1cs, prog = example_program
    inp = nzcp.circuit_input(nzcp.to_be_signed(nzcp.EXAMPLE_PASS_URI), bytes(range(1, 21)),
                             nzcp.EXAMPLE_TOBESIGNED_MAX)
    good = nzcp.input_signals(inp)
    n_in = len(good) // 32
    n_bits = n_in - 161

    def put(raw, k, v):
        return raw[:32 * k] + v.to_bytes(32, "little") + raw[32 * (k + 1):]

    inputs = [good,
              put(good, n_bits + 1, 1),                                         # other data: another valid witness
              put(good, 40, 2),                                                 # a toBeSigned signal that is no bit
              put(good, n_bits, int.from_bytes(good[32 * n_bits:32 * n_bits + 32], "little") + 1)]  # a wrong length
    wp = nzcb.WitnessProgram(prog)
    host, dev = nzcb.R1cs(r1cs, device=HOST), nzcb.R1cs(r1cs, device=0)
    stride = 32 * wp.n_wires + 64
    d_in, d_wit = nzcb.dev_alloc(len(good) * 4), nzcb.dev_alloc(stride * 4)
    try:
        assert dev.info["n_wires"] == wp.n_wires
        nzcb.h2d(d_in, b"".join(inputs))
        status = wp.run_dev(d_in, 4, d_wit, stride)
        got = dev.check_dev(d_wit, 4, stride, bad_cap=16)
        raw = nzcb.d2h(d_wit, stride * 3 + 32 * wp.n_wires)
        want = host.check(raw, count=4, bad_cap=16, stride=stride)
    finally:
        nzcb.dev_free(d_in)
        nzcb.dev_free(d_wit)
        wp.close()
        host.close()
        dev.close()
    assert got == want
    assert status[0] == 0 and got[0] == {"n_bad": 0, "first_bad": None, "bad": []}
    assert status[1] == 0 and got[1]["n_bad"] == 0
    assert status[2] != 0 and got[2]["n_bad"] > 0          # rejected by the calculator and by a constraint


# ---------------------------------------------------------------- nzcp_live soundness probe
@pytest.fixture(scope="module")
def live():
    """nzcp_live: the Circuit (for the expected sets), its r1cs and a golden passing witness
    from the GPU witness VM."""
    from nzcb import nzcpgen, nzcplive
    r1cs, prog, c = nzcplive.build()
    if c is None:
        c = nzcpgen.nzcp_pub_identity(**nzcpgen.LIVE)
    with open(os.path.join(GOLD, "nzcp_cases.json")) as f:
        gold = json.load(f)
    case = next(cs for cs, exp in zip(gold["cases"], gold["expected"])
                if cs["params"]["is_live"] and exp["status"] == 0)
    wp = nzcb.WitnessProgram(prog)
    try:
        raw, st = wp.run(NC.case_input_bytes(case), 1)
    finally:
        wp.close()
    assert st == [0] and len(raw) == 32 * c.n_wires
    return c, r1cs, raw


def test_nzcp_live_single_wire_soundness_probe(live):
    """32 copies of a passing nzcp_live witness, each with one wire replaced by value + 1, in
    one check_dev call. Copy j's failing set is computed in Python over the constraints that
    mention its wire."""
    c, r1cs, raw = live
    used = set()
    for cons in c.constraints:
        for part in cons:
            used.update(part)
    wires = random.Random(0x6E7A).sample(sorted(used), 32)
    touching = {w: [] for w in wires}
    for k, cons in enumerate(c.constraints):
        for part in cons:
            for w in part.keys() & touching.keys():
                if not touching[w] or touching[w][-1] != k:
                    touching[w].append(k)
    wit = [int.from_bytes(raw[i:i + 32], "little") for i in range(0, len(raw), 32)]
    n = c.n_wires
    dev = nzcb.R1cs(r1cs, device=0)
    d_wit = nzcb.dev_alloc(33 * 32 * n)
    try:
        assert dev.info["n_constraints"] == len(c.constraints) and dev.info["n_wires"] == n
        nzcb.h2d(d_wit, raw)
        for j in range(1, 33):
            nzcb.d2d(d_wit + j * 32 * n, d_wit, 32 * n)
        for j, w in enumerate(wires):
            nzcb.h2d(d_wit + j * 32 * n + 32 * w, ((wit[w] + 1) % R).to_bytes(32, "little"))
        got = dev.check_dev(d_wit, 33, 32 * n, bad_cap=16)
    finally:
        nzcb.dev_free(d_wit)
        dev.close()
    assert got[32] == {"n_bad": 0, "first_bad": None, "bad": []}          # the unmodified witness
    failing = 0
    for j, w in enumerate(wires):
        old = wit[w]
        wit[w] = (old + 1) % R
        bad = C.violated(c, wit, touching[w])
        wit[w] = old
        failing += bool(bad)
        assert got[j] == {"n_bad": len(bad), "first_bad": bad[0] if bad else None, "bad": bad[:16]}, (j, w)
    assert failing                                                         # the probe is not vacuous


# ---------------------------------------------------------------- concurrency
def test_check_while_a_context_proves():
    import threading
    case, _ = C.long_rows_case(64)
    name, data, wits = case
    host = nzcb.R1cs(data, device=HOST)
    want = C.check_all(host, case)
    host.close()
    ctx, wtns = nzcb.synth_context(12)
    bl = bytes(range(1, 33)) * 11
    dev = nzcb.R1cs(data, device=0)
    made, errors = [], []

    def prove():
        try:
            for _ in range(6):
                made.append(ctx.prove_raw(wtns, bl))
        except Exception as e:  # noqa: BLE001 (reported by the assertion below)
            errors.append(e)

    try:
        first = ctx.prove_raw(wtns, bl)
        t = threading.Thread(target=prove)
        t.start()
        try:
            got = [C.check_all(dev, case) for _ in range(6)]
        finally:
            t.join()
        vk = ctx.vk
    finally:
        dev.close()
        ctx.close()
    assert errors == [] and made == [first] * 6
    assert nzcb.verify(vk, *first)
    assert got == [want] * 6


# ---------------------------------------------------------------- Node
@pytest.mark.skipif(shutil.which("node") is None or not os.path.exists(os.path.join(JS, "build", "nzcb.node")),
                    reason="node or the built addon is unavailable")
def test_node_wtns_check_and_r1cs_info(tmp_path):
    name, data, wits = C.random_cases()[1]
    (tmp_path / "c.r1cs").write_bytes(data)
    (tmp_path / "good.wtns").write_bytes(C.wtns_file(wits[0]))
    mutated = next(w for w in wits[1:] if C.expected(data, w)["n_bad"])
    (tmp_path / "bad.wtns").write_bytes(C.wtns_file(mutated))
    script = f"""
const m = require('./');
(async () => {{
  const lines = [];
  const logger = {{ info: (s) => lines.push(s), warn: (s) => lines.push(s), debug: () => {{}} }};
  const good = await m.wtns.check({json.dumps(str(tmp_path / "c.r1cs"))}, {json.dumps(str(tmp_path / "good.wtns"))}, logger);
  const bad = await m.wtns.check({json.dumps(str(tmp_path / "c.r1cs"))}, {json.dumps(str(tmp_path / "bad.wtns"))}, logger,
                                 {{device: 0}});
  const host = await m.wtns.check({json.dumps(str(tmp_path / "c.r1cs"))}, {json.dumps(str(tmp_path / "bad.wtns"))}, null,
                                  {{device: -1}});
  const info = await m.r1cs.info({json.dumps(str(tmp_path / "c.r1cs"))});
  console.log(JSON.stringify({{good, bad, host, info, lines}}));
}})().catch((err) => {{ console.error(err); process.exit(1); }});
"""
    p = subprocess.run(["node", "-e", script], capture_output=True, text=True, timeout=120, cwd=JS)
    assert p.returncode == 0, p.stderr
    out = json.loads(p.stdout)
    want = C.expected(data, mutated)
    assert out["good"] is True and out["bad"] is False and out["host"] is False
    assert out["lines"][:2] == ["WITNESS IS CORRECT", "WITNESS CHECKING FAILED"]
    assert out["lines"][2:2 + len(want["bad"])] == [f"constraint {k} is not satisfied" for k in want["bad"]]
    host = nzcb.R1cs(data, device=HOST)
    info = host.info
    host.close()
    assert out["info"] == {"nVars": info["n_wires"], "nOutputs": info["n_outputs"], "nPubInputs": info["n_pub_inputs"],
                           "nPrvInputs": info["n_prv_inputs"], "nConstraints": info["n_constraints"]}
    assert (info["n_outputs"], info["n_pub_inputs"], info["n_prv_inputs"]) == (2, 1, 3)
    cli = os.path.join(JS, "cli.js")
    for wtns, code, first in (("good.wtns", 0, "WITNESS IS CORRECT"), ("bad.wtns", 1, "WITNESS CHECKING FAILED")):
        p = subprocess.run(["node", cli, "wtns", "check", str(tmp_path / "c.r1cs"), str(tmp_path / wtns)],
                           capture_output=True, text=True, timeout=120)
        assert p.returncode == code and p.stdout.splitlines()[0] == first, (p.stdout, p.stderr)
    p = subprocess.run(["node", cli, "r1cs", "info", str(tmp_path / "c.r1cs")], capture_output=True, text=True,
                       timeout=120)
    assert p.returncode == 0 and f"# of Constraints: {info['n_constraints']}" in p.stdout.splitlines()
