"""bench.py --dump-outputs (host side): the timed proofs and public signals as float32 .npy,
one row per proof and one value per byte, and the seeded row sample of an oversized batch."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402


def _proofs(count):
    return [(bytes((i + k) % 256 for k in range(800)), bytes((3 * i + k) % 256 for k in range(96)))
            for i in range(count)]


def test_dump_outputs_bytes_exact(tmp_path):
    proofs = _proofs(7)
    bench.dump_outputs(str(tmp_path / "out"), proofs, 0)
    bench.dump_outputs(str(tmp_path / "out"), proofs[:2], 3)
    assert sorted(os.listdir(tmp_path / "out")) == ["proofs.npy", "proofs.rank3.npy", "public_signals.npy",
                                                    "public_signals.rank3.npy"]
    for k, (name, width) in enumerate((("proofs", 800), ("public_signals", 96))):
        a = np.load(tmp_path / "out" / f"{name}.npy")
        assert a.dtype == np.float32 and a.shape == (7, width)
        assert [bytes(row.astype(np.uint8)) for row in a] == [p[k] for p in proofs]
        assert np.load(tmp_path / "out" / f"{name}.rank3.npy").shape == (2, width)


def test_dump_outputs_sample_is_seeded_and_bounded(tmp_path, monkeypatch):
    proofs = _proofs(50)
    monkeypatch.setattr(bench, "DUMP_MAX_BYTES", 10 * 4 * 896 + 5)   # room for 10 rows
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), proofs, 0)
    a, b = (np.load(tmp_path / d / "proofs.npy") for d in ("a", "b"))
    assert a.shape == (10, 800) and np.array_equal(a, b)
    rows = [bytes(r.astype(np.uint8)) for r in a]
    picked = [[p for p, _ in proofs].index(r) for r in rows]
    assert picked == sorted(set(picked))                              # distinct rows of the batch, in order
    total = sum(os.path.getsize(tmp_path / "a" / f) for f in os.listdir(tmp_path / "a"))
    assert total <= bench.DUMP_MAX_BYTES + 2 * 128                    # the .npy headers


def test_dump_outputs_empty_rank(tmp_path):
    bench.dump_outputs(str(tmp_path / "e"), [], 1)
    assert os.listdir(tmp_path / "e") == []
