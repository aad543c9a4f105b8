"""bench.py --dump-outputs: the match records of one frame as float arrays, and the seeded sample above the size limit.
CPU only (the records are made up here; the GPU path is covered by the bench run of test_gpu_parity.py)."""
import numpy as np

import bench
from openfdcm_amd import _capi


def _records(n):
    r = np.zeros(n, dtype=_capi.MATCH_DTYPE)
    r["tmpl_idx"] = np.arange(n) * 7 % 1001
    r["score"] = np.linspace(0.0, 3.0, n, dtype=np.float32)
    r["transform"] = np.arange(6 * n, dtype=np.float32).reshape(n, 6) / np.float32(3.0)
    return r


def test_dump_writes_every_field_as_float(tmp_path):
    r = _records(500)
    doc = bench.dump_outputs(str(tmp_path), r)
    assert doc["files"] == ["score.npy", "tmpl_idx.npy", "transform.npy"] and not doc["sampled"] and doc["rows_written"] == 500
    idx, score, tr = (np.load(str(tmp_path / f"{k}.npy")) for k in ("tmpl_idx", "score", "transform"))
    assert idx.dtype == np.float64 and np.array_equal(idx, r["tmpl_idx"].astype(np.float64))
    assert score.dtype == np.float32 and score.tobytes() == r["score"].tobytes()
    assert tr.dtype == np.float32 and tr.shape == (500, 6) and tr.tobytes() == r["transform"].tobytes()


def test_dump_above_the_limit_is_a_fixed_sample(tmp_path, monkeypatch):
    r = _records(2000)
    monkeypatch.setattr(bench, "DUMP_LIMIT_BYTES", 20000)
    a, b = tmp_path / "a", tmp_path / "b"
    doc = bench.dump_outputs(str(a), r)
    bench.dump_outputs(str(b), r)
    assert doc["sampled"] and "row.npy" in doc["files"]
    assert sum((a / f).stat().st_size - 128 for f in doc["files"]) <= 20000  # (minus the .npy headers)
    row = np.load(str(a / "row.npy"))
    assert row.dtype == np.float64 and len(row) == doc["rows_written"] and np.all(np.diff(row) > 0)
    assert np.array_equal(np.load(str(a / "score.npy")), r["score"][row.astype(np.int64)])
    for f in doc["files"]:
        assert (a / f).read_bytes() == (b / f).read_bytes()
