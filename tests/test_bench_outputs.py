"""CPU tests of bench.py's command line and of what --dump-outputs writes (no GPU: the helper is fed record arrays as the
decode path returns them)."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def _records(n, seed):
    import rtlsdr_ft8d_amd as ft8
    rng = np.random.default_rng(seed)
    raw = rng.integers(0, 256, (n, ft8.MAX_MESSAGES * ft8.RESULT_DTYPE.itemsize), dtype=np.uint8)
    return raw, rng.integers(0, 51, n).astype(np.int32)


def test_a_plain_run_is_the_default_and_the_extras_need_full():
    import bench
    a = bench.parse_args(["--gpus", "1", "--steps", "7", "--warmup", "2"])
    assert a.steps == 7 and a.warmup == 2 and a.full is False and a.dump_outputs is None
    b = bench.parse_args(["--gpus", "1", "--steps", "7", "--warmup", "2", "--full", "--dump-outputs", "out"])
    assert b.full is True and b.dump_outputs == "out"


def test_dump_outputs_writes_every_record_byte_as_float(tmp_path):
    import bench
    import rtlsdr_ft8d_amd as ft8
    raw, counts = _records(300, 1)
    info = bench.dump_outputs(str(tmp_path), raw, counts)
    assert info["frames"] == info["of_frames"] == 300
    assert info["files"] == ["frame_index.npy", "freq.npy", "n_results.npy", "records.npy", "snr.npy"]
    got = {f[:-len(".npy")]: np.load(tmp_path / f) for f in info["files"]}
    assert all(a.dtype in (np.float32, np.float64) for a in got.values())
    assert np.array_equal(got["records"].astype(np.uint8).reshape(300, -1), raw)
    slots = raw.view(ft8.RESULT_DTYPE).reshape(300, ft8.MAX_MESSAGES)
    assert np.array_equal(got["freq"], slots["freq"]) and np.array_equal(got["snr"], slots["snr"])
    assert np.array_equal(got["n_results"], counts) and np.array_equal(got["frame_index"], np.arange(300))
    assert info["bytes"] == sum(a.nbytes for a in got.values())


def test_dump_outputs_samples_large_outputs_the_same_way_every_time(tmp_path):
    import bench
    n = bench.DUMP_MAX_FRAMES + 1000
    raw, counts = _records(n, 2)
    a = bench.dump_outputs(str(tmp_path / "a"), raw, counts)
    b = bench.dump_outputs(str(tmp_path / "b"), raw, counts)
    assert a["frames"] == bench.DUMP_MAX_FRAMES and a["of_frames"] == n
    assert a["bytes"] <= 64 * 10 ** 6
    idx = np.load(tmp_path / "a" / "frame_index.npy")
    assert np.all(np.diff(idx) > 0) and np.array_equal(idx, np.load(tmp_path / "b" / "frame_index.npy"))
    rows = idx.astype(np.int64)
    assert np.array_equal(np.load(tmp_path / "a" / "records.npy").astype(np.uint8).reshape(len(rows), -1), raw[rows])
    assert np.array_equal(np.load(tmp_path / "a" / "n_results.npy"), counts[rows])
