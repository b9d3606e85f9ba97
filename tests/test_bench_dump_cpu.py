"""bench.py --dump-outputs, host side (no GPU): what it writes, and that a sample of an output
above the size limit is the same skeletons in every run."""
import importlib.util
import os

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def load_bench():
    spec = importlib.util.spec_from_file_location("bench_mod", os.path.join(ROOT, "bench.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_dump_outputs_writes_the_poses_as_float32(tmp_path):
    b = load_bench()
    pose = np.random.default_rng(1).standard_normal((7, 3, 10)).astype(np.float32)
    d = tmp_path / "a" / "b"                       # created on demand
    info = b.dump_outputs(str(d), pose, 0, 1)
    got = np.load(d / "pose_out.npy")
    assert got.dtype == np.float32 and np.array_equal(got.view(np.uint32), pose.view(np.uint32))
    assert info["file"] == "pose_out.npy" and info["shape"] == [7, 3, 10] and not info["sampled"]
    assert b.dump_outputs(str(d), pose, 1, 2)["file"] == "pose_out_rank1.npy"


def test_dump_outputs_samples_above_the_limit(tmp_path, monkeypatch):
    b = load_bench()
    monkeypatch.setattr(b, "DUMP_LIMIT_BYTES", 4096 + 40 * 120)   # room for 40 skeletons of 120 bytes
    pose = np.arange(100 * 3 * 10, dtype=np.float32).reshape(100, 3, 10)
    a = b.dump_outputs(str(tmp_path / "x"), pose, 0, 1)
    c = b.dump_outputs(str(tmp_path / "y"), pose, 0, 1)
    x, y = np.load(tmp_path / "x" / "pose_out.npy"), np.load(tmp_path / "y" / "pose_out.npy")
    assert a["sampled"] and a["shape"] == [40, 3, 10] and a == dict(c, dir=a["dir"])
    assert np.array_equal(x, y)
    first = x[:, 0, 0] / 30                                       # the skeleton each row came from
    assert np.all(np.diff(first) > 0) and np.array_equal(x, pose[first.astype(int)])
    assert os.path.getsize(tmp_path / "x" / "pose_out.npy") <= b.DUMP_LIMIT_BYTES
