"""tools/san/clip_shapes_san: clip_shapes.h's host paths (mbik_clip_sample_shapes_cpu's and
mbik_clip_sample_shapes_layers_cpu's cores) under ASan + UBSan on exact-size heap tables (a
stand-alone program with its own main; nothing is loaded into python)."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_clip_shapes_san_runs_clean():
    exe = os.path.join(ROOT, "build", "san", "clip_shapes_san")
    subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "tools", "san"), exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    out = r.stdout
    assert "plain_untracked: ok P=4 clips=2 count=68 K=0 floats=272 nan=0 init=272" in out
    assert "plain_single_keys: ok P=4 clips=2 count=68 K=0 floats=272 nan=24 init=0" in out   # 6 non-finite times x 4 shapes
    assert "plain_times_on_keys: ok" in out and "plain_wrap_branches: ok" in out
    assert "plain_invalid: ok P=7 clips=3 count=34 K=0 floats=238 nan=238 init=0" in out
    for mode in ("plain", "normalize"):
        assert f"layers_untracked_{mode}: ok P=4 clips=2 count=68 K=2 floats=272 nan=0 init=272" in out
        assert f"layers_single_keys_{mode}: ok" in out and f"layers_times_on_keys_{mode}: ok" in out
        assert f"layers_wrap_branches_{mode}: ok" in out
        assert f"off_layers_{mode}: ok P=7 clips=3 count=31 K=3 floats=217 nan=0 init=217" in out
        assert f"invalid_layers_{mode}: ok P=7 clips=3 count=31 K=3 floats=217 nan=217 init=0" in out
        assert f"zero_totals_{mode}: ok P=7 clips=3 count=31 K=4 floats=217 nan=0 init=217" in out
        assert f"nan_weights_{mode}: ok P=7 clips=3 count=31 K=2 " in out
        assert f"k1_{mode}: ok P=7 clips=3 count=31 K=1 floats=217 nan=0 " in out
        assert f"k8_{mode}: ok P=7 clips=3 count=31 K=8 floats=217 nan=0 " in out
    assert "FAILED" not in out and len(out.splitlines()) == 25
    assert "ERROR" not in r.stderr and "runtime error" not in r.stderr
