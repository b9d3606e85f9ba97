"""tools/san/clip_san: clip.h's and clip_layers.h's host paths (mbik_clip_sample_cpu's and
mbik_clip_sample_layers_cpu's cores) under ASan + UBSan (a stand-alone program with its own main;
nothing is loaded into python)."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_clip_san_runs_clean():
    exe = os.path.join(ROOT, "build", "san", "clip_san")
    subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "tools", "san"), exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    out = r.stdout
    assert "plain_empty_tracks: ok B=4 clips=2 count=68 K=0 floats=2720 nan=0 rest=2720" in out
    assert "plain_single_keys: ok" in out and "plain_times_on_keys: ok" in out and "plain_wrap_branches: ok" in out
    for mode in ("plain", "normalize"):
        assert f"layers_empty_tracks_{mode}: ok B=4 clips=2 count=68 K=2 floats=2720 nan=0 rest=2720" in out
        assert f"layers_single_keys_{mode}: ok" in out and f"layers_times_on_keys_{mode}: ok" in out
        assert f"layers_wrap_branches_{mode}: ok" in out
        assert f"off_layers_{mode}: ok B=5 clips=3 count=31 K=3 floats=1550 nan=0 rest=1550" in out
        assert f"invalid_layers_{mode}: ok B=5 clips=3 count=31 K=3 floats=1550 nan=1550 rest=0" in out
        assert f"zero_totals_{mode}: ok B=5 clips=3 count=31 K=4 floats=1550 nan=0 rest=1550" in out
        assert f"nan_weights_{mode}: ok B=5 clips=3 count=31 K=2 " in out
        assert f"k1_{mode}: ok B=5 clips=3 count=31 K=1 floats=1550 nan=0 " in out
        assert f"k8_{mode}: ok B=5 clips=3 count=31 K=8 floats=1550 nan=0 " in out
    assert "FAILED" not in out and len(out.splitlines()) == 24
    assert "ERROR" not in r.stderr and "runtime error" not in r.stderr
