"""tools/san/root_motion_san: root_motion.h's host paths (mbik_clip_root_motion[_layers]_cpu's and
mbik_root_motion_apply_cpu's cores) under ASan + UBSan on exact-size heap tables (a stand-alone
program with its own main; nothing is loaded into python)."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_root_motion_san_runs_clean():
    exe = os.path.join(ROOT, "build", "san", "root_motion_san")
    subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "tools", "san"), exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    out = r.stdout
    for case in ("untracked_root", "single_keys"):     # nothing changes over a frame: every record is the start values
        assert f"plain_{case}: ok B=3 clips=2 count=392 K=0 floats=3920 nan=0 start=3920 fixed=392" in out
    for case in ("times_on_keys", "seam_branches"):
        assert f"plain_{case}: ok B=3 clips=2 count=392 K=0 floats=3920 nan=0 " in out
    for mode in ("plain", "normalize"):
        for K in (1, 8):
            for case in ("untracked_root", "single_keys"):
                assert f"layers_{case}_k{K}_{mode}: ok B=3 clips=2 count=392 K={K} floats=3920 nan=0 start=3920 fixed=392" in out
            for case in ("times_on_keys", "seam_branches"):
                assert f"layers_{case}_k{K}_{mode}: ok B=3 clips=2 count=392 K={K} floats=3920 nan=0 " in out
        assert f"off_layers_{mode}: ok B=3 clips=3 count=196 K=3 floats=1960 nan=0 start=1960 fixed=196" in out
        assert f"invalid_layers_{mode}: ok B=3 clips=3 count=196 K=3 floats=1960 nan=1960 start=0 fixed=0" in out
        assert f"nonfinite_times_{mode}: ok B=3 clips=3 count=196 K=2 floats=1960 nan=1960 start=0 fixed=196" in out
    assert "plain_invalid: ok B=3 clips=3 count=196 K=0 floats=1960 nan=1960 start=0 fixed=0" in out
    assert "apply_plain: ok count=64 " in out and "apply_orthonormalize: ok count=64 " in out
    assert "FAILED" not in out and len(out.splitlines()) == 29
    assert "ERROR" not in r.stderr and "runtime error" not in r.stderr
