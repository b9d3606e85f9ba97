"""tools/san/bounds_san: bounds.h's bone-box builder, used-bone table packing and the three host paths
under ASan + UBSan (a stand-alone program with its own main; nothing is loaded into python)."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_bounds_san_runs_clean():
    exe = os.path.join(ROOT, "build", "san", "bounds_san")
    subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "tools", "san"), exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "one_vertex: ok B=3 V=1 K=4 used=" in r.stdout and "every_bone: ok B=32 V=400 K=8 used=32 " in r.stdout
    assert "every_third_bone: ok B=200 V=300 K=4 used=67 " in r.stdout
    assert "no_bone_used: ok B=7 V=20 K=4 used=0 " in r.stdout and "no_vertices: ok B=5 V=0 K=8 used=0 " in r.stdout
    assert "no_skeletons: ok" in r.stdout and "no_bones: ok B=0" in r.stdout
    assert "max_bones: ok B=3413 V=5000 K=4 used=" in r.stdout and "planes=16" in r.stdout
    assert "ERROR" not in r.stderr and "runtime error" not in r.stderr
