"""tools/san/skin_san: skin.h's mesh validation, packing and host skinning path under ASan + UBSan
(a stand-alone program with its own main; nothing is loaded into python)."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_skin_san_runs_clean():
    exe = os.path.join(ROOT, "build", "san", "skin_san")
    subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "tools", "san"), exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "one_vertex_k4: ok B=3 V=1 K=4" in r.stdout and "one_vertex_k8: ok B=3 V=1 K=8" in r.stdout
    assert "max_bones: ok B=3413" in r.stdout and "last_bone_k8: ok" in r.stdout
    assert "index_is_bone_count: refused" in r.stdout and "index_negative: refused" in r.stdout
    assert "UNEXPECTED" not in r.stdout
    assert "ERROR" not in r.stderr and "runtime error" not in r.stderr
