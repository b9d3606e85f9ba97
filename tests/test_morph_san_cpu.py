"""tools/san/morph_san: morph.h's shape validation, packing and host path under ASan + UBSan (a
stand-alone program with its own main; nothing is loaded into python)."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_morph_san_runs_clean():
    exe = os.path.join(ROOT, "build", "san", "morph_san")
    subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "tools", "san"), exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "one_vertex_one_shape: ok B=3 V=1 K=4 P=1" in r.stdout and "one_vertex_one_shape_normals: ok B=3 V=1 K=8 P=1" in r.stdout
    assert "last_plane_odd: ok B=37 V=65 K=8 P=17" in r.stdout and "last_plane_even: ok" in r.stdout
    assert "lds_limit: ok B=3413 V=130 K=4 P=4" in r.stdout
    assert "five_shapes_at_max_bones: refused" in r.stdout and "four_shapes_at_max_bones: accepted" in r.stdout
    assert "normals_on_mesh_only: refused" in r.stdout and "null_positions: refused" in r.stdout
    assert "UNEXPECTED" not in r.stdout
    assert "ERROR" not in r.stderr and "runtime error" not in r.stderr
