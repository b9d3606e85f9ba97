"""tools/san/skin_tangent_san: the tangent stream's validation, layout, packing and host paths (mbik_skin_vertices_call_cpu's
core) under ASan + UBSan (a stand-alone program with its own main; nothing is loaded into python)."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_skin_tangent_san_runs_clean():
    exe = os.path.join(ROOT, "build", "san", "skin_tangent_san")
    subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "tools", "san"), exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "plain: layout ok V=41 K=4 P=0" in r.stdout and "relative: layout ok V=33 K=8 P=3" in r.stdout
    assert "normalized: layout ok" in r.stdout and "one_vertex: layout ok V=1 K=8 P=1" in r.stdout
    assert "range: ok B=5 V=41 K=4 P=0 skeletons=6 max_list=0 list_count=0 rows_written=6" in r.stdout
    assert "range_relative: ok B=9 V=33 K=8 P=3 skeletons=6 max_list=0 list_count=0 rows_written=12" in r.stdout
    assert "range_normalized: ok" in r.stdout and "range_one_vertex: ok" in r.stdout
    assert "count_zero: ok B=9 V=33 K=8 P=3 skeletons=6 max_list=3 list_count=0 rows_written=0" in r.stdout
    assert "all: ok B=5 V=41 K=4 P=0 skeletons=6 max_list=6 list_count=6 rows_written=12" in r.stdout
    assert "out_of_range: ok B=4 V=17 K=4 P=5 skeletons=6 max_list=5 list_count=5 rows_written=12" in r.stdout
    assert "duplicates: ok" in r.stdout and "count_above_buffer: ok" in r.stdout and "list_longer_than_batch: ok" in r.stdout
    assert "ERROR" not in r.stderr and "runtime error" not in r.stderr
