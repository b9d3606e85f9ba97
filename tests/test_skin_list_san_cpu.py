"""tools/san/skin_list_san: skin_list.h's host path (mbik_skin_vertices_listed_cpu's core) under ASan + UBSan
(a stand-alone program with its own main; nothing is loaded into python)."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_skin_list_san_runs_clean():
    exe = os.path.join(ROOT, "build", "san", "skin_list_san")
    subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "tools", "san"), exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "empty_list: ok B=5 V=40 K=4 P=0 skeletons=6 max_list=0 list_count=0 n=0 rows_written=0" in r.stdout
    assert "count_zero: ok" in r.stdout and "count_negative: ok B=4 V=17 K=4 P=5 skeletons=6 max_list=2 list_count=-7 n=0 rows_written=0" in r.stdout
    assert "all: ok B=5 V=40 K=4 P=0 skeletons=6 max_list=6 list_count=6 n=6 rows_written=24" in r.stdout
    assert "all_shaped: ok B=9 V=33 K=8 P=3 skeletons=6 max_list=6 list_count=6 n=6 rows_written=48" in r.stdout
    assert "descending: ok" in r.stdout and "out_of_range: ok B=5 V=40 K=4 P=0 skeletons=6 max_list=5 list_count=5 n=5 rows_written=12" in r.stdout
    assert "out_of_range_shaped: ok" in r.stdout and "only_out_of_range: ok" in r.stdout and "rows_written=0\n" in r.stdout
    assert "duplicates: ok" in r.stdout and "duplicates_shaped: ok" in r.stdout
    assert "count_above_buffer: ok B=4 V=17 K=4 P=5 skeletons=6 max_list=2 list_count=1000 n=2 " in r.stdout
    assert "stale_tail: ok B=5 V=40 K=4 P=0 skeletons=6 max_list=5 list_count=2 n=2 rows_written=8" in r.stdout
    assert "list_longer_than_batch: ok" in r.stdout
    assert "ERROR" not in r.stderr and "runtime error" not in r.stderr
