"""tools/san/lod_san: lod.h's host path (mbik_cull_lod_cpu's core) under ASan + UBSan (a stand-alone
program with its own main; nothing is loaded into python)."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_lod_san_runs_clean():
    exe = os.path.join(ROOT, "build", "san", "lod_san")
    subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "tools", "san"), exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "no_skeletons: ok skeletons=0 ranges=3 flags=0 planes=6 listed=0" in r.stdout
    assert "one_skeleton: ok skeletons=1 ranges=1 " in r.stdout and "wave_and_one: ok skeletons=65 ranges=3 flags=1 " in r.stdout
    assert "no_level: ok skeletons=257 " in r.stdout and "most_planes: ok skeletons=300 ranges=2 flags=1 planes=16 " in r.stdout
    for n in range(1, 9):
        assert f"ranges_{n}: ok skeletons=1000 ranges={n} flags={n & 1} " in r.stdout
    assert "ERROR" not in r.stderr and "runtime error" not in r.stderr
