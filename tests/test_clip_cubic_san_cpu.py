"""tools/san/clip_cubic_san: the samplers' CUBIC forms -- the host paths behind mbik_clip_call_cpu,
all six kinds -- under ASan + UBSan on exact-size heap tables, at 1, 2, 3 and 4 keys a track (a
stand-alone program with its own main; nothing is loaded into python)."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_clip_cubic_san_runs_clean():
    exe = os.path.join(ROOT, "build", "san", "clip_cubic_san")
    subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "tools", "san"), exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    out = r.stdout
    for n in (1, 2, 3, 4):
        for wrap in ("wrap", "clamp"):
            for where in ("inside", "ends"):
                assert f"cubic_n{n}_{wrap}_{where}: ok n={n} " in out
    assert "FAILED" not in out and len(out.splitlines()) == 16
    assert "ERROR" not in r.stderr and "runtime error" not in r.stderr
