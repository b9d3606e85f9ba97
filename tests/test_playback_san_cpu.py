"""tools/san/playback_san: playback.h's host path (mbik_playback_advance_cpu's core) under ASan +
UBSan on exact-size heap arrays (a stand-alone program with its own main; nothing is loaded into
python)."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = ("no_cmds", "first", "last", "stop_last", "past_the_crowd", "before_the_crowd", "bad_clip", "bad_clip_low", "bad_speed", "overflow",
         "unsorted")
CMDS = {"no_cmds": 0, "overflow": 12, "unsorted": 4}


def test_playback_san_runs_clean():
    exe = os.path.join(ROOT, "build", "san", "playback_san")
    subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "tools", "san"), exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    out = r.stdout
    lines = {line.split(":")[0]: line for line in out.splitlines()}
    for K in (1, 8):
        for fill in ("empty", "full"):
            for case in CASES:
                for desc in ("plain", "desc"):
                    line = lines[f"{case}_{fill}_k{K}_{desc}"]
                    assert f": ok K={K} count=70 cmds={CMDS.get(case, 1)} " in line, line
                    fades = int(line.rsplit("fades=", 1)[1])
                    assert fades == 0 if K == 1 else (fades > 0 or not (fill == "full" or desc == "desc" or case in ("first", "overflow", "unsorted"))), line
    events = lambda name: int(lines[name].split("events=")[1].split()[0])
    assert events("bad_clip_full_k8_plain") & 16 and events("bad_clip_low_empty_k1_desc") & 16 and events("bad_speed_full_k8_desc") & 16
    assert events("overflow_full_k8_desc") & 32 and events("first_empty_k1_plain") & 32 and not events("no_cmds_full_k8_desc") & 48
    assert events("no_cmds_empty_k1_desc") & 8 and not events("no_cmds_empty_k1_plain") & 8
    assert "FAILED" not in out and len(out.splitlines()) == 88
    assert "ERROR" not in r.stderr and "runtime error" not in r.stderr
