"""Times mbik_pose_globals against a device-to-device copy of the same byte count and against
one solve step, on the GPU, with device events.

    python tools/fk_bench.py [--configs 2,5] [--steps 20] [--warmup 3] [--out profiles/fk_bench.json]

Per config (C2: 4,096 x 32 bones; C5: 16,384 x 200 bones) the three candidates alternate inside
one process after a warm-up: pose_globals with globals and pin distances, torch's copy of a
count x bones x 88 B buffer (88 B per bone is what the call itself moves, 40 B of pose in and
48 B of globals out; the copy reads and writes that many, twice the traffic), and plan.solve.
The yardstick is the copy; no threshold is fixed.  C2's 11.5 MB sits inside the 256 MiB Infinity
Cache, so only the C5 size (288 MB) speaks for HBM.  Needs a GPU: there is no CPU fallback.
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if HERE not in sys.path:
    sys.path.insert(0, HERE)

SKELETONS = {2: 4096, 3: 65536, 4: 32768, 5: 16384}


def measure(cfg: int, steps: int, warmup: int) -> dict:
    import torch
    from many_bone_ik_amd import workloads as W
    from many_bone_ik_amd.solver import Plan

    dev = torch.device("cuda", 0)
    n = SKELETONS[cfg]
    print(f"fk_bench: C{cfg}: generating {n} skeletons and their plan", file=sys.stderr, flush=True)
    wl = W.generate(cfg, n)
    plan = Plan.from_workload(wl)
    print(f"fk_bench: C{cfg}: timing", file=sys.stderr, flush=True)
    B, P = wl.bone_count, int(wl.topo.pins.shape[0])
    pose_in = torch.from_numpy(wl.pose).to(dev)
    targets = torch.from_numpy(wl.targets).to(dev)
    pose_out = torch.empty_like(pose_in)
    glob = torch.empty((n, B, 12), dtype=torch.float32, device=dev)
    dist = torch.empty((n, P), dtype=torch.float32, device=dev)
    copy_bytes = n * B * 88
    src = torch.empty(copy_bytes // 4, dtype=torch.float32, device=dev).normal_()
    dst = torch.empty_like(src)
    plan.autotune(pose_in.data_ptr(), targets.data_ptr(), pose_out.data_ptr())   # the solve as bench.py times it
    stream = torch.cuda.current_stream(dev).cuda_stream

    def fk():
        plan.pose_globals(pose_out.data_ptr(), glob.data_ptr(), n, targets_ptr=targets.data_ptr(),
                          pin_distance_ptr=dist.data_ptr(), stream=stream)

    def copy():
        dst.copy_(src)

    def solve():
        plan.solve(pose_in.data_ptr(), targets.data_ptr(), pose_out.data_ptr(), stream=stream)

    cands = {"fk": fk, "copy": copy, "solve": solve}
    solve()
    for _ in range(warmup):
        for f in cands.values():
            f()
    torch.cuda.synchronize(dev)
    ms = {k: [] for k in cands}
    for _ in range(steps):
        for k, f in cands.items():   # alternating: fk, copy, solve, fk, ...
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            f()
            b.record()
            b.synchronize()
            ms[k].append(a.elapsed_time(b))
    med = {k: statistics.median(v) for k, v in ms.items()}
    info = plan.info()
    fk_bytes = n * B * 88 + n * P * (12 + 4)   # pose in, globals out; target origins' rows in, distances out
    plan.close()
    return {
        "config": f"C{cfg}", "skeletons": n, "bones": B, "pins": P, "steps": steps, "warmup": warmup,
        "fk_ms": med["fk"], "copy_ms": med["copy"], "solve_ms": med["solve"],
        "fk_ms_min_max": [min(ms["fk"]), max(ms["fk"])], "copy_ms_min_max": [min(ms["copy"]), max(ms["copy"])],
        "fk_over_copy": med["fk"] / med["copy"], "fk_over_solve": med["fk"] / med["solve"],
        "copy_buffer_bytes": copy_bytes, "fk_bytes": fk_bytes,
        "fk_bytes_per_s": fk_bytes / (med["fk"] * 1e-3),
        "copy_bytes_per_s": 2 * copy_bytes / (med["copy"] * 1e-3),   # the copy reads and writes its buffer
        "solve_layout": f"autotuned: lanes {info['lanes_per_skeleton']}, skeletons/block {info['skeletons_per_block']}, "
                        f"placement {info['state_placement']}, wave roles {info['wave_roles']}",
        "in_infinity_cache": copy_bytes < 256 * 2 ** 20,
    }


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", default="2,5")
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(HERE, "profiles", "fk_bench.json"))
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("fk_bench needs a GPU (no CPU fallback)")
    res = {
        "what": "mbik_pose_globals (globals + pin distances) vs a device-to-device copy of count x bones x 88 B vs one "
                "mbik_solve step; medians of device-event times, candidates alternating in one process",
        "note": "C2's 11.5 MB sits inside the 256 MiB Infinity Cache; only the C5 size (288 MB) speaks for HBM. "
                "fk_bytes_per_s counts the call's own bytes once (pose in + globals out + targets in + distances out); "
                "copy_bytes_per_s counts the copy's read and write of its count x bones x 88 B buffer.",
        "device": torch.cuda.get_device_name(0),
        "results": [measure(int(c), args.steps, args.warmup) for c in args.configs.split(",")],
    }
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(res, fh, indent=1)
        fh.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
