"""Times mbik_pose_blend against a device-to-device copy that moves the same bytes and against
one solve step, on the GPU, with device events.

    python tools/blend_bench.py [--configs 2,5] [--steps 20] [--warmup 3] [--out profiles/blend_bench.json]

Per config (C2: 4,096 x 32 bones; C5: 16,384 x 200 bones) the candidates alternate inside one
process after a warm-up: pose_blend of the solve's input and output with a per-skeleton weight
buffer (uniform weights in 0.05..0.95, so every bone is blended -- the whole arithmetic on every
lane), the same call with every weight 1 (every wave takes the early-out: the staging alone),
torch's copy of a count x bones x 60 B buffer (the call reads 80 B and writes 40 B per bone; the
copy reads and writes 60 B, the same 120 B), and plan.solve with the autotuned layout.  The
yardstick is the copy; no threshold is fixed.  C2's 15.7 MB sits inside the 256 MiB Infinity
Cache, so only the C5 size (393 MB) speaks for HBM.  Needs a GPU: there is no CPU fallback.
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
    print(f"blend_bench: C{cfg}: generating {n} skeletons and their plan", file=sys.stderr, flush=True)
    wl = W.generate(cfg, n)
    plan = Plan.from_workload(wl)
    print(f"blend_bench: C{cfg}: timing", file=sys.stderr, flush=True)
    B = wl.bone_count
    pose_in = torch.from_numpy(wl.pose).to(dev)
    targets = torch.from_numpy(wl.targets).to(dev)
    pose_mod = torch.empty_like(pose_in)
    pose_out = torch.empty_like(pose_in)
    weights = torch.empty(n, dtype=torch.float32, device=dev).uniform_(0.05, 0.95)
    ones = torch.ones(n, dtype=torch.float32, device=dev)
    copy_bytes = n * B * 60
    src = torch.empty(copy_bytes // 4, dtype=torch.float32, device=dev).normal_()
    dst = torch.empty_like(src)
    plan.autotune(pose_in.data_ptr(), targets.data_ptr(), pose_mod.data_ptr())   # the solve as bench.py times it
    stream = torch.cuda.current_stream(dev).cuda_stream

    def blend():
        plan.pose_blend(pose_in.data_ptr(), pose_mod.data_ptr(), pose_out.data_ptr(), n, influence_ptr=weights.data_ptr(),
                        stream=stream)

    def blend_off():
        plan.pose_blend(pose_in.data_ptr(), pose_mod.data_ptr(), pose_out.data_ptr(), n, influence_ptr=ones.data_ptr(),
                        stream=stream)

    def copy():
        dst.copy_(src)

    def solve():
        plan.solve(pose_in.data_ptr(), targets.data_ptr(), pose_mod.data_ptr(), stream=stream)

    cands = {"blend": blend, "blend_off": blend_off, "copy": copy, "solve": solve}
    solve()
    for _ in range(warmup):
        for f in cands.values():
            f()
    torch.cuda.synchronize(dev)
    changed = float((pose_mod != pose_in).any(dim=2).float().mean())   # bones the solve moved: the others take the early-out
    ms = {k: [] for k in cands}
    for _ in range(steps):
        for k, f in cands.items():   # alternating: blend, blend_off, copy, solve, blend, ...
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            f()
            b.record()
            b.synchronize()
            ms[k].append(a.elapsed_time(b))
    med = {k: statistics.median(v) for k, v in ms.items()}
    info = plan.info()
    plan.close()
    blend_bytes = n * B * 120 + n * 4
    return {
        "config": f"C{cfg}", "skeletons": n, "bones": B, "steps": steps, "warmup": warmup,
        "blend_ms": med["blend"], "blend_off_ms": med["blend_off"], "copy_ms": med["copy"], "solve_ms": med["solve"],
        "blend_ms_min_max": [min(ms["blend"]), max(ms["blend"])],
        "blend_off_ms_min_max": [min(ms["blend_off"]), max(ms["blend_off"])],
        "copy_ms_min_max": [min(ms["copy"]), max(ms["copy"])],
        "solve_ms_min_max": [min(ms["solve"]), max(ms["solve"])],
        "blend_over_copy": med["blend"] / med["copy"], "blend_off_over_copy": med["blend_off"] / med["copy"],
        "blend_over_solve": med["blend"] / med["solve"],
        "bones_moved_by_the_solve": changed,
        "copy_buffer_bytes": copy_bytes, "blend_bytes": blend_bytes,
        "blend_bytes_per_s": blend_bytes / (med["blend"] * 1e-3),
        "copy_bytes_per_s": 2 * copy_bytes / (med["copy"] * 1e-3),   # the copy reads and writes its buffer
        "solve_layout": f"autotuned: lanes {info['lanes_per_skeleton']}, skeletons/block {info['skeletons_per_block']}, "
                        f"placement {info['state_placement']}, wave roles {info['wave_roles']}",
        "in_infinity_cache": 2 * copy_bytes < 256 * 2 ** 20,
    }


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", default="2,5")
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(HERE, "profiles", "blend_bench.json"))
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("blend_bench needs a GPU (no CPU fallback)")
    res = {
        "what": "mbik_pose_blend (per-skeleton weights in 0.05..0.95; blend_off: every weight 1) vs a device-to-device copy "
                "of count x bones x 60 B vs one autotuned mbik_solve step; medians of device-event times, candidates "
                "alternating in one process",
        "note": "C2's 15.7 MB sits inside the 256 MiB Infinity Cache; only the C5 size (393 MB) speaks for HBM. "
                "blend_bytes_per_s counts the call's own bytes once (two poses in, one out, the weights); "
                "copy_bytes_per_s counts the copy's read and write of its count x bones x 60 B buffer.",
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
