"""Times mbik_clip_sample against what it replaces and what surrounds it, on the GPU, with device
events.

    python tools/clip_bench.py [--configs 2,5] [--steps 20] [--warmup 3] [--out profiles/clip_bench.json]
    python tools/clip_bench.py --configs 5 --only sample --steps 5   (a bare loop of the call, for a counter run)

Per config (C2: 4,096 x 32 bones; C5: 16,384 x 200 bones) the candidates alternate inside one
process after a warm-up:

  sample  mbik_clip_sample of a set of 3 clips with 60 keys on every channel of every bone, each
          skeleton at its own random time (one loop before to two loops after the clip) in its own
          random clip: count x 12 B in, count x bones x 40 B out
  fill    a device fill of the same count x bones x 40 B (the least a producer of pose_in can cost)
  upload  hipMemcpyAsync of those bytes from pageable host memory (torch's copy_ of an unpinned CPU
          tensor), which is what the call replaces in a frame
  solve   one mbik_solve step with the autotuned layout

Needs a GPU: there is no CPU fallback.
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
CLIPS, KEYS = 3, 60


def measure(cfg: int, steps: int, warmup: int, only: str | None) -> dict:
    import numpy as np
    import torch
    from many_bone_ik_amd import animation as A
    from many_bone_ik_amd import workloads as W
    from many_bone_ik_amd.solver import Plan

    dev = torch.device("cuda", 0)
    n = SKELETONS[cfg]
    print(f"clip_bench: C{cfg}: generating {n} skeletons, their plan and the clip set", file=sys.stderr, flush=True)
    wl = W.generate(cfg, n)
    B = wl.bone_count
    rest, clips = A.synthetic_clips(1600 + cfg, B, clip_count=CLIPS, key_counts=(KEYS,))
    cs = A.ClipSet(B, rest, clips)
    rng = np.random.default_rng(cfg)
    ci = rng.integers(0, CLIPS, n).astype(np.int32)
    t = rng.uniform(-1.0, 3.0, n) * np.array([c["length"] for c in clips])[ci]
    d_t, d_c = torch.from_numpy(t).to(dev), torch.from_numpy(ci).to(dev)
    pose_in = torch.from_numpy(wl.pose).to(dev)
    sampled = torch.empty_like(pose_in)
    filled = torch.empty_like(pose_in)
    uploaded = torch.empty_like(pose_in)
    host_pose = torch.from_numpy(wl.pose.copy())   # pageable: not pinned
    assert not host_pose.is_pinned()
    stream = torch.cuda.current_stream(dev).cuda_stream

    def sample():
        cs.sample(d_t.data_ptr(), sampled.data_ptr(), n, clip_index_ptr=d_c.data_ptr(), stream=stream)

    def fill():
        filled.fill_(1.0)

    def upload():
        uploaded.copy_(host_pose, non_blocking=True)

    cands = {"sample": sample, "fill": fill, "upload": upload}
    plan = None
    if only is None:
        targets = torch.from_numpy(wl.targets).to(dev)
        pose_out = torch.empty_like(pose_in)
        plan = Plan.from_workload(wl)
        plan.autotune(pose_in.data_ptr(), targets.data_ptr(), pose_out.data_ptr())   # the solve as bench.py times it

        def solve():
            plan.solve(pose_in.data_ptr(), targets.data_ptr(), pose_out.data_ptr(), stream=stream)

        cands["solve"] = solve
    else:
        cands = {only: cands[only]}
    print(f"clip_bench: C{cfg}: timing", file=sys.stderr, flush=True)
    for _ in range(warmup):
        for f in cands.values():
            f()
    torch.cuda.synchronize(dev)
    ms = {k: [] for k in cands}
    for _ in range(steps):
        for k, f in cands.items():   # alternating: sample, fill, upload, solve, sample, ...
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            f()
            b.record()
            b.synchronize()
            ms[k].append(a.elapsed_time(b))
    med = {k: statistics.median(v) for k, v in ms.items()}
    pose_bytes = n * B * 40
    res = {"config": f"C{cfg}", "skeletons": n, "bones": B, "steps": steps, "warmup": warmup, "clips": CLIPS,
           "keys_per_channel": KEYS, "pose_bytes": pose_bytes, "per_frame_input_bytes": n * 12,
           "clip_set_bytes": CLIPS * B * 3 * (16 + KEYS * 24) + B * 40 + CLIPS * 16}
    for k in cands:
        res[f"{k}_ms"] = med[k]
        res[f"{k}_ms_min_max"] = [min(ms[k]), max(ms[k])]
    if only is None:
        # the sampled poses are finite and every skeleton got its own (a sanity check, not a parity test)
        h = sampled.cpu().numpy()
        assert np.isfinite(h).all() and (h[0] != h[1]).any()
        info = plan.info()
        plan.close()
        res.update({
            "sample_over_fill": med["sample"] / med["fill"], "sample_over_upload": med["sample"] / med["upload"],
            "sample_over_solve": med["sample"] / med["solve"],
            "sample_bytes_per_s": pose_bytes / (med["sample"] * 1e-3), "fill_bytes_per_s": pose_bytes / (med["fill"] * 1e-3),
            "upload_bytes_per_s": pose_bytes / (med["upload"] * 1e-3),
            "solve_layout": f"autotuned: lanes {info['lanes_per_skeleton']}, skeletons/block {info['skeletons_per_block']}, "
                            f"placement {info['state_placement']}, wave roles {info['wave_roles']}",
            "in_infinity_cache": pose_bytes < 256 * 2 ** 20,
        })
    cs.close()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", default="2,5")
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--only", choices=["sample", "fill", "upload"], default=None,
                    help="time one candidate alone and write no file (for a profiler run of its own)")
    ap.add_argument("--out", default=os.path.join(HERE, "profiles", "clip_bench.json"))
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("clip_bench needs a GPU (no CPU fallback)")
    res = {
        "what": "mbik_clip_sample (3 clips x 60 keys on every channel of every bone, per-skeleton random times and clip "
                "indices) vs a device fill of count x bones x 40 B vs hipMemcpyAsync of those bytes from pageable host "
                "memory vs one autotuned mbik_solve step; medians of device-event times, candidates alternating in one process",
        "note": "The upload is the copy a frame makes without the call; the fill is the floor of any producer of pose_in. "
                "Both pose buffers (C2 5.2 MB, C5 131 MB) fit the 256 MiB Infinity Cache, and the clip set "
                "(0.4 MB, 2.6 MB) fits an XCD's 4 MiB L2.",
        "device": torch.cuda.get_device_name(0),
        "results": [measure(int(c), args.steps, args.warmup, args.only) for c in args.configs.split(",")],
    }
    if args.only is None:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            json.dump(res, fh, indent=1)
            fh.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
