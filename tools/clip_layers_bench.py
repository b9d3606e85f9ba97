"""Times mbik_clip_sample_layers against the three calls it replaces, on the GPU, with device events
(§16's protocol).

    python tools/clip_layers_bench.py [--configs 2,5] [--layers 2] [--steps 20] [--warmup 3] [--out profiles/clip_layers_bench.json]
    python tools/clip_layers_bench.py --configs 5 --only layers --steps 5   (a bare loop of the call, for a counter run)

Per config (C2: 4,096 x 32 bones; C5: 16,384 x 200 bones), tools/clip_bench.py's clip set (3 clips
with 60 keys on every channel of every bone), every layer at its own random time in its own random
clip, per-skeleton random weights w and 1 - w.  The candidates alternate inside one process after a
warm-up:

  layers       mbik_clip_sample_layers with K layers (normalize mode: a cross-fade)
  three_calls  the workaround it replaces at K = 2: two mbik_clip_sample into two scratch pose
               buffers, then mbik_pose_blend with the per-skeleton weight
  single       one plain mbik_clip_sample
  layers_off90 the new call with the second layer off for 90 % of the skeletons (a crowd mostly
               not in transition)

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

SKELETONS = {2: 4096, 5: 16384}
CLIPS, KEYS = 3, 60


def measure(cfg: int, K: int, steps: int, warmup: int, only: str | None) -> dict:
    import numpy as np
    import torch
    from many_bone_ik_amd import animation as A
    from many_bone_ik_amd import workloads as W
    from many_bone_ik_amd.solver import Plan

    dev = torch.device("cuda", 0)
    n = SKELETONS[cfg]
    print(f"clip_layers_bench: C{cfg}: generating the rig, its plan and the clip set", file=sys.stderr, flush=True)
    wl = W.generate(cfg, 64)   # the plan only lends mbik_pose_blend its rig: count may exceed its skeletons
    B = wl.bone_count
    rest, clips = A.synthetic_clips(1600 + cfg, B, clip_count=CLIPS, key_counts=(KEYS,))
    cs = A.ClipSet(B, rest, clips)
    plan = Plan.from_workload(wl)
    rng = np.random.default_rng(cfg)
    ci = rng.integers(0, CLIPS, (n, K)).astype(np.int32)
    t = rng.uniform(-1.0, 3.0, (n, K)) * np.array([c["length"] for c in clips])[ci]
    w = rng.uniform(0.0, 1.0, (n, K)).astype(np.float32)
    if K == 2:
        w[:, 1] = np.float32(1.0) - w[:, 0]
    layers = A.pack_layers(t, ci, w)
    off90 = layers.copy()
    off90["clip"][rng.uniform(0.0, 1.0, n) < 0.9, 1:] = A.LAYER_OFF

    def up(a):
        return torch.from_numpy(np.ascontiguousarray(a).reshape(-1).view(np.uint8)).to(dev)

    d_layers, d_off90 = up(layers), up(off90)
    d_t0, d_t1 = up(t[:, 0]), up(t[:, min(1, K - 1)])
    d_c0, d_c1 = up(ci[:, 0]), up(ci[:, min(1, K - 1)])
    d_w = up(w[:, min(1, K - 1)])   # the second clip's share: pose_blend moves scratch0 towards scratch1 by it
    out = torch.empty((n, B, 10), dtype=torch.float32, device=dev)
    scratch0, scratch1, out3, out1 = (torch.empty_like(out) for _ in range(4))
    stream = torch.cuda.current_stream(dev).cuda_stream

    def run_layers():
        cs.sample_layers(d_layers.data_ptr(), out.data_ptr(), n, K, flags=A.LAYERS_NORMALIZE, stream=stream)

    def run_off90():
        cs.sample_layers(d_off90.data_ptr(), out.data_ptr(), n, K, flags=A.LAYERS_NORMALIZE, stream=stream)

    def run_three():
        cs.sample(d_t0.data_ptr(), scratch0.data_ptr(), n, clip_index_ptr=d_c0.data_ptr(), stream=stream)
        cs.sample(d_t1.data_ptr(), scratch1.data_ptr(), n, clip_index_ptr=d_c1.data_ptr(), stream=stream)
        plan.pose_blend(scratch0.data_ptr(), scratch1.data_ptr(), out3.data_ptr(), count=n, influence_ptr=d_w.data_ptr(), stream=stream)

    def run_single():
        cs.sample(d_t0.data_ptr(), out1.data_ptr(), n, clip_index_ptr=d_c0.data_ptr(), stream=stream)

    cands = {"layers": run_layers, "three_calls": run_three, "single": run_single, "layers_off90": run_off90}
    if only is not None:
        cands = {only: cands[only]}
    print(f"clip_layers_bench: C{cfg}: timing", file=sys.stderr, flush=True)
    for _ in range(warmup):
        for f in cands.values():
            f()
    torch.cuda.synchronize(dev)
    ms = {k: [] for k in cands}
    for _ in range(steps):
        for k, f in cands.items():   # alternating
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            f()
            b.record()
            b.synchronize()
            ms[k].append(a.elapsed_time(b))
    med = {k: statistics.median(v) for k, v in ms.items()}
    res = {"config": f"C{cfg}", "skeletons": n, "bones": B, "layers": K, "steps": steps, "warmup": warmup, "clips": CLIPS,
           "keys_per_channel": KEYS, "pose_bytes": n * B * 40, "per_frame_input_bytes": n * K * 16,
           "three_calls_scratch_bytes": 2 * n * B * 40}
    for k in cands:
        res[f"{k}_ms"] = med[k]
        res[f"{k}_ms_min_max"] = [min(ms[k]), max(ms[k])]
        res[f"{k}_spread"] = (max(ms[k]) - min(ms[k])) / med[k]
    if only is None:
        run_layers()
        torch.cuda.synchronize(dev)
        h = out.cpu().numpy()   # a sanity check, not a parity test: finite, each skeleton its own, near the workaround
        assert np.isfinite(h).all() and (h[0] != h[1]).any()
        res.update({
            "layers2_over_three_calls" if K == 2 else "layers_over_three_calls": med["layers"] / med["three_calls"],
            "layers2_over_single" if K == 2 else "layers_over_single": med["layers"] / med["single"],
            "layers_off90_over_single": med["layers_off90"] / med["single"],
            "max_position_distance_to_three_calls": float(np.abs(h[:, :, 4:7] - out3.cpu().numpy()[:, :, 4:7]).max()),
        })
    plan.close()
    cs.close()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", default="2,5")
    ap.add_argument("--layers", type=int, default=2)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--only", choices=["layers", "three_calls", "single", "layers_off90"], default=None,
                    help="time one candidate alone and write no file (for a profiler run of its own)")
    ap.add_argument("--out", default=os.path.join(HERE, "profiles", "clip_layers_bench.json"))
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("clip_layers_bench needs a GPU (no CPU fallback)")
    res = {
        "what": "mbik_clip_sample_layers (K layers a skeleton, normalize mode, per-skeleton random weights, 3 clips x 60 keys on "
                "every channel of every bone) vs two mbik_clip_sample into scratch + mbik_pose_blend with a per-skeleton weight "
                "vs one mbik_clip_sample vs the new call with the second layer off for 90 % of the skeletons; medians of "
                "device-event times, candidates alternating in one process; spread = (max - min) / median",
        "device": torch.cuda.get_device_name(0),
        "results": [measure(int(c), args.layers, args.steps, args.warmup, args.only) for c in args.configs.split(",")],
    }
    if args.only is None:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            json.dump(res, fh, indent=1)
            fh.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
