"""Times mbik_clip_sample_shapes and mbik_clip_sample_shapes_layers against what they replace, on the
GPU, with device events (tools/clip_bench.py's protocol).

    python tools/clip_shapes_bench.py [--sizes A,B] [--steps 20] [--warmup 3] [--out profiles/clip_shapes_bench.json]
    python tools/clip_shapes_bench.py --sizes B --only shapes --steps 5   (a bare loop of the call, for a counter run)

Per size (A: 4,096 x 52 shapes; B: 16,384 x 52 shapes) the candidates alternate inside one process
after a warm-up:

  shapes         mbik_clip_sample_shapes of a set of 3 clips with 60 keys on every shape, each skeleton
                 at its own random time (one loop before to two loops after the clip) in its own random
                 clip: count x 12 B in, count x 52 x 4 B out
  shapes_layers  mbik_clip_sample_shapes_layers with K = 2 in normalize mode (a cross-fade: weights w and
                 1 - w, random times and clips): count x 32 B in
  fill           a device fill of the same count x 52 x 4 B (the least a producer of the weights can cost)
  upload         hipMemcpyAsync of those bytes from pageable host memory (torch's copy_ of an unpinned CPU
                 tensor), which is the copy the call replaces in a frame; the count x 52 track evaluations
                 on the host that the call also removes are not in it
  pose           for context, mbik_clip_sample on a 52-bone set with 60 keys on every channel: the same
                 number of lanes on clip.h's split layout (three channels and 40 B out a lane)
  pose_position  the same with position tracks only: one search a lane, as a shape lane has

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

SKELETONS = {"A": 4096, "B": 16384}
SHAPES, CLIPS, KEYS = 52, 3, 60


def measure(size: str, steps: int, warmup: int, only: str | None) -> dict:
    import numpy as np
    import torch
    from many_bone_ik_amd import animation as A

    dev = torch.device("cuda", 0)
    n, P = SKELETONS[size], SHAPES
    print(f"clip_shapes_bench: {size}: {n} skeletons, building the sets", file=sys.stderr, flush=True)
    rest, clips = A.synthetic_clips(2300, P, clip_count=CLIPS, key_counts=(KEYS,))
    shaped = A.synthetic_shape_tracks(2301, P, clips, key_counts=(KEYS,))
    init = np.zeros(P, np.float32)
    cs = A.ClipSet(P, rest, shaped, shape_count=P, shape_init=init)
    pos_only = [dict(c, tracks=[t for t in c["tracks"] if t["channel"] == A.POSITION]) for c in clips]
    cs_pos = A.ClipSet(P, rest, pos_only)
    rng = np.random.default_rng(23)
    lengths = np.array([c["length"] for c in clips])
    ci = rng.integers(0, CLIPS, n).astype(np.int32)
    t = rng.uniform(-1.0, 3.0, n) * lengths[ci]
    ci2 = rng.integers(0, CLIPS, (n, 2)).astype(np.int32)
    w = rng.uniform(0.0, 1.0, n).astype(np.float32)
    layers = A.pack_layers(rng.uniform(-1.0, 3.0, (n, 2)) * lengths[ci2], ci2, np.stack([w, np.float32(1) - w], axis=1))
    d_t, d_c = torch.from_numpy(t).to(dev), torch.from_numpy(ci).to(dev)
    d_l = torch.from_numpy(layers.reshape(-1).view(np.uint8)).to(dev)
    out = {k: torch.empty((n, P), dtype=torch.float32, device=dev) for k in ("shapes", "shapes_layers", "fill", "upload")}
    pose = torch.empty((n, P, 10), dtype=torch.float32, device=dev)
    host_w = torch.from_numpy(rng.uniform(0.0, 1.0, (n, P)).astype(np.float32))   # pageable: not pinned
    assert not host_w.is_pinned()
    stream = torch.cuda.current_stream(dev).cuda_stream

    cands = {
        "shapes": lambda: cs.sample_shapes(d_t.data_ptr(), out["shapes"].data_ptr(), n, clip_index_ptr=d_c.data_ptr(), stream=stream),
        "shapes_layers": lambda: cs.sample_shapes_layers(d_l.data_ptr(), out["shapes_layers"].data_ptr(), n, 2,
                                                         flags=A.LAYERS_NORMALIZE, stream=stream),
        "fill": lambda: out["fill"].fill_(1.0),
        "upload": lambda: out["upload"].copy_(host_w, non_blocking=True),
        "pose": lambda: cs.sample(d_t.data_ptr(), pose.data_ptr(), n, clip_index_ptr=d_c.data_ptr(), stream=stream),
        "pose_position": lambda: cs_pos.sample(d_t.data_ptr(), pose.data_ptr(), n, clip_index_ptr=d_c.data_ptr(), stream=stream),
    }
    if only is not None:
        cands = {only: cands[only]}
    print(f"clip_shapes_bench: {size}: timing", file=sys.stderr, flush=True)
    for _ in range(warmup):
        for f in cands.values():
            f()
    torch.cuda.synchronize(dev)
    ms = {k: [] for k in cands}
    for _ in range(steps):
        for k, f in cands.items():   # alternating: shapes, shapes_layers, fill, upload, pose, pose_position, shapes, ...
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            f()
            b.record()
            b.synchronize()
            ms[k].append(a.elapsed_time(b))
    med = {k: statistics.median(v) for k, v in ms.items()}
    weight_bytes = n * P * 4
    res = {"size": size, "skeletons": n, "shapes": P, "steps": steps, "warmup": warmup, "clips": CLIPS, "keys_per_shape": KEYS,
           "weight_bytes": weight_bytes, "per_frame_input_bytes": {"shapes": n * 12, "shapes_layers": n * 32},
           "shape_table_bytes": CLIPS * P * (16 + KEYS * 16) + 16 + P * 4 + CLIPS * 16,
           "host_track_evaluations_removed": n * P}
    for k in cands:
        res[f"{k}_ms"] = med[k]
        res[f"{k}_ms_min_max"] = [min(ms[k]), max(ms[k])]
        res[f"{k}_spread"] = (max(ms[k]) - min(ms[k])) / med[k]
    if only is None:
        # the sampled weights are finite and every skeleton got its own (a sanity check, not a parity test)
        for k in ("shapes", "shapes_layers"):
            h = out[k].cpu().numpy()
            assert np.isfinite(h).all() and (h[0] != h[1]).any()
        for k in ("shapes", "shapes_layers"):
            tag = "sample" if k == "shapes" else "layers"
            res[f"{tag}_over_fill"] = med[k] / med["fill"]
            res[f"{tag}_over_upload"] = med[k] / med["upload"]
            # below 1 by more than both spreads: the slowest call is faster than the fastest upload
            res[f"{tag}_below_upload_beyond_spreads"] = max(ms[k]) < min(ms["upload"])
        res["shapes_over_pose_lanes"] = med["shapes"] / med["pose"]
        res["shapes_over_pose_position_lanes"] = med["shapes"] / med["pose_position"]
        res["upload_bytes_per_s"] = weight_bytes / (med["upload"] * 1e-3)
        res["shapes_lanes_per_s"] = n * P / (med["shapes"] * 1e-3)
        res["pose_position_lanes_per_s"] = n * P / (med["pose_position"] * 1e-3)
    cs.close()
    cs_pos.close()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="A,B")
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--only", choices=["shapes", "shapes_layers", "fill", "upload", "pose", "pose_position"], default=None,
                    help="time one candidate alone and write no file (for a profiler run of its own)")
    ap.add_argument("--out", default=os.path.join(HERE, "profiles", "clip_shapes_bench.json"))
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("clip_shapes_bench needs a GPU (no CPU fallback)")
    res = {
        "what": "mbik_clip_sample_shapes and mbik_clip_sample_shapes_layers (K = 2, normalize) on 3 clips x 60 keys on every one "
                "of 52 shapes, per-skeleton random times and clips, vs a device fill of count x 52 x 4 B vs hipMemcpyAsync of "
                "those bytes from pageable host memory vs mbik_clip_sample on a 52-bone set with the same key counts; medians "
                "of device-event times, candidates alternating in one process, spread = (max - min) / median",
        "note": "The upload is the copy a frame makes without the call; the count x 52 track evaluations on the host that the "
                "call also removes are not in that ratio.  The fill is the floor of any producer of the weights.",
        "device": torch.cuda.get_device_name(0),
        "results": [measure(s, args.steps, args.warmup, args.only) for s in args.sizes.split(",")],
    }
    if args.only is None:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            json.dump(res, fh, indent=1)
            fh.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
