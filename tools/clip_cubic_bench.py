"""Times the clip calls on a cubic set against the same keys as linear tracks, on the GPU, with
device events (§16's protocol).

    python tools/clip_cubic_bench.py [--configs 2,5] [--steps 20] [--warmup 3] [--out profiles/clip_cubic_bench.json]

Per config (C2: 4,096 x 32 bones; C5: 16,384 x 200 bones) three sets of §16's shape -- 3 clips with
60 keys on every channel of every bone and on each of 16 blend shapes -- are made from one key table:

  linear_create  every track linear, made by mbik_clipset_create_shaped: the path before cubic tracks
  linear_desc    the same tracks, made by mbik_clipset_create_desc: it must run the same kernels
  cubic          the same keys with every track cubic, made by mbik_clipset_create_desc

and each is timed for sample, sample_layers (K = 2, NORMALIZE, both layers on), sample_shapes and
root_motion, each skeleton at its own random time in its own random clip.  The twelve candidates
alternate inside one process after a warm-up, the set that runs first within a call rotating from
step to step (the first launch of a kernel behind another call's runs slower: a 9 us kernel shows
it); medians of `steps` device-event times with [min, max].

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
CLIPS, KEYS, SHAPES, LAYERS = 3, 60, 16, 2
CALLS = ("sample", "sample_layers", "sample_shapes", "root_motion")
SETS = ("linear_create", "linear_desc", "cubic")


def with_interpolation(clips, kind):
    return [dict(c, tracks=[dict(t, interpolation=kind) for t in c["tracks"]],
                 shape_tracks=[dict(t, interpolation=kind) for t in c["shape_tracks"]]) for c in clips]


def measure(cfg: int, steps: int, warmup: int) -> dict:
    import numpy as np
    import torch
    from many_bone_ik_amd import animation as A
    from many_bone_ik_amd import workloads as W

    dev = torch.device("cuda", 0)
    n = SKELETONS[cfg]
    B = W.generate(cfg, 1).bone_count
    print(f"clip_cubic_bench: C{cfg}: {n} skeletons of {B} bones, building the sets", file=sys.stderr, flush=True)
    rest, clips = A.synthetic_clips(1600 + cfg, B, clip_count=CLIPS, key_counts=(KEYS,))
    clips = A.synthetic_shape_tracks(2600 + cfg, SHAPES, clips, key_counts=(KEYS,))
    sets = {"linear_create": A.ClipSet(B, rest, with_interpolation(clips, A.LINEAR), shape_count=SHAPES),
            "linear_desc": A.ClipSet(B, rest, with_interpolation(clips, A.LINEAR), shape_count=SHAPES, cubic=True),
            "cubic": A.ClipSet(B, rest, with_interpolation(clips, A.CUBIC), shape_count=SHAPES, cubic=True)}
    rng = np.random.default_rng(cfg)
    ci = rng.integers(0, CLIPS, (n, LAYERS)).astype(np.int32)
    length = np.array([c["length"] for c in clips])[ci]
    t = rng.uniform(-1.0, 3.0, (n, LAYERS)) * length
    prev = t - rng.uniform(0.0, 0.05, (n, LAYERS)) * length   # a frame of up to a twentieth of the clip
    layers = A.pack_layers(t, ci, rng.uniform(0.2, 1.0, (n, LAYERS)).astype(np.float32))
    d_t, d_prev, d_c = (torch.from_numpy(np.ascontiguousarray(a[:, 0])).to(dev) for a in (t, prev, ci))
    d_layers = torch.from_numpy(layers.reshape(-1).view(np.uint8).copy()).to(dev)
    pose = torch.empty((n, B, 10), dtype=torch.float32, device=dev)
    weights = torch.empty((n, SHAPES), dtype=torch.float32, device=dev)
    motion = torch.empty((n, 10), dtype=torch.float32, device=dev)
    stream = torch.cuda.current_stream(dev).cuda_stream

    def calls(cs):
        return {
            "sample": lambda: cs.sample(d_t.data_ptr(), pose.data_ptr(), n, clip_index_ptr=d_c.data_ptr(), stream=stream),
            "sample_layers": lambda: cs.sample_layers(d_layers.data_ptr(), pose.data_ptr(), n, LAYERS, flags=A.LAYERS_NORMALIZE, stream=stream),
            "sample_shapes": lambda: cs.sample_shapes(d_t.data_ptr(), weights.data_ptr(), n, clip_index_ptr=d_c.data_ptr(), stream=stream),
            "root_motion": lambda: cs.root_motion(d_prev.data_ptr(), d_t.data_ptr(), motion.data_ptr(), n, 0, clip_index_ptr=d_c.data_ptr(), stream=stream),
        }

    cands = {(s, c): f for s in SETS for c, f in calls(sets[s]).items()}
    for _ in range(warmup):
        for f in cands.values():
            f()
    torch.cuda.synchronize(dev)
    ms = {k: [] for k in cands}
    for step in range(steps):
        for call in CALLS:   # alternating: the three sets of one call side by side, then the next call; the set that goes
            for s in SETS[step % 3:] + SETS[:step % 3]:   # first -- behind another call's kernel, its code not yet hot -- rotates
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                cands[s, call]()
                b.record()
                b.synchronize()
                ms[s, call].append(a.elapsed_time(b))
    assert torch.isfinite(pose).all() and torch.isfinite(weights).all() and torch.isfinite(motion).all()
    res = {"config": f"C{cfg}", "skeletons": n, "bones": B, "shapes": SHAPES, "layers": LAYERS, "steps": steps, "warmup": warmup,
           "clips": CLIPS, "keys_per_channel": KEYS}
    for call in CALLS:
        r = {}
        for s in SETS:
            r[f"{s}_ms"] = statistics.median(ms[s, call])
            r[f"{s}_ms_min_max"] = [min(ms[s, call]), max(ms[s, call])]
        lo, hi = r["linear_create_ms_min_max"]
        r["cubic_over_linear"] = r["cubic_ms"] / r["linear_create_ms"]
        r["linear_desc_inside_linear_create_min_max"] = bool(lo <= r["linear_desc_ms"] <= hi)
        res[call] = r
    for cs in sets.values():
        cs.close()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", default="2,5")
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(HERE, "profiles", "clip_cubic_bench.json"))
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("clip_cubic_bench needs a GPU (no CPU fallback)")
    res = {
        "what": "mbik_clip_sample, _sample_layers (K = 2), _sample_shapes and mbik_clip_root_motion on three sets made from one "
                "key table (3 clips x 60 keys on every channel of every bone and on 16 shapes): linear tracks through "
                "mbik_clipset_create_shaped, the same through mbik_clipset_create_desc, and every track cubic; medians of "
                "device-event times with [min, max], candidates alternating in one process",
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
