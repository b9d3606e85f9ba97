"""Times the root-motion calls against the upload they replace and against the pose sample of the same
crowd, on the GPU, with device events (§16's protocol).

    python tools/root_motion_bench.py [--configs 2,5] [--steps 20] [--warmup 3] [--out profiles/root_motion_bench.json]
    python tools/root_motion_bench.py --configs 5 --only layers2 --steps 5   (a bare loop of one candidate, for a counter run)

Per config (C2: 4,096 x 32 bones; C5: 16,384 x 200 bones), tools/clip_bench.py's clip set (3 clips
with 60 keys on every channel of every bone, the root bone 0 among them), every skeleton at its own
random time in its own random clip, one frame of 1/60 s behind it -- so a frame in a hundred crosses
its clip's seam.  The candidates alternate inside one process after a warm-up:

  plain          mbik_clip_root_motion (with the pose fix-up) + mbik_root_motion_apply
  layers2        mbik_clip_root_motion_layers at K = 2 (normalize mode) + mbik_root_motion_apply
  plain_extract, layers2_extract, apply   the three calls on their own
  upload         hipMemcpyAsync of count x 48 bytes from pageable host memory into skeleton_global:
                 what a host that evaluates the locomotion itself sends every frame
  sample, sample_layers2   the pose sample of the same crowd (profiles/clip_bench.json's and
                 profiles/clip_layers_bench.json's calls, re-measured here)

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
BONES = {2: 32, 5: 200}
CLIPS, KEYS, ROOT, DT = 3, 60, 0, 1.0 / 60.0
CANDIDATES = ("plain", "layers2", "plain_extract", "layers2_extract", "apply", "upload", "sample", "sample_layers2")


def measure(cfg: int, steps: int, warmup: int, only: str | None) -> dict:
    import numpy as np
    import torch
    from many_bone_ik_amd import animation as A

    dev = torch.device("cuda", 0)
    n, B = SKELETONS[cfg], BONES[cfg]
    print(f"root_motion_bench: C{cfg}: generating the clip set", file=sys.stderr, flush=True)
    rest, clips = A.synthetic_clips(1600 + cfg, B, clip_count=CLIPS, key_counts=(KEYS,))
    cs = A.ClipSet(B, rest, clips)
    rng = np.random.default_rng(cfg)
    ci = rng.integers(0, CLIPS, (n, 2)).astype(np.int32)
    t1 = rng.uniform(0.0, 3.0, (n, 2)) * np.array([c["length"] for c in clips])[ci]
    t0 = t1 - DT
    w = rng.uniform(0.0, 1.0, n).astype(np.float32)
    layers = A.pack_layers(t1, ci, np.stack([w, np.float32(1.0) - w], axis=1))

    def up(a):
        return torch.from_numpy(np.ascontiguousarray(a).reshape(-1).view(np.uint8)).to(dev)

    d_layers, d_prev2 = up(layers), up(t0)
    d_t0, d_t1, d_ci = up(t0[:, 0]), up(t1[:, 0]), up(ci[:, 0])
    pose = torch.empty((n, B, 10), dtype=torch.float32, device=dev)
    motion = torch.empty((n, 10), dtype=torch.float32, device=dev)
    identity = np.tile(np.array([1, 0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0], np.float32), (n, 1))
    h_sg = torch.from_numpy(identity.copy())            # pageable host memory
    assert not h_sg.is_pinned()
    d_sg = torch.from_numpy(identity.copy()).to(dev)
    d_up = torch.empty_like(d_sg)
    stream = torch.cuda.current_stream(dev).cuda_stream
    flags = A.LAYERS_NORMALIZE

    def plain_extract():
        cs.root_motion(d_t0.data_ptr(), d_t1.data_ptr(), motion.data_ptr(), n, ROOT, clip_index_ptr=d_ci.data_ptr(), pose_ptr=pose.data_ptr(),
                       stream=stream)

    def layers2_extract():
        cs.root_motion_layers(d_layers.data_ptr(), d_prev2.data_ptr(), motion.data_ptr(), n, 2, ROOT, flags=flags, pose_ptr=pose.data_ptr(),
                              stream=stream)

    def apply():
        cs.apply_root_motion(motion.data_ptr(), d_sg.data_ptr(), n, flags=A.ROOT_MOTION_ORTHONORMALIZE, stream=stream)

    def plain():
        plain_extract()
        apply()

    def layers2():
        layers2_extract()
        apply()

    def upload():
        d_up.copy_(h_sg, non_blocking=True)

    def sample():
        cs.sample(d_t1.data_ptr(), pose.data_ptr(), n, clip_index_ptr=d_ci.data_ptr(), stream=stream)

    def sample_layers2():
        cs.sample_layers(d_layers.data_ptr(), pose.data_ptr(), n, 2, flags=flags, stream=stream)

    cands = {"plain": plain, "layers2": layers2, "plain_extract": plain_extract, "layers2_extract": layers2_extract, "apply": apply,
             "upload": upload, "sample": sample, "sample_layers2": sample_layers2}
    assert tuple(cands) == CANDIDATES
    if only is not None:
        cands = {only: cands[only]}
    print(f"root_motion_bench: C{cfg}: timing", file=sys.stderr, flush=True)
    sample()
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
    res = {"config": f"C{cfg}", "skeletons": n, "bones": B, "steps": steps, "warmup": warmup, "clips": CLIPS, "keys_per_channel": KEYS,
           "upload_bytes": n * 48}
    lengths = np.array([c["length"] for c in clips])[ci]
    loops = np.array([c["loop_mode"] for c in clips])[ci] == 1
    res["frames_across_the_seam"] = int((loops[:, 0] & (np.fmod(t1[:, 0], lengths[:, 0]) < np.fmod(np.maximum(t0[:, 0], 0.0), lengths[:, 0]))).sum())
    for k in cands:
        res[f"{k}_ms"] = med[k]
        res[f"{k}_ms_min_max"] = [min(ms[k]), max(ms[k])]
        res[f"{k}_spread"] = (max(ms[k]) - min(ms[k])) / med[k]
    if only is None:
        sample()
        plain()
        torch.cuda.synchronize(dev)
        h_m, h_g = motion.cpu().numpy(), d_sg.cpu().numpy()   # a sanity check, not a parity test
        assert np.isfinite(h_m).all() and np.isfinite(h_g).all() and (h_m[0] != h_m[1]).any()
        assert np.array_equal(pose[:, ROOT].contiguous().cpu().numpy().view(np.uint32), np.tile(rest[ROOT], (n, 1)).view(np.uint32))
        res.update({
            "plain_over_upload": med["plain"] / med["upload"],
            "layers2_over_upload": med["layers2"] / med["upload"],
            "plain_extract_over_sample": med["plain_extract"] / med["sample"],
            "layers2_extract_over_sample": med["layers2_extract"] / med["sample"],
            "layers2_extract_over_sample_layers2": med["layers2_extract"] / med["sample_layers2"],
        })
    cs.close()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", default="2,5")
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--only", choices=CANDIDATES, default=None, help="time one candidate alone and write no file (for a profiler run of its own)")
    ap.add_argument("--out", default=os.path.join(HERE, "profiles", "root_motion_bench.json"))
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("root_motion_bench needs a GPU (no CPU fallback)")
    res = {
        "what": "mbik_clip_root_motion / mbik_clip_root_motion_layers (K = 2, normalize mode) with the pose fix-up, plus "
                "mbik_root_motion_apply with orthonormalisation (3 clips x 60 keys on every channel of every bone, root bone 0, frames "
                "of 1/60 s) vs a hipMemcpyAsync of count x 48 bytes from pageable host memory vs mbik_clip_sample / "
                "mbik_clip_sample_layers of the same crowd; medians of device-event times, candidates alternating in one process; "
                "spread = (max - min) / median",
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
