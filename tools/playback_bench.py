"""Times mbik_playback_advance against the upload it replaces, on the GPU, with device events
(§16's protocol).

    python tools/playback_bench.py [--configs 2,5] [--layers 1,2,4] [--steps 20] [--warmup 3] [--out profiles/playback_bench.json]

Per config (C2: 4,096 x 32 bones; C5: 16,384 x 200 bones) and slot count K, tools/clip_bench.py's
clip set (3 clips with 60 keys on every channel of every bone), a crowd seeded at desynchronised
positions in the two looping clips, every tenth skeleton with a fade behind it (K > 1).  The
candidates alternate inside one process after a warm-up:

  advance        mbik_playback_advance with no command (a frame on which nobody starts a clip)
  advance_cmds   the same with blended play commands for 1 % of the crowd, already on the device
  upload         what the advance replaces: one asynchronous copy of count * K * 24 bytes (the layer
                 records and the previous times) from pageable host memory, through torch's
                 Tensor.copy_(non_blocking=True), which issues hipMemcpyAsync
  sample_layers  mbik_clip_sample_layers of the same crowd from the advance's records, for scale

What the ratios leave out: the host's own per-character state machine, and the wait for it before
the frame can start.  Neither is timed.  Needs a GPU: there is no CPU fallback.
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


def measure(cfg: int, K: int, steps: int, warmup: int) -> dict:
    import numpy as np
    import torch
    from many_bone_ik_amd import animation as A
    from many_bone_ik_amd import workloads as W

    dev = torch.device("cuda", 0)
    n = SKELETONS[cfg]
    print(f"playback_bench: C{cfg} K={K}: generating the rig and the clip set", file=sys.stderr, flush=True)
    B = W.generate(cfg, 1).bone_count
    rest, clips = A.synthetic_clips(1600 + cfg, B, clip_count=CLIPS, key_counts=(KEYS,))
    looping = [c for c, clip in enumerate(clips) if clip["loop_mode"] == A.LOOP_LINEAR]
    rng = np.random.default_rng(cfg * 10 + K)
    st, fl = A.empty_state(n, K)
    ci = rng.choice(looping, n)
    st["clip"][:, 0], st["speed"][:, 0] = ci, 1.0
    st["pos"][:, 0] = rng.uniform(0.0, 1.0, n) * np.array([c["length"] for c in clips])[ci]
    if K > 1:
        fading = np.arange(0, n, 10)
        st["clip"][fading, 1], st["speed"][fading, 1], st["blend_left"][fading, 1], st["blend_time"][fading, 1] = looping[0], 1.0, 0.5, 1e6
        st["pos"][fading, 1] = 0.25
    who = np.sort(rng.choice(n, max(1, n // 100), replace=False))
    cmds = A.pack_commands(who, rng.choice(looping, len(who)), blend_time=0.3)
    cs = A.ClipSet(B, rest, clips)
    pb = A.Playback(cs, n, K, next=[-1] * CLIPS)
    pb.write(st, fl)
    d_cmds = torch.from_numpy(cmds.view(np.uint8).copy()).to(dev)
    d_layers = torch.empty(n * K * 16, dtype=torch.uint8, device=dev)
    d_prev = torch.empty(n * K, dtype=torch.float64, device=dev)
    d_ev = torch.empty(n, dtype=torch.uint8, device=dev)
    d_up = torch.empty(n * K * 24, dtype=torch.uint8, device=dev)
    h_up = torch.from_numpy(rng.integers(0, 255, n * K * 24, dtype=np.uint8))   # pageable
    pose = torch.empty((n, B, 10), dtype=torch.float32, device=dev)
    stream = torch.cuda.current_stream(dev).cuda_stream
    delta = 1.0 / 60.0

    def run_advance():
        pb.advance(delta, d_layers.data_ptr(), d_prev.data_ptr(), n, events_ptr=d_ev.data_ptr(), stream=stream)

    def run_cmds():
        pb.advance(delta, d_layers.data_ptr(), d_prev.data_ptr(), n, cmds_ptr=d_cmds.data_ptr(), cmd_count=len(cmds), events_ptr=d_ev.data_ptr(),
                   stream=stream)

    def run_upload():
        d_up.copy_(h_up, non_blocking=True)

    def run_sample():
        cs.sample_layers(d_layers.data_ptr(), pose.data_ptr(), n, K, flags=A.LAYERS_NORMALIZE, stream=stream)

    cands = {"advance": run_advance, "advance_cmds": run_cmds, "upload": run_upload, "sample_layers": run_sample}
    print(f"playback_bench: C{cfg} K={K}: timing", file=sys.stderr, flush=True)
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
    res = {"config": f"C{cfg}", "skeletons": n, "bones": B, "layers": K, "steps": steps, "warmup": warmup, "commands": len(cmds),
           "upload_bytes": n * K * 24, "command_bytes": len(cmds) * 24}
    for k in cands:
        res[f"{k}_ms"] = med[k]
        res[f"{k}_ms_min_max"] = [min(ms[k]), max(ms[k])]
    res["advance_over_upload"] = med["advance"] / med["upload"]
    res["advance_cmds_over_upload"] = med["advance_cmds"] / med["upload"]
    res["advance_over_sample_layers"] = med["advance"] / med["sample_layers"]
    # a sanity check, not a parity test: the crowd is playing and its records are what the sampler takes
    got, _ = pb.read()
    h = pose.cpu().numpy()
    assert (got["clip"][:, 0] >= 0).all() and np.isfinite(got["pos"]).all() and np.isfinite(h).all()
    pb.close()
    cs.close()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", default="2,5")
    ap.add_argument("--layers", default="1,2,4")
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(HERE, "profiles", "playback_bench.json"))
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("playback_bench needs a GPU (no CPU fallback)")
    res = {
        "what": "mbik_playback_advance (K slots a skeleton, no command / blended play commands for 1 % of the crowd) vs one asynchronous "
                "copy of count * K * 24 bytes from pageable host memory (the layer records and previous times the host would upload) vs "
                "mbik_clip_sample_layers of the same crowd; medians of device-event times, candidates alternating in one process; the "
                "host's own playback state machine and the wait for it are not timed",
        "device": torch.cuda.get_device_name(0),
        "results": [measure(int(c), int(k), args.steps, args.warmup) for c in args.configs.split(",") for k in args.layers.split(",")],
    }
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(res, fh, indent=1)
        fh.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
