"""Times mbik_skin_bounds and mbik_cull_boxes (Mesh.bounds, Mesh.cull) on the GPU against the traffic
they cannot avoid and the readback they replace, with device events.

    python tools/bounds_bench.py [--cases 0,1] [--steps 20] [--warmup 3] [--out profiles/bounds_bench.json]

Two cases, every bone used: C2 rig (32 bones) x 4,096 skeletons -- 6.3 MB of skin transforms; C5 rig
(200 bones) x 16,384 skeletons -- 157 MB.  The mesh is skinning.synthetic_mesh's (2,048 / 4,096
vertices, K = 4 / 8; only its bone boxes matter here).  The skin transforms are pose_globals of the
workload's poses with the rest pose's inverse bind.

Per case the candidates alternate inside one process after a warm-up:
  bounds        Mesh.bounds: reads count x B x 48 bytes, writes count x 24
  copy_d2d      torch's device-to-device copy of those count x B x 48 bytes: the floor of the bounds call
  copy_d2h      the same bytes copied to pageable host memory: what a caller without this stage pays
                to learn the boxes (timed like the others, with events around the blocking copy)
  solve         one autotuned mbik_solve step
  cull          Mesh.cull with six planes, writing visible, indices and visible_count
  cull_fill     torch's fills of the cull's three outputs
Medians of `steps` with min and max; no threshold is fixed.  Before timing, the first two skeletons'
boxes and the whole visible list are compared with mbik_skin_bounds_cpu and mbik_cull_boxes_cpu.
Needs a GPU: there is no CPU fallback.
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys

import numpy as np

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if HERE not in sys.path:
    sys.path.insert(0, HERE)

from tools.skin_bench import inverse_bind  # noqa: E402

# (config, skeletons, vertices, influences)
CASES = [(2, 4096, 2048, 4), (5, 16384, 4096, 8)]


def frustum(boxes: np.ndarray) -> np.ndarray:
    """Six outward axis planes, each culling the tenth of the boxes that lies farthest out on its side."""
    begin, end = boxes[:, :3], boxes[:, :3] + boxes[:, 3:]
    planes = []
    for a in range(3):
        n = np.zeros(3)
        n[a] = 1.0
        planes.append([*n, np.quantile(begin[:, a], 0.9)])       # culled: begin over the plane
        planes.append([*(-n), -np.quantile(end[:, a], 0.1)])     # culled: end under it
    return np.asarray(planes, np.float32)


def measure(case, steps: int, warmup: int) -> dict:
    import torch
    from many_bone_ik_amd import workloads as W
    from many_bone_ik_amd.skinning import Mesh, cull_boxes_cpu, skin_bounds_cpu, synthetic_mesh
    from many_bone_ik_amd.solver import Plan, pose_globals_cpu

    cfg, n, V, K = case
    dev = torch.device("cuda", 0)
    print(f"bounds_bench: C{cfg} x {n} skeletons: generating", file=sys.stderr, flush=True)
    wl = W.generate(cfg, n)
    plan = Plan.from_workload(wl)
    parents = wl.topo.parents.tolist()
    B = wl.bone_count
    rest, _ = pose_globals_cpu(parents, [], wl.pose[:1])
    pos, _, idx, w = synthetic_mesh(parents, rest[0], V, K, seed=1)
    mesh = Mesh(B, pos, idx, w)
    bone_boxes, used = mesh.bone_boxes()
    assert used.all(), "every bone is meant to be used"
    print("bounds_bench: timing", file=sys.stderr, flush=True)
    pose_in = torch.from_numpy(wl.pose).to(dev)
    targets = torch.from_numpy(wl.targets).to(dev)
    pose_out = torch.empty_like(pose_in)
    inv_bind = torch.from_numpy(inverse_bind(rest[0])).to(dev)
    skin = torch.empty((n, B, 12), dtype=torch.float32, device=dev)
    skin_copy = torch.empty_like(skin)
    skin_host = torch.empty((n, B, 12), dtype=torch.float32)       # pageable
    boxes = torch.empty((n, 6), dtype=torch.float32, device=dev)
    visible = torch.empty(n, dtype=torch.uint8, device=dev)
    indices = torch.empty(n, dtype=torch.int32, device=dev)
    vcount = torch.empty(1, dtype=torch.int32, device=dev)
    plan.autotune(pose_in.data_ptr(), targets.data_ptr(), pose_out.data_ptr())   # the solve as bench.py times it
    stream = torch.cuda.current_stream(dev).cuda_stream
    plan.pose_globals(pose_in.data_ptr(), skin.data_ptr(), n, inv_bind_ptr=inv_bind.data_ptr(), stream=stream)

    # the timed code computes what the host code does
    mesh.bounds(skin.data_ptr(), boxes.data_ptr(), n, stream=stream)
    torch.cuda.synchronize(dev)
    h_boxes = boxes.cpu().numpy()
    ref2 = skin_bounds_cpu(bone_boxes, used, skin[:2].cpu().numpy())
    same_boxes = bool(np.array_equal(h_boxes[:2].view(np.uint32), ref2.view(np.uint32)))
    assert same_boxes and bool(np.isfinite(h_boxes).all()), "the device boxes differ from mbik_skin_bounds_cpu"
    planes = frustum(h_boxes)
    mesh.cull(boxes.data_ptr(), n, planes, visible_ptr=visible.data_ptr(), indices_ptr=indices.data_ptr(),
              visible_count_ptr=vcount.data_ptr(), stream=stream)
    torch.cuda.synchronize(dev)
    ref_vis, ref_ind = cull_boxes_cpu(h_boxes, planes)
    nvis = int(vcount.cpu().numpy()[0])
    same_list = bool(nvis == len(ref_ind) and np.array_equal(visible.cpu().numpy(), ref_vis) and
                     np.array_equal(indices.cpu().numpy()[:nvis], ref_ind))
    assert same_list, "the device's visible list differs from mbik_cull_boxes_cpu"

    def cull():
        mesh.cull(boxes.data_ptr(), n, planes, visible_ptr=visible.data_ptr(), indices_ptr=indices.data_ptr(),
                  visible_count_ptr=vcount.data_ptr(), stream=stream)

    def cull_fill():
        visible.fill_(1), indices.fill_(1), vcount.fill_(1)

    cands = {"bounds": lambda: mesh.bounds(skin.data_ptr(), boxes.data_ptr(), n, stream=stream),
             "copy_d2d": lambda: skin_copy.copy_(skin), "copy_d2h": lambda: skin_host.copy_(skin),
             "solve": lambda: plan.solve(pose_in.data_ptr(), targets.data_ptr(), pose_out.data_ptr(), stream=stream),
             "cull": cull, "cull_fill": cull_fill}
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
    info = plan.info()
    mesh.close()
    plan.close()
    skin_bytes = n * B * 48
    res = {"config": f"C{cfg}", "skeletons": n, "bones": B, "used_bones": int(used.sum()), "steps": steps, "warmup": warmup,
           "skin_bytes": skin_bytes, "in_infinity_cache": skin_bytes < 256 * 2 ** 20, "planes": 6, "visible": nvis,
           "boxes_match_cpu_bitwise": same_boxes, "visible_list_matches_cpu": same_list}
    for k in cands:
        res[f"{k}_ms"] = med[k]
        res[f"{k}_ms_min_max"] = [min(ms[k]), max(ms[k])]
    res.update({
        "bounds_over_copy_d2d": med["bounds"] / med["copy_d2d"],
        "bounds_over_copy_d2h": med["bounds"] / med["copy_d2h"],
        "bounds_over_solve": med["bounds"] / med["solve"],
        "cull_over_fill": med["cull"] / med["cull_fill"],
        "bounds_read_bytes_per_s": skin_bytes / (med["bounds"] * 1e-3),
        "copy_d2d_bytes_per_s": 2 * skin_bytes / (med["copy_d2d"] * 1e-3),   # the copy reads and writes its buffer
        "copy_d2h_bytes_per_s": skin_bytes / (med["copy_d2h"] * 1e-3),
        "solve_layout": f"autotuned: lanes {info['lanes_per_skeleton']}, skeletons/block {info['skeletons_per_block']}, "
                        f"placement {info['state_placement']}, wave roles {info['wave_roles']}",
    })
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", default="0,1")
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(HERE, "profiles", "bounds_bench.json"))
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("bounds_bench needs a GPU (no CPU fallback)")
    res = {
        "what": "mbik_skin_bounds vs a device-to-device and a pageable device-to-host copy of the count x B x 48 bytes it reads vs "
                "one autotuned mbik_solve step; mbik_cull_boxes (six planes; visible, indices and visible_count) vs fills of its "
                "outputs; medians of device-event times, candidates alternating in one process",
        "note": "copy_d2d is the floor of the bounds call (it reads the same bytes and writes as many again); copy_d2h is what "
                "the stage replaces, so bounds_over_copy_d2h must be below 1.  The 6.3 MB case sits inside the 256 MiB Infinity "
                "Cache; the cull moves kilobytes, so cull_over_fill compares launch counts as much as traffic.",
        "device": torch.cuda.get_device_name(0),
        "results": [],
    }
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    for c in args.cases.split(","):
        res["results"].append(measure(CASES[int(c)], args.steps, args.warmup))
        with open(args.out, "w") as fh:   # (after every case: a long run leaves what it has)
            json.dump(res, fh, indent=1)
            fh.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
