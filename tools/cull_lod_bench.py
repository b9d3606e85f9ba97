"""Times mbik_cull_lod (Mesh.cull_lod) against mbik_cull_boxes, and a frame's skinning with one mesh per level
of detail against one full mesh, on the GPU with device events.

    python tools/cull_lod_bench.py [--cases 0,1] [--steps 20] [--warmup 3] [--out profiles/cull_lod_bench.json]

The crowds, their skin transforms and the frustum are tools/bounds_bench.py's: the C2 rig
with 4,096 skeletons and the C5 rig with 16,384.  Each rig gets three meshes of 4,096, 1,024 and 256
vertices, and three adjacent ranges whose edges are the terciles of the visible boxes' distances from
the camera (the corner of the crowd's bounds), with margins of 2 % of an edge: every band holds about a
third of the visible crowd, and the split is recorded.  The lists are exclusive and the state starts
lenient (0xFF).

Per row the candidates alternate inside one process after a warm-up:
  cull         mbik_cull_boxes with indices and visible_count (three launches)
  select       mbik_cull_lod with state, level, three lists (three launches)
  one          the 4,096-vertex mesh, listed, over mbik_cull_boxes' whole visible list
  three_full   one listed call per level, each with max_list = count (empty blocks exit)
  three_tight  the same with each list's true length as its bound
Before timing, select's outputs are compared bitwise with mbik_cull_lod_cpu and three listed rows of each
level with mbik_skin_vertices_listed_cpu.  Medians of device-event times with min and max; no threshold
is fixed.  Needs a GPU: there is no CPU fallback.
"""
from __future__ import annotations

import argparse
import datetime
import json
import os
import statistics
import sys

import numpy as np

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if HERE not in sys.path:
    sys.path.insert(0, HERE)

from tools.bounds_bench import frustum  # noqa: E402
from tools.skin_bench import inverse_bind  # noqa: E402

# (config, skeletons, influences)
CASES = [(2, 4096, 4), (5, 16384, 8)]
VERTICES = (4096, 1024, 256)


def measure(case, steps: int, warmup: int) -> dict:
    import torch
    from many_bone_ik_amd import _lib
    from many_bone_ik_amd import workloads as W
    from many_bone_ik_amd.skinning import Mesh, MeshLod, cull_boxes_cpu, cull_lod_cpu, skin_vertices_listed_cpu, synthetic_mesh
    from many_bone_ik_amd.solver import Plan, pose_globals_cpu

    cfg, n, K = case
    dev = torch.device("cuda", 0)
    print(f"cull_lod_bench: C{cfg} x {n}, K={K}: generating", file=sys.stderr, flush=True)
    wl = W.generate(cfg, n)
    plan = Plan.from_workload(wl)
    parents = wl.topo.parents.tolist()
    B = wl.bone_count
    rest, _ = pose_globals_cpu(parents, [], wl.pose[:1])
    arrays = [synthetic_mesh(parents, rest[0], V, K, seed=1 + i) for i, V in enumerate(VERTICES)]
    meshes = [Mesh(B, pos, idx, w) for pos, _, idx, w in arrays]
    pose_in = torch.from_numpy(wl.pose).to(dev)
    inv_bind = torch.from_numpy(inverse_bind(rest[0])).to(dev)
    skin = torch.empty((n, B, 12), dtype=torch.float32, device=dev)
    boxes = torch.empty((n, 6), dtype=torch.float32, device=dev)
    stream = torch.cuda.current_stream(dev).cuda_stream
    plan.pose_globals(pose_in.data_ptr(), skin.data_ptr(), n, inv_bind_ptr=inv_bind.data_ptr(), stream=stream)
    meshes[0].bounds(skin.data_ptr(), boxes.data_ptr(), n, stream=stream)
    torch.cuda.synchronize(dev)
    h_boxes = boxes.cpu().numpy()
    planes = frustum(h_boxes)
    ref_vis, ref_ind = cull_boxes_cpu(h_boxes, planes)
    # the camera at the corner of the crowd, the range edges at the terciles of the visible distances
    centre = h_boxes[:, :3].astype(np.float64) + 0.5 * h_boxes[:, 3:]
    camera = np.nanmin(h_boxes[:, :3], axis=0).astype(np.float32)
    dist = np.linalg.norm(centre - camera, axis=1)[ref_vis == 1]
    q1, q2 = (float(np.float32(q)) for q in np.quantile(dist, [1 / 3, 2 / 3]))
    ranges = np.array([[0, q1, 0, 0.02 * q1], [q1, q2, 0.02 * q1, 0.02 * q2], [q2, 0, 0.02 * q2, 0]], np.float32)
    lod = MeshLod(meshes, ranges)
    R = len(meshes)
    state = torch.full((n,), 0xFF, dtype=torch.uint8, device=dev)
    level = torch.zeros(n, dtype=torch.uint8, device=dev)
    lists = torch.full((R, n), -1, dtype=torch.int32, device=dev)
    counts = torch.zeros(R, dtype=torch.int32, device=dev)
    vis_list = torch.zeros(n, dtype=torch.int32, device=dev)
    vis_count = torch.zeros(1, dtype=torch.int32, device=dev)
    outs = [torch.empty((n, V, 3), dtype=torch.float32, device=dev) for V in VERTICES]

    def cull():
        meshes[0].cull(boxes.data_ptr(), n, planes, indices_ptr=vis_list.data_ptr(), visible_count_ptr=vis_count.data_ptr(), stream=stream)

    def select():
        lod.select(boxes.data_ptr(), n, planes, camera, state.data_ptr(), lists.data_ptr(), counts.data_ptr(), level_ptr=level.data_ptr(),
                   stream=stream)

    # the timed code computes what the host entries do
    cull()
    select()
    torch.cuda.synchronize(dev)
    ref_state, ref_level, ref_lists = cull_lod_cpu(h_boxes, planes, camera, ranges, np.full(n, 0xFF, np.uint8), flags=_lib.LOD_EXCLUSIVE)
    h_lists, h_counts = lists.cpu().numpy(), counts.cpu().numpy()
    select_ok = bool(np.array_equal(state.cpu().numpy(), ref_state) and np.array_equal(level.cpu().numpy(), ref_level) and
                     h_counts.tolist() == [len(l) for l in ref_lists] and
                     all(np.array_equal(h_lists[r, :len(l)], l) and (h_lists[r, len(l):] == -1).all() for r, l in enumerate(ref_lists)))
    assert select_ok, "the device lists differ from mbik_cull_lod_cpu"
    assert int(vis_count.cpu().numpy()[0]) == len(ref_ind) and sum(h_counts) == len(ref_ind), (h_counts, len(ref_ind))
    true_lengths = [int(c) for c in h_counts]
    assert min(true_lengths) >= 0.1 * len(ref_ind), true_lengths

    def one():
        meshes[0].skin_listed(skin.data_ptr(), outs[0].data_ptr(), n, vis_list.data_ptr(), vis_count.data_ptr(), stream=stream)

    def three_full():
        lod.skin(skin.data_ptr(), [o.data_ptr() for o in outs], n, lists.data_ptr(), counts.data_ptr(), stream=stream)

    def three_tight():
        lod.skin(skin.data_ptr(), [o.data_ptr() for o in outs], n, lists.data_ptr(), counts.data_ptr(), max_lists=true_lengths, stream=stream)

    h_skin = skin.cpu().numpy()
    rows_ok = {}
    for name, f in (("three_full", three_full), ("three_tight", three_tight)):
        for o in outs:
            o.fill_(float("nan"))
        f()
        torch.cuda.synchronize(dev)
        ok = True
        for (pos, _, idx, w), o, l in zip(arrays, outs, ref_lists):
            probe = np.array([l[0], l[len(l) // 2], l[-1]], np.int32)
            want = skin_vertices_listed_cpu(B, pos, idx, w, h_skin, probe, 3, compact=True)[0]
            got = o[torch.from_numpy(probe.astype(np.int64)).to(dev)].cpu().numpy()
            ok = ok and bool(np.array_equal(got.view(np.uint32), want.view(np.uint32)))
        rows_ok[name] = ok
        assert ok, f"{name}: the device rows differ from mbik_skin_vertices_listed_cpu"
    print("cull_lod_bench: timing", file=sys.stderr, flush=True)
    cands = {"cull": cull, "select": select, "one": one, "three_full": three_full, "three_tight": three_tight}
    for _ in range(warmup):
        for f in cands.values():
            f()
    torch.cuda.synchronize(dev)
    ms = {k: [] for k in cands}
    for _ in range(steps):
        for k, f in cands.items():   # alternating
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            f()
            e1.record()
            e1.synchronize()
            ms[k].append(e0.elapsed_time(e1))
    med = {k: statistics.median(v) for k, v in ms.items()}
    for m in meshes:
        m.close()
    plan.close()
    res = {"config": f"C{cfg}", "skeletons": n, "bones": B, "influences": K, "vertices": list(VERTICES), "visible": len(ref_ind),
           "ranges": ranges.tolist(), "camera": camera.tolist(), "split": true_lengths, "steps": steps, "warmup": warmup,
           "select_matches_cpu": select_ok, "rows_match_cpu": rows_ok}
    for k in cands:
        res[f"{k}_ms"] = med[k]
        res[f"{k}_ms_min_max"] = [min(ms[k]), max(ms[k])]
        res[f"{k}_spread"] = (max(ms[k]) - min(ms[k])) / med[k]
    res.update({"select_over_cull": med["select"] / med["cull"], "three_full_over_one": med["three_full"] / med["one"],
                "three_tight_over_one": med["three_tight"] / med["one"], "three_tight_over_three_full": med["three_tight"] / med["three_full"]})
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", default="0,1")
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(HERE, "profiles", "cull_lod_bench.json"))
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("cull_lod_bench needs a GPU (no CPU fallback)")
    res = {
        "what": "mbik_cull_lod vs mbik_cull_boxes (select, cull), and a frame's listed skinning with one mesh per level of detail "
                "(three_full: max_list = count; three_tight: the true lengths) vs one 4,096-vertex mesh over the whole visible list "
                "(one); medians of device-event times, candidates alternating in one process",
        "device": torch.cuda.get_device_name(0),
        "date": datetime.date.today().isoformat(),
        "results": [],
    }
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    for c in args.cases.split(","):
        res["results"].append(measure(CASES[int(c)], args.steps, args.warmup))
        with open(args.out, "w") as fh:   # (after every row: a long run leaves what it has)
            json.dump(res, fh, indent=1)
            fh.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
