"""Times mbik_skin_vertices_listed (Mesh.skin_listed) against the existing skinning calls on the GPU, with
device events.

    python tools/skin_list_bench.py [--cases 0,1] [--steps 20] [--warmup 3] [--out profiles/skin_list_bench.json]

The cases: C2 rig (32 bones), 4,096 skeletons x 2,048 vertices, K = 4; C5 rig (200 bones), 16,384 x 4,096
vertices, K = 8.  Each runs plain and shaped (16 shapes, every weight active), positions only.  The
meshes, the skin transforms and the frustum are tools/bounds_bench.py's: about half of the
crowd is visible, and the list is what mbik_cull_boxes left on the device.

Per row the candidates alternate inside one process after a warm-up:
  a          the existing call over the whole batch
  b          listed, every skeleton listed (0 .. count-1): b / a is the price of the gather and the count read
  c          listed with the frustum's list, in place
  c_compact  the same list, compact outputs
  d          the existing call over a contiguous count / 2
  d_same     the existing call over the first len(list) skeletons: c / d_same is the price of scattered runs
Before timing, rows of b, c and c_compact are compared bitwise with mbik_skin_vertices_listed_cpu.  Medians
of device-event times with min and max; no threshold is fixed.  Needs a GPU: there is no CPU fallback.
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

# (config, skeletons, vertices, influences)
CASES = [(2, 4096, 2048, 4), (5, 16384, 4096, 8)]
SHAPES = 16


def measure(case, shaped: bool, steps: int, warmup: int, only=None) -> dict:
    import torch
    from many_bone_ik_amd import workloads as W
    from many_bone_ik_amd.skinning import Mesh, cull_boxes_cpu, skin_vertices_listed_cpu, synthetic_mesh, synthetic_shapes
    from many_bone_ik_amd.solver import Plan, pose_globals_cpu

    cfg, n, V, K = case
    dev = torch.device("cuda", 0)
    print(f"skin_list_bench: C{cfg} x {n} x {V}, K={K}, {'shaped' if shaped else 'plain'}: generating", file=sys.stderr, flush=True)
    wl = W.generate(cfg, n)
    plan = Plan.from_workload(wl)
    parents = wl.topo.parents.tolist()
    B = wl.bone_count
    rest, _ = pose_globals_cpu(parents, [], wl.pose[:1])
    pos, _, idx, w = synthetic_mesh(parents, rest[0], V, K, seed=1)
    sp = synthetic_shapes(pos, None, SHAPES, seed=2)[0] if shaped else None
    mesh = Mesh(B, pos, idx, w, shape_positions=sp)
    pose_in = torch.from_numpy(wl.pose).to(dev)
    inv_bind = torch.from_numpy(inverse_bind(rest[0])).to(dev)
    skin = torch.empty((n, B, 12), dtype=torch.float32, device=dev)
    boxes = torch.empty((n, 6), dtype=torch.float32, device=dev)
    stream = torch.cuda.current_stream(dev).cuda_stream
    plan.pose_globals(pose_in.data_ptr(), skin.data_ptr(), n, inv_bind_ptr=inv_bind.data_ptr(), stream=stream)
    mesh.bounds(skin.data_ptr(), boxes.data_ptr(), n, stream=stream)
    torch.cuda.synchronize(dev)
    h_boxes = boxes.cpu().numpy()
    planes = frustum(h_boxes)
    vis_list = torch.zeros(n, dtype=torch.int32, device=dev)
    vis_count = torch.zeros(1, dtype=torch.int32, device=dev)
    mesh.cull(boxes.data_ptr(), n, planes, indices_ptr=vis_list.data_ptr(), visible_count_ptr=vis_count.data_ptr(), stream=stream)
    torch.cuda.synchronize(dev)
    nvis = int(vis_count.cpu().numpy()[0])
    ref_ind = cull_boxes_cpu(h_boxes, planes)[1]
    assert nvis == len(ref_ind) and 0 < nvis < n, (nvis, len(ref_ind))
    all_list = torch.arange(n, dtype=torch.int32, device=dev)
    all_count = torch.tensor([n], dtype=torch.int32, device=dev)
    cw_host = np.random.default_rng(3).uniform(0.02, 0.1, (n, SHAPES)).astype(np.float32) if shaped else None
    cw = torch.from_numpy(cw_host).to(dev) if shaped else None
    wp = cw.data_ptr() if shaped else 0
    out = torch.empty((n, V, 3), dtype=torch.float32, device=dev)

    def a():
        mesh.skin(skin.data_ptr(), out.data_ptr(), n, stream=stream, shape_weights_ptr=wp)

    def b():
        mesh.skin_listed(skin.data_ptr(), out.data_ptr(), n, all_list.data_ptr(), all_count.data_ptr(), shape_weights_ptr=wp, stream=stream)

    def c():
        mesh.skin_listed(skin.data_ptr(), out.data_ptr(), n, vis_list.data_ptr(), vis_count.data_ptr(), shape_weights_ptr=wp, stream=stream)

    def c_compact():
        mesh.skin_listed(skin.data_ptr(), out.data_ptr(), n, vis_list.data_ptr(), vis_count.data_ptr(), compact=True,
                         shape_weights_ptr=wp, stream=stream)

    def d():
        mesh.skin(skin.data_ptr(), out.data_ptr(), n // 2, stream=stream, shape_weights_ptr=wp)

    def d_same():
        mesh.skin(skin.data_ptr(), out.data_ptr(), nvis, stream=stream, shape_weights_ptr=wp)

    # the timed code computes what the host entry does: three listed skeletons of each listed candidate
    h_skin = skin.cpu().numpy()
    probe = np.array([ref_ind[0], ref_ind[len(ref_ind) // 2], ref_ind[-1]], np.int32)
    want = skin_vertices_listed_cpu(B, pos, idx, w, h_skin, probe, 3, compact=True, shape_positions=sp, shape_weights=cw_host)[0]
    where = np.searchsorted(ref_ind, probe)
    checks = {}
    for name, f, rows in (("b", b, probe), ("c", c, probe), ("c_compact", c_compact, where)):
        if only and name not in only:
            continue
        out.fill_(float("nan"))
        f()
        torch.cuda.synchronize(dev)
        got = out[torch.from_numpy(np.asarray(rows, np.int64)).to(dev)].cpu().numpy()
        checks[name] = bool(np.array_equal(got.view(np.uint32), want.view(np.uint32)))
        assert checks[name], f"{name}: the device rows differ from mbik_skin_vertices_listed_cpu"
    print("skin_list_bench: timing", file=sys.stderr, flush=True)
    cands = {"a": a, "b": b, "c": c, "c_compact": c_compact, "d": d, "d_same": d_same}
    if only:   # (A/B builds of the library, MBIK_LIB_OVERRIDE: e.g. a, b for -DMBIK_LIST_CONTIGUOUS)
        cands = {k: f for k, f in cands.items() if k in only}
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
    S, chunks = mesh.launch_shape(n)
    mesh.close()
    plan.close()
    res = {"config": f"C{cfg}", "skeletons": n, "bones": B, "vertices": V, "influences": K, "shaped": shaped,
           "shapes": SHAPES if shaped else 0, "listed": nvis, "steps": steps, "warmup": warmup, "skeletons_per_block": S,
           "vertex_chunks": chunks, "output_bytes_whole_batch": n * V * 12, "rows_match_cpu": checks}
    for k in cands:
        res[f"{k}_ms"] = med[k]
        res[f"{k}_ms_min_max"] = [min(ms[k]), max(ms[k])]
    if only:
        if "a" in med and "b" in med:
            res["b_over_a"] = med["b"] / med["a"]
        return res
    res.update({"b_over_a": med["b"] / med["a"], "a_spread": (max(ms["a"]) - min(ms["a"])) / med["a"],
                "c_over_a": med["c"] / med["a"], "c_over_d": med["c"] / med["d"], "c_over_d_same": med["c"] / med["d_same"],
                "c_compact_over_c": med["c_compact"] / med["c"]})
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", default="0,1")
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--only", default="", help="comma-separated candidates (A/B builds); plain rows only")
    ap.add_argument("--out", default=os.path.join(HERE, "profiles", "skin_list_bench.json"))
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("skin_list_bench needs a GPU (no CPU fallback)")
    res = {
        "what": "mbik_skin_vertices_listed vs mbik_skin_vertices / mbik_skin_vertices_shaped: a whole batch, b listed with every "
                "skeleton, c listed with the frustum's list (in place / compact), d the existing call over count / 2, d_same "
                "over len(list) contiguous skeletons; medians of device-event times, candidates alternating in one process",
        "device": torch.cuda.get_device_name(0),
        "date": datetime.date.today().isoformat(),
        "library": os.environ.get("MBIK_LIB_OVERRIDE", "libmbik.so"),
        "results": [],
    }
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    for c in args.cases.split(","):
        only = [k for k in args.only.split(",") if k]
        for shaped in ((False,) if only else (False, True)):
            res["results"].append(measure(CASES[int(c)], shaped, args.steps, args.warmup, only))
            with open(args.out, "w") as fh:   # (after every row: a long run leaves what it has)
                json.dump(res, fh, indent=1)
                fh.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
