"""Times mbik_skin_vertices_shaped (Mesh.skin with shape weights) against mbik_skin_vertices on the same
mesh, a device fill of the output bytes and the least traffic of an unfused morph pass, on the GPU,
with device events.

    python tools/morph_bench.py [--cases 0,1] [--steps 20] [--warmup 3] [--out profiles/morph_bench.json]

Two of tools/skin_bench.py's cases, here with normals (the shapes morph both arrays): C2 rig (32
bones), 4,096 skeletons x 2,048 vertices, K = 4 -- 201 MB of output, inside the 256 MiB Infinity
Cache; C5 rig (200 bones), 16,384 x 4,096 vertices, K = 8 -- 1.6 GB, which speaks for HBM.  P = 16
dense shapes from skinning.synthetic_shapes, relative mode, with three weight sets: all 16 active,
2 of 16 active per skeleton (a different pair each), none active.  The skin transforms are
pose_globals of the workload's poses with the rest pose's inverse bind.

Per case the candidates alternate inside one process after a warm-up: the shaped call with each
weight set; Mesh.skin without weights on the same mesh (the merged path, the yardstick); the
"none active" call and the plain call once more for positions only (no normal is renormalised
there, which splits the cost of "none active" into the walk over the weights and the normals' side); torch's
fill of a buffer of the output's size; torch's copy of count x V x 32 bytes (a morphed position and
normal record a vertex, written once and read once: the least an unfused morph pass would add to
the plain call).  Medians of `steps` with min and max; no threshold is fixed.  The first two
skeletons of the all-active run are compared bitwise with mbik_skin_vertices_shaped_cpu.  Needs a
GPU: there is no CPU fallback.
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
SHAPES = 16


def weight_sets(n: int, seed: int) -> dict:
    rng = np.random.default_rng(seed)
    dense = rng.uniform(0.02, 0.1, (n, SHAPES)).astype(np.float32)
    pick = np.argsort(rng.uniform(0.0, 1.0, (n, SHAPES)), axis=1)[:, :2]
    two = np.zeros_like(dense)
    np.put_along_axis(two, pick, np.take_along_axis(dense, pick, axis=1) * 4.0, axis=1)
    return {"all_active": dense, "two_active": two, "none_active": np.zeros_like(dense)}


def measure(case, steps: int, warmup: int) -> dict:
    import torch
    from many_bone_ik_amd import workloads as W
    from many_bone_ik_amd.skinning import Mesh, skin_vertices_cpu, synthetic_mesh, synthetic_shapes
    from many_bone_ik_amd.solver import Plan, pose_globals_cpu

    cfg, n, V, K = case
    dev = torch.device("cuda", 0)
    print(f"morph_bench: C{cfg} x {n} skeletons x {V} vertices, K={K}, P={SHAPES}: generating", file=sys.stderr, flush=True)
    wl = W.generate(cfg, n)
    plan = Plan.from_workload(wl)
    parents = wl.topo.parents.tolist()
    B = wl.bone_count
    rest, _ = pose_globals_cpu(parents, [], wl.pose[:1])
    pos, nrm, idx, w = synthetic_mesh(parents, rest[0], V, K, seed=1)
    sp, sn = synthetic_shapes(pos, nrm, SHAPES, seed=2)
    mesh = Mesh(B, pos, idx, w, normals=nrm, shape_positions=sp, shape_normals=sn)
    print("morph_bench: timing", file=sys.stderr, flush=True)
    pose = torch.from_numpy(wl.pose).to(dev)
    inv_bind = torch.from_numpy(inverse_bind(rest[0])).to(dev)
    skin = torch.empty((n, B, 12), dtype=torch.float32, device=dev)
    out_p = torch.empty((n, V, 3), dtype=torch.float32, device=dev)
    out_n = torch.empty((n, V, 3), dtype=torch.float32, device=dev)
    out_bytes = n * V * 24
    unfused_bytes = n * V * 32
    fill_buf = torch.empty(out_bytes // 4, dtype=torch.float32, device=dev)
    src = torch.empty(unfused_bytes // 4, dtype=torch.float32, device=dev).normal_()
    dst = torch.empty_like(src)
    sets = weight_sets(n, seed=3)
    d_sets = {k: torch.from_numpy(v).to(dev) for k, v in sets.items()}
    stream = torch.cuda.current_stream(dev).cuda_stream
    plan.pose_globals(pose.data_ptr(), skin.data_ptr(), n, inv_bind_ptr=inv_bind.data_ptr(), stream=stream)

    def shaped(name):
        return lambda: mesh.skin(skin.data_ptr(), out_p.data_ptr(), n, out_normals_ptr=out_n.data_ptr(), stream=stream,
                                 shape_weights_ptr=d_sets[name].data_ptr())

    def plain():
        mesh.skin(skin.data_ptr(), out_p.data_ptr(), n, out_normals_ptr=out_n.data_ptr(), stream=stream)

    # positions only: no normal is morphed or renormalised, so what "none active" costs over the plain
    # call there is the weight staging and the walk alone
    def shaped_none_positions():
        mesh.skin(skin.data_ptr(), out_p.data_ptr(), n, stream=stream, shape_weights_ptr=d_sets["none_active"].data_ptr())

    def plain_positions():
        mesh.skin(skin.data_ptr(), out_p.data_ptr(), n, stream=stream)

    cands = {"shaped_all_active": shaped("all_active"), "shaped_two_active": shaped("two_active"),
             "shaped_none_active": shaped("none_active"), "plain": plain, "fill": lambda: fill_buf.fill_(1.0),
             "copy": lambda: dst.copy_(src), "shaped_none_active_positions": shaped_none_positions,
             "plain_positions": plain_positions}
    # the timed code computes what the host code does (first two skeletons, all shapes active)
    cands["shaped_all_active"]()
    torch.cuda.synchronize(dev)
    ref_p, ref_n = skin_vertices_cpu(B, pos, idx, w, skin[:2].cpu().numpy(), normals=nrm, shape_positions=sp, shape_normals=sn,
                                     shape_weights=sets["all_active"][:2])
    same = bool(np.array_equal(out_p[:2].cpu().numpy().view(np.uint32), ref_p.view(np.uint32)) and
                np.array_equal(out_n[:2].cpu().numpy().view(np.uint32), ref_n.view(np.uint32)))
    assert same and bool(torch.isfinite(out_p).all()), "the device result differs from mbik_skin_vertices_shaped_cpu"
    for _ in range(warmup):
        for f in cands.values():
            f()
    torch.cuda.synchronize(dev)
    ms = {k: [] for k in cands}
    for _ in range(steps):
        for k, f in cands.items():   # alternating: shaped x 3, plain, fill, copy, the positions-only pair, shaped, ...
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            f()
            b.record()
            b.synchronize()
            ms[k].append(a.elapsed_time(b))
    med = {k: statistics.median(v) for k, v in ms.items()}
    S, chunks = mesh.launch_shape(n)
    mesh.close()
    plan.close()
    res = {"config": f"C{cfg}", "skeletons": n, "bones": B, "vertices": V, "influences": K, "normals": True, "shapes": SHAPES,
           "mode": "relative", "steps": steps, "warmup": warmup, "skeletons_per_block": S, "vertex_chunks": chunks,
           "output_bytes": out_bytes, "unfused_copy_bytes": unfused_bytes, "in_infinity_cache": out_bytes < 256 * 2 ** 20,
           "matches_cpu_bitwise": same}
    for k in cands:
        res[f"{k}_ms"] = med[k]
        res[f"{k}_ms_min_max"] = [min(ms[k]), max(ms[k])]
    lo, hi = min(ms["plain"]) / med["plain"], max(ms["plain"]) / med["plain"]
    res["plain_spread_over_median"] = [lo, hi]
    for k in ("all_active", "two_active", "none_active"):
        t = med[f"shaped_{k}"]
        res[f"{k}_shaped_over_plain"] = t / med["plain"]
        res[f"{k}_shaped_over_fill"] = t / med["fill"]
        res[f"{k}_shaped_over_unfused"] = t / (med["plain"] + med["copy"])   # unfused: the plain call plus the least morph traffic
    res["none_active_inside_plain_spread"] = bool(lo <= res["none_active_shaped_over_plain"] <= hi)
    res["none_active_positions_shaped_over_plain"] = med["shaped_none_active_positions"] / med["plain_positions"]
    # of what "none active" costs over the plain call: the walk and staging (positions only), the rest is the normals' side
    res["none_active_extra_ms"] = med["shaped_none_active"] - med["plain"]
    res["none_active_extra_ms_positions_only"] = med["shaped_none_active_positions"] - med["plain_positions"]
    res["fill_bytes_per_s"] = out_bytes / (med["fill"] * 1e-3)
    res["copy_bytes_per_s"] = 2 * unfused_bytes / (med["copy"] * 1e-3)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", default="0,1")
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(HERE, "profiles", "morph_bench.json"))
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("morph_bench needs a GPU (no CPU fallback)")
    res = {
        "what": "mbik_skin_vertices_shaped (16 dense shapes, relative mode, positions and normals; all / 2 of 16 / no weights "
                "active) vs mbik_skin_vertices on the same mesh vs a device fill of the output bytes vs a device copy of "
                "count x V x 32 bytes; medians of device-event times, candidates alternating in one process",
        "note": "shaped_over_unfused = shaped / (plain + copy): the copy is the least traffic an unfused morph pass would add "
                "(one morphed position and normal record a vertex, written and read once).  The 201 MB case sits inside the "
                "256 MiB Infinity Cache; only the 1.6 GB case speaks for HBM.",
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
