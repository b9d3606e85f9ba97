"""Times mbik_skin_vertices (Mesh.skin) against a device fill and a device-to-device copy of its
output byte count, against mbik_pose_globals and against one solve step, on the GPU, with device
events.

    python tools/skin_bench.py [--cases 0,1,2,3] [--steps 20] [--warmup 3] [--out profiles/skin_bench.json]

The cases: C2 rig (32 bones), 4,096 skeletons x 2,048 vertices, K = 4 -- 100 MB of output, inside
the 256 MiB Infinity Cache, so it says nothing about HBM; C2, 4,096 x 8,192 vertices with normals,
805 MB; C5 rig (200 bones), 16,384 x 4,096 vertices, K = 8, 805 MB -- these two speak for HBM;
C2, 8 skeletons x 262,144 vertices, the vertex-split grid.  The meshes come from
skinning.synthetic_mesh (neighbouring vertices share bones), the skin transforms from the solved
poses through pose_globals with the rest pose's inverse bind.

Per case the candidates alternate inside one process after a warm-up: Mesh.skin; torch's fill of a
buffer of the output's size (write-only: the kernel's roof); torch's copy of such a buffer (reads
and writes it: twice the traffic); pose_globals with inv_bind; plan.solve after plan.autotune.
Medians with min and max; no threshold is fixed.  Needs a GPU: there is no CPU fallback.
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

# (config, skeletons, vertices, influences, normals)
CASES = [(2, 4096, 2048, 4, False), (2, 4096, 8192, 4, True), (5, 16384, 4096, 8, False), (2, 8, 262144, 4, False)]


def inverse_bind(rest: np.ndarray) -> np.ndarray:
    """[bones][12] affine inverses of the rest globals (basis rows, origin), through float64."""
    r = rest.astype(np.float64)
    basis = np.linalg.inv(r[:, :9].reshape(-1, 3, 3))
    origin = -np.einsum("bij,bj->bi", basis, r[:, 9:])
    return np.concatenate([basis.reshape(-1, 9), origin], axis=1).astype(np.float32)


def measure(case, steps: int, warmup: int) -> dict:
    import torch
    from many_bone_ik_amd import workloads as W
    from many_bone_ik_amd.skinning import Mesh, synthetic_mesh
    from many_bone_ik_amd.solver import Plan, pose_globals_cpu

    cfg, n, V, K, normals = case
    dev = torch.device("cuda", 0)
    print(f"skin_bench: C{cfg} x {n} skeletons x {V} vertices, K={K}: generating", file=sys.stderr, flush=True)
    wl = W.generate(cfg, n)
    plan = Plan.from_workload(wl)
    parents = wl.topo.parents.tolist()
    B = wl.bone_count
    rest, _ = pose_globals_cpu(parents, [], wl.pose[:1])
    pos, nrm, idx, w = synthetic_mesh(parents, rest[0], V, K, seed=1)
    mesh = Mesh(B, pos, idx, w, normals=nrm if normals else None)
    print("skin_bench: timing", file=sys.stderr, flush=True)
    pose_in = torch.from_numpy(wl.pose).to(dev)
    targets = torch.from_numpy(wl.targets).to(dev)
    pose_out = torch.empty_like(pose_in)
    inv_bind = torch.from_numpy(inverse_bind(rest[0])).to(dev)
    skin = torch.empty((n, B, 12), dtype=torch.float32, device=dev)
    out_p = torch.empty((n, V, 3), dtype=torch.float32, device=dev)
    out_n = torch.empty((n, V, 3), dtype=torch.float32, device=dev) if normals else None
    out_bytes = n * V * 12 * (2 if normals else 1)
    fill_buf = torch.empty(out_bytes // 4, dtype=torch.float32, device=dev)
    src = torch.empty(out_bytes // 4, dtype=torch.float32, device=dev).normal_()
    dst = torch.empty_like(src)
    plan.autotune(pose_in.data_ptr(), targets.data_ptr(), pose_out.data_ptr())   # the solve as bench.py times it
    stream = torch.cuda.current_stream(dev).cuda_stream

    def solve():
        plan.solve(pose_in.data_ptr(), targets.data_ptr(), pose_out.data_ptr(), stream=stream)

    def fk():
        plan.pose_globals(pose_out.data_ptr(), skin.data_ptr(), n, inv_bind_ptr=inv_bind.data_ptr(), stream=stream)

    def do_skin():
        mesh.skin(skin.data_ptr(), out_p.data_ptr(), n, out_normals_ptr=out_n.data_ptr() if normals else 0, stream=stream)

    def fill():
        fill_buf.fill_(1.0)

    def copy():
        dst.copy_(src)

    cands = {"skin": do_skin, "fill": fill, "copy": copy, "pose_globals": fk, "solve": solve}
    solve()
    fk()
    for _ in range(warmup):
        for f in cands.values():
            f()
    torch.cuda.synchronize(dev)
    assert bool(torch.isfinite(out_p).all())
    ms = {k: [] for k in cands}
    for _ in range(steps):
        for k, f in cands.items():   # alternating: skin, fill, copy, pose_globals, solve, skin, ...
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            f()
            b.record()
            b.synchronize()
            ms[k].append(a.elapsed_time(b))
    med = {k: statistics.median(v) for k, v in ms.items()}
    info = plan.info()
    S, chunks = mesh.launch_shape(n)
    mesh_bytes = V * (16 * (2 if normals else 1) + 2 * K + 4 * K)
    skin_bytes = out_bytes + n * B * 48 + mesh_bytes   # outputs, matrices in, the mesh once
    mesh.close()
    plan.close()
    res = {"config": f"C{cfg}", "skeletons": n, "bones": B, "vertices": V, "influences": K, "normals": normals,
           "steps": steps, "warmup": warmup, "skeletons_per_block": S, "vertex_chunks": chunks,
           "output_bytes": out_bytes, "in_infinity_cache": out_bytes < 256 * 2 ** 20}
    for k in cands:
        res[f"{k}_ms"] = med[k]
        res[f"{k}_ms_min_max"] = [min(ms[k]), max(ms[k])]
    res.update({
        "skin_over_fill": med["skin"] / med["fill"], "skin_over_copy": med["skin"] / med["copy"],
        "skin_over_solve": med["skin"] / med["solve"], "skin_over_pose_globals": med["skin"] / med["pose_globals"],
        "skin_bytes": skin_bytes, "skin_bytes_per_s": skin_bytes / (med["skin"] * 1e-3),
        "fill_bytes_per_s": out_bytes / (med["fill"] * 1e-3),
        "copy_bytes_per_s": 2 * out_bytes / (med["copy"] * 1e-3),   # the copy reads and writes its buffer
        "solve_layout": f"autotuned: lanes {info['lanes_per_skeleton']}, skeletons/block {info['skeletons_per_block']}, "
                        f"placement {info['state_placement']}, wave roles {info['wave_roles']}",
    })
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", default="0,1,2,3")
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(HERE, "profiles", "skin_bench.json"))
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("skin_bench needs a GPU (no CPU fallback)")
    res = {
        "what": "mbik_skin_vertices vs a device fill and a device-to-device copy of its output byte count vs mbik_pose_globals "
                "(with inv_bind) vs one autotuned mbik_solve step; medians of device-event times, candidates alternating in "
                "one process",
        "note": "The 100 MB case sits inside the 256 MiB Infinity Cache; only the 805 MB cases speak for HBM. "
                "skin_bytes_per_s counts the call's own bytes once (outputs + skin transforms in + the mesh once); "
                "fill_bytes_per_s counts the fill's writes, copy_bytes_per_s the copy's read and write.",
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
