"""Times the tangent stream of mbik_skin_vertices_call against the calls it replaces, on the GPU, with device events
(DESIGN.md §22), by tools/skin_bench.py's protocol.

    python tools/skin_tangent_bench.py [--cases 0,1] [--steps 20] [--warmup 3] [--out profiles/skin_tangent_bench.json]

The cases are skin_bench.py's two that speak for HBM: C2 rig (32 bones), 4,096 skeletons x 8,192 vertices, K = 4, and C5 rig
(200 bones), 16,384 x 4,096 vertices, K = 8.  Meshes from skinning.synthetic_mesh with synthetic_tangents; the shaped mesh
adds 8 shapes (synthetic_shapes, synthetic_shape_tangents) and per-skeleton weights of which about a third are zero.  The
skin transforms are pose_globals' of the workload's poses with the rest pose's inverse bind.

Candidates, alternating inside one process after a warm-up, medians of `steps` with min and max:
  a   the existing positions + normals call (mbik_skin_vertices): the parent's kernels, the baseline
  b   mbik_skin_vertices_call with out_tangents
  c   what a user did before: a, plus a second existing call on a mesh whose normals are the tangents, into a second pair
      of buffers (the positions written twice; the sign not written at all)
  as  the shaped form of a (mbik_skin_vertices_shaped)
  d   b on the shaped mesh
Before anything is timed, three rows (the first, the middle and the last skeleton) of every candidate's outputs are compared
bitwise with mbik_skin_vertices_call_cpu.  Reported: b/a, b/c, d/as, and the bytes each call moves by the model
outputs + matrices in + the mesh once.  No threshold is fixed.  Needs a GPU: there is no CPU fallback.
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

# (config, skeletons, vertices, influences): skin_bench.py's C2 and C5 cases that do not fit the Infinity Cache
CASES = [(2, 4096, 8192, 4), (5, 16384, 4096, 8)]
SHAPES = 8


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    na, nb = np.isnan(a), np.isnan(b)
    return a.shape == b.shape and bool(np.array_equal(na, nb) and np.array_equal(a.view(np.uint32)[~na], b.view(np.uint32)[~nb]))


def measure(case, steps: int, warmup: int) -> dict:
    import torch
    from many_bone_ik_amd import workloads as W
    from many_bone_ik_amd.skinning import (Mesh, skin_vertices_cpu, synthetic_mesh, synthetic_shape_tangents, synthetic_shapes,
                                           synthetic_tangents)
    from many_bone_ik_amd.solver import Plan, pose_globals_cpu

    cfg, n, V, K = case
    dev = torch.device("cuda", 0)
    print(f"skin_tangent_bench: C{cfg} x {n} skeletons x {V} vertices, K={K}: generating", file=sys.stderr, flush=True)
    wl = W.generate(cfg, n)
    plan = Plan.from_workload(wl)
    parents = wl.topo.parents.tolist()
    B = wl.bone_count
    rest, _ = pose_globals_cpu(parents, [], wl.pose[:1])
    pos, nrm, idx, w = synthetic_mesh(parents, rest[0], V, K, seed=1)
    tan = synthetic_tangents(pos, nrm, seed=2)
    sp, sn = synthetic_shapes(pos, nrm, SHAPES, seed=3)
    stn = synthetic_shape_tangents(tan, SHAPES, seed=4)
    rng = np.random.default_rng(5)
    cw = rng.uniform(-0.3, 0.3, (n, SHAPES)).astype(np.float32)
    cw[rng.uniform(0.0, 1.0, cw.shape) < 0.33] = 0.0
    tan3 = np.ascontiguousarray(tan[:, :3])
    mesh_n = Mesh(B, pos, idx, w, normals=nrm)                                          # a
    mesh_t = Mesh(B, pos, idx, w, normals=nrm, tangents=tan)                            # b
    mesh_as_n = Mesh(B, pos, idx, w, normals=tan3)                                      # c's second call
    shaped = dict(shape_positions=sp, shape_normals=sn, shape_mode="relative")
    mesh_sn = Mesh(B, pos, idx, w, normals=nrm, **shaped)                               # as
    mesh_st = Mesh(B, pos, idx, w, normals=nrm, tangents=tan, shape_tangents=stn, **shaped)   # d

    pose = torch.from_numpy(wl.pose).to(dev)
    inv_bind = torch.from_numpy(inverse_bind(rest[0])).to(dev)
    skin = torch.empty((n, B, 12), dtype=torch.float32, device=dev)
    d_cw = torch.from_numpy(cw).to(dev)
    out_p, out_n = (torch.empty((n, V, 3), dtype=torch.float32, device=dev) for _ in range(2))
    out_t = torch.empty((n, V, 4), dtype=torch.float32, device=dev)
    out_p2, out_n2 = (torch.empty((n, V, 3), dtype=torch.float32, device=dev) for _ in range(2))
    stream = torch.cuda.current_stream(dev).cuda_stream
    plan.pose_globals(pose.data_ptr(), skin.data_ptr(), n, inv_bind_ptr=inv_bind.data_ptr(), stream=stream)
    torch.cuda.synchronize(dev)

    def a():
        mesh_n.skin(skin.data_ptr(), out_p.data_ptr(), n, out_normals_ptr=out_n.data_ptr(), stream=stream)

    def b():
        mesh_t.skin(skin.data_ptr(), out_p.data_ptr(), n, out_normals_ptr=out_n.data_ptr(), out_tangents_ptr=out_t.data_ptr(), stream=stream)

    def c():
        a()
        mesh_as_n.skin(skin.data_ptr(), out_p2.data_ptr(), n, out_normals_ptr=out_n2.data_ptr(), stream=stream)

    def a_shaped():
        mesh_sn.skin(skin.data_ptr(), out_p.data_ptr(), n, out_normals_ptr=out_n.data_ptr(), shape_weights_ptr=d_cw.data_ptr(), stream=stream)

    def d():
        mesh_st.skin(skin.data_ptr(), out_p.data_ptr(), n, out_normals_ptr=out_n.data_ptr(), out_tangents_ptr=out_t.data_ptr(),
                     shape_weights_ptr=d_cw.data_ptr(), stream=stream)

    cands = {"a": a, "b": b, "c": c, "a_shaped": a_shaped, "d": d}

    # three rows of every candidate against the _cpu entry, before anything is timed
    rows = [0, n // 2, n - 1]
    h_skin = skin[rows].cpu().numpy()
    ref = skin_vertices_cpu(B, pos, idx, w, h_skin, normals=nrm, tangents=tan)
    ref_s = skin_vertices_cpu(B, pos, idx, w, h_skin, normals=nrm, tangents=tan, shape_tangents=stn, shape_weights=cw[rows], **shaped)
    verified = {}
    for name, f in cands.items():
        for t in (out_p, out_n, out_t, out_p2, out_n2):
            t[rows] = float("nan")
        f()
        torch.cuda.synchronize(dev)
        want = ref_s if name in ("a_shaped", "d") else ref
        ok = same_bits(out_p[rows].cpu().numpy(), want[0]) and same_bits(out_n[rows].cpu().numpy(), want[1])
        if name in ("b", "d"):
            ok = ok and same_bits(out_t[rows].cpu().numpy(), want[2])
        if name == "c":   # the second call's normals are the tangents' xyz
            ok = ok and same_bits(out_p2[rows].cpu().numpy(), want[0]) and same_bits(out_n2[rows].cpu().numpy(), want[2][..., :3])
        verified[name] = bool(ok)
    if not all(verified.values()):
        sys.exit(f"skin_tangent_bench: a candidate's rows differ from mbik_skin_vertices_call_cpu: {verified}")

    print("skin_tangent_bench: timing", file=sys.stderr, flush=True)
    for _ in range(warmup):
        for f in cands.values():
            f()
    torch.cuda.synchronize(dev)
    ms = {k: [] for k in cands}
    for _ in range(steps):
        for k, f in cands.items():   # alternating: a, b, c, a_shaped, d, a, ...
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            f()
            e1.record()
            e1.synchronize()
            ms[k].append(e0.elapsed_time(e1))
    med = {k: statistics.median(v) for k, v in ms.items()}
    S, chunks = mesh_t.launch_shape(n)
    Ss, chunks_s = mesh_st.launch_shape(n)
    for m in (mesh_n, mesh_t, mesh_as_n, mesh_sn, mesh_st):
        m.close()
    plan.close()
    mesh_bytes = V * (32 + 6 * K)            # positions, normals, indices, weights
    matrices = n * B * 48
    model = {"a": n * V * 24 + matrices + mesh_bytes, "b": n * V * 40 + matrices + mesh_bytes + V * 16,
             "c": 2 * (n * V * 24 + matrices + mesh_bytes)}
    res = {"config": f"C{cfg}", "skeletons": n, "bones": B, "vertices": V, "influences": K, "shapes": SHAPES, "steps": steps,
           "warmup": warmup, "skeletons_per_block": S, "vertex_chunks": chunks, "shaped_skeletons_per_block": Ss,
           "shaped_vertex_chunks": chunks_s, "rows_verified_bitwise": verified, "model_bytes": model,
           "model_b_over_a": model["b"] / model["a"], "model_b_over_c": model["b"] / model["c"]}
    for k in cands:
        res[f"{k}_ms"] = med[k]
        res[f"{k}_ms_min_max"] = [min(ms[k]), max(ms[k])]
    res.update({"b_over_a": med["b"] / med["a"], "b_over_c": med["b"] / med["c"], "d_over_a_shaped": med["d"] / med["a_shaped"],
                "a_bytes_per_s": model["a"] / (med["a"] * 1e-3), "b_bytes_per_s": model["b"] / (med["b"] * 1e-3),
                "b_and_a_separate": max(ms["a"]) < min(ms["b"]) or max(ms["b"]) < min(ms["a"]),
                "b_and_c_separate": max(ms["b"]) < min(ms["c"]) or max(ms["c"]) < min(ms["b"]),
                "d_and_a_shaped_separate": max(ms["a_shaped"]) < min(ms["d"]) or max(ms["d"]) < min(ms["a_shaped"])})
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", default="0,1")
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(HERE, "profiles", "skin_tangent_bench.json"))
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("skin_tangent_bench needs a GPU (no CPU fallback)")
    res = {
        "what": "mbik_skin_vertices_call with out_tangents (b; d on a shaped mesh) vs the existing positions + normals call (a; a_shaped) "
                "vs two existing calls with the tangents passed as normals the second time (c); medians of device-event times, "
                "candidates alternating in one process, three rows of every candidate verified bitwise against the _cpu entry first",
        "note": "model_bytes counts a call's outputs, its skin transforms and the mesh once: 24 bytes written a vertex and skeleton for a, "
                "40 for b, 48 for c.  *_separate: the [min, max] intervals of the two candidates do not overlap.",
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
