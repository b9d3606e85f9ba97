"""Counter run of mbik_skin_vertices_shaped's kernel: the program that `rocprofv3 --pmc`
profiles, and the summary of its counter files.

    rocprofv3 --pmc <counters> -d DIR -o run --output-format csv -- python tools/morph_pmc.py --run 1 [--weights all_active]
    python tools/morph_pmc.py --sum DIR [DIR ...] --out profiles/morph_pmc.json

--run builds tools/morph_bench.py's case (same mesh, shapes, weights and skin transforms) and launches
the shaped call three times after one warm-up launch; nothing else of the library runs in between.
Counters are collected alone, one group per process, never together with tracing.  --sum adds up
every counter over the dispatches of mbik_skin_shaped_kernel found under the directories and divides
by the number of dispatches seen for that counter.
"""
from __future__ import annotations

import argparse
import csv
import glob
import json
import os
import sys
from collections import defaultdict

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if HERE not in sys.path:
    sys.path.insert(0, HERE)

KERNEL = "mbik_skin_shaped_kernel"


def run(case_index: int, weights: str, launches: int) -> None:
    import torch
    from many_bone_ik_amd import workloads as W
    from many_bone_ik_amd.skinning import Mesh, synthetic_mesh, synthetic_shapes
    from many_bone_ik_amd.solver import Plan, pose_globals_cpu
    from tools.morph_bench import CASES, SHAPES, weight_sets
    from tools.skin_bench import inverse_bind

    cfg, n, V, K = CASES[case_index]
    dev = torch.device("cuda", 0)
    wl = W.generate(cfg, n)
    plan = Plan.from_workload(wl)
    parents, B = wl.topo.parents.tolist(), wl.bone_count
    rest, _ = pose_globals_cpu(parents, [], wl.pose[:1])
    pos, nrm, idx, w = synthetic_mesh(parents, rest[0], V, K, seed=1)
    sp, sn = synthetic_shapes(pos, nrm, SHAPES, seed=2)
    mesh = Mesh(B, pos, idx, w, normals=nrm, shape_positions=sp, shape_normals=sn)
    pose = torch.from_numpy(wl.pose).to(dev)
    inv_bind = torch.from_numpy(inverse_bind(rest[0])).to(dev)
    skin = torch.empty((n, B, 12), dtype=torch.float32, device=dev)
    out_p = torch.empty((n, V, 3), dtype=torch.float32, device=dev)
    out_n = torch.empty((n, V, 3), dtype=torch.float32, device=dev)
    d_c = torch.from_numpy(weight_sets(n, seed=3)[weights]).to(dev)
    stream = torch.cuda.current_stream(dev).cuda_stream
    plan.pose_globals(pose.data_ptr(), skin.data_ptr(), n, inv_bind_ptr=inv_bind.data_ptr(), stream=stream)
    for _ in range(1 + launches):
        mesh.skin(skin.data_ptr(), out_p.data_ptr(), n, out_normals_ptr=out_n.data_ptr(), stream=stream, shape_weights_ptr=d_c.data_ptr())
        torch.cuda.synchronize(dev)
    assert bool(torch.isfinite(out_p).all())
    mesh.close()
    plan.close()
    print(json.dumps({"case": f"C{cfg} x {n} x {V}, K={K}, P={SHAPES}", "weights": weights, "launches": 1 + launches}))


def summarise(dirs, out: str, note: str) -> None:
    total, seen = defaultdict(float), defaultdict(int)
    for d in dirs:
        for path in glob.glob(os.path.join(d, "**", "*counter_collection.csv"), recursive=True):
            for row in csv.DictReader(open(path)):
                if KERNEL not in row.get("Kernel_Name", ""):
                    continue
                total[row["Counter_Name"]] += float(row["Counter_Value"])
                seen[row["Counter_Name"]] += 1
    per = {k: total[k] / seen[k] for k in sorted(total)}
    res = {"what": f"rocprofv3 --pmc (counters alone, no tracing; one group per process) over the launches of {KERNEL}; "
                   "mean per launch, summed over the device", "note": note, "dispatches_seen": dict(sorted(seen.items())),
           "per_launch": per}
    with open(out, "w") as fh:
        json.dump(res, fh, indent=1)
        fh.write("\n")
    print(json.dumps(res))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--run", type=int, default=None, help="index into tools/morph_bench.py's CASES")
    ap.add_argument("--weights", default="all_active", choices=["all_active", "two_active", "none_active"])
    ap.add_argument("--launches", type=int, default=3)
    ap.add_argument("--sum", nargs="+", default=None)
    ap.add_argument("--out", default=os.path.join(HERE, "profiles", "morph_pmc.json"))
    ap.add_argument("--note", default="")
    args = ap.parse_args()
    if args.sum:
        summarise(args.sum, args.out, args.note)
    elif args.run is not None:
        run(args.run, args.weights, args.launches)
    else:
        ap.error("--run or --sum")


if __name__ == "__main__":
    main()
