"""The launch layout mbik_plan_get_info reports, for a matrix of plans and settings: the table two
builds of the library must agree on byte for byte when host-side layout code is refactored.

    [MBIK_LIB_OVERRIDE=other/libmbik.so] python tools/layout_table.py OUT.json

Rigs: C1-C5, C3 in constraint_mode, C2 with a stabilization pass; counts 6, 48 and 16384.  On each
plan every setter at each of its legal values (mbik_plan_set_layout: a handful), one at a time from
the automatic state, plus the pinned layouts of tests/test_gpu_layouts.py's full-size test.  Per
setting three reports: right after the setter (no launch yet), after a whole-plan solve, and after
a sub-range solve of another count.  A setting the plan refuses is recorded with its error."""
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

from many_bone_ik_amd import _lib  # noqa: E402
from many_bone_ik_amd import workloads as W  # noqa: E402
from many_bone_ik_amd.solver import Plan  # noqa: E402

FIELDS = ("lanes_per_skeleton", "skeletons_per_block", "lds_bytes_per_block", "checkpoint_interval", "heading_staging",
          "state_placement", "waves_per_simd", "helper_wave", "wave_roles", "device_bytes")
RIGS = [("c1", 1, {}), ("c2", 2, {}), ("c3", 3, {}), ("c4", 4, {}), ("c5", 5, {}),
        ("c3_constraint_mode", 3, {"constraint_mode": True}), ("c2_stab1", 2, {"stabilization_passes": 1})]
COUNTS = (6, 48, 16384)


def settings():
    out = [("auto", [])]
    out += [(f"launch{k}", [("set_launch", k)]) for k in (1, 2, 4, 8, 16, 32, 64)]
    out += [(f"layout{a}_{b}_{c}", [("set_layout", a, b, c)])
            for a, b, c in ((0, 1, 0), (0, 3, 0), (0, 64, 0), (0, 0, 1), (0, 0, 2), (0, 0, 3), (0, 0, 1 << 20), (2, 5, 2), (4, 8, 1))]
    out += [(f"staging{s}", [("set_heading_staging", s)]) for s in range(0, 6)]
    out += [(f"placement{s}", [("set_locals_placement", s)]) for s in (0, 1, 2)]
    out += [(f"waves{s}", [("set_waves_per_simd", s)]) for s in (1, 2)]
    out += [(f"helper{s}", [("set_helper_wave", s)]) for s in (0, 1)]
    out += [(f"roles{s}", [("set_wave_roles", s)]) for s in (0, 1)]
    out += [("tab64", [("set_table_addressing", 1)])]
    for lanes, spw, interval, staging, placement, waves in ((8, 8, 2, 4, 2, 2), (8, 8, 1, 0, 2, 2), (8, 8, 1, 4, 2, 2), (4, 16, 1, 4, 2, 2)):
        out.append((f"pinned{lanes}_{spw}_{interval}_{staging}_{placement}_{waves}",
                    [("set_layout", lanes, spw, interval), ("set_heading_staging", staging), ("set_locals_placement", placement),
                     ("set_waves_per_simd", waves)]))
    return out


def reset(plan):
    plan.set_layout(0, 0, 0)
    plan.set_heading_staging(-1)
    plan.set_locals_placement(-1)
    plan.set_waves_per_simd(-1)
    plan.set_helper_wave(-1)
    plan.set_wave_roles(-1)
    plan.set_table_addressing(0)


def report(plan):
    info = plan.info()
    return [int(info[f]) for f in FIELDS]


def main(out_path):
    dev = torch.device("cuda", 0)
    table = {"fields": list(FIELDS), "plans": {}}
    for name, cfg, kw in RIGS:
        for n in COUNTS:
            wl = W.generate(cfg, n)
            plan = Plan.from_workload(wl, **kw)
            pi = torch.from_numpy(wl.pose).to(dev)
            tg = torch.from_numpy(wl.targets).to(dev)
            po = torch.empty_like(pi)
            sub = (1, 3) if n == 6 else (1, n // 2 + 1)
            rows = {}
            for label, calls in settings():
                reset(plan)
                for call in calls:
                    getattr(plan, call[0])(*call[1:])
                row = [report(plan)]
                for first, count in ((0, n), sub):
                    try:
                        plan.solve(pi[first:].data_ptr(), tg[first:].data_ptr(), po[first:].data_ptr(), first, count)
                        torch.cuda.synchronize()
                        row.append(report(plan))
                    except _lib.MbikError as e:
                        row.append({"error": e.code, "message": str(e)})
                rows[label] = row
            table["plans"][f"{name}_n{n}"] = rows
            print(f"{name} n={n}: {len(rows)} settings", flush=True)
            plan.close()
    with open(out_path, "w") as f:
        f.write(json.dumps(table, sort_keys=True, separators=(",", ":")).replace('],"', '],\n"') + "\n")


if __name__ == "__main__":
    main(sys.argv[1])
