"""The host side's launch decision (pins -> LayoutRequest -> build_schedule -> SolveLaunch,
DESIGN.md "Launch layout") seen from outside:

* a launch does not change the plan: a sub-range solve of another count leaves mbik_plan_get_info
  as it was, and the next whole-plan solve is bitwise what a fresh plan with the same pins gives;
* the non-finite flag buffer of mbik_solve_checked is used by that call alone;
* the layout a small pinned plan reports is the one recorded in tests/golden/layout_info_small.json
  (written by the library before the layout code was gathered in one place: record_golden()).
Needs an MI355X: -m gpu."""
import json
import os

import numpy as np
import pytest

from many_bone_ik_amd import workloads as W
from many_bone_ik_amd.solver import Plan

from .test_gpu_layout_limits import fan_rig

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "layout_info_small.json")
GOLDEN_FIELDS = ("lanes_per_skeleton", "skeletons_per_block", "checkpoint_interval", "heading_staging", "state_placement",
                 "waves_per_simd", "wave_roles", "helper_wave", "lds_bytes_per_block")

# C1 x 8 and C5 x 6: the launches fit the chip, so the occupancy query cannot change the answer
RIGS = {
    "c1": lambda: (W.generate(1, 8, first=3), {}),
    "c5": lambda: (W.generate(5, 6, first=5), {}),
    "c5_constraint_mode": lambda: (W.generate(5, 6, first=5), {"constraint_mode": True}),
    "c5_stab1": lambda: (W.generate(5, 6, first=5), {"stabilization_passes": 1}),
    "fan40": lambda: (W.generate(22, 6, topo=fan_rig(40)), {}),
}


def apply_pins(plan, pins):
    for call in pins:
        getattr(plan, call[0])(*call[1:])


def reset_pins(plan):
    apply_pins(plan, [("set_layout", 0, 0, 0), ("set_heading_staging", -1), ("set_locals_placement", -1),
                      ("set_waves_per_simd", -1), ("set_helper_wave", -1), ("set_wave_roles", -1), ("set_table_addressing", 0)])


LAY, STG, LOC, WAV, HLP, ROL, TAB = ("set_layout", "set_heading_staging", "set_locals_placement", "set_waves_per_simd",
                                     "set_helper_wave", "set_wave_roles", "set_table_addressing")
# label -> (rig, setter calls): every setter, and the two fall-backs of wave roles (a stabilized
# plan; a block that exceeds the LDS, as test_many_pins_wave_roles_pinned_falls_back)
GOLDEN_ROWS = {
    "c1_auto": ("c1", []),
    "c1_launch4": ("c1", [("set_launch", 4)]),
    "c1_layout_spw3": ("c1", [(LAY, 0, 3, 0)]),
    "c1_layout_interval2": ("c1", [(LAY, 0, 0, 2)]),
    "c1_staging0": ("c1", [(STG, 0)]),
    "c1_placement1": ("c1", [(LOC, 1)]),
    "c1_placement2": ("c1", [(LOC, 2)]),
    "c1_waves2": ("c1", [(WAV, 2)]),
    "c1_helper1": ("c1", [(HLP, 1)]),
    "c1_roles1": ("c1", [(ROL, 1)]),
    "c1_tab64": ("c1", [(TAB, 1)]),
    "c5_auto": ("c5", []),
    "c5_launch4": ("c5", [("set_launch", 4)]),
    "c5_launch16": ("c5", [("set_launch", 16)]),
    "c5_layout_8_4_2": ("c5", [(LAY, 8, 4, 2)]),
    "c5_layout_no_checkpoints": ("c5", [(LAY, 0, 0, 1 << 20)]),
    "c5_staging0": ("c5", [(STG, 0)]),
    "c5_staging2": ("c5", [(STG, 2)]),
    "c5_staging3": ("c5", [(STG, 3)]),
    "c5_staging4_waves2": ("c5", [(STG, 4), (WAV, 2)]),
    "c5_staging5_waves2": ("c5", [(STG, 5), (WAV, 2)]),
    "c5_staging4_waves2_tab64": ("c5", [(STG, 4), (WAV, 2), (TAB, 1)]),
    "c5_staging5_waves2_tab64": ("c5", [(STG, 5), (WAV, 2), (TAB, 1)]),
    "c5_placement1": ("c5", [(LOC, 1)]),
    "c5_placement2": ("c5", [(LOC, 2)]),
    "c5_waves2": ("c5", [(WAV, 2)]),
    "c5_helper1": ("c5", [(HLP, 1)]),
    "c5_helper1_lanes4": ("c5", [(HLP, 1), (LAY, 4, 2, 0)]),
    "c5_roles1": ("c5", [(ROL, 1)]),
    "c5_roles1_lanes8_waves2": ("c5", [(ROL, 1), (LAY, 8, 0, 0), (WAV, 2)]),
    "c5_roles1_spw16": ("c5", [(ROL, 1), (LAY, 0, 16, 2)]),
    "c5_tab64": ("c5", [(TAB, 1)]),
    "c5_pinned_8_8_2_4_2_2": ("c5", [(LAY, 8, 8, 2), (STG, 4), (LOC, 2), (WAV, 2)]),
    "cm_auto": ("c5_constraint_mode", []),
    "cm_launch8": ("c5_constraint_mode", [("set_launch", 8)]),
    "cm_spw4": ("c5_constraint_mode", [(LAY, 0, 4, 0)]),
    "cm_roles1": ("c5_constraint_mode", [(ROL, 1)]),
    "cm_roles1_lanes8_spw16": ("c5_constraint_mode", [(ROL, 1), (LAY, 8, 16, 0)]),
    "stab_roles1_falls_back": ("c5_stab1", [(ROL, 1)]),
    "stab_waves2": ("c5_stab1", [(WAV, 2)]),
    "fan40_roles1_falls_back": ("fan40", [(LAY, 4, 0, 0), (WAV, 2), (ROL, 1)]),
}


class Rig:
    def __init__(self, name):
        import torch
        self.wl, self.kw = RIGS[name]()
        dev = torch.device("cuda", 0)
        self.torch = torch
        self.pi = torch.from_numpy(self.wl.pose).to(dev)
        self.tg = torch.from_numpy(self.wl.targets).to(dev)

    def plan(self, pins=()):
        plan = Plan.from_workload(self.wl, **self.kw)
        apply_pins(plan, pins)
        return plan

    def solve(self, plan, first=0, count=None, flags=None):
        """One solve of [first, first + count) into a fresh NaN-filled buffer of the whole batch."""
        po = self.torch.full_like(self.pi, float("nan"))
        args = (self.pi[first:].data_ptr(), self.tg[first:].data_ptr(), po[first:].data_ptr())
        if flags is None:
            plan.solve(*args, first, count)
        else:
            plan.solve_checked(*args, flags.data_ptr(), first, count)
        self.torch.cuda.synchronize()
        return po.cpu().numpy().view(np.uint32)


def measure_rows(rig_name):
    """{label: GOLDEN_FIELDS' values after a whole-plan solve} for the rig's rows, on one plan."""
    rig = Rig(rig_name)
    plan = rig.plan()
    out = {}
    for label, (name, pins) in GOLDEN_ROWS.items():
        if name != rig_name:
            continue
        reset_pins(plan)
        apply_pins(plan, pins)
        rig.solve(plan)
        info = plan.info()
        out[label] = [int(info[f]) for f in GOLDEN_FIELDS]
    return out


def record_golden(path=GOLDEN):
    """Writes the golden file from the loaded library (run with the parent revision's build)."""
    rows = {}
    for name in RIGS:
        rows.update(measure_rows(name))
    with open(path, "w") as f:
        json.dump({"fields": GOLDEN_FIELDS, "rows": rows}, f, indent=0, sort_keys=True)
        f.write("\n")


@pytest.mark.parametrize("rig_name", list(RIGS))
def test_pinned_small_layouts_match_the_record(mbik, rig_name):
    with open(GOLDEN) as f:
        golden = json.load(f)
    assert tuple(golden["fields"]) == GOLDEN_FIELDS
    got = measure_rows(rig_name)
    assert got, rig_name
    for label, values in got.items():
        assert dict(zip(GOLDEN_FIELDS, values)) == dict(zip(GOLDEN_FIELDS, golden["rows"][label])), label


LAUNCH_CASES = {
    "classic": ("c5", []),
    "placement2": ("c5", [(LOC, 2)]),
    "wave_roles": ("c5", [(ROL, 1)]),
    "helper_wave": ("c5", [(HLP, 1), (LAY, 4, 2, 0)]),
    "constraint_mode": ("c5_constraint_mode", []),
    "constraint_mode_roles": ("c5_constraint_mode", [(ROL, 1)]),
}


@pytest.mark.parametrize("case", list(LAUNCH_CASES))
def test_a_launch_does_not_change_the_plan(mbik, case):
    """A solve of skeletons [1, 4) between two whole-plan solves: the reported layout stays, and the
    second whole-plan solve is bitwise a fresh plan's.  constraint_mode results depend on the frames
    a skeleton has seen (its node caches), so there the fresh plan runs the same frames, the
    sub-range one as three single-skeleton launches."""
    rig_name, pins = LAUNCH_CASES[case]
    rig = Rig(rig_name)
    cm = bool(rig.kw.get("constraint_mode"))
    a = rig.plan(pins)
    first_a = rig.solve(a)
    info = a.info()
    assert info["wave_roles"] == (1 if "roles" in case else 0) and info["helper_wave"] == (1 if case == "helper_wave" else 0)
    sub = rig.solve(a, 1, 3)
    assert a.info() == info
    again = rig.solve(a)
    b = rig.plan(pins)
    if cm:
        assert np.array_equal(rig.solve(b), first_a)
        for s in (1, 2, 3):
            assert np.array_equal(rig.solve(b, s, 1)[s], sub[s])
    assert np.array_equal(rig.solve(b), again)
    assert b.info() == info


@pytest.mark.parametrize("rig_name", ["c5", "c5_constraint_mode", "c1"])
def test_nonfinite_flags_belong_to_their_call(mbik, rig_name):
    """mbik_solve_checked's flag buffer is not kept by the plan: a plain mbik_solve afterwards leaves
    every byte of the (still allocated) buffer alone and computes the same poses as a checked
    call with the same history -- a second plan's second checked frame."""
    rig = Rig(rig_name)
    n = rig.wl.pose.shape[0]
    a, b = rig.plan(), rig.plan()
    flags = rig.torch.full((n,), 0x55, dtype=rig.torch.uint8, device=rig.pi.device)
    frame1 = rig.solve(a, flags=flags)
    assert not flags.cpu().numpy().any()             # finite inputs: every flag written, as 0
    flags.fill_(0xAB)
    frame2 = rig.solve(a)
    assert (flags.cpu().numpy() == 0xAB).all()
    fb = rig.torch.zeros_like(flags)
    assert np.array_equal(rig.solve(b, flags=fb), frame1)
    assert np.array_equal(rig.solve(b, flags=fb), frame2)
    if not rig.kw.get("constraint_mode"):
        assert np.array_equal(frame2, frame1)
