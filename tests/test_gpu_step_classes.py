"""Row-uniform bone-step classes (csrc/plan.h StepClassShape): where every role of a schedule row
has a step of one shape, the one-wave kernels run a bone_step with the shape's topology tests
compiled in; everywhere else the general one.  Same operations either way, so every solve stays
bitwise equal to the oracle.  The host classification is checked without a GPU; the solves need
an MI355X (-m gpu)."""
import math

import numpy as np
import pytest

from many_bone_ik_amd import workloads as W
from many_bone_ik_amd.solver import Plan, describe_step_classes

from .test_gpu_parity import assert_parity

gpu = pytest.mark.gpu
ITER = 3
TWIST = (0.0, 2.0 * math.pi)


def _rig(lengths, cones=2):
    """Chains of the given lengths under one root bone, every chain bone constrained."""
    parents, pins = [-1], []
    for n in lengths:
        p = 0
        for _ in range(n):
            parents.append(p)
            p = len(parents) - 1
        pins.append(p)
    return W.custom_topology(parents, pins, np.arange(1, len(parents)), cones_per_bone=cones, twist=TWIST, iterations=ITER)


def _uneven(n=9):
    """Chains of 3, 2, 2 and 1 bones: the roles run out of steps at different step indices."""
    return W.generate(12, n, topo=_rig((3, 2, 2, 1)))


def _mixed_kinds(n=9):
    """Four chains of three bones that differ in kind: unconstrained; constrained without cones (only
    the twist limit acts: a Kusudama constraint always sets both the swing and the twist flag, so
    'swing only' and 'twist only' are not separate flag sets here); one cone; two cones."""
    topo = _rig((3, 3, 3, 3))
    topo.constrained = np.arange(4, 13, dtype=np.int32)   # chain 0 (bones 1-3) unconstrained
    wl = W.generate(13, n, topo=topo)
    wl.cone_count = np.array([0, 0, 0, 1, 1, 1, 2, 2, 2], np.int32)
    return wl


def _partly_uniform(n=9):
    """Four chains of four bones, two cones everywhere but on one bone of one chain: that step index
    is class 0, the row's other steps keep their class."""
    wl = W.generate(14, n, topo=_rig((4, 4, 4, 4)))
    cc = np.full(16, 2, np.int32)
    cc[list(wl.topo.constrained).index(6)] = 1            # chain 1's second bone from its root
    wl.cone_count = cc
    return wl


def _classes(wl, lanes=0):
    return [c.tolist() for c in describe_step_classes(wl.topo.parents, wl.pins(), wl.constraints(), lanes=lanes)]


def test_host_classification():
    """C2's chain row: the tips' step is the pinned class, every other step the chain class --
    also the eighth, which the 7-bone chain lacks; the single-bone translating root row is general."""
    assert _classes(W.generate(2, 1)) == [[2, 1, 1, 1, 1, 1, 1, 1], [0]]
    # unconstrained chains (C3) match no shape
    assert _classes(W.generate(3, 1)) == [[0] * 8, [0]]
    # roles running out of steps at different indices do not break uniformity
    assert _classes(_uneven(1)) == [[2, 1, 1], [0]]
    # roles that disagree: class 0
    assert _classes(_mixed_kinds(1)) == [[0, 0, 0], [0]]
    # tip, then bones 3, 2 (the odd one among them), 1 of each chain
    assert _classes(_partly_uniform(1)) == [[2, 1, 0, 1], [0]]


_REF = {}


def _ref(oracle, key, make):
    """One oracle solve per rig, shared by the cases that slice it."""
    if key not in _REF:
        wl = make()
        _REF[key] = (wl, oracle.Oracle(wl, iterations=ITER).solve(wl.pose, wl.targets, threads=8))
    return _REF[key]


def _solve(wl, helper, lanes=0):
    plan = Plan.from_workload(wl, iterations=ITER)
    if lanes:
        plan.set_layout(lanes, 0, 0)
    plan.set_helper_wave(helper)
    got = plan.solve_host(wl.pose, wl.targets)
    # (64 one-lane skeletons a block leave no LDS for the helper's ring: that launch runs without it)
    assert plan.info()["helper_wave"] == (helper if not lanes else 0)
    return plan, got


@gpu
@pytest.mark.parametrize("helper", [1, 0])
@pytest.mark.parametrize("n", [1, 15, 17, 33])
def test_c2_sizes(oracle, mbik, n, helper):
    """A partly filled group, a partly filled block and a second block (16 skeletons a block)."""
    _, ref = _ref(oracle, "c2", lambda: W.generate(2, 33))
    wl = W.generate(2, n)
    plan, got = _solve(wl, helper)
    assert [c.tolist() for c in plan.step_classes()] == [[2, 1, 1, 1, 1, 1, 1, 1], [0]]
    assert_parity(got, ref[:n], f"C2 n={n} helper={helper}")


@gpu
@pytest.mark.parametrize("helper", [1, 0])
def test_c2_other_priorities(oracle, mbik, helper):
    """Non-default effector priorities: the run-time heading slots (PM = 0) with the classes."""
    def make():
        wl = W.generate(2, 17)
        wl.pin_priority = np.tile(np.array([0.3, 0.5, 0.1], np.float32), (4, 1))
        return wl
    wl, ref = _ref(oracle, "c2_prio", make)
    plan, got = _solve(wl, helper)
    assert plan.info()["heading_slots"] == 0
    assert_parity(got, ref, f"C2 priorities helper={helper}")


@gpu
@pytest.mark.parametrize("helper", [1, 0])
@pytest.mark.parametrize("rig", ["uneven", "mixed_kinds", "partly_uniform"])
def test_rigs(oracle, mbik, rig, helper):
    make = {"uneven": _uneven, "mixed_kinds": _mixed_kinds, "partly_uniform": _partly_uniform}[rig]
    wl, ref = _ref(oracle, rig, make)
    plan, got = _solve(wl, helper)
    assert [c.tolist() for c in plan.step_classes()] == _classes(wl)
    assert_parity(got, ref, f"{rig} helper={helper}")


@gpu
def test_c2_one_lane_packed_level(oracle, mbik):
    """One lane per skeleton: the four chains run back to back as a packed level, whose lanes are
    at different steps, so the classic kernel keeps them on the general step."""
    _, ref = _ref(oracle, "c2", lambda: W.generate(2, 33))
    plan, got = _solve(W.generate(2, 17), 0, lanes=1)
    assert_parity(got, ref[:17], "C2 one lane")


@gpu
@pytest.mark.parametrize("helper", [1, 0])
def test_c2_segment_solve(oracle, mbik, helper):
    """mbik_segment_solve masks the roles outside its segment: the one role left runs the row's class."""
    import torch
    dev = torch.device("cuda", 0)
    wl = W.generate(2, 17)
    o = oracle.Oracle(wl)
    plan = Plan.from_workload(wl)
    plan.set_helper_wave(helper)
    for seg in (0, 3, plan.info()["segment_count"] - 1):
        ref = o.segment_solve(seg, wl.pose, wl.targets)
        pose = torch.from_numpy(wl.pose.copy()).to(dev)
        tg = torch.from_numpy(wl.targets).to(dev)
        plan.segment_solve(seg, pose.data_ptr(), tg.data_ptr())
        torch.cuda.synchronize()
        assert_parity(pose.cpu().numpy(), ref, f"C2 segment {seg} helper={helper}")


@gpu
def test_saved_plan_rebuilds_classes(oracle, mbik):
    """The classes are derived data: a loaded plan has them again and solves the same bits."""
    wl, ref = _ref(oracle, "partly_uniform", _partly_uniform)
    plan, _ = _solve(wl, 1)
    loaded = Plan.load(plan.save())
    assert [c.tolist() for c in loaded.step_classes()] == [[2, 1, 0, 1], [0]]
    assert_parity(loaded.solve_host(wl.pose, wl.targets), ref, "loaded plan")
    loaded.close()


@gpu
@pytest.mark.parametrize("helper", [1, 0])
def test_c2_realistic_rest(oracle, mbik, helper):
    wl, ref = _ref(oracle, "c2_realistic", lambda: W.generate(2, 17, rest="realistic"))
    _, got = _solve(wl, helper)
    assert_parity(got, ref, f"C2 realistic helper={helper}")
