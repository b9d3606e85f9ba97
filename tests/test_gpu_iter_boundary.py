"""The boundary between two iterations of a fully resident solve: the translating root step --
which the one-wave default-priority kernels run with its shape compiled in where the schedule row
carries the root-row mark (csrc/plan.h SCHED_ROOT4, csrc/bone_step.h StepRoot) -- and the helper
wave's global pass behind it.  Same operations in the same order, so every solve stays bitwise
equal to the oracle, on the rigs that take the compiled root row and on those that must not (three
effectors, a two-bone root, other priorities, a limited root bone, sub-range solves).  The solves
need an MI355X (-m gpu)."""
import math

import numpy as np
import pytest

from many_bone_ik_amd import workloads as W
from many_bone_ik_amd.solver import Plan

from .test_gpu_parity import assert_parity

gpu = pytest.mark.gpu
TWIST = (0.0, 2.0 * math.pi)
C2_CLASSES = [[2, 1, 1, 1, 1, 1, 1, 1], [0]]


def _rig(lengths, root_bones=1, iterations=3):
    """Chains of the given lengths under a root segment of `root_bones` bones, constrained as C2:
    every bone but the parentless one, two cones, a full-turn twist range."""
    parents, pins = [-1], []
    for _ in range(root_bones - 1):
        parents.append(len(parents) - 1)
    branch = len(parents) - 1
    for n in lengths:
        p = branch
        for _ in range(n):
            parents.append(p)
            p = len(parents) - 1
        pins.append(p)
    return W.custom_topology(parents, pins, np.arange(1, len(parents)), cones_per_bone=2, twist=TWIST, iterations=iterations)


def _c2_other_priorities(n=17):
    wl = W.generate(2, n)
    wl.pin_priority[2] = (0.3, 0.5, 0.1)
    return wl


def _c2_root_limit(n=17):
    """C2 with a Kusudama on the root bone as well (the generator draws no cones for a parentless
    bone: its two cones are set here)."""
    t = W.topology(2)
    B = t.parents.shape[0]
    topo = W.custom_topology(t.parents, t.pins, np.arange(0, B), cones_per_bone=2, twist=TWIST, iterations=t.iterations)
    with np.errstate(invalid="ignore"):
        wl = W.generate(2, n, topo=topo)
    s = math.sqrt(0.5)
    wl.cones[:, 0, 0] = (0.0, 1.0, 0.0, math.radians(35.0))
    wl.cones[:, 0, 1] = (0.0, s, s, math.radians(20.0))
    return wl


RIGS = {
    # a long chain, unequal lengths, a one-bone chain (three effectors: the general root step)
    "chains_11_3_1": (lambda: W.generate(21, 17, topo=_rig((11, 3, 1))), 3),
    "two_chains": (lambda: W.generate(22, 17, topo=_rig((5, 4))), 3),
    "three_chains": (lambda: W.generate(23, 17, topo=_rig((4, 3, 3))), 3),
    # the root row has two steps
    "two_bone_root": (lambda: W.generate(24, 17, topo=_rig((3, 2, 2), root_bones=2, iterations=2)), 2),
    "c2_priorities": (_c2_other_priorities, 3),
    "c2_root_limit": (_c2_root_limit, 3),
}

_REF = {}


def _ref(oracle, key, make, iterations):
    """One oracle solve per input, shared by the cases that slice it; an input is used only if the
    oracle's own result for it is finite (multi-bone roots diverge after many iterations)."""
    if key not in _REF:
        wl = make()
        ref = oracle.Oracle(wl, iterations=iterations).solve(wl.pose, wl.targets, threads=8)
        assert np.isfinite(ref).all(), f"{key}: the oracle's result is not finite"
        _REF[key] = (wl, ref)
    return _REF[key]


def _plan(wl, helper, iterations, interval=0):
    plan = Plan.from_workload(wl, iterations=iterations)
    if interval:
        plan.set_layout(0, 0, interval)
    plan.set_helper_wave(helper)
    return plan


@gpu
@pytest.mark.parametrize("helper", [1, 0])
@pytest.mark.parametrize("iterations", [1, 2, 16])
@pytest.mark.parametrize("n", [1, 17])
def test_c2(oracle, mbik, n, iterations, helper):
    """One skeleton; a full 16-skeleton block plus a one-skeleton block.  The second iteration is
    the first that starts from a global pass over solved locals."""
    _, ref = _ref(oracle, f"c2_i{iterations}", lambda: W.generate(2, 17), iterations)
    wl = W.generate(2, n)
    plan = _plan(wl, helper, iterations)
    got = plan.solve_host(wl.pose, wl.targets)
    assert plan.info()["helper_wave"] == helper
    assert_parity(got, ref[:n], f"C2 n={n} iterations={iterations} helper={helper}")
    plan.close()


@gpu
@pytest.mark.parametrize("interval", [2, 4])
def test_c2_sparse_checkpoints(oracle, mbik, interval):
    """Checkpoint every second / fourth bone: the records rebuild parent globals from the
    checkpoints the pass stored."""
    _, ref = _ref(oracle, "c2_i3", lambda: W.generate(2, 17), 3)
    wl = W.generate(2, 5)
    plan = _plan(wl, 1, 3, interval)
    got = plan.solve_host(wl.pose, wl.targets)
    info = plan.info()
    assert info["helper_wave"] == 1 and info["checkpoint_interval"] == interval
    assert_parity(got, ref[:5], f"C2 checkpoint interval {interval}")
    plan.close()


@gpu
@pytest.mark.parametrize("helper", [1, 0])
@pytest.mark.parametrize("rig", sorted(RIGS))
def test_rigs(oracle, mbik, rig, helper):
    make, iterations = RIGS[rig]
    wl, ref = _ref(oracle, rig, make, iterations)
    plan = _plan(wl, helper, iterations)
    got = plan.solve_host(wl.pose, wl.targets)
    assert plan.info()["helper_wave"] == helper
    assert_parity(got, ref, f"{rig} helper={helper}")
    plan.close()


@gpu
def test_c2_segment_solve(oracle, mbik):
    """A sub-range solve: the root segment alone, one chain alone.  The pass still covers every
    segment; a sub-range takes the general root step."""
    import torch
    dev = torch.device("cuda", 0)
    wl = W.generate(2, 17)
    o = oracle.Oracle(wl)
    plan = Plan.from_workload(wl)
    plan.set_helper_wave(1)
    for seg in (0, 1, plan.info()["segment_count"] - 1):
        ref = o.segment_solve(seg, wl.pose, wl.targets)
        assert np.isfinite(ref).all()
        pose = torch.from_numpy(wl.pose.copy()).to(dev)
        tg = torch.from_numpy(wl.targets).to(dev)
        plan.segment_solve(seg, pose.data_ptr(), tg.data_ptr())
        torch.cuda.synchronize()
        assert plan.info()["helper_wave"] == 1
        assert_parity(pose.cpu().numpy(), ref, f"C2 segment {seg}")
    plan.close()


@gpu
def test_c2_classes_and_saved_plan(oracle, mbik):
    """The step-class table is what it was, and a saved and reloaded plan solves the same bits."""
    _, ref = _ref(oracle, "c2_i3", lambda: W.generate(2, 17), 3)
    wl = W.generate(2, 5)
    plan = _plan(wl, 1, 3)
    assert [c.tolist() for c in plan.step_classes()] == C2_CLASSES
    loaded = Plan.load(plan.save())
    assert [c.tolist() for c in loaded.step_classes()] == C2_CLASSES
    assert_parity(loaded.solve_host(wl.pose, wl.targets), ref[:5], "loaded plan")
    assert_parity(plan.solve_host(wl.pose, wl.targets), ref[:5], "saved plan")
    loaded.close()
    plan.close()
