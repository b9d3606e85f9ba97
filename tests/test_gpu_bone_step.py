"""The solve kernels' bone-steps against the float64 model of tests/bone_step_f64.py: the cases,
measures and limits of tests/test_bone_step_cpu.py (tests/bone_step_cases.py) on every kernel form --
one-wave classic with the helper wave on and off, one lane per skeleton, two waves per SIMD, state
placement 2, wave roles, the stabilization instantiation, and C2's topology at the default
priorities, whose root row runs bone_step<StepRoot> -- through mbik_solve at one and two iterations
and mbik_segment_solve of every segment.  Every output is also bitwise the oracle's, and the rows
around the pose buffer keep their sentinel.  33 skeletons end inside a wave and cross a block; wave
roles take 65, one more than a block.  Needs an MI355X: -m gpu."""
import numpy as np
import pytest

from many_bone_ik_amd.solver import Plan, describe_step_classes

from . import bone_step_cases as B
from .test_gpu_parity import assert_parity, torch_dev  # noqa: F401 (fixture)
from .test_gpu_solve_invariants import FAMILIES

pytestmark = pytest.mark.gpu

GUARD = 64                               # rows of sentinels on each side: the most skeletons a block owns
SENTINEL = np.float32(-12345.678)
FORM_RIGS = [("uneven", "realistic_unit_scale"), ("c2", "plus_y")]


def configured(c, family, iterations, **kw):
    plan = Plan.from_workload(c.wl, iterations=iterations, **kw)
    want = FAMILIES[family][0](plan) if family else {}
    return plan, want


def launch(torch_dev, plan, c, want, segment=None):
    """mbik_solve (or mbik_segment_solve, in place) of the case's input between sentinel rows."""
    torch, dev = torch_dev
    n = c.wl.n
    host = np.full((GUARD + n + GUARD,) + c.pose_in.shape[1:], SENTINEL, np.float32)
    if segment is not None:
        host[GUARD:GUARD + n] = c.pose_in
    out = torch.from_numpy(host).to(dev)
    tg = torch.from_numpy(c.wl.targets).to(dev)
    row = out.data_ptr() + GUARD * c.pose_in.shape[1] * 40
    if segment is None:
        pose = torch.from_numpy(c.pose_in).to(dev)
        plan.solve(pose.data_ptr(), tg.data_ptr(), row)
    else:
        plan.segment_solve(segment, row, tg.data_ptr())
    torch.cuda.synchronize()
    got = out.cpu().numpy()
    info = plan.info()
    assert {k: info[k] for k in want} == want, info
    guard = np.concatenate([got[:GUARD], got[GUARD + n:]])
    assert (guard.view(np.uint32) == SENTINEL.view(np.uint32)).all(), "a row outside the pose buffer was written"
    return got[GUARD:GUARD + n]


def assert_root_row(plan, c):
    """C2's topology at the default priorities on a one-wave placement-0 kernel: the schedule's root
    row is the four-effector translating step that bone_step<StepRoot> runs (csrc/plan.h SCHED_ROOT4);
    the row keeps class 0, as tests/test_gpu_iter_boundary.py asserts for the constrained rig."""
    info = plan.info()
    classes = [k.tolist() for k in plan.step_classes()]
    assert classes == [k.tolist() for k in describe_step_classes(c.wl.topo.parents, c.wl.pins(), c.wl.constraints())]
    assert classes == [[0] * 8, [0]]
    assert info["lanes_per_skeleton"] == 4 and info["state_placement"] == 0 and info["waves_per_simd"] == 1
    assert info["heading_slots"] != 0          # the build for the default priorities


# --- whole iterations, every kernel form ---------------------------------------------------------------
@pytest.mark.parametrize("iterations", [1, 2])
@pytest.mark.parametrize("rig,rest", FORM_RIGS)
@pytest.mark.parametrize("family", list(FAMILIES))
def test_iterations_on_every_form(oracle, mbik, torch_dev, family, rig, rest, iterations):
    c = B.base_case(rig, rest, "default", n=FAMILIES[family][1])
    plan, want = configured(c, family, iterations)
    out = launch(torch_dev, plan, c, want)
    if rig == "c2" and family in ("helper_on", "helper_off"):
        assert_root_row(plan, c)
    plan.close()
    label = f"{c.label} {family} {iterations} iterations"
    assert_parity(out, B.oracle_out(oracle, c, "solve", iterations), label)
    B.check_iterations(c, out, iterations, label)


@pytest.mark.parametrize("iterations", [1, 2])
@pytest.mark.parametrize("rig,rest,pins", B.BASE, ids=["-".join(k) for k in B.BASE])
def test_iterations_on_every_case(oracle, mbik, torch_dev, rig, rest, pins, iterations):
    """The CPU module's base cases -- the mid-chain pins, the three-bone translating segment, the
    mixed weights and the one-point path among them -- on the automatic layout."""
    c = B.base_case(rig, rest, pins)
    plan, want = configured(c, None, iterations)
    out = launch(torch_dev, plan, c, want)
    plan.close()
    label = f"{c.label} {iterations} iterations"
    assert_parity(out, B.oracle_out(oracle, c, "solve", iterations), label)
    B.check_iterations(c, out, iterations, label)


# --- mbik_segment_solve of every segment ---------------------------------------------------------------
@pytest.mark.parametrize("rig,rest", FORM_RIGS)
@pytest.mark.parametrize("family", list(FAMILIES))
def test_segment_solve_on_every_form(oracle, mbik, torch_dev, family, rig, rest):
    c = B.base_case(rig, rest, "default", n=FAMILIES[family][1])
    plan, want = configured(c, family, 1)
    for seg in range(len(c.topo.segments)):
        out = launch(torch_dev, plan, c, want, segment=seg)
        label = f"{c.label} {family} segment {seg}"
        assert_parity(out, B.oracle_out(oracle, c, "segment", seg), label)
        B.check_segment(c, out, seg, label)
    plan.close()


@pytest.mark.parametrize("rig,rest,pins", [k for k in B.BASE if k[0] in ("midpin", "chain3")],
                         ids=["-".join(k) for k in B.BASE if k[0] in ("midpin", "chain3")])
def test_segment_solve_midpin_and_chain(oracle, mbik, torch_dev, rig, rest, pins):
    c = B.base_case(rig, rest, pins)
    plan, want = configured(c, None, 1)
    for seg in range(len(c.topo.segments)):
        out = launch(torch_dev, plan, c, want, segment=seg)
        label = f"{c.label} segment {seg}"
        assert_parity(out, B.oracle_out(oracle, c, "segment", seg), label)
        B.check_segment(c, out, seg, label)
    plan.close()


# --- the damp clamp's classes ----------------------------------------------------------------------------
@pytest.mark.parametrize("rig,rest,d", B.DAMP_CASES, ids=["-".join(k) for k in B.DAMP_CASES])
def test_damp_classes(oracle, mbik, torch_dev, rig, rest, d):
    c = B.damp_case(rig, rest, d)
    plan, want = configured(c, None, 1)
    out = launch(torch_dev, plan, c, want)
    plan.close()
    assert_parity(out, B.oracle_out(oracle, c, "solve", 1), f"{c.label} damp {d}")
    B.check_damp_classes(c, out, f"{c.label} damp {d}")


@pytest.mark.parametrize("family", list(FAMILIES))
def test_damp_classes_on_every_form(oracle, mbik, torch_dev, family):
    c = B.damp_case("uneven", "plus_y", "5deg", n=FAMILIES[family][1])
    plan, want = configured(c, family, 1)
    out = launch(torch_dev, plan, c, want)
    plan.close()
    assert_parity(out, B.oracle_out(oracle, c, "solve", 1), f"{c.label} damp {family}")
    B.check_damp_classes(c, out, f"{c.label} damp {family}")


# --- the stabilization instantiation -------------------------------------------------------------------
@pytest.mark.parametrize("lanes", [0, 1])
@pytest.mark.parametrize("iterations", [1, 2])
@pytest.mark.parametrize("passes", [1, 3])
@pytest.mark.parametrize("rest", B.RESTS)
def test_stabilization(oracle, mbik, torch_dev, rest, passes, iterations, lanes):
    c = B.stabilized_case(rest, passes)
    plan = Plan.from_workload(c.wl, iterations=iterations, stabilization_passes=passes, lanes=lanes)
    out = launch(torch_dev, plan, c, {})
    plan.close()
    label = f"{c.label} passes {passes} iterations {iterations} lanes {lanes}"
    assert_parity(out, B.oracle_out(oracle, c, "solve", iterations), label)
    B.check_stabilized(c, out, iterations, label)


@pytest.mark.parametrize("rest", B.RESTS)
def test_stabilization_segment_solve(oracle, mbik, torch_dev, rest):
    """(include/mbik.h refuses no pairing of mbik_segment_solve with stabilization or a placement.)"""
    c = B.stabilized_case(rest, 1)
    plan = Plan.from_workload(c.wl, iterations=1, stabilization_passes=1)
    out = launch(torch_dev, plan, c, {}, segment=0)
    plan.close()
    assert_parity(out, B.oracle_out(oracle, c, "segment", 0), f"{c.label} stabilized segment")
    B.check_stabilized(c, out, 1, f"{c.label} stabilized segment")


def test_stabilization_on_c2(oracle, mbik, torch_dev):
    """The stabilization instantiation on C2's topology: a one-bone root always accepts."""
    c = B.case("c2", "plus_y", "default", stabilization=1)
    plan = Plan.from_workload(c.wl, iterations=2, stabilization_passes=1)
    out = launch(torch_dev, plan, c, {})
    plan.close()
    assert_parity(out, B.oracle_out(oracle, c, "solve", 2), "c2 stabilized")
    _, records = c.model_iterations(2)
    assert all(r["accepted"].all() for r in records)
    B.check_iterations(c, out, 2, "c2 stabilized")


# --- weight 0 ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rig", B.RIGS)
def test_weight_zero_is_the_identity(oracle, mbik, torch_dev, rig):
    c = B.case(rig, "realistic_unit_scale", "weight0")
    plan, want = configured(c, None, 1)
    out = launch(torch_dev, plan, c, want)
    plan.close()
    assert_parity(out, B.oracle_out(oracle, c, "solve", 1), f"{c.label}")
    B.check_weight0(c, out, c.label)
