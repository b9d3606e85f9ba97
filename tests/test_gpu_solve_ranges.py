"""Sub-range, in-place and guard-band behaviour of every solve path (tests/solve_range_cases.py
has the harness and says what each launch is checked for): mbik_solve over every kernel family,
one plan over changing launch sizes, mbik_solve_checked, mbik_segment_solve, mbik_group_solve,
mbik_multi_solve's staged path, and constraint_mode over frames with mixed ranges.  The
expectation is always the oracle.  Needs an MI355X: -m gpu."""
import numpy as np
import pytest

from many_bone_ik_amd.solver import Group, Multi, Plan

from . import solve_range_cases as R
from .test_gpu_parity import torch_dev  # noqa: F401 (fixture)

pytestmark = pytest.mark.gpu

C2_FAMILIES = ["classic_pl0", "classic_pl1_w2", "classic_pl2_w1", "classic_pl2_w2", "split_exchange", "helper_wave",
               "roles_k2", "roles_k4", "stabilization", "table64", "cmode_classic", "cmode_roles"]
# C5 and dropped_branch: families 1, 3, 5 and 6 (K = 8 runs on C5, the rig with eight roles' worth of siblings)
SMALL_FAMILIES = ["classic_pl0", "classic_pl2_w1", "classic_pl2_w2", "helper_wave", "roles_k2", "roles_k4"]
CASES = ([("C2", f, r) for f in C2_FAMILIES for r in R.RIGS["C2"][1]] +
         [("C5", f, r) for f in SMALL_FAMILIES + ["roles_k8"] for r in R.RIGS["C5"][1]] +
         [("dropped_branch", f, r) for f in SMALL_FAMILIES for r in R.RIGS["dropped_branch"][1]])


class Refs:
    """The rigs' workloads and the oracle's results for them, each computed once and never written."""

    def __init__(self, oracle):
        self.oracle, self._wl, self._ref = oracle, {}, {}

    def wl(self, rig):
        if rig not in self._wl:
            self._wl[rig] = R.workload(rig)
        return self._wl[rig]

    def ref(self, rig, family):
        kw = R.ref_kwargs(family)
        key = (rig, tuple(sorted(kw.items())))
        if key not in self._ref:
            wl = self.wl(rig)
            o = self.oracle.Oracle(wl, **kw)
            ref = o.solve(wl.pose, wl.targets, threads=8)
            o.close()
            ref.setflags(write=False)
            self._ref[key] = ref
        return self._ref[key]


@pytest.fixture(scope="module")
def refs(oracle):
    return Refs(oracle)


@pytest.fixture(scope="module")
def side_stream(torch_dev):
    torch, dev = torch_dev
    return torch.cuda.Stream(dev)


def test_dropped_branch_leaves_bones_out_of_the_bone_list(mbik, refs):
    """The pass-through copy of pose_in needs bones outside the IK bone list: 3 and 4 here."""
    from many_bone_ik_amd.solver import describe_topology
    wl = refs.wl("dropped_branch")
    bl = describe_topology(wl.topo.parents, wl.pins(), wl.constraints())["bone_list"].tolist()
    assert sorted(set(range(wl.pose.shape[1])) - set(bl)) == [3, 4]


@pytest.mark.parametrize("in_place", [False, True], ids=["out_of_place", "in_place"])
@pytest.mark.parametrize("rig,family,rng", CASES, ids=[f"{r}-{f}-{a}+{c}" for r, f, (a, c) in CASES])
def test_solve_range(oracle, mbik, torch_dev, refs, side_stream, rig, family, rng, in_place):
    """Every kernel family on every range, out of place (default stream) and in place (a stream
    of the caller's).  constraint_mode: a fresh plan's first frame against a fresh oracle graph's."""
    wl = refs.wl(rig)
    plan = R.make_plan(wl, family)
    R.run_range(plan, wl, refs.ref(rig, family), rng[0], rng[1], in_place, stream=side_stream.cuda_stream if in_place else 0,
                what=f"{rig} {family}")
    R.check_family(plan, family)
    plan.close()


@pytest.mark.parametrize("in_place", [False, True], ids=["out_of_place", "in_place"])
@pytest.mark.parametrize("family", ["classic_pl0", "classic_pl2_w2", "roles_k4"])
def test_one_plan_changing_launch_sizes(oracle, mbik, torch_dev, refs, family, in_place):
    """mbik_solve rebuilds the schedule from the launch's count: one plan and one set of buffers
    over 83, 18, 1 and 83 skeletons; the device state areas must serve each of them."""
    wl = refs.wl("C2")
    plan = R.make_plan(wl, family)
    bufs = None
    for a, c in [(0, 83), (15, 18), (82, 1), (0, 83)]:
        bufs = R.run_range(plan, wl, refs.ref("C2", family), a, c, in_place, bufs=bufs, what=f"C2 {family}")
        R.check_family(plan, family)
    plan.close()


@pytest.mark.parametrize("in_place", [False, True], ids=["out_of_place", "in_place"])
@pytest.mark.parametrize("family", ["cmode_classic", "cmode_roles"])
@pytest.mark.parametrize("frames", [[(0, 83), (15, 18), (82, 1), (0, 83)], [(0, 83), (15, 18), (30, 53), (0, 83)]],
                         ids=["changing_sizes", "mixed_ranges"])
def test_constraint_mode_frames_over_ranges(oracle, mbik, torch_dev, family, frames, in_place):
    """constraint_mode's block shape follows the launch's count too, and its node caches persist:
    a sub-range frame advances exactly the caches of its own skeletons."""
    plan = R.make_plan(R.workload("C2"), family)
    R.run_cmode_frames(oracle, plan, "C2", frames, in_place, seed=7, family=family)
    plan.close()


@pytest.mark.parametrize("in_place", [False, True], ids=["out_of_place", "in_place"])
@pytest.mark.parametrize("family", ["classic_pl0", "roles_k4", "cmode_classic", "cmode_roles"])
def test_solve_checked_range(oracle, mbik, torch_dev, family, in_place):
    """mbik_solve_checked on [15, 33): skeletons 15 and 32, the two ends of the range, carry a
    NaN rotation (as test_gpu_degenerate.test_nonfinite_flags); the flags are 1 exactly there,
    the poses equal the oracle's (a NaN only has to be a NaN) and no guard byte changes."""
    a, c = 15, 18
    wl = R.workload("C2")
    wl.pose[[15, 32], 5, 0] = np.nan
    o = oracle.Oracle(wl, **R.ref_kwargs(family))
    ref = o.solve(wl.pose, wl.targets, threads=8)
    o.close()
    assert np.isfinite(ref[[14, 16, 31, 33]]).all()
    want = np.zeros(c, np.uint8)
    want[[0, c - 1]] = 1
    plan = R.make_plan(wl, family)
    R.run_range(plan, wl, ref, a, c, in_place, checked=True, flags_want=want, nan_aware=True, what=f"C2 {family} checked")
    R.check_family(plan, family)
    plan.close()


@pytest.mark.parametrize("family", ["classic_pl0", "helper_wave", "roles_k4"])
@pytest.mark.parametrize("which", ["leaf", "root"])
def test_segment_solve_range(oracle, mbik, torch_dev, refs, family, which):
    """mbik_segment_solve (always in place) of a leaf segment and of the root segment on
    [15, 33), against the oracle's segment solve of those skeletons."""
    a, c = 15, 18
    wl = refs.wl("C2")
    o = oracle.Oracle(wl)
    seg = 0 if which == "leaf" else o.segment_count() - 1
    ref = np.full_like(wl.pose, np.nan)
    ref[a:a + c] = o.segment_solve(seg, wl.pose[a:a + c], wl.targets[a:a + c], first=a)
    o.close()
    assert not np.array_equal(ref[a:a + c], wl.pose[a:a + c])
    plan = R.make_plan(wl, family)
    R.run_range(plan, wl, ref, a, c, True, segment=seg, what=f"C2 {family} segment {seg}")
    R.check_family(plan, family)
    plan.close()


def test_group_solve_ranges(oracle, mbik, torch_dev):
    """mbik_group_solve with per-plan ranges at non-zero first (the rigs of
    test_gpu_group.test_group_subranges_and_repeat): guard bands and NaN-poisoned neighbours per
    plan, two frames on one stream, the oracle as the expectation; a plan with count 0 is untouched."""
    from .test_gpu_group import rigs
    torch, dev = torch_dev
    cases = rigs()[:3]
    plans = [Plan.from_workload(wl, **kw) for wl, kw in cases]
    g = Group(plans)
    first, count = [5, 1, 10], [40, 3, 0]
    for in_place in (False, True):
        rc = [R.RangeCase(R.RangeBuffers.of(torch, dev, wl), wl.pose, wl.targets, f, c, in_place)
              for (wl, _), f, c in zip(cases, first, count)]
        g.solve([x.pose_in_ptr for x in rc], [x.targets_ptr for x in rc], [x.pose_out_ptr for x in rc], first=first, count=count)
        if not in_place:        # a second frame reuses the group's tables
            g.solve([x.pose_in_ptr for x in rc], [x.targets_ptr for x in rc], [x.pose_out_ptr for x in rc], first=first,
                    count=count)
        for (wl, kw), x in zip(cases, rc):
            ref = oracle.Oracle(wl, stabilization_passes=kw.get("stabilization_passes", 0)).solve(wl.pose, wl.targets, threads=8)
            x.check(ref, f"group {wl.topo.name} in_place={in_place}")
    g.close()


def test_multi_solve_staged_guard_rows(oracle, mbik, torch_dev, refs, side_stream):
    """mbik_multi_solve with MBIK_MULTI_STAGE_ALL (scatter, solve, gather through the handle's
    own buffers), C2 x 83 cut at 17: the gather writes pose_out's 83 rows and nothing around them."""
    from .test_gpu_multi import shard_plans
    torch, dev = torch_dev
    wl = refs.wl("C2")
    cuts = [0, 17, 83]
    m = Multi(shard_plans(wl, cuts), root_device=0, stage_all=True)
    assert m.skeletons() == (83, cuts)
    case = R.RangeCase(R.RangeBuffers.of(torch, dev, wl), wl.pose, wl.targets, 0, 83, False)
    m.solve(case.pose_in_ptr, case.targets_ptr, case.pose_out_ptr, side_stream.cuda_stream)
    side_stream.synchronize()
    case.check(refs.ref("C2", "classic_pl0"), "multi stage_all")
    m.close()
