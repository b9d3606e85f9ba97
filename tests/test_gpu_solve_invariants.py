"""What a solved pose means, on the GPU: tests/test_solve_invariants_cpu.py's checks on the kernels'
own output, with the same float64 models and the same limits (tests/solve_invariants.py), plus
bit equality with the oracle.  The function-level pin runs both constraint_mode kernels; the
end-state invariants run each solve kernel family at its smallest shape.  Stabilized solves are
excluded for the reason the CPU module gives.  Needs an MI355X: -m gpu."""
import numpy as np
import pytest

from many_bone_ik_amd.solver import Group, Plan

from . import geometry_f64 as G
from . import solve_invariants as S
from .test_gpu_parity import assert_parity, torch_dev  # noqa: F401 (fixture)
from .test_solve_invariants_cpu import N_CMODE, cmode_case, cmode_rotation_check

pytestmark = pytest.mark.gpu


# --- one snap at a time: both constraint_mode kernels ----------------------------------------------
def cmode_gpu(wl, pose_in, roles):
    plan = Plan.from_workload(wl, constraint_mode=True, iterations=1, lanes=4)
    plan.set_wave_roles(roles)
    out = plan.solve_host(pose_in, wl.targets)
    assert plan.info()["wave_roles"] == roles
    plan.close()
    return out


@pytest.mark.parametrize("roles", [0, 1])
@pytest.mark.parametrize("twist", S.TWISTS)
@pytest.mark.parametrize("ncones", [0, 1])
@pytest.mark.parametrize("rest", ["plus_y", "realistic_unit_scale"])
def test_constraint_mode_snaps_to_the_expected_rotation(oracle, mbik, rest, ncones, twist, roles):
    wl, pose_in, ref = cmode_case(oracle, rest, ncones, twist)
    out = cmode_gpu(wl, pose_in, roles)
    assert cmode_rotation_check(wl, pose_in, out, f"{rest} {ncones} cones {twist} roles={roles}") <= S.CMODE_ROTATION_LIMIT
    assert S.TwistModel(wl).excess(wl, out).max() <= S.CMODE_TWIST_LIMIT
    assert_parity(out, ref, "constraint_mode vs oracle")


@pytest.mark.parametrize("roles", [0, 1])
@pytest.mark.parametrize("twist", S.TWISTS)
def test_constraint_mode_two_cones(oracle, mbik, twist, roles):
    wl, pose_in, ref = cmode_case(oracle, "plus_y", 2, twist, zero_positions=True)
    out = cmode_gpu(wl, pose_in, roles)
    res = S.swing_residual(wl, out, S.direction_frames(wl), S.regions(wl))[0]
    assert res.max() <= S.SWING_BAND_LIMIT and S.TwistModel(wl).excess(wl, out).max() <= S.CMODE_TWIST_LIMIT
    assert_parity(out, ref, "constraint_mode two cones vs oracle")


@pytest.mark.parametrize("roles", [0, 1])
def test_constraint_mode_leaves_other_bones_alone(oracle, mbik, roles):
    """As on the oracle: positions bitwise, rotations and scales within the measured bounds."""
    every = np.arange(1, 32)
    wl = S.workload("c2", N_CMODE, 1, S.TWISTS[0], S.CMODE_RADII[1], 1, constrained=every[::2])
    pose_in = S.perturb(wl.pose, np.random.default_rng(5), (0.0, 1.2), 1.5)
    out = cmode_gpu(wl, pose_in, roles)
    free = np.setdiff1d(np.arange(32), wl.topo.constrained)
    turn = max(G.rotation_angle(S.rotation(out[s, b, 0:4]), S.rotation(pose_in[s, b, 0:4])) for s in range(wl.n) for b in free)
    assert np.array_equal(out[..., 4:7], pose_in[..., 4:7])
    assert turn <= S.CMODE_UNTOUCHED_LIMIT and np.abs(out[..., 7:10] - pose_in[..., 7:10]).max() <= S.CMODE_SCALE_LIMIT


# --- end state of the ordinary solve, per kernel family ----------------------------------------------
def classic(plan, helper):
    plan.set_helper_wave(helper)
    return dict(helper_wave=helper, wave_roles=0)


def one_lane(plan):
    plan.set_layout(1, 0, 0)
    return dict(lanes_per_skeleton=1)


def two_waves(plan):
    plan.set_waves_per_simd(2)
    return dict(waves_per_simd=2)


def placement2(plan):
    plan.set_locals_placement(2)
    return dict(state_placement=2)


def wave_roles(plan):
    plan.set_layout(4, 0, 0)
    plan.set_waves_per_simd(2)
    plan.set_wave_roles(1)
    return dict(wave_roles=1, skeletons_per_block=64)


# family -> (configure, skeletons: a partly filled block and a second one)
FAMILIES = {
    "helper_on": (lambda p: classic(p, 1), 33),
    "helper_off": (lambda p: classic(p, 0), 33),
    "one_lane": (one_lane, 33),
    "two_waves": (two_waves, 33),
    "placement2": (placement2, 33),
    "wave_roles": (wave_roles, 65),
}
# what each family solves: swing under a full twist range, and a twist range with one cone
CHECKS = [("swing", 2, S.FULL_TWIST), ("twist", 1, S.TWISTS[1])]


def solve(c, configure):
    plan = Plan.from_workload(c.wl)
    want = configure(plan)
    out = plan.solve_host(c.pose_in, c.wl.targets)
    info = plan.info()
    assert {k: info[k] for k in want} == want, info
    plan.close()
    return out


def judge(oracle, c, out, what, label):
    if what == "swing":
        S.check_swing(c, out, label)
        S.check_rigid(c, out, label)
    else:
        S.check_twist(c, out, label)
    assert_parity(out, S.oracle_solve(oracle, c), label)


@pytest.mark.parametrize("what,ncones,twist", CHECKS)
@pytest.mark.parametrize("it", [1, 16])
@pytest.mark.parametrize("rest", ["plus_y", "realistic_unit_scale"])
@pytest.mark.parametrize("family", list(FAMILIES))
def test_c2_end_state(oracle, mbik, family, rest, it, what, ncones, twist):
    configure, n = FAMILIES[family]
    c = S.case("c2", rest, it, ncones, twist, n)
    judge(oracle, c, solve(c, configure), what, f"c2 {family} {rest} {it} iterations {what}")


@pytest.mark.parametrize("ncones,twist", [(1, S.FULL_TWIST), (3, S.FULL_TWIST), (0, S.TWISTS[0]), (1, S.TWISTS[0])])
@pytest.mark.parametrize("it", [1, 16])
@pytest.mark.parametrize("rest", ["plus_y", "realistic_unit_scale"])
def test_c2_cone_counts_and_twists(oracle, mbik, rest, it, ncones, twist):
    """The cone counts and the twist pair that the families above leave out, on the default layout."""
    c = S.case("c2", rest, it, ncones, twist, 33)
    judge(oracle, c, solve(c, lambda p: {}), "swing" if twist == S.FULL_TWIST else "twist", f"c2 {rest} {it} iterations {ncones} cones")


@pytest.mark.parametrize("what,ncones,twist", CHECKS)
@pytest.mark.parametrize("it", [1, 16])
@pytest.mark.parametrize("rest", ["plus_y", "realistic_unit_scale"])
@pytest.mark.parametrize("family", ["helper_on", "helper_off", "wave_roles"])
def test_uneven_rig_end_state(oracle, mbik, family, rest, it, what, ncones, twist):
    """Chains of 3, 2, 2 and 1: the roles run out of steps at different step indices."""
    configure, n = FAMILIES[family]
    c = S.case("uneven", rest, it, ncones, twist, n)
    judge(oracle, c, solve(c, configure), what, f"uneven {family} {rest} {it} iterations {what}")


@pytest.mark.parametrize("it", [1, 16])
def test_group_of_two_rigs(oracle, mbik, torch_dev, it):
    torch, dev = torch_dev
    cases = [S.case("c2", "plus_y", it, 2, S.FULL_TWIST, 33), S.case("uneven", "realistic_unit_scale", it, 1, S.TWISTS[1], 33)]
    plans = [Plan.from_workload(c.wl) for c in cases]
    bufs = [(torch.from_numpy(c.pose_in).to(dev), torch.from_numpy(c.wl.targets).to(dev)) for c in cases]
    outs = [torch.empty_like(b[0]) for b in bufs]
    g = Group(plans)
    g.solve([b[0].data_ptr() for b in bufs], [b[1].data_ptr() for b in bufs], [o.data_ptr() for o in outs])
    torch.cuda.synchronize()
    judge(oracle, cases[0], outs[0].cpu().numpy(), "swing", f"group c2 {it} iterations")
    judge(oracle, cases[1], outs[1].cpu().numpy(), "twist", f"group uneven {it} iterations")
    g.close()


def test_bones_in_no_segment_are_unchanged(oracle, mbik):
    c = S.case("uneven_spare", "plus_y", 16, 1, S.TWISTS[0], 33, constrained=np.arange(1, 9))
    inl = S.list_bones(c.wl)
    plan = Plan.from_workload(c.free)
    out = plan.solve_host(c.pose_in, c.free.targets)
    assert np.array_equal(out[:, ~inl], c.pose_in[:, ~inl])
    assert not np.array_equal(out[:, inl], c.pose_in[:, inl])


@pytest.mark.parametrize("rig", ["c2", "uneven"])
def test_float64_direction_frames_match_the_plan(mbik, rig):
    """The float64 bone-direction frames (the reference of the swing checks) against the D rows of
    the plan's setup tables on the realistic rest, where they leave the identity."""
    c = S.case(rig, "realistic_unit_scale", 16, 1, S.FULL_TWIST, 33)
    plan = Plan.from_workload(c.wl)
    D = plan.setup_tables()[0]                       # [bone][9][skeleton], row-major 3x3
    plan.close()
    pos = c.wl.pose[..., 4:7].astype(np.float64)
    worst, moved, near = 0.0, 0, 0
    for s in range(c.wl.n):
        for b in range(D.shape[0]):
            kids = np.flatnonzero(c.wl.topo.parents == b)
            if len(kids) and G.near_deadband(G.angle(pos[s, kids].mean(axis=0), G.Y_AXIS)):
                near += 1
                continue
            got = D[b, :, s].reshape(3, 3).astype(np.float64)
            worst = max(worst, G.rotation_angle(got, c.frames[s, b]))
            moved += G.rotation_angle(c.frames[s, b], np.eye(3)) > 0.1
    print(f"{rig}: float64 frames to D rows max {worst:.3g} rad, limit {S.FRAME_D_LIMIT:.3g}; {moved} frames off the identity")
    assert near <= S.LEFT_OUT_CAP * D.shape[0] * c.wl.n
    assert moved > c.wl.n * D.shape[0] // 3
    assert worst <= S.FRAME_D_LIMIT
