"""What a solved pose means, on the CPU oracle: the constraint frames, the twist limit and the swing
snap against float64 models written from their definitions (tests/geometry_f64.py), first one
snap at a time through constraint_mode, then as end-state invariants of the ordinary solve.
tests/test_gpu_solve_invariants.py asks the same of the kernels, with the same limits.

constraint_mode runs the snaps only and every frame is parent-relative, so on a fresh plan's first
frame with one iteration each constrained bone's output rotation is a function of its own input
local, cones and twist alone: that frame pins the snaps themselves.

The end-state invariants exclude stabilized solves: a stabilization pass that does not bring the
tips closer restores the bone's transform from before the step (ik_bone_segment_3d.cpp:163-180),
snaps included, so a bone may legitimately end where it started, outside its limits.

Every limit is 4 x the worst value these tests measure on the oracle (printed by each test; DESIGN.md
section 7a holds the table), except SWING_BAND_LIMIT, which is derived (solve_invariants.py)."""
import numpy as np
import pytest

from . import geometry_f64 as G
from . import solve_invariants as S

N_CMODE = 16            # x 31 constraints of C2's topology = 496 per case


def cmode_case(oracle, rest, ncones, twist, zero_positions=False):
    """(workload, input pose, oracle output) of one constraint_mode frame on a fresh object graph."""
    wl = S.workload("c2", N_CMODE, ncones, twist, S.CMODE_RADII[ncones], 1, rest=rest)
    # rolls spread about the range's centre by +-range: about half of them end outside +-range/2
    pose_in = S.perturb(wl.pose, np.random.default_rng(5), (0.0, 1.2), twist[1], roll_centre=2 * twist[0])
    if zero_positions:
        pose_in[:, 1:, 4:7] = 0.0
    o = oracle.Oracle(wl, constraint_mode=True, iterations=1)
    out = o.solve(pose_in, wl.targets)
    o.close()
    return wl, pose_in, out


QUANTITY = 25           # of 496: how many constraints of each input class a case must hold


def cmode_rotation_check(wl, pose_in, out, label, twist_model=None, radius_scale=1.0):
    """Worst angle between the output rotations and the float64 expected ones, over the constraints
    whose arcs are clear of the deadband.  With the right model it also asserts that the input
    classes occur in quantity: twist inside and outside its range, direction inside and outside
    its cap, both outside at once."""
    tm = S.TwistModel(wl) if twist_model is None else twist_model
    exp, tw, sw = S.expected_cmode(wl, pose_in, S.direction_frames(wl), tm, radius_scale)
    if twist_model is None and radius_scale == 1.0:
        tw_out = np.abs(tw) > tm.half * tm.range
        if tm.range.max() < 6.0:
            assert min(tw_out.sum(), (~tw_out).sum()) >= QUANTITY, (tw_out.sum(), tw_out.size)
        if wl.cone_count[0]:
            sw_out = sw > 0
            assert min(sw_out.sum(), (~sw_out).sum()) >= QUANTITY, (sw_out.sum(), sw_out.size)
            assert (sw_out & tw_out).sum() >= QUANTITY or tm.range.max() >= 6.0
    left_out = G.near_deadband(sw) | G.near_deadband(tm.arc)
    assert left_out.mean() <= S.LEFT_OUT_CAP
    err = S.rotation_errors(wl, out, exp)[~left_out]
    print(f"{label}: rotation error max {err.max():.3g} rad, limit {S.CMODE_ROTATION_LIMIT:.3g} ({left_out.sum()} left out)")
    return err.max()


@pytest.mark.parametrize("twist", S.TWISTS)
@pytest.mark.parametrize("ncones", [0, 1])
@pytest.mark.parametrize("rest", ["plus_y", "realistic_unit_scale"])
def test_constraint_mode_snaps_to_the_expected_rotation(oracle, rest, ncones, twist):
    wl, pose_in, out = cmode_case(oracle, rest, ncones, twist)
    assert cmode_rotation_check(wl, pose_in, out, f"{rest} {ncones} cones {twist}") <= S.CMODE_ROTATION_LIMIT
    ex = S.TwistModel(wl).excess(wl, out)
    print(f"twist beyond range/2 max {ex.max():.3g}, limit {S.CMODE_TWIST_LIMIT:.3g}")
    assert ex.max() <= S.CMODE_TWIST_LIMIT


@pytest.mark.parametrize("twist", S.TWISTS)
def test_constraint_mode_two_cones(oracle, twist):
    """No expected rotation for two cones: the direction ends in the region or on its boundary and
    the twist in its range.  +Y rest, where the twist about the frame's +Y leaves the direction
    alone, and zero local positions, because constraint_mode measures the tip from the parent's
    origin and turns only the bone: with an offset the snapped direction does
    not land on the boundary."""
    wl, pose_in, out = cmode_case(oracle, "plus_y", 2, twist, zero_positions=True)
    fr, regs = S.direction_frames(wl), S.regions(wl)
    before = S.swing_residual(wl, pose_in, fr, regs)[0]
    assert (before > 10 * S.SWING_BAND_LIMIT).sum() >= 100 and (before == 0).sum() >= 40
    res = S.swing_residual(wl, out, fr, regs)[0]
    ex = S.TwistModel(wl).excess(wl, out)
    print(f"two cones {twist}: swing residual max {res.max():.3g} (limit {S.SWING_BAND_LIMIT:.3g}), twist {ex.max():.3g}")
    assert res.max() <= S.SWING_BAND_LIMIT and ex.max() <= S.CMODE_TWIST_LIMIT


def test_constraint_mode_leaves_other_bones_alone(oracle):
    """Unconstrained and parentless bones keep their rotation, and every bone its position and
    scale.  Positions are bitwise; rotations and scales are not, on the oracle: the output is
    re-extracted from the basis (ik_bone_3d.cpp:170-179), so they hold within a measured bound."""
    every = np.arange(1, 32)
    wl = S.workload("c2", N_CMODE, 1, S.TWISTS[0], S.CMODE_RADII[1], 1, constrained=every[::2])
    pose_in = S.perturb(wl.pose, np.random.default_rng(5), (0.0, 1.2), 1.5)
    o = oracle.Oracle(wl, constraint_mode=True, iterations=1)
    out = o.solve(pose_in, wl.targets)
    free = np.setdiff1d(np.arange(32), wl.topo.constrained)
    assert len(free) == 16 and 0 in free
    turn = max(G.rotation_angle(S.rotation(out[s, b, 0:4]), S.rotation(pose_in[s, b, 0:4])) for s in range(wl.n) for b in free)
    scale = np.abs(out[..., 7:10] - pose_in[..., 7:10]).max()
    print(f"untouched rotations max {turn:.3g} (limit {S.CMODE_UNTOUCHED_LIMIT:.3g}), scales {scale:.3g} (limit {S.CMODE_SCALE_LIMIT:.3g})")
    assert np.array_equal(out[..., 4:7], pose_in[..., 4:7])
    assert turn <= S.CMODE_UNTOUCHED_LIMIT and scale <= S.CMODE_SCALE_LIMIT
    moved = max(G.rotation_angle(S.rotation(out[0, b, 0:4]), S.rotation(pose_in[0, b, 0:4])) for b in wl.topo.constrained)
    assert moved > 0.1


# --- controls on the function-level pin: each wrong model must fail on the same inputs -------------
@pytest.mark.parametrize("name,kw", [("centre at min applied once", dict(centre_times=1)),
                                     ("range not halved", dict(half=1.0)),
                                     ("frame arc reversed", dict(reverse_arc=True))])
def test_wrong_twist_models_fail(oracle, name, kw):
    wl, pose_in, out = cmode_case(oracle, "plus_y", 1, S.TWISTS[1])
    worst = cmode_rotation_check(wl, pose_in, out, name, twist_model=S.TwistModel(wl, **kw))
    assert worst > 10 * S.CMODE_ROTATION_LIMIT


def test_wrong_swing_models_fail(oracle):
    wl, pose_in, out = cmode_case(oracle, "realistic_unit_scale", 1, S.FULL_TWIST)
    assert cmode_rotation_check(wl, pose_in, out, "right model") <= S.CMODE_ROTATION_LIMIT
    assert cmode_rotation_check(wl, pose_in, out, "cone 1 % narrower", radius_scale=0.99) > 10 * S.CMODE_ROTATION_LIMIT
    no_d = S.direction_frames(wl, identity=True)
    # (without the frame other bones are outside the cap: only the error is asserted)
    exp = S.expected_cmode(wl, pose_in, no_d, S.TwistModel(wl))[0]
    assert S.rotation_errors(wl, out, exp).max() > 10 * S.CMODE_ROTATION_LIMIT


# --- end state of the ordinary solve ---------------------------------------------------------------
N_SOLVE = 33
END_STATES = [(rig, rest, it) for rig in ("c2", "uneven") for rest in ("plus_y", "realistic_unit_scale") for it in (1, 16)]


@pytest.mark.parametrize("twist", S.TWISTS)
@pytest.mark.parametrize("ncones", [0, 1])
@pytest.mark.parametrize("rig,rest,it", END_STATES)
def test_solve_ends_inside_the_twist_range(oracle, rig, rest, it, ncones, twist):
    c = S.case(rig, rest, it, ncones, twist, N_SOLVE)
    before = c.twist_excess(c.pose_in)
    assert (before > 0.1).mean() > 0.5
    S.check_twist(c, S.oracle_solve(oracle, c), f"{rig} {rest} {it} iterations {ncones} cones {twist}")


@pytest.mark.parametrize("ncones", [1, 2, 3])
@pytest.mark.parametrize("rig,rest,it", END_STATES)
def test_solve_ends_inside_the_swing_region(oracle, rig, rest, it, ncones):
    c = S.case(rig, rest, it, ncones, S.FULL_TWIST, N_SOLVE)
    assert (c.swing(c.pose_in) > 10 * S.SWING_BAND_LIMIT).mean() > 0.5
    out = S.oracle_solve(oracle, c)
    label = f"{rig} {rest} {it} iterations {ncones} cones"
    S.check_swing(c, out, label)
    S.check_rigid(c, out, label)


def test_bones_in_no_segment_are_unchanged(oracle):
    c = S.case("uneven_spare", "plus_y", 16, 1, S.TWISTS[0], N_SOLVE, constrained=np.arange(1, 9))
    inl = S.list_bones(c.wl)
    assert (~inl).sum() == 2
    wl = c.free                                     # (the spare chain carries no constraint)
    o = oracle.Oracle(wl)
    out = o.solve(c.pose_in, wl.targets, threads=8)
    assert np.array_equal(out[:, ~inl], c.pose_in[:, ~inl])
    assert not np.array_equal(out[:, inl], c.pose_in[:, inl])


# --- controls on the end state ---------------------------------------------------------------------
ACTING = [("c2", "plus_y", 16), ("c2", "realistic_unit_scale", 16), ("c2", "plus_y", 1), ("uneven", "realistic_unit_scale", 1)]


@pytest.mark.parametrize("rig,rest,it", ACTING)
def test_twist_limits_act(oracle, rig, rest, it):
    """The same rig solved without constraints, judged by the same twist ranges."""
    c = S.case(rig, rest, it, 1, S.TWISTS[0], N_SOLVE)
    ex = c.twist_excess(S.oracle_solve(oracle, c, constrained=False))
    print(f"unconstrained: {(ex > 10 * S.SOLVE_TWIST_LIMIT).mean():.2f} of the twist limits violated")
    assert (ex > 10 * S.SOLVE_TWIST_LIMIT).mean() >= 0.5


@pytest.mark.parametrize("ncones", [1, 2])
@pytest.mark.parametrize("rig,rest,it", ACTING)
def test_swing_limits_act(oracle, rig, rest, it, ncones):
    c = S.case(rig, rest, it, ncones, S.FULL_TWIST, N_SOLVE)
    res = c.swing(S.oracle_solve(oracle, c, constrained=False))
    print(f"unconstrained: {(res > 10 * S.SWING_BAND_LIMIT).mean():.2f} of the swing limits violated")
    assert (res > 10 * S.SWING_BAND_LIMIT).mean() >= 0.5


@pytest.mark.parametrize("name,kw", [("centre at min applied once", dict(centre_times=1)),
                                     ("range not halved", dict(half=1.0)),
                                     ("frame arc reversed", dict(reverse_arc=True))])
def test_wrong_twist_models_fail_on_the_end_state(oracle, name, kw):
    """A range taken twice as wide cannot be violated by a pose inside the right one: that model
    fails by calling the unconstrained solve's violations acceptable instead."""
    c = S.case("c2", "plus_y", 16, 1, S.TWISTS[1], N_SOLVE)
    wrong = S.TwistModel(c.wl, **kw)
    if name == "range not halved":
        free = S.oracle_solve(oracle, c, constrained=False)
        right, loose = c.twist_excess(free), wrong.excess(c.wl, free)
        assert ((right > 10 * S.SOLVE_TWIST_LIMIT) & (loose <= 0)).sum() >= 40
    else:
        assert wrong.excess(c.wl, S.oracle_solve(oracle, c)).max() > 10 * S.SOLVE_TWIST_LIMIT


def test_wrong_swing_models_fail_on_the_end_state(oracle):
    c = S.case("c2", "realistic_unit_scale", 16, 1, S.FULL_TWIST, N_SOLVE)
    out = S.oracle_solve(oracle, c)
    narrow = S.swing_residual(c.wl, out, c.frames, S.regions(c.wl, 0.99))[0]
    assert narrow.max() > S.SWING_BAND_LIMIT
    no_d = S.swing_residual(c.wl, out, S.direction_frames(c.wl, identity=True), c.regions)[0]
    assert (no_d > 10 * S.SWING_BAND_LIMIT).mean() > 0.25
