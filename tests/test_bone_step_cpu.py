"""The CPU oracle's bone-steps against the float64 model of tests/bone_step_f64.py: segmentation and
heading counts exactly, then every segment_solver call, one and two whole iterations, the damp
clamp's two classes, the stabilization decisions and the weight-0 identity, judged by rotation angle
and relative origin error (tests/bone_step_cases.py holds the rigs, measures and limits; DESIGN.md
section 7a, "The bone-step: what one step means", the table).  The negative controls read the model
wrongly one way at a time and must fall outside the same limits."""
import numpy as np
import pytest

from many_bone_ik_amd.solver import describe_topology

from . import bone_step_cases as B
from . import bone_step_f64 as M

BASE_IDS = ["-".join(k) for k in B.BASE]


@pytest.mark.parametrize("rig", B.RIGS)
@pytest.mark.parametrize("pins", ["default", "origin_only", "weight0"])
def test_segmentation_and_heading_counts(oracle, mbik, rig, pins):
    """The model's bone list, post-order segment table and heading counts are the library's and the
    oracle's, exactly.  On midpin the factor-0 pin cuts a descent: its segment sees one pin."""
    c = B.case(rig, "plus_y", pins)
    o = c.oracle(oracle)
    root, tip, nh = o.segment_table()
    d = describe_topology(c.wl.topo.parents, c.wl.pins(), [], iterations=1)
    for name, got in (("oracle", (o.bone_list(), root, tip, nh)), ("library", (d["bone_list"], d["seg_root"], d["seg_tip"], d["seg_headings"]))):
        assert list(got[0]) == c.topo.bone_list, name
        for a, b in zip(got[1:], c.topo.table):
            assert np.array_equal(a, b), (name, a, b)
    o.close()
    if rig == "midpin":
        per_pin = 1 if pins == "origin_only" else 5
        assert sorted(c.topo.table[2].tolist()) == sorted([per_pin] * 4 + [2 * per_pin] * 2 + [5 * per_pin])
        cut = [s for s in c.topo.segments if s.tip == 2][0]
        assert len(cut.effectors) == 1 and len(cut.children) == 1


def test_falloff_weights():
    """Heading weights of the midpin rig's parentless segment: weight * falloff once, then
    weight * (priority / max priority) * falloff twice per positive priority; the chain under the
    factor-0.5 pin weighs half, the one under the factor-0 pin is not reached."""
    c = B.base_case("midpin", "plus_y", "mixed")
    w = c.topo.segments[-1].weights
    lo, hi = float(np.float32(0.35)), 1.0
    pins_w = c.wl.pin_weight.astype(np.float64)
    assert pins_w.tolist() == [lo, hi, lo, hi, lo, hi]
    want = []
    for i, fall in ((0, 1.0), (2, 1.0), (3, 0.5), (4, 1.0), (5, 1.0)):     # mid 0 | mid 0.5, its leaf | mid 1, its leaf
        want += [pins_w[i] * fall] * 3 + [pins_w[i] * 0.5 * fall] * 2     # priorities (1, 0.5, 0)
    assert np.allclose(w, want, rtol=1e-15, atol=0)


@pytest.mark.parametrize("rig,rest,pins", B.BASE, ids=BASE_IDS)
def test_segment_solve(oracle, rig, rest, pins):
    """segment_solver of every segment: stepped bones against the model, all others untouched."""
    c = B.base_case(rig, rest, pins)
    lo = []
    for seg in range(len(c.topo.segments)):
        out = B.oracle_out(oracle, c, "segment", seg)
        lo.append(B.check_segment(c, out, seg, f"{c.label} segment {seg}"))
    share = float(np.mean(np.concatenate(lo)))
    print(f"{c.label}: {share:.4f} of {sum(len(x) for x in lo)} steps left out")
    assert share <= B.LEFT_OUT_CAP


@pytest.mark.parametrize("iterations", [1, 2])
@pytest.mark.parametrize("rig,rest,pins", B.BASE, ids=BASE_IDS)
def test_iterations(oracle, rig, rest, pins, iterations):
    c = B.base_case(rig, rest, pins)
    B.check_iterations(c, B.oracle_out(oracle, c, "solve", iterations), iterations, f"{c.label} {iterations} iterations")


def test_one_point_path_is_taken(oracle):
    """With priorities (0, 0, 0) every segment that sees one pin fits one heading, and the angle the
    reference turns by there is not the angle between the two headings."""
    c = B.base_case("uneven", "plus_y", "origin_only")
    _, records = c.model_iterations(1)
    one = [r for r in records if len(r["segment"].weights) == 1]
    assert len(one) == 8 and all(np.isinf(r["nsq"]).all() for r in one)
    state = M.State(c.pose_in)
    r = one[1]          # the first chain's second bone from the tip: both headings have length
    for prior in records[:1]:
        state.basis[:, prior["bone"]], state.origin[:, prior["bone"]] = prior["post"]
    Gb, Go = state.globals(c.rig.parents)
    Tb, To = M._targets(c.wl.targets)
    target, tip = M.headings(c.rig, r["segment"], r["bone"], Gb, Go, c.D, Tb, To)
    between = B.G.angle(tip[:, 0], target[:, 0])
    assert np.abs(r["fit_angle"] - between).max() > 0.05


@pytest.mark.parametrize("rig,rest,d", B.DAMP_CASES, ids=["-".join(k) for k in B.DAMP_CASES])
def test_damp_classes(oracle, rig, rest, d):
    c = B.damp_case(rig, rest, d)
    damps = {M.damp_of(c.rig, s, b) for s in c.topo.segments if s.parent is not None for b in s.bones}
    assert len(damps) == 2 and max(damps) == float(np.float32(B.DAMPS[d][0]))     # an entry below the default, and the default
    B.check_damp_classes(c, B.oracle_out(oracle, c, "solve", 1), f"{c.label} damp {d}")
    B.check_iterations(c, B.oracle_out(oracle, c, "solve", 1), 1, f"{c.label} damp {d}")


@pytest.mark.parametrize("iterations", [1, 2])
@pytest.mark.parametrize("passes", [1, 3])
@pytest.mark.parametrize("rest", B.RESTS)
def test_stabilization(oracle, rest, passes, iterations):
    c = B.stabilized_case(rest, passes)
    B.check_stabilized(c, B.oracle_out(oracle, c, "solve", iterations), iterations, f"{c.label} passes {passes} iterations {iterations}")


@pytest.mark.parametrize("rest", B.RESTS)
@pytest.mark.parametrize("rig", B.RIGS)
def test_weight_zero_is_the_identity(oracle, rig, rest):
    c = B.case(rig, rest, "weight0")
    B.check_weight0(c, B.oracle_out(oracle, c, "solve", 1), f"{c.label}")


# --- negative controls: the model read wrongly, on the same inputs --------------------------------------
def _stabilized():
    return [B.stabilized_case(rest, passes) for rest in B.RESTS for passes in (1, 3)]


# misreading -> (cases, iterations, rotation limit, origin limit, share of cases observed outside the limit)
CONTROLS = {
    "swapped_sets": (lambda: [B.base_case(*k) for k in B.BASE], 1, B.ITERATION_ROTATION_LIMIT, B.ITERATION_ORIGIN_LIMIT, 22 / 24),
    "target_origin_of_stepped_bone": (lambda: [B.base_case(*k) for k in B.BASE], 1, B.ITERATION_ROTATION_LIMIT, B.ITERATION_ORIGIN_LIMIT, 24 / 24),
    "target_pairs_unweighted": (lambda: [B.base_case(*k) for k in B.BASE], 1, B.ITERATION_ROTATION_LIMIT, B.ITERATION_ORIGIN_LIMIT, 10 / 24),
    "tip_without_priority": (lambda: [B.base_case(*k) for k in B.BASE], 1, B.ITERATION_ROTATION_LIMIT, B.ITERATION_ORIGIN_LIMIT, 16 / 24),
    "no_distance_scale": (lambda: [B.base_case(*k) for k in B.BASE], 1, B.ITERATION_ROTATION_LIMIT, B.ITERATION_ORIGIN_LIMIT, 15 / 24),
    "no_falloff": (lambda: [B.base_case(*k) for k in B.BASE], 1, B.ITERATION_ROTATION_LIMIT, B.ITERATION_ORIGIN_LIMIT, 6 / 24),
    "clamp_cos_damp": (lambda: [B.damp_case(*k) for k in B.DAMP_CASES], 1, B.ITERATION_ROTATION_LIMIT, B.ITERATION_ORIGIN_LIMIT, 8 / 8),
    "larger_damp": (lambda: [B.damp_case(*k) for k in B.DAMP_CASES], 1, B.ITERATION_ROTATION_LIMIT, B.ITERATION_ORIGIN_LIMIT, 8 / 8),
    "root_damped": (lambda: [B.base_case(*k) for k in B.BASE], 1, B.ITERATION_ROTATION_LIMIT, B.ITERATION_ORIGIN_LIMIT, 22 / 24),
    "translate_everywhere": (lambda: [B.base_case(*k) for k in B.BASE], 1, B.ITERATION_ROTATION_LIMIT, B.ITERATION_ORIGIN_LIMIT, 18 / 24),
    "msd_divided_once": (_stabilized, 2, B.STABILIZED_ROTATION_LIMIT, B.STABILIZED_ORIGIN_LIMIT, 0 / 4),
    "previous_never_reset": (_stabilized, 2, B.STABILIZED_ROTATION_LIMIT, B.STABILIZED_ORIGIN_LIMIT, 4 / 4),
}
assert tuple(CONTROLS) == M.MISREADINGS


@pytest.mark.parametrize("misread", M.MISREADINGS)
def test_negative_control(oracle, misread):
    """The share of cases whose worst error against the wrongly read model exceeds the limit is at
    least half of what was observed when the limits were set."""
    make, iterations, rot_limit, origin_limit, observed = CONTROLS[misread]
    cases = make()
    outside = 0
    for c in cases:
        rot, org = B.control_error(c, B.oracle_out(oracle, c, "solve", iterations), iterations, misread)
        outside += rot > rot_limit or org > origin_limit
    share = outside / len(cases)
    print(f"{misread}: {outside}/{len(cases)} cases outside the limit ({share:.3f}; observed {observed:.3f})")
    assert share >= observed / 2
