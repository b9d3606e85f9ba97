"""The CPU oracle against independent float64 geometry (tests/geometry_f64.py): what the QCP
fit, the Kusudama swing limit, its tangent circles and the Transform3D ops *mean*, beyond the
reference's handful of known-answer tests.  Every other test pins bits to the oracle; these pin
the oracle to the mathematics, so a misreading that the oracle and the kernels share fails here.
tests/test_gpu_geometry.py runs the same generators and checks on the device code.

Every limit is 4 x the worst value this module measures over its fixed seeds (run with -s to see
the figures; DESIGN.md section 7a tabulates them).  Each family has a negative control: the same
comparison against a subtly wrong model must fail.

Not covered, because the reference departs from the textbook operation there:
the one-point QCP path (qcp.cpp:59-78) and the twist limit (ik_kusudama_3d.cpp:103-115)."""
import math
import zlib

import numpy as np
import pytest

from . import geometry_f64 as G

QCP_N = (2, 3, 4, 5, 7, 20, 40, 80)
QCP_CLASSES = [(n, False) for n in QCP_N] + [(n, True) for n in QCP_N if n - n // 3 >= 3 and n // 3 >= 1]
QCP_PRECISION = 1.0e-6  # the solve's own (ik_bone_segment_3d.h:85)
# Two points about their own centroid are antiparallel: the covariance has rank one, the rotation
# about their axis is undetermined, Horn's largest eigenvalue is double and the adjugate vanishes.
# The reference then returns the identity (qcp.cpp:108-109), so no direction claim is made there;
# unit length and the translation still are.
QCP_RANK_ONE = (2, True)
CONE_COUNTS = (1, 2, 3, 4)
# ik_kusudama_3d.cpp:317 accepts a point of a tangent triangle when its projection onto the tangent
# circle has Math::is_equal_approx(cos(angle), 1), CMP_EPSILON = 1e-5: the reference's region reaches
# acos(1 - 1e-5) = 4.47e-3 rad into each tangent cap.  1e-4 more for the float32 cosine's rounding.
TANGENT_CAP_SLACK = math.acos(1.0 - 1.0e-5) + 1.0e-4
LATTICE_BAND = 4 * math.sqrt(4 * math.pi / G.LATTICE_POINTS)


def _seed(*key):
    return zlib.crc32(repr(key).encode())


# --- QCP ------------------------------------------------------------------------------------
def qcp_cases(n, zero_third, translate, count):
    """`count` exact-fit cases of one class; a shorter list is a prefix of a longer one.
    moved ~ N(0, 1) float32, target = float32(R moved [+ t]), R a random-axis rotation by an
    angle uniform in [0, 170] degrees, weights from {0.25, 0.5, 1, 2} and, with zero_third, n//3
    of them zero.  Ill-conditioned draws are redrawn, never skipped: the weighted covariance needs
    sigma_2 >= 0.05 sigma_1 for n >= 3, two points an angle in [20, 160] degrees between them.

    Also redrawn: a fit whose unnormalised eigenvector (geometry_f64.qcp_eigenvector_norm_sq) has a
    squared norm below 100 x the precision.  Below the precision itself the reference gives up and
    returns the identity (qcp.cpp:108-109); that happens for small, lightly weighted point sets
    turned by nearly 180 degrees.  Two points with translate always do: see QCP_RANK_ONE."""
    rng = np.random.default_rng(_seed("qcp", n, zero_third, translate))
    cases = []
    while len(cases) < count:
        moved = rng.normal(size=(n, 3)).astype(np.float32)
        R = G.axis_angle_matrix(rng.normal(size=3), math.radians(rng.uniform(0.0, 170.0)))
        offset = rng.normal(size=3) if translate else np.zeros(3)
        target = (moved.astype(np.float64) @ R.T + offset).astype(np.float32)
        w = rng.choice([0.25, 0.5, 1.0, 2.0], n)
        if zero_third:
            w[rng.choice(n, n // 3, replace=False)] = 0.0
        Rk, S = G.kabsch(moved, target, w, translate)[:2]
        if n == 2:
            ok = math.radians(20) <= G.angle(moved[0], moved[1]) <= math.radians(160)
        else:
            ok = S[1] >= 0.05 * S[0]
        if (n, translate) != QCP_RANK_ONE:
            ok = ok and G.qcp_eigenvector_norm_sq(Rk, S) >= 100 * QCP_PRECISION
        if ok:
            cases.append(dict(moved=moved, target=target, w=w, translate=translate, n=n))
    return cases


def qcp_figures(case, rot, trans, conjugate_model=False):
    """The float64 figures of one result.  conjugate_model: the negative control's wrong model,
    which expects the inverse rotation."""
    R, _, dt, mc, tc = G.kabsch(case["moved"], case["target"], case["w"], case["translate"])
    Rq = G.quat_to_matrix(np.asarray(rot, np.float64))
    if conjugate_model:
        R = R.T
    nz = case["w"] > 0
    m, t = case["moved"].astype(np.float64)[nz] - mc, case["target"].astype(np.float64)[nz] - tc
    fig = dict(unit=abs(np.linalg.norm(np.asarray(rot, np.float64)) - 1.0),
               translation=np.linalg.norm(np.asarray(trans, np.float64) - dt) / (1 + np.linalg.norm(tc) + np.linalg.norm(mc)))
    if (case["n"], case["translate"]) != QCP_RANK_ONE:
        key = "direction_deg" if case["n"] >= 3 else "direction2_deg"
        fig[key] = math.degrees(G.angle(m @ (Rq.T if conjugate_model else Rq).T, t).max())
    if case["n"] >= 3:
        fig["kabsch_deg"] = math.degrees(G.rotation_angle(Rq, R))
    return fig


def worst(figs):
    keys = sorted({k for f in figs for k in f})
    return {k: max(f[k] for f in figs if k in f) for k in keys}


def qcp_failures(w):
    """The names of the limits that a dict of worst figures breaks."""
    limits = dict(unit=G.QCP_UNIT_LIMIT, direction_deg=G.QCP_DIRECTION_LIMIT_DEG, direction2_deg=G.QCP_DIRECTION2_LIMIT_DEG,
                  kabsch_deg=G.QCP_KABSCH_LIMIT_DEG, translation=G.QCP_TRANSLATION_LIMIT)
    return [k for k, v in w.items() if not v <= limits[k]]


@pytest.mark.parametrize("translate", [False, True], ids=["fixed", "translate"])
@pytest.mark.parametrize("n,zero_third", QCP_CLASSES, ids=lambda v: f"n{v}" if not isinstance(v, bool) else ("zeros" if v else "dense"))
def test_qcp_exact_fit_is_the_kabsch_rotation(oracle, n, zero_third, translate):
    figs = []
    for case in qcp_cases(n, zero_third, translate, 200):
        rot, trans = oracle.qcp(case["moved"], case["target"], case["w"], translate, QCP_PRECISION)
        figs.append(qcp_figures(case, rot, trans))
    w = worst(figs)
    print(f"qcp n={n} zeros={zero_third} translate={translate}: " + " ".join(f"{k}={v:.3g}" for k, v in w.items()))
    assert not qcp_failures(w), w


def test_qcp_noisy_fit_is_unit_and_finite(oracle):
    """With noise the fit is approximate: the reference keeps max_eigenvalue at its initial value
    (ss1 + ss2) / 2 and takes no Newton step (qcp.cpp:215), which is the largest eigenvalue only
    for an exact fit.  So only unit length and finiteness are asserted.  Characterisation, not a
    bound: at Gaussian noise 1e-3 on the targets the angle to the Kabsch rotation was up to
    1.7e-3 degrees over these seeds (printed)."""
    rng = np.random.default_rng(_seed("qcp-noise"))
    seen = 0.0
    for n in QCP_N[1:]:
        for translate in (False, True):
            for case in qcp_cases(n, False, translate, 25):
                noisy = dict(case, target=(case["target"] + rng.normal(scale=1e-3, size=(n, 3))).astype(np.float32))
                rot, trans = oracle.qcp(noisy["moved"], noisy["target"], noisy["w"], translate, QCP_PRECISION)
                assert np.isfinite(rot).all() and np.isfinite(trans).all()
                fig = qcp_figures(noisy, rot, trans)
                assert fig["unit"] <= G.QCP_UNIT_LIMIT
                seen = max(seen, fig["kabsch_deg"])
    print(f"qcp noise 1e-3: angle to Kabsch up to {seen:.3g} deg (not asserted)")


def test_control_conjugated_rotation_fails(oracle):
    for n, translate in ((2, False), (3, True), (20, False), (80, True)):
        figs = []
        for case in qcp_cases(n, False, translate, 200):
            rot, trans = oracle.qcp(case["moved"], case["target"], case["w"], translate, QCP_PRECISION)
            figs.append(qcp_figures(case, rot, trans, conjugate_model=True))
        bad = qcp_failures(worst(figs))
        assert ("direction_deg" in bad and "kabsch_deg" in bad) if n >= 3 else "direction2_deg" in bad, (n, bad)


# --- cone chains ------------------------------------------------------------------------------
def random_chain(rng, k):
    """k cones [k][4] float32: consecutive control points 0.5-2.0 rad apart, radii 0.1-0.7 rad.
    A draw whose consecutive caps nest (distance <= |rA - rB| + 0.05) is redrawn: no circle is
    tangent to both caps then, and the tangent-circle definition has no solution."""
    while True:
        c = [G.unit(rng.normal(size=3))]
        for _ in range(k - 1):
            side = G.unit(np.cross(c[-1], rng.normal(size=3)))
            d = rng.uniform(0.5, 2.0)
            c.append(math.cos(d) * c[-1] + math.sin(d) * side)
        r = rng.uniform(0.1, 0.7, k)
        cones = np.concatenate([np.array(c), r[:, None]], axis=1).astype(np.float32)
        if all(G.angle(cones[i, :3], cones[i + 1, :3]) > abs(float(cones[i, 3]) - float(cones[i + 1, 3])) + 0.05 for i in range(k - 1)):
            return cones


def chains(k, count, tag="swing"):
    rng = np.random.default_rng(_seed(tag, k))
    return [random_chain(rng, k) for _ in range(count)]


def query_points(cones, count):
    rng = np.random.default_rng(_seed("points", cones.tobytes()))
    return G.unit(rng.normal(size=(count, 3))).astype(np.float32)


def tangent_figures(cone_tangents, swap_sides=False, radius_offset=0.0):
    """Worst figures of cone_tangents(cones) -> [n][8] (tc1, tc2, radius, cos) over 200 chains of
    2-4 cones against the closed form.  swap_sides / radius_offset: the controls' wrong models."""
    rng = np.random.default_rng(_seed("tangents"))
    fig = dict(pair=0.0, ordered=0.0, radius=0.0, wrong_side=0)
    for _ in range(200):
        cones = random_chain(rng, int(rng.integers(2, 5)))
        got = np.asarray(cone_tangents(cones), np.float64)
        for i in range(len(cones) - 1):
            A, B = cones[i, :3].astype(np.float64), cones[i + 1, :3].astype(np.float64)
            tn, tp, tr = G.tangent_circles(A, float(cones[i, 3]), B, float(cones[i + 1, 3]))
            if swap_sides:
                tn, tp = tp, tn
            t1, t2 = got[i, :3], got[i, 3:6]
            straight = max(np.linalg.norm(t1 - tn), np.linalg.norm(t2 - tp))
            crossed = max(np.linalg.norm(t1 - tp), np.linalg.norm(t2 - tn))
            fig["pair"] = max(fig["pair"], min(straight, crossed))   # as an unordered pair
            fig["ordered"] = max(fig["ordered"], straight)           # tc1 is the centre on the negative side of A x B
            fig["wrong_side"] += int(not (t1 @ np.cross(A, B) < 0 < t2 @ np.cross(A, B))) if not swap_sides else \
                int(not (t1 @ np.cross(A, B) > 0 > t2 @ np.cross(A, B)))
            fig["radius"] = max(fig["radius"], abs(got[i, 6] - (tr + radius_offset)))
    return fig


def tangent_failures(fig):
    bad = [k for k, lim in (("pair", G.TANGENT_CENTRE_LIMIT), ("ordered", G.TANGENT_CENTRE_LIMIT), ("radius", G.TANGENT_RADIUS_LIMIT))
           if not fig[k] <= lim]
    return bad + (["wrong_side"] if fig["wrong_side"] else [])


def test_tangent_circles_match_the_closed_form(oracle):
    """The centres as an unordered pair, then that tc1 is the one on the negative side of A x B
    (the tangent-triangle test relies on it), and the radius (pi - rA - rB) / 2."""
    fig = tangent_figures(oracle.cone_tangents)
    print(f"tangent circles: centre error {fig['pair']:.3g} (ordered {fig['ordered']:.3g}), radius error {fig['radius']:.3g}, "
          f"wrong-side pairs {fig['wrong_side']}")
    assert not tangent_failures(fig), fig


def test_control_wrong_tangent_model_fails(oracle):
    """The centres on each other's sides still match as a pair and must fail the side test; a
    radius 0.01 rad larger must fail the radius."""
    bad = tangent_failures(tangent_figures(oracle.cone_tangents, swap_sides=True))
    assert "ordered" in bad and "wrong_side" in bad and "pair" not in bad, bad
    assert tangent_failures(tangent_figures(oracle.cone_tangents, radius_offset=0.01)) == ["radius"]


# --- swing limit --------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lattice():
    return G.fibonacci_sphere()


def swing_figures(cones, points, query, lattice, model=G.SwingRegion):
    """Assertions (a)-(e) as figures for one chain.  query(point) -> (result [3], in_bounds);
    model(cones) builds the float64 region (the controls pass a wrong one)."""
    region = model(cones)
    p = G.unit(points)
    member, left = region.member(p), region.left_out(p, TANGENT_CAP_SLACK)
    results = [query(pt) for pt in points]
    out = np.array([r[0] for r in results], np.float64)
    inb = np.array([r[1] > 0 for r in results])
    fig = dict(points=len(points), left_out=int(left.sum()), misclassified=int(((inb != member) & ~left).sum()))
    if inb.any():
        fig["unchanged"] = np.abs(out[inb] - p[inb]).max()
    o = ~inb
    if o.any():
        members = region.members_near_boundary(lattice, LATTICE_BAND)
        fig["unit"] = np.abs(np.linalg.norm(out[o], axis=1) - 1.0).max()
        fig["boundary"] = region.boundary_distance(out[o]).max()
        fig["nearest"] = (G.angle(out[o], p[o]) - G.nearest_members(members, p[o])[1]).max()
        fig["region"] = G.nearest_members(members, out[o])[1].max()
    return fig


def swing_total(figs):
    tot = worst(figs)
    for k in ("points", "left_out", "misclassified"):
        tot[k] = sum(f[k] for f in figs)
    return tot


def swing_failures(t):
    limits = dict(unchanged=G.SWING_UNCHANGED_LIMIT, unit=G.SWING_UNIT_LIMIT, boundary=G.SWING_BOUNDARY_LIMIT,
                  nearest=G.SWING_NEAREST_LIMIT, region=G.SWING_REGION_LIMIT)
    bad = [k for k, lim in limits.items() if k in t and not t[k] <= lim]
    if t["misclassified"]:
        bad.append("misclassified")
    if t["left_out"] > G.LEFT_OUT_CAP * t["points"]:
        bad.append("left_out")
    return bad


@pytest.mark.parametrize("k", CONE_COUNTS)
def test_swing_limit_is_the_nearest_point_of_the_region(oracle, lattice, k):
    """(a) in_bounds > 0 exactly for members of the float64 region, (b) a member comes back as the
    normalised input, (c) any other result is unit and on a boundary circle, (d) no farther from
    the query than the nearest lattice member and (e) within a lattice spacing of a member.

    Left out of (a) only: points within 1e-3 rad of a boundary circle, and points of a tangent cap
    up to acos(1 - 1e-5) = 4.5e-3 rad inside it, where ik_kusudama_3d.cpp:317 accepts a tangent
    triangle's projection by Math::is_equal_approx(cos, 1).  The share is asserted <= 2 %."""
    figs = [swing_figures(c, query_points(c, 150), lambda p: oracle.local_point_in_limits(c, p), lattice) for c in chains(k, 12)]
    t = swing_total(figs)
    print(f"swing {k} cones: left out {t['left_out']}/{t['points']} = {t['left_out'] / t['points']:.2%} " +
          " ".join(f"{key}={v:.3g}" for key, v in t.items() if key not in ("points", "left_out")))
    assert not swing_failures(t), t


def _wider_cone(cones):
    r = G.SwingRegion(cones)
    r.r[0] *= 1.01
    return G.SwingRegion(np.concatenate([r.c, r.r[:, None]], axis=1))


CONTROLS = [("radius_1pct", _wider_cone, (1, 2, 3, 4), "boundary"),
            ("swapped_sides", lambda c: G.SwingRegion(c, swap_sides=True), (2, 3, 4), "misclassified"),
            ("tangent_radius_plus_0.01", lambda c: G.SwingRegion(c, tangent_radius_offset=0.01), (2, 3, 4), "boundary")]


@pytest.mark.parametrize("name,model,counts,must_fail", CONTROLS, ids=[c[0] for c in CONTROLS])
def test_control_wrong_swing_model_fails(oracle, lattice, name, model, counts, must_fail):
    """A cone 1 % wider, the tangent centres on each other's sides, a tangent radius 0.01 rad
    larger: against each the oracle must miss the named check, on the same chains and points.
    Measured: the boundary residual becomes 5.9e-3 to 1.0e-2 rad against a limit of 6.8e-4, and
    swapped sides misclassify a quarter to a half of the points."""
    for k in counts:
        figs = [swing_figures(c, query_points(c, 150), lambda p: oracle.local_point_in_limits(c, p), lattice, model)
                for c in chains(k, 12)]
        bad = swing_failures(swing_total(figs))
        print(f"control {name}, {k} cones: fails {bad}")
        assert must_fail in bad, (name, k, bad)


# --- Transform3D ----------------------------------------------------------------------------------
def xform_cases(count=200):
    """Random affine transforms (rows | origin, float32) with condition number <= 100, in pairs."""
    rng = np.random.default_rng(_seed("xform"))
    out = []
    while len(out) < 2 * count:
        x = rng.normal(size=12).astype(np.float32)
        if np.linalg.cond(x[:9].reshape(3, 3).astype(np.float64)) <= 100:
            out.append(x)
    return list(zip(out[::2], out[1::2]))


def xform_ratios(a, b, mul, inv, wrong_order=False):
    """worst |error| / bound of a * b and of affine_inverse(a); the bounds come from the operands
    (geometry_f64.xform_*_f64), no tuned constant.  wrong_order: the control's model, b * a."""
    val, bound = G.xform_mul_f64(b, a) if wrong_order else G.xform_mul_f64(a, b)
    ival, ibound = G.xform_affine_inverse_f64(a)
    return (np.abs(mul.astype(np.float64) - val) / bound).max(), (np.abs(inv.astype(np.float64) - ival) / ibound).max()


def test_transform_ops_within_rounding_bounds_of_float64(oracle):
    rm = ri = rc = 0.0
    for a, b in xform_cases():
        mul, inv = oracle.xform_mul(a, b), oracle.xform_affine_inverse(a)
        m, i = xform_ratios(a, b, mul, inv)
        rm, ri = max(rm, m), max(ri, i)
        rc = max(rc, xform_ratios(a, b, mul, inv, wrong_order=True)[0])
    print(f"transform: worst error / bound: product {rm:.3f}, affine inverse {ri:.3f}; control (b * a) {rc:.3g}")
    assert rm <= 1.0 and ri <= 1.0
    assert rc > 1.0  # negative control: the product in the other order is outside the bound
