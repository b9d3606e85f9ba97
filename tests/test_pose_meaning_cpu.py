"""What the four pose stages around the solve mean: mbik_clip_sample_cpu, mbik_pose_blend_cpu,
mbik_pose_globals_cpu and the capture arithmetic against the independent float64 models of
tests/pose_models_f64.py, whose docstring derives every bound used here.  The bitwise recipe tests
(test_clip_sample_cpu, test_pose_blend_cpu, test_pose_globals_cpu, test_gpu_capture) pin the bits; a
misreading shared by a recipe and the code would pass them, and fails here.

Derived bounds (pose_models_f64): lerped positions and scales of a clip sample, the blend's origin,
every global, skin transform and pin distance, every captured target.  Copied keys, rest poses and
the blend's early outs are compared exactly.

Measured tolerances.  Two quantities have no derived bound, because the float32 code reaches them
through acosf / sinf or through a decomposition.  Each was measured on the CPU as the float32 recipe
(blend_recipe.expected, clip_recipe.expected: not the code under test) against the float64 model over
the seeded cases of this module (python -m tests.test_pose_meaning_cpu prints them); the tests allow
4 times the observed maximum, the margin covering seeds not tried:
    clip rotation   angle between the sampled quaternion and the model's, over the interpolated
                    rotations of clip_case() whose key arc is below pi - 0.05:
                    observed 2.85e-7 rad over 5,692 rotations, allowed 1.14e-6 rad (CLIP_ANGLE_BOUND)
    blend           max |R(q_out) diag(s_out) - R_w diag(S_w)| / max |S_w| over the judged bones of
                    blend_cases() (mixed_inputs(3, 8000) at BLEND_WEIGHTS, and at 0.5 on the pairs
                    whose determinants agree in sign):
                    observed 7.23e-7 (at w = 0.75) over 36,789 bones, allowed 2.89e-6 (BLEND_BOUND)

Conditions (not measurements): a blended bone is judged only where the rotation from R_A to R_M is
below pi - 0.05 and min |S_w| >= 0.1; a clip rotation only where the arc between its two keys is
below pi - 0.05.  At most 10 % of the blended bones may be left out in all and at most half of any
input kind (the model alone leaves out 7.2 % and 46.4 % of near_pi_axis).

Every control test swaps one wrong reading into the model -- the long arc, diag(s) R, local * parent,
the wrap pair (first, second), a key search with side="left", inverse(node) * skeleton -- and the
entry must then leave the bound on the stated share of the cases the reading touches."""
import math

import numpy as np
import pytest

from many_bone_ik_amd import _lib
from many_bone_ik_amd import animation as A
from many_bone_ik_amd import workloads as W
from many_bone_ik_amd.solver import pose_blend_cpu

from . import blend_recipe as BR
from . import clip_recipe as CR
from . import pose_globals_recipe as GR
from . import pose_models_f64 as M

CLIP_ANGLE_OBSERVED = 2.85e-7
CLIP_ANGLE_BOUND = 4 * CLIP_ANGLE_OBSERVED
BLEND_OBSERVED = 7.23e-7
BLEND_BOUND = 4 * BLEND_OBSERVED

KEY_COUNTS = tuple(range(21)) + (31, 32, 33, 63, 64, 65)
CLIP_MODES = ((A.LOOP_NONE, 1), (A.LOOP_LINEAR, 1), (A.LOOP_LINEAR, 0))   # (loop_mode, loop_wrap)
BLEND_WEIGHTS = (0.0, 1e-7, 0.25, 0.75, 0.9, 1.0 - 2.0 ** -24)
LEFT_OUT_TOTAL, LEFT_OUT_KIND = 0.10, 0.5


# --- clip sampling ----------------------------------------------------------------------------
def meaning_clips(seed, B):
    """(rest, clips): six clips -- LOOP_NONE, LOOP_LINEAR with loop_wrap, LOOP_LINEAR without, each
    twice with nearest and linear exchanged -- whose (bone, channel) tracks cycle through KEY_COUNTS,
    the three channels of a bone nine counts apart (so the shared search starts above a channel's own
    power of two).  Key rotations are unrelated unit quaternions.  A third of the tracks keep their
    keys inside (0, length), a third have keys at 0 and at length, a third at 0 only."""
    rng = np.random.default_rng(seed)
    q = rng.normal(0.0, 1.0, (B, 4))
    rest = np.concatenate([q / np.linalg.norm(q, axis=1, keepdims=True), rng.uniform(-1.0, 1.0, (B, 3)),
                           rng.uniform(0.5, 1.5, (B, 3))], axis=1).astype(np.float32)
    clips = []
    for k in range(6):
        loop_mode, wrap = CLIP_MODES[k % 3]
        length = float(rng.uniform(1.0, 3.0))
        tracks = []
        for bone in range(B):
            for ch in (A.POSITION, A.ROTATION, A.SCALE):
                n = KEY_COUNTS[(bone + 9 * ch + 5 * (k % 3)) % len(KEY_COUNTS)]
                if n == 0:
                    continue
                times = np.sort(rng.uniform(0.05 * length, 0.95 * length, n))
                assert n == 1 or np.diff(times).min() > 0
                edge = (bone + ch + k) % 3
                if edge >= 1:
                    times[0] = 0.0
                if edge == 1 and n > 1:
                    times[-1] = length
                if ch == A.ROTATION:
                    v = rng.normal(0.0, 1.0, (n, 4))
                    v /= np.linalg.norm(v, axis=1, keepdims=True)
                else:
                    v = rng.uniform(-1.0, 1.0, (n, 3)) if ch == A.POSITION else rng.uniform(0.5, 1.5, (n, 3))
                tracks.append(dict(bone=bone, channel=ch, interpolation=(bone + ch + k // 3) % 2, loop_wrap=wrap,
                                   times=times, values=v.astype(np.float32)))
        clips.append(dict(length=length, loop_mode=loop_mode, tracks=tracks))
    return rest, clips


def meaning_times(seed, clips, tracks_per_clip=5, keys_per_track=6, uniform=12):
    """(time [n], clip_index [n]): per clip the times below 0, beyond the length, at 0 and at the
    length, several lengths away; exactly on keys of some of its tracks, and those keys one and two
    lengths away; half way into the gap across the loop; and uniform ones."""
    rng = np.random.default_rng(seed)
    t, ci = [], []
    for k, clip in enumerate(clips):
        L = clip["length"]
        ts = [0.0, L, -0.3 * L, -L, -2.5 * L, 1.5 * L, 3.0 * L, 7.25 * L, 41.625 * L, -17.3 * L, 0.5 * L]
        for j in rng.permutation(len(clip["tracks"]))[:tracks_per_clip]:
            T = clip["tracks"][j]["times"]
            some = {0, len(T) - 1} | set(rng.integers(0, len(T), keys_per_track - 2).tolist())
            for x in T[sorted(some)]:
                ts += [x, x + L, x - 2.0 * L]
            ts += [T[0] / 2.0, (T[-1] + L) / 2.0]
        ts += list(rng.uniform(-L, 2.0 * L, uniform))
        t += ts
        ci += [k] * len(ts)
    return np.array(t, np.float64), np.array(ci, np.int32)


def clip_case(B=27, seed=61):
    rest, clips = meaning_clips(seed, B)
    t, ci = meaning_times(seed + 1, clips)
    return B, rest, clips, t, ci


def clip_figures(got, model):
    """(exact mismatches, worst lerp error over its bound, judged rotation angles, left-out share) of
    sampled poses got [n][B][10] against a clip_sample_f64 result."""
    g = got.astype(np.float64)
    bound, value = model["bound"], model["value"]
    exact = bound == 0
    mismatches = int((g[exact] != value[exact]).sum())
    lerped = bound > 0
    ratio = float((np.abs(g[lerped] - value[lerped]) / bound[lerped]).max())
    rot = model["interp"][:, :, M.ROTATION]
    judged = rot & (model["arc"] < math.pi - M.ARC_MARGIN)
    angles = M.quat_angle(g[judged][:, 0:4], value[judged][:, 0:4])
    return mismatches, ratio, angles, 1.0 - judged.sum() / rot.sum()


@pytest.fixture(scope="module")
def clip_results(mbik):
    """(case, entry's poses, model), computed once."""
    case = clip_case()
    B, rest, clips, t, ci = case
    return case, A.clip_sample_cpu(B, rest, clips, t, ci), M.clip_sample_f64(B, rest, clips, t, ci)


def test_clip_inputs_cover_the_issue(clip_results):
    (B, rest, clips, t, ci), got, model = clip_results
    seen = {(tr["channel"], len(tr["times"]), tr["interpolation"], clip["loop_mode"], tr["loop_wrap"])
            for clip in clips for tr in clip["tracks"]}
    for ch in (0, 1, 2):
        for n in KEY_COUNTS[1:]:
            for interpolation in (0, 1):
                for mode in CLIP_MODES:
                    assert (ch, n, interpolation) + mode in seen, (ch, n, interpolation, mode)
    per_bone = {}
    for tr in clips[0]["tracks"]:
        per_bone.setdefault(tr["bone"], set()).add(len(tr["times"]))
    assert all(len(v) == 3 for b, v in per_bone.items() if len([1 for tr in clips[0]["tracks"] if tr["bone"] == b]) == 3)
    how = model["how"]
    for code in (M.UNTRACKED, M.SINGLE, M.CLAMP_FIRST, M.CLAMP_LAST, M.INTERIOR, M.WRAP_BEFORE, M.WRAP_AFTER):
        assert (how == code).sum() >= 200, code
    assert model["on_key"].sum() >= 500 and (model["on_key"] & model["interp"]).sum() >= 100
    L = np.array([c["length"] for c in clips])[ci]
    assert (t < 0).sum() >= 30 and (t > L).sum() >= 30 and (t == 0).sum() >= 6 and (t == L).sum() >= 6 and (np.abs(t) > 5 * L).sum() >= 12


def test_clip_entry_stays_within_the_float64_meaning(clip_results):
    case, got, model = clip_results
    assert np.isfinite(got).all()
    mismatches, ratio, angles, left_out = clip_figures(got, model)
    print(f"clip: {model['interp'].sum()} interpolated channels; worst lerp error over its bound {ratio:.3f}; "
          f"worst rotation angle {angles.max():.3e} rad over {angles.size} (bound {CLIP_ANGLE_BOUND:.3e}); "
          f"rotations left out {left_out:.3%}")
    assert mismatches == 0            # copied keys and rest poses: the same keys, no tolerance
    assert ratio <= 1.0
    assert (angles <= CLIP_ANGLE_BOUND).all()
    assert left_out <= LEFT_OUT_TOTAL and angles.size >= 3000


def _clip_control(clip_results, **wrong):
    (B, rest, clips, t, ci), got, right = clip_results
    return got, right, M.clip_sample_f64(B, rest, clips, t, ci, **wrong)


def test_control_long_arc_slerp_fails_clip(clip_results):
    """A slerp that never negates the second key goes the long way round wherever the keys' dot
    product is negative: about half of the interpolated rotations; at least 30 % must leave the bound."""
    got, right, wrong = _clip_control(clip_results, long_arc=True)
    judged = right["interp"][:, :, M.ROTATION] & (right["arc"] < math.pi - M.ARC_MARGIN) & (right["arc"] > 0.1)
    angles = M.quat_angle(got[judged][:, 0:4].astype(np.float64), wrong["value"][judged][:, 0:4])
    share = (angles > CLIP_ANGLE_BOUND).mean()
    print(f"control long arc (clip): {share:.1%} of {angles.size} rotations outside the bound")
    assert share >= 0.30


def test_control_wrap_pair_first_second_fails(clip_results):
    """Wrapping from the second key instead of the last: every wrap sample of a track with three or
    more keys interpolates from another key; at least 90 % of those lerps must leave the bound."""
    got, right, wrong = _clip_control(clip_results, wrap_pair="second")
    g = got.astype(np.float64)
    wraps = (right["how"] >= M.WRAP_BEFORE) & right["interp"]
    wraps[:, :, M.ROTATION] = False
    counts = np.zeros(right["how"].shape[1:], int)
    for tr in clip_results[0][2][1]["tracks"]:      # clip 1 is the wrapping one; its key counts hold for clip 4 too
        counts[tr["bone"], tr["channel"]] = len(tr["times"])
    ci = clip_results[0][4]
    wraps &= ((ci == 1)[:, None, None] & (counts >= 3)[None])
    bad = np.zeros(wraps.shape, bool)
    for ch in (M.POSITION, M.SCALE):
        sl = M.SLICE[ch]
        b = np.where(wrong["bound"][:, :, sl] > 0, wrong["bound"][:, :, sl], right["bound"][:, :, sl])
        bad[:, :, ch] = (np.abs(g[:, :, sl] - wrong["value"][:, :, sl]) > b).any(axis=2)
    share = bad[wraps].mean()
    print(f"control wrap pair: {share:.1%} of {wraps.sum()} wrapped lerps outside the bound")
    assert wraps.sum() >= 300 and share >= 0.90


def test_control_key_search_side_left_fails(clip_results):
    """searchsorted(side="left") finds the last key < t': on a nearest track sampled exactly on a key
    (not the first of a clamped track) it copies the key before; every such sample must differ."""
    got, right, wrong = _clip_control(clip_results, side="left")
    g = got.astype(np.float64)
    cases = np.zeros(right["how"].shape, bool)
    differs = np.zeros(right["how"].shape, bool)
    for ch in (0, 1, 2):
        sl = M.SLICE[ch]
        cases[:, :, ch] = (wrong["value"][:, :, sl] != right["value"][:, :, sl]).any(axis=2)
        differs[:, :, ch] = (g[:, :, sl] != wrong["value"][:, :, sl]).any(axis=2)
    cases &= right["on_key"] & ~right["interp"] & ~wrong["interp"]      # the wrong reading copies another key
    share = differs[cases].mean()
    print(f"control side=left: {share:.1%} of {cases.sum()} copied on-key samples differ from the wrong model")
    assert cases.sum() >= 100 and share == 1.0


# --- modifier blend ---------------------------------------------------------------------------
def blend_cases():
    """[(w, pose_in [m][10], pose_mod [m][10], kind [m])]: mixed_inputs(3, 8000) at each of
    BLEND_WEIGHTS, then w = 0.5 on the pairs whose determinants have the same sign."""
    a, m, kind = BR.mixed_inputs(3, 8000)
    out = [(w, a, m, kind) for w in BLEND_WEIGHTS]
    same = M.blend_f64(a, m, np.full(len(a), 0.5, np.float32))["same_sign"]
    assert 0.3 < same.mean() < 0.9
    out.append((0.5, a[same], m[same], kind[same]))
    return out


def blend_entry(a, m, w, libm_variant=0):
    return pose_blend_cpu(a.reshape(-1, 1, 10), m.reshape(-1, 1, 10), float(w), libm_variant).reshape(-1, 10)


def blend_figures(got, a, m, w, kind, **wrong):
    """(model, judged mask, transform errors [m], worst origin error over its bound) of blended poses got [m][10]."""
    model = M.blend_f64(a, m, np.full(len(a), w, np.float32), **wrong)
    judged = M.blend_judged(model)
    err = M.blend_transform_error(got, model)
    live = ~model["early"]
    origin = np.abs(got[live, 4:7].astype(np.float64) - model["origin"][live]) / model["origin_bound"][live]
    return model, judged, err, float(origin.max())


def test_blend_entry_stays_within_the_float64_meaning(mbik):
    blended = left_out = 0
    kinds = np.zeros((len(BR.KINDS), 2), int)
    for w, a, m, kind in blend_cases():
        got = blend_entry(a, m, w)
        assert np.isfinite(got).all()
        model, judged, err, origin = blend_figures(got, a, m, w, kind)
        early = model["early"]
        assert BR.same_bits(got[early], m[early])                  # the modifier's bits exactly
        assert early[np.isin(kind, [BR.KINDS.index("q_vs_minus_q"), BR.KINDS.index("identical")])].all()
        live = ~early
        print(f"w = {w!r}: worst transform error {err[judged].max():.3e} over {judged.sum()} bones (bound {BLEND_BOUND:.3e}); "
              f"worst origin error over its bound {origin:.3f}; left out {(live & ~judged).sum()} of {live.sum()}")
        assert (err[judged] <= BLEND_BOUND).all()
        assert origin <= 1.0
        if w != 0.5:
            blended += live.sum()
            left_out += (live & ~judged).sum()
            kinds[:, 0] += np.bincount(kind[live], minlength=len(BR.KINDS))
            kinds[:, 1] += np.bincount(kind[live & ~judged], minlength=len(BR.KINDS))
    share = kinds[:, 1] / np.maximum(kinds[:, 0], 1)
    print(f"left out {left_out / blended:.1%} in all; by kind " + ", ".join(f"{k} {s:.1%}" for k, s in zip(BR.KINDS, share)))
    assert left_out / blended <= LEFT_OUT_TOTAL and (share <= LEFT_OUT_KIND).all()


def test_blend_early_outs_keep_the_modifiers_bits(mbik):
    a, m, kind = BR.mixed_inputs(3, 800)
    for w in (1.0, 1.5, float("nan"), float("inf")):
        assert M.blend_f64(a, m, np.full(len(a), w, np.float32))["early"].all()
        assert BR.same_bits(blend_entry(a, m, w), m)


def _blend_control(wrong, kinds, weights=(0.25, 0.75, 0.9)):
    a, m, kind = BR.mixed_inputs(3, 8000)
    pick = np.isin(kind, [BR.KINDS.index(k) for k in kinds])
    a, m, kind = a[pick], m[pick], kind[pick]
    out = []
    for w in weights:
        got = blend_entry(a, m, w)
        _, judged, _, _ = blend_figures(got, a, m, w, kind)
        _, _, err, _ = blend_figures(got, a, m, w, kind, **wrong)
        out.append((err[judged] > BLEND_BOUND).mean())
    return out


def test_control_long_arc_slerp_fails_blend(mbik):
    """The geodesic taken the long way round: at weights 0.25, 0.75 and 0.9 at least 95 % of the judged
    general, far_rotation and unit bones must leave the bound."""
    shares = _blend_control(dict(long_arc=True), ("general", "far_rotation", "unit"))
    print("control long arc (blend): outside the bound", ", ".join(f"{s:.1%}" for s in shares))
    assert min(shares) >= 0.95


def test_control_scale_before_rotation_fails_blend(mbik):
    """diag(s) R instead of R diag(s): with non-uniform scales and unrelated rotations (general,
    far_rotation) at least 95 % of the judged bones must leave the bound."""
    shares = _blend_control(dict(scale_first=True), ("general", "far_rotation"))
    print("control diag(s) R (blend): outside the bound", ", ".join(f"{s:.1%}" for s in shares))
    assert min(shares) >= 0.95


# --- bone globals -----------------------------------------------------------------------------
STAR400 = [-1] + [0] * 400


def globals_rigs():
    """name -> (parents, pins, skeletons, scale spread)"""
    t = W.topology(2)
    return {"c2": (t.parents.tolist(), t.pins.tolist(), 8, 0.4),
            "unsorted_parents": GR.EDGE_RIGS["unsorted_parents"] + (3, 0.4),
            "chain300": (GR.CHAIN300, [299], 2, 0.1),
            "star400": (STAR400, [1, 400], 3, 0.4)}


def globals_ratios(got_globals, got_skin, got_dist, model):
    """worst |error| / bound of the globals, the skin transforms and the distances."""
    r = lambda got, key: float((np.abs(got.astype(np.float64) - model[key]) / np.maximum(model[key + "_bound"], 1e-300)).max())   # noqa: E731
    return r(got_globals, "globals"), r(got_skin, "skin"), r(got_dist, "dist")


@pytest.fixture(scope="module")
def globals_results(mbik):
    """name -> (parents, pins, pose, inv_bind, targets, entry's globals, skinned globals, distances), computed once."""
    out = {}
    for i, (name, (parents, pins, n, spread)) in enumerate(globals_rigs().items()):
        pose, inv_bind, targets = GR.random_inputs(700 + i, n, len(parents), len(pins), spread)
        rc, g, d = GR.pose_globals_cpu_raw(parents, pins, pose, None, targets)
        assert rc == _lib.MBIK_OK
        rc, s, d2 = GR.pose_globals_cpu_raw(parents, pins, pose, inv_bind, targets)
        assert rc == _lib.MBIK_OK and GR.same_bits(d, d2)
        out[name] = (parents, pins, pose, inv_bind, targets, g, s, d)
    return out


@pytest.mark.parametrize("name", list(globals_rigs()))
def test_globals_entry_stays_within_the_float64_meaning(globals_results, name):
    parents, pins, pose, inv_bind, targets, g, s, d = globals_results[name]
    assert np.isfinite(g).all() and np.isfinite(s).all()
    model = M.globals_f64(parents, pins, pose, inv_bind, targets)
    ratios = globals_ratios(g, s, d, model)
    scale = np.abs(model["globals"][:, :, :9]).max(axis=2)
    print(f"{name}: worst error over its bound: globals {ratios[0]:.3f}, skin {ratios[1]:.3f}, distances {ratios[2]:.3f}; "
          f"largest basis bound relative to the basis {(model['globals_bound'][:, :, 0] / scale).max():.2e}")
    assert max(ratios) <= 1.0
    levels = np.array([len(c) for c in M.ancestor_chains(parents)])
    assert (model["globals_bound"][:, :, 0] <= 1e-5 * levels * scale).all()   # the bound stays a small part of what it bounds


@pytest.mark.parametrize("wrong,rigs,least", [("child_first", ("c2", "unsorted_parents", "chain300"), 0.9),
                                              ("scale_first", ("c2", "chain300", "star400"), 0.9)])
def test_control_wrong_globals_model_fails(globals_results, wrong, rigs, least):
    """local * parent instead of parent * local, and diag(s) R instead of R diag(s) for the local: at
    least 90 % of the bones the reading touches (those with a parent; all) must leave the bound."""
    for name in rigs:
        parents, pins, pose, inv_bind, targets, g, s, d = globals_results[name]
        model = M.globals_f64(parents, pins, pose, **{wrong: True})
        bad = (np.abs(g.astype(np.float64) - model["globals"]) > model["globals_bound"]).any(axis=2)
        touched = np.array(parents) >= 0 if wrong == "child_first" else np.ones(len(parents), bool)
        share = bad[:, touched].mean()
        print(f"control {wrong}, {name}: {share:.1%} of the bones outside the bound")
        assert share >= least


# --- target capture ---------------------------------------------------------------------------
def capture_inputs(seed, n, P):
    """(skeleton globals [n][12], target globals [n][P][12]): rotations with scales 0.5 .. 2 and origins within 10."""
    rng = np.random.default_rng(seed)

    def xforms(shape):
        q = rng.normal(size=shape + (4,))
        basis = M.rotations(q) * rng.uniform(0.5, 2.0, shape + (1, 3))
        return np.concatenate([basis.reshape(shape + (9,)), rng.uniform(-10, 10, shape + (3,))], axis=-1).astype(np.float32)

    return xforms((n,)), xforms((n, P))


def capture_ratios(got, skel, node, **wrong):
    """[n][P]: worst |error| / bound of captured targets got [n][P][12] against the model."""
    out = np.zeros(got.shape[:2])
    for s in range(got.shape[0]):
        for e in range(got.shape[1]):
            val, bound = M.capture_f64(skel[s], node[s, e], **wrong)
            out[s, e] = (np.abs(got[s, e].astype(np.float64) - val) / bound).max()
    return out


def test_capture_arithmetic_stays_within_the_float64_meaning(oracle):
    """The oracle primitives mbik_capture_targets equals bitwise on the device (test_gpu_capture)."""
    skel, node = capture_inputs(5, 40, 4)
    got = np.stack([np.stack([oracle.xform_mul(oracle.xform_affine_inverse(skel[s]), node[s, e]) for e in range(4)]) for s in range(40)])
    ratios = capture_ratios(got, skel, node)
    print(f"capture: worst error over its bound {ratios.max():.3f}")
    assert ratios.max() <= 1.0
    wrong = capture_ratios(got, skel, node, swapped=True)
    print(f"control inverse(node) * skeleton: {(wrong > 1).mean():.1%} outside the bound")
    assert (wrong > 1).all()


# --- the measurements behind the two tolerances ---------------------------------------------------
def measure():
    from oracle import pyoracle
    pyoracle.build()
    B, rest, clips, t, ci = clip_case()
    want, _ = CR.expected(B, rest, clips, t, ci)
    _, ratio, angles, left_out = clip_figures(want, M.clip_sample_f64(B, rest, clips, t, ci))
    print(f"clip recipe against the model: worst rotation angle {angles.max():.3e} rad over {angles.size} "
          f"(left out {left_out:.2%}); worst lerp error over its bound {ratio:.3f}")
    worst = 0.0
    for w, a, m, kind in blend_cases():
        want, _ = BR.expected(pyoracle, a, m, np.full(len(a), w, np.float32))
        _, judged, err, origin = blend_figures(want, a, m, w, kind)
        print(f"blend recipe against the model, w = {w!r}: worst transform error {err[judged].max():.3e} over {judged.sum()}; "
              f"origin over its bound {origin:.3f}")
        worst = max(worst, err[judged].max())
    print(f"blend recipe against the model: worst transform error {worst:.3e}")


if __name__ == "__main__":
    measure()
