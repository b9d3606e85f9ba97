"""Shared rigs, generators, measures and limits of tests/test_bone_step_cpu.py and
tests/test_gpu_bone_step.py: the oracle's and the kernels' bone-steps judged by the float64 model of
tests/bone_step_f64.py.  The measures take poses as arrays, so the same code judges both.

Limits: 4 x the worst value of the CPU oracle over the fixed seeds below ("The
bone-step: what one step means"), except the clamped angle, whose bound bone_step_f64 derives."""
import math

import numpy as np

from many_bone_ik_amd import workloads as W

from . import bone_step_f64 as M
from . import geometry_f64 as G
from . import solve_invariants as S

# --- asserted limits: measured worst of the CPU oracle x 4, one DESIGN row each ------------------
SEGMENT_ROTATION_LIMIT = 4 * 9.73e-6          # rad, a stepped bone's local rotation after one segment_solver call
SEGMENT_ORIGIN_LIMIT = 4 * 2.61e-6            # the translating segment's local origins after it, relative to 1 + |origin|
ITERATION_ROTATION_LIMIT = 4 * 1.57e-5        # rad, one whole iteration (the base cases and the damp cases)
ITERATION_ORIGIN_LIMIT = 4 * 3.70e-6
TWO_ITERATIONS_ROTATION_LIMIT = 4 * 2.84e-5   # rad: the second iteration starts from float32 state that the model does not share
TWO_ITERATIONS_ORIGIN_LIMIT = 4 * 8.35e-6
DAMP_UNCLAMPED_LIMIT = 4 * 6.63e-6            # rad, applied angle to the model's fit angle, fit below the damp
DAMP_AXIS_LIMIT = 4 * 2.60e-5                 # rad, applied axis to the model's fit axis, fit above the damp
STABILIZED_ROTATION_LIMIT = 4 * 4.40e-7       # rad, a stabilized step to the model's choice of the stepped or the pre-step pose
STABILIZED_ORIGIN_LIMIT = 4 * 6.46e-7
UNCHANGED_ROTATION_LIMIT = 4 * 3.51e-7        # rad, a bone the pass does not step, or steps with the identity (weight 0)
# derived, not measured: a clamped step's angle to the damp, bone_step_f64.clamp_angle_bound (worst seen: 0.42 of it)

LEFT_OUT_CAP = G.LEFT_OUT_CAP
NSQ_FACTOR = 100.0        # a squared norm this close to the precision may fall on either side in float32
DAMP_MARGIN = 1.0e-4      # rad: a fit angle this close to the damp may be clamped or not
MSD_MARGIN = 1.0e-4       # relative: an msd this close to previous * 1.0001 may be accepted or not
CLASS_MIN = 25            # steps each asserted class must hold
N = 33                    # skeletons of a CPU case

C2_PARENTS, C2_PINS = S.C2_PARENTS, S.C2_PINS


def midpin_rig():
    """Three chains under one root bone, each two bones down to a pin and two more to a second pin;
    the mid-chain pins' propagation factors are 0, 0.5 and 1."""
    parents, pins, prop = [-1], [], []
    for f in (0.0, 0.5, 1.0):
        p = 0
        for k in range(4):
            parents.append(p)
            p = len(parents) - 1
            if k == 1:
                pins.append(p)
                prop.append(f)
        pins.append(p)
        prop.append(1.0)
    return np.array(parents, np.int32), np.array(pins, np.int32), np.array(prop, np.float32)


def rig_arrays(name):
    if name == "uneven":
        return S.uneven_parents() + (None,)
    if name == "c2":
        return C2_PARENTS, C2_PINS, None
    if name == "midpin":
        return midpin_rig()
    if name == "chain3":
        return np.array([-1, 0, 1], np.int32), np.array([2], np.int32), None
    raise ValueError(name)


RIGS = ("uneven", "c2", "midpin", "chain3")
RESTS = ("plus_y", "realistic_unit_scale")
PINS = {
    "default": dict(priority=(0.2, 0.0, 0.2), weight=(1.0,)),          # the reference's default priorities
    "mixed": dict(priority=(1.0, 0.5, 0.0), weight=(0.35, 1.0)),       # weights alternate over the pins
    "origin_only": dict(priority=(0.0, 0.0, 0.0), weight=(1.0,)),      # one heading per pin: the one-point path
    "weight0": dict(priority=(0.2, 0.0, 0.2), weight=(0.0,)),          # the reference's default weight
}

# Generator per pin setting.  A pin's tip bone fits headings that all scale with min(|target - tip|, 1)
# and with the pin's weight, so the fit's squared norm goes with their sixth power: under a 0.35 weight
# a tip near its target sits on the precision threshold.  The mixed setting therefore swings every bone
# further from rest than the targets were drawn (30 degrees), which keeps the tips away from them.
GEN = {"mixed": dict(swing=(0.7, 1.1))}


class Case:
    """One rig, rest and pin setting: an unconstrained workload of n skeletons, a perturbed input
    pose and the model's Rig."""

    def __init__(self, rig, rest, pins="default", n=N, default_damp=math.radians(5.0), bone_damp=None, stabilization=0,
                 swing=(0.0, 0.6), roll=0.5, seed=11, stream=31):
        self.key = (rig, rest, pins, n, default_damp, None if bone_damp is None else tuple(bone_damp), stabilization, swing, roll, seed)
        parents, pin_bones, prop = rig_arrays(rig)
        topo = W.custom_topology(parents, pin_bones, [], cones_per_bone=0, twist=None, iterations=1, name=rig)
        wl = W.generate(stream, n, topo=topo, rest=rest)
        P = len(pin_bones)
        setting = PINS[pins]
        wl.pin_priority = np.tile(np.array(setting["priority"], np.float32), (P, 1))
        # a rig with one pin takes the last weight: under 0.35 chain3's tip sits on the precision threshold in 9 % of steps
        wl.pin_weight = np.array([setting["weight"][i % len(setting["weight"]) if P > 1 else -1] for i in range(P)], np.float32)
        if prop is not None:
            wl.pin_propagation = prop
        wl.default_damp = float(default_damp)
        wl.bone_damp = None if bone_damp is None else np.asarray(bone_damp, np.float32)
        self.wl, self.stabilization = wl, stabilization
        self.pose_in = S.perturb(wl.pose, np.random.default_rng(seed), swing, roll)
        self.rig = M.Rig(parents, pin_bones, wl.pin_weight, wl.pin_priority, wl.pin_propagation, wl.pose[..., 4:7],
                         wl.default_damp, () if bone_damp is None else tuple(wl.bone_damp), stabilization)
        self.topo = M.topology(self.rig)
        self.D = M.direction_frames(self.rig)
        near = [G.near_deadband(G.angle(wl.pose[s, np.flatnonzero(parents == b), 4:7].astype(np.float64).mean(0), G.Y_AXIS))
                for s in range(n) for b in range(len(parents)) if (parents == b).any()]
        assert not any(near), "a bone-direction arc sits on the shortest-arc deadband: pick another stream"
        self._memo = {}

    @property
    def label(self):
        return " ".join(str(k) for k in self.key[:3])

    def oracle(self, pyoracle, iterations=1):
        return pyoracle.Oracle(self.wl, iterations=iterations, stabilization_passes=self.stabilization)

    def model_segment(self, segment, misread=frozenset()):
        k = ("seg", segment, misread)
        if k not in self._memo:
            topo = self.topo if not misread else M.topology(self.rig, misread)
            self._memo[k] = M.segment_pass(self.rig, self.pose_in, self.wl.targets, segment, misread, topo=topo, D=self.D)
        return self._memo[k]

    def model_iterations(self, iterations, misread=frozenset()):
        """(State, all step records) after `iterations` iterations followed in float64."""
        k = ("it", iterations, misread)
        if k not in self._memo:
            topo = self.topo if not misread else M.topology(self.rig, misread)
            state, records = M.State(self.pose_in), []
            for it in range(iterations):
                state, rec = M.iteration(self.rig, state, self.wl.targets, misread, it, topo, self.D)
                records += rec
            self._memo[k] = (state, records)
        return self._memo[k]


_CASES = {}


def case(*a, **kw):
    k = (a, tuple(sorted((n, v if not isinstance(v, (list, np.ndarray)) else tuple(v)) for n, v in kw.items())))
    if k not in _CASES:
        _CASES[k] = Case(*a, **kw)
    return _CASES[k]


# --- what is left out of a judgement ---------------------------------------------------------------
def related(parents):
    """[bone][bone]: b is a, an ancestor of a or a descendant of a."""
    B = len(parents)
    anc = np.eye(B, dtype=bool)
    for a in range(B):
        p = int(parents[a])
        while p >= 0:
            anc[a, p] = True
            p = int(parents[p])
    return anc | anc.T


def left_out(rig, records):
    """Per record, [skeleton] True where the step is not judged: its squared norm is within
    NSQ_FACTOR of the precision, its fit angle within DAMP_MARGIN of the damp, its msd within
    MSD_MARGIN of the acceptance threshold, or it reads the result of a step of the last kind -- a
    step reads the transforms of the stepped bone's ancestors and descendants."""
    rel = related(rig.parents)
    n = len(records[0]["fit_angle"])
    tainted = np.zeros((n, len(rig.parents)), bool)
    out = []
    for r in records:
        near = (r["nsq"] > M.PRECISION / NSQ_FACTOR) & (r["nsq"] < M.PRECISION * NSQ_FACTOR)
        near |= np.abs(r["fit_angle"] - r["limit"]) < DAMP_MARGIN
        undecided = (np.abs(r["margin"]) < MSD_MARGIN) | (tainted & rel[r["bone"]]).any(axis=1)
        tainted[:, r["bone"]] |= undecided
        out.append(near | undecided)
    return out


def last_steps(records):
    """bone -> index of its last record."""
    return {r["bone"]: i for i, r in enumerate(records)}


def rotations(pose):
    return M.quat_to_matrix(np.asarray(pose[..., 0:4], np.float64))


def judge(c, out, state, records, label, want_origin=True):
    """(worst rotation error rad, worst relative origin error, left-out share) of a float32 output
    pose against the model's state over the stepped bones, each judged unless its last step is
    left out."""
    lo = left_out(c.rig, records)
    last = last_steps(records)
    bones = sorted(last)
    skip = np.stack([lo[last[b]] for b in bones], 1)
    share = np.mean(np.concatenate(lo))
    rot = M.rotation_angle(rotations(out[:, bones]), state.basis[:, bones])
    worst_rot = float(np.where(skip, 0.0, rot).max())
    rs = [b for b in bones if records[last[b]]["segment"].parent is None]
    worst_o = 0.0
    if rs and want_origin:
        o = state.origin[:, rs]
        err = np.linalg.norm(out[:, rs, 4:7].astype(np.float64) - o, axis=-1) / (1.0 + np.linalg.norm(o, axis=-1))
        worst_o = float(np.where(np.stack([lo[last[b]] for b in rs], 1), 0.0, err).max())
    print(f"{label}: rotation {worst_rot:.3g} rad, origin {worst_o:.3g}, left out {share:.4f} of {sum(len(x) for x in lo)} steps")
    return worst_rot, worst_o, float(share)


def check_untouched(c, out, stepped, label):
    """Bones the pass does not step keep their rotation (within the float32 round trip through a
    basis that every listed bone's pose takes) and position; local positions outside the translating
    segment and every scale hold as in solve_invariants.check_rigid; bones in no segment are bitwise."""
    B = len(c.rig.parents)
    listed = np.isin(np.arange(B), c.topo.bone_list)
    assert np.array_equal(out[:, ~listed], c.pose_in[:, ~listed]), label
    rest = [b for b in range(B) if b not in stepped]
    if rest:
        turn = M.rotation_angle(rotations(out[:, rest]), rotations(c.pose_in[:, rest])).max()
        assert turn <= UNCHANGED_ROTATION_LIMIT, f"{label}: an unstepped bone turned {turn:.3g} rad"
        assert np.array_equal(out[:, rest, 4:7], c.pose_in[:, rest, 4:7]), label
    rs = S.root_segment_bones(c.wl)
    if (~rs).any():
        S.check_rigid(c, out, label)
    else:       # every bone translates: the scales alone
        assert np.abs(out[..., 7:10].astype(np.float64) - c.pose_in[..., 7:10]).max() <= S.SOLVE_SCALE_LIMIT, label
    return 0.0 if not rest else float(turn)


def segment_bones(c, segment):
    """Bones that segment_solver of post-order segment `segment` steps."""
    out = []

    def run(seg):
        for ch in seg.children:
            run(ch)
        out.extend(seg.bones)

    run(c.topo.segments[segment])
    return out


# --- the checks, shared by the CPU and GPU modules; each prints its figures before it asserts ----------
WORST = {}      # check name -> worst figure seen in this process (for the DESIGN table)


def _note(name, value):
    WORST[name] = max(WORST.get(name, 0.0), float(value))


def check_segment(c, out, segment, label):
    """One segment_solver call: the stepped bones against the model, the rest untouched."""
    state, records = c.model_segment(segment)
    rot, org, share = judge(c, out, state, records, label)
    _note("segment rotation", rot), _note("segment origin", org)
    _note("unstepped rotation", check_untouched(c, out, segment_bones(c, segment), label))
    assert rot <= SEGMENT_ROTATION_LIMIT and org <= SEGMENT_ORIGIN_LIMIT, label
    return np.concatenate(left_out(c.rig, records))


def check_iterations(c, out, iterations, label):
    state, records = c.model_iterations(iterations)
    rot, org, share = judge(c, out, state, records, label)
    _note(f"{iterations} iteration rotation", rot), _note(f"{iterations} iteration origin", org)
    check_untouched(c, out, c.topo.bone_list, label)
    assert share <= LEFT_OUT_CAP, f"{label}: {share:.4f} of the steps left out"
    lim = (ITERATION_ROTATION_LIMIT, ITERATION_ORIGIN_LIMIT) if iterations == 1 else (TWO_ITERATIONS_ROTATION_LIMIT, TWO_ITERATIONS_ORIGIN_LIMIT)
    assert rot <= lim[0] and org <= lim[1], label


def check_damp_classes(c, out, label):
    """One iteration: the rotation each damped step applied is out local * input local^-1 (a parent is
    stepped after its children, so the parent's transform is the input's).  Below the damp its angle
    is the fit's; above, its angle is the damp and its axis the fit's."""
    state, records = c.model_iterations(1)
    lo = left_out(c.rig, records)
    Gb0, _ = M.State(c.pose_in).globals(c.rig.parents)
    Mx = rotations(out) @ np.swapaxes(rotations(c.pose_in), -1, -2)
    ang, axis = M.rotation_angle(Mx, np.broadcast_to(np.eye(3), Mx.shape)), M.rotation_axis(Mx)
    below = above = 0
    worst = dict(unclamped=0.0, clamped=0.0, axis=0.0, excess=0.0)
    for r, skip in zip(records, lo):
        if r["segment"].parent is None:
            continue
        b, keep = r["bone"], ~skip
        cl, un = keep & r["clamped"], keep & ~r["clamped"]
        below, above = below + int(un.sum()), above + int(cl.sum())
        if un.any():
            worst["unclamped"] = max(worst["unclamped"], np.abs(ang[un, b] - r["fit_angle"][un]).max())
        if cl.any():
            err = np.abs(ang[cl, b] - r["damp"])
            worst["clamped"] = max(worst["clamped"], err.max())
            worst["excess"] = max(worst["excess"], (err / M.clamp_angle_bound(r["damp"])).max())
            fit_axis = np.einsum("nji,nj->ni", Gb0[:, int(c.rig.parents[b])], r["axis"])     # into the parent frame
            worst["axis"] = max(worst["axis"], G.angle(axis[cl, b], fit_axis[cl]).max())
    share = float(np.mean(np.concatenate(lo)))
    print(f"{label}: {below} steps below the damp, angle to the fit's {worst['unclamped']:.3g} rad; {above} above, angle to the damp "
          f"{worst['clamped']:.3g} rad ({worst['excess']:.3g} of the derived bound), axis to the fit's {worst['axis']:.3g} rad; left out {share:.4f}")
    _note("damp unclamped angle", worst["unclamped"]), _note("damp clamped angle / bound", worst["excess"]), _note("damp axis", worst["axis"])
    assert below >= CLASS_MIN and above >= CLASS_MIN, f"{label}: {below} below and {above} above the damp"
    assert share <= LEFT_OUT_CAP, label
    assert worst["unclamped"] <= DAMP_UNCLAMPED_LIMIT and worst["excess"] <= 1.0 and worst["axis"] <= DAMP_AXIS_LIMIT, label


def check_stabilized(c, out, iterations, label):
    """Every bone's output is its last step's stepped pose or pre-step pose, whichever the model chose."""
    state, records = c.model_iterations(iterations)
    lo = left_out(c.rig, records)
    last = last_steps(records)
    accepted = sum(int(r["accepted"].sum()) for r in records)
    restored = sum(int((~r["accepted"]).sum()) for r in records)
    worst_rot = worst_o = 0.0
    wrong = 0
    for b, i in last.items():
        r, keep = records[i], ~lo[i]
        got_b, got_o = rotations(out[:, b]), out[:, b, 4:7].astype(np.float64)
        err = {}
        for k in ("pre", "post"):
            e_rot = M.rotation_angle(got_b, r[k][0])
            e_o = np.linalg.norm(got_o - r[k][1], axis=-1) / (1.0 + np.linalg.norm(r[k][1], axis=-1))
            err[k] = (e_rot, e_o)
        chosen = np.where(r["accepted"], err["post"][0], err["pre"][0]), np.where(r["accepted"], err["post"][1], err["pre"][1])
        other = np.where(r["accepted"], err["pre"][0], err["post"][0])
        wrong += int((keep & (chosen[0] > STABILIZED_ROTATION_LIMIT) & (other <= STABILIZED_ROTATION_LIMIT)).sum())
        worst_rot = max(worst_rot, np.where(keep, chosen[0], 0.0).max())
        worst_o = max(worst_o, np.where(keep, chosen[1], 0.0).max())
    share = float(np.mean(np.concatenate(lo)))
    print(f"{label}: {accepted} accepted, {restored} restored; to the model's choice rotation {worst_rot:.3g} rad, origin {worst_o:.3g}; "
          f"{wrong} match the other pose instead; left out {share:.4f}")
    _note("stabilized rotation", worst_rot), _note("stabilized origin", worst_o)
    assert accepted >= CLASS_MIN and restored >= CLASS_MIN, label
    assert share <= LEFT_OUT_CAP, label
    assert wrong == 0, f"{label}: {wrong} steps took the other decision"
    assert worst_rot <= STABILIZED_ROTATION_LIMIT and worst_o <= STABILIZED_ORIGIN_LIMIT, label


def check_weight0(c, out, label):
    """Every heading weight 0: each fit is the identity, so the pose comes back."""
    state, records = c.model_iterations(1)
    assert all((s.weights == 0).all() for s in c.topo.segments)
    assert all((r["fit_angle"] == 0).all() and (r["nsq"] == 0).all() for r in records), label
    turn = M.rotation_angle(rotations(out), rotations(c.pose_in)).max()
    drift = np.abs(out[..., 4:10].astype(np.float64) - c.pose_in[..., 4:10]).max()
    print(f"{label}: rotation {turn:.3g} rad (limit {UNCHANGED_ROTATION_LIMIT:.3g}), position and scale drift {drift:.3g}")
    _note("weight 0 rotation", turn)
    assert turn <= UNCHANGED_ROTATION_LIMIT and drift <= S.SOLVE_POSITION_LIMIT, label


def control_error(c, out, iterations, misread):
    """Worst rotation error of `out` against the model read wrongly (its own left-out steps aside)."""
    state, records = c.model_iterations(iterations, frozenset([misread]))
    lo = left_out(c.rig, records)
    last = last_steps(records)
    bones = sorted(last)
    rot = M.rotation_angle(rotations(out[:, bones]), state.basis[:, bones])
    org = np.linalg.norm(out[:, bones, 4:7].astype(np.float64) - state.origin[:, bones], axis=-1)
    org = org / (1.0 + np.linalg.norm(state.origin[:, bones], axis=-1))
    skip = np.stack([lo[last[b]] for b in bones], 1)
    return float(np.where(skip, 0.0, rot).max()), float(np.where(skip, 0.0, org).max())


# --- the case lists ------------------------------------------------------------------------------------
BASE = [(rig, rest, pins) for rig in RIGS for rest in RESTS for pins in ("default", "mixed", "origin_only")]
DAMPS = {"5deg": (math.radians(5.0), (0.5, 0.03, 0.2, 0.03, 0.2)), "0.6rad": (0.6, (0.1, 0.25, 0.9, 0.25, 0.9))}
DAMP_CASES = [(rig, rest, d) for rig in ("uneven", "c2") for rest in RESTS for d in DAMPS]


def base_case(rig, rest, pins, n=N):
    return case(rig, rest, pins, n=n, **GEN.get(pins, {}))


def damp_case(rig, rest, d, n=N):
    """bone_damp is shorter than the rig, with entries below and above the default."""
    return case(rig, rest, "default", n=n, default_damp=DAMPS[d][0], bone_damp=DAMPS[d][1])


def stabilized_case(rest, passes, n=N):
    return case("chain3", rest, "default", n=n, stabilization=passes)


_ORACLE = {}


def oracle_out(pyoracle, c, what, arg):
    """The CPU oracle's output of a case, once: what = "segment" (arg: post-order index) or
    "solve" (arg: iterations)."""
    k = (c.key, what, arg)
    if k not in _ORACLE:
        o = c.oracle(pyoracle, arg if what == "solve" else 1)
        _ORACLE[k] = o.segment_solve(arg, c.pose_in, c.wl.targets) if what == "segment" else o.solve(c.pose_in, c.wl.targets)
        o.close()
    return _ORACLE[k]
