"""Shared rigs and measures of tests/test_solve_invariants_cpu.py and tests/test_gpu_solve_invariants.py:
what a solved pose means, judged by the float64 models of tests/geometry_f64.py alone.  The
measures take poses as arrays, so the same code judges the oracle's output and the GPU's.

A constrained bone's local rotation L, its bone-direction frame D and its cones all live in the
parent's frame, so no forward kinematics is needed: the swing limit judges L * D * (+Y) against
the cones and the twist limit judges the twist of centre^-1 * frame^-1 * L about +Y.

Limits: 4 x the worst value of the CPU oracle over the fixed seeds below,
except SWING_BAND_LIMIT, which follows from the reference's shortest-arc deadband."""
import math

import numpy as np

from many_bone_ik_amd import workloads as W

from . import geometry_f64 as G

# --- asserted limits: DESIGN.md section 7a, one row each (measured worst x 4) --------------------
CMODE_ROTATION_LIMIT = 4 * 4.31e-6     # rad, constraint_mode output to the float64 expected rotation
CMODE_TWIST_LIMIT = 4 * 9.91e-7        # rad, twist beyond range/2 after constraint_mode
CMODE_UNTOUCHED_LIMIT = 4 * 2.07e-7    # rad, rotation of an unconstrained or parentless bone, constraint_mode
CMODE_SCALE_LIMIT = 4 * 4.17e-7        # local scale of any bone after constraint_mode
SOLVE_TWIST_LIMIT = 4 * 1.40e-6        # rad, twist beyond range/2 after the ordinary solve
SOLVE_POSITION_LIMIT = 4 * 8.58e-6     # local position drift outside the translating root segment
SOLVE_SCALE_LIMIT = 4 * 9.36e-6        # local scale drift
FRAME_D_LIMIT = 4 * 5.35e-7            # rad, float64 bone-direction frame to the plan's D rows (host-built tables)
# Not measured but derived: a snap whose arc is below Godot's shortest-arc deadband is not made, so a
# direction may stay that far from the snap's target, which itself lies within section 7a's
# "result to nearest boundary circle" limit of a boundary circle.
SWING_BAND_LIMIT = G.ARC_DEADBAND + G.SWING_BOUNDARY_LIMIT

LEFT_OUT_CAP = G.LEFT_OUT_CAP
FULL_TWIST = (0.0, 2.0 * math.pi)
TWISTS = [(0.3, 0.5), (-1.0, 1.2)]     # (min, range): a positive and a negative min
RADII = {0: (), 1: (0.6,), 2: (0.6, 0.4), 3: (0.6, 0.4, 0.4)}   # end-state cones: 1 % of 0.6 rad exceeds SWING_BAND_LIMIT
CMODE_RADII = {0: (), 1: (0.3,), 2: (0.3, 0.2)}

C2_PARENTS = W.topology(2).parents
C2_PINS = W.topology(2).pins


def uneven_parents(spare=False):
    """Chains of 3, 2, 2 and 1 bones under one root bone (tests/test_gpu_step_classes.py); with
    `spare`, also an unpinned chain of 2 under the first chain's first bone: bones in no segment."""
    parents, pins = [-1], []
    for n in (3, 2, 2, 1):
        p = 0
        for _ in range(n):
            parents.append(p)
            p = len(parents) - 1
        pins.append(p)
    if spare:
        parents += [1, len(parents)]
    return np.array(parents, np.int32), np.array(pins, np.int32)


def workload(rig, n, ncones, twist, radii, iterations, rest="plus_y", constrained=None, first=0, stream=21):
    """C2's topology ("c2") or the uneven rig, every parented bone constrained (or `constrained`),
    cones of the given radii (rad, one per cone) around generate()'s control points; a third
    control point is the second turned a quarter turn about the first.  The pose stream does not
    depend on `constrained`, `radii` or `twist`."""
    parents, pins = (C2_PARENTS, C2_PINS) if rig == "c2" else uneven_parents(spare=rig == "uneven_spare")
    every = np.arange(1, len(parents), dtype=np.int32)
    topo = W.custom_topology(parents, pins, every, cones_per_bone=min(ncones, 2) if ncones else 1, twist=twist,
                             iterations=iterations)
    wl = W.generate(stream, n, first=first, topo=topo, rest=rest)
    cones = np.zeros((n, len(every), max(1, ncones), 4), np.float32)
    cones[:, :, :min(max(ncones, 1), 2)] = wl.cones[:, :, :min(max(ncones, 1), 2)]
    if ncones >= 3:
        c0, c1 = cones[:, :, 0, :3].astype(np.float64), cones[:, :, 1, :3].astype(np.float64)
        cones[:, :, 2, :3] = np.cross(c0, c1) + c0 * np.sum(c0 * c1, -1, keepdims=True)
    for k in range(ncones):
        cones[:, :, k, 3] = np.float32(radii[k])
    wl.cones = cones
    wl.cone_count = np.full(len(every), ncones, np.int32)
    wl.twist[..., 0], wl.twist[..., 1] = np.float32(twist[0]), np.float32(twist[1])
    if constrained is not None:
        keep = np.isin(every, np.asarray(constrained, np.int32))
        topo.constrained = every[keep]
        wl.cones, wl.twist, wl.cone_count = wl.cones[:, keep], wl.twist[:, keep], wl.cone_count[keep]
    return wl


def perturb(pose, rng, swing, twist, roll_centre=0.0):
    """pose with every bone's local rotation turned by swing[0]..swing[1] rad about a random axis
    perpendicular to its +Y direction (so that direction moves by the whole angle), then rolled
    about its own +Y by roll_centre +- up to `twist` rad."""
    out = pose.copy()
    n, B = pose.shape[:2]
    q0 = pose[..., 0:4].astype(np.float64)
    ax = G.unit(np.cross(W._quat_to_mat(q0)[..., :, 1], rng.normal(size=(n, B, 3))))
    q = W._quat_mul(W._quat_from_axis_angle(ax, rng.uniform(swing[0], swing[1], (n, B))), q0)
    roll = W._quat_from_axis_angle(np.broadcast_to(G.Y_AXIS, (n, B, 3)), roll_centre + rng.uniform(-twist, twist, (n, B)))
    out[..., 0:4] = W._quat_mul(q, roll)
    return out


def rotation(q):
    return G.quat_to_matrix(np.asarray(q, np.float64) / np.linalg.norm(np.asarray(q, np.float64)))


def list_bones(wl):
    """Bones the solve touches: those with a pinned descendant or a pin (ik_bone_segment_3d.cpp:390-393)."""
    parents = wl.topo.parents
    inl = np.zeros(len(parents), bool)
    for p in wl.topo.pins:
        b = int(p)
        while b >= 0 and not inl[b]:
            inl[b] = True
            b = int(parents[b])
    return inl


def direction_frames(wl, identity=False):
    """[skeleton][bone] float64 bone-direction frames of the rest pose wl.pose (unit scales)."""
    n, B = wl.pose.shape[:2]
    if identity:
        return np.broadcast_to(np.eye(3), (n, B, 3, 3))
    inl = list_bones(wl)
    return np.stack([G.bone_direction_frames(wl.topo.parents, wl.pose[s, :, 4:7].astype(np.float64), inl) for s in range(n)])


class TwistModel:
    """The twist frame, centre and range of every constraint, with section 4's wrong variants."""

    def __init__(self, wl, centre_times=2, half=0.5, reverse_arc=False):
        n, C = wl.twist.shape[:2]
        self.half = half
        self.frame = np.empty((n, C, 3, 3))
        self.centre = np.empty((n, C, 3, 3))
        self.range = wl.twist[..., 1].astype(np.float64)
        self.arc = np.zeros((n, C))             # angle of the frame's arc before the deadband
        for s in range(n):
            for c in range(C):
                self.frame[s, c] = G.twist_frame(wl.cones[s, c, :wl.cone_count[c]], reverse_arc)
                self.centre[s, c] = G.twist_centre(wl.twist[s, c, 0], centre_times)
                if wl.cone_count[c]:
                    self.arc[s, c] = G.angle(G.Y_AXIS, G.twist_direction(wl.cones[s, c, :wl.cone_count[c]]))

    def offsets(self, wl, pose):
        """[skeleton][constraint] twist angle away from the range's centre."""
        n, C = wl.twist.shape[:2]
        return np.array([[G.twist_offset(rotation(pose[s, b, 0:4]), self.frame[s, c], self.centre[s, c])
                          for c, b in enumerate(wl.topo.constrained)] for s in range(n)])

    def excess(self, wl, pose):
        """[skeleton][constraint] |twist| - range/2 (<= 0 inside the limit)."""
        return np.abs(self.offsets(wl, pose)) - self.half * self.range


def regions(wl, radius_scale=1.0):
    n, C = wl.twist.shape[:2]
    out = []
    for s in range(n):
        row = []
        for c in range(C):
            cones = wl.cones[s, c, :wl.cone_count[c]].astype(np.float64)
            cones[:, 3] *= radius_scale
            row.append(G.SwingRegion(cones))
        out.append(row)
    return out


def swing_residual(wl, pose, frames, regs, offsets=False):
    """([skeleton][constraint] distance of a non-member direction to the nearest boundary circle, 0
    for members; the same shape, True where the direction is less than acos(1 - 1e-5) inside a
    tangent cap, which the reference accepts and the region does not).  offsets: constraint_mode's
    tip point, the bone's local position + L * D * (+Y)."""
    n, C = wl.twist.shape[:2]
    res = np.zeros((n, C))
    slack = np.zeros((n, C), bool)
    for s in range(n):
        for c, b in enumerate(wl.topo.constrained):
            d = G.unit(G.bone_direction(rotation(pose[s, b, 0:4]), frames[s, b],
                                        pose[s, b, 4:7].astype(np.float64) if offsets else None))[None]
            reg = regs[s][c]
            if not reg.member(d)[0]:
                res[s, c] = reg.boundary_distance(d)[0]
                sd = reg.signed_circle_distances(d)[:, 0]
                tang = np.array([k for _, _, k in reg.circles()])
                slack[s, c] = bool(tang.any() and ((sd[tang] < 0) & (sd[tang] > -G.ARC_DEADBAND)).any())
    return res, slack


def expected_cmode(wl, pose_in, frames, twist_model, radius_scale=1.0):
    """([skeleton][constraint] expected rotation of one constraint_mode frame from a fresh plan,
    twist angle before, swing excess before): the swing snap (0 or 1 cones; the orientation frame's
    origin is the parent's, so the tip point includes the bone's local position), then the twist
    limit on its result."""
    n, C = wl.twist.shape[:2]
    exp = np.empty((n, C, 3, 3))
    tw = np.empty((n, C))
    sw = np.full((n, C), -1.0)
    for s in range(n):
        for c, b in enumerate(wl.topo.constrained):
            L = rotation(pose_in[s, b, 0:4])
            if wl.cone_count[c] == 1:
                L, sw[s, c] = G.swing_snap_one_cone(L, frames[s, b], wl.cones[s, c, 0], pose_in[s, b, 4:7].astype(np.float64),
                                                    radius_scale)
            exp[s, c], tw[s, c] = G.twist_limit(L, twist_model.frame[s, c], twist_model.centre[s, c],
                                                twist_model.range[s, c], twist_model.half)
    return exp, tw, sw


def rotation_errors(wl, pose, expected):
    n, C = wl.twist.shape[:2]
    return np.array([[G.rotation_angle(rotation(pose[s, b, 0:4]), expected[s, c]) for c, b in enumerate(wl.topo.constrained)]
                     for s in range(n)])


def root_segment_bones(wl):
    """Bones of the translating root segments: from a parentless bone down to the first bone with
    more than one solved child, or a pin (ik_bone_segment_3d.cpp:183-208)."""
    parents = wl.topo.parents
    inl = list_bones(wl)
    pins = set(int(p) for p in wl.topo.pins)
    out = np.zeros(len(parents), bool)
    for r in np.flatnonzero((parents < 0) & inl):
        b = int(r)
        while True:
            out[b] = True
            kids = [c for c in range(len(parents)) if parents[c] == b and inl[c]]
            if len(kids) != 1 or b in pins:
                break
            b = kids[0]
    return out


# --- end-state cases of the ordinary solve: built once, shared by the CPU and GPU modules -------------
class Case:
    """One rig, rest, iteration count, cone count and twist: the workload, a perturbed input pose
    that violates most limits, and the float64 frames."""

    def __init__(self, rig, rest, iterations, ncones, twist, n, constrained=None):
        self.key = (rig, rest, iterations, ncones, twist, n, None if constrained is None else tuple(constrained))
        self.wl = workload(rig, n, ncones, twist, RADII[ncones], iterations, rest=rest)
        self.free = workload(rig, n, ncones, twist, RADII[ncones], iterations, rest=rest,
                             constrained=[] if constrained is None else constrained)
        assert np.array_equal(self.free.pose, self.wl.pose) and np.array_equal(self.free.targets, self.wl.targets)
        self.pose_in = perturb(self.wl.pose, np.random.default_rng(7), (0.8, 1.5), 1.5)
        self._frames = self._regions = self._twist = None
        self._memo = {}

    @property
    def frames(self):
        if self._frames is None:
            self._frames = direction_frames(self.wl)
        return self._frames

    @property
    def regions(self):
        if self._regions is None:
            self._regions = regions(self.wl)
        return self._regions

    @property
    def twist(self):
        if self._twist is None:
            self._twist = TwistModel(self.wl)
        return self._twist

    def _memoised(self, name, pose, fn):
        """A measure is a pure function of the pose: bitwise equal poses share one evaluation."""
        k = (name, pose.tobytes())
        if k not in self._memo:
            self._memo[k] = fn()
        return self._memo[k]

    def swing(self, pose):
        return self._memoised("swing", pose, lambda: swing_residual(self.wl, pose, self.frames, self.regions)[0])

    def twist_excess(self, pose):
        return self._memoised("twist", pose, lambda: self.twist.excess(self.wl, pose))

    def twist_left_out(self):
        """Constraints whose twist-frame arc is too close to the deadband to model."""
        return G.near_deadband(self.twist.arc)


_CASES = {}


def case(rig, rest, iterations, ncones, twist, n, constrained=None):
    k = (rig, rest, iterations, ncones, twist, n, None if constrained is None else tuple(constrained))
    if k not in _CASES:
        _CASES[k] = Case(rig, rest, iterations, ncones, twist, n, constrained)
    return _CASES[k]


_ORACLE = {}


def oracle_solve(oracle, c, constrained=True):
    """The CPU oracle's solve of a case (or of its unconstrained twin), once."""
    k = (c.key, constrained)
    if k not in _ORACLE:
        wl = c.wl if constrained else c.free
        o = oracle.Oracle(wl)
        _ORACLE[k] = o.solve(c.pose_in, wl.targets, threads=8)
        o.close()
    return _ORACLE[k]


def check_swing(c, pose, label):
    res = c.swing(pose)
    print(f"{label}: swing residual max {res.max():.3g} rad, {np.count_nonzero(res > G.SWING_BOUNDARY_LIMIT)}/{res.size} "
          f"inside the deadband, limit {SWING_BAND_LIMIT:.3g}")
    assert res.max() <= SWING_BAND_LIMIT, f"{label}: a direction ends {res.max():.3g} rad outside its region"


def check_twist(c, pose, label):
    ex = c.twist_excess(pose)
    out = c.twist_left_out()
    assert out.mean() <= LEFT_OUT_CAP, f"{label}: {out.sum()} constraints left out"
    worst = ex[~out].max()
    print(f"{label}: twist beyond range/2 max {worst:.3g} rad ({out.sum()} left out), limit {SOLVE_TWIST_LIMIT:.3g}")
    assert worst <= SOLVE_TWIST_LIMIT, f"{label}: a twist ends {worst:.3g} rad outside its range"


def check_rigid(c, pose, label):
    """Local positions outside the translating root segment and local scales stay put."""
    rs = root_segment_bones(c.wl)
    dp = np.abs(pose[:, ~rs, 4:7].astype(np.float64) - c.pose_in[:, ~rs, 4:7]).max()
    ds = np.abs(pose[..., 7:10].astype(np.float64) - c.pose_in[..., 7:10]).max()
    print(f"{label}: position drift {dp:.3g} (limit {SOLVE_POSITION_LIMIT:.3g}), scale drift {ds:.3g} (limit {SOLVE_SCALE_LIMIT:.3g})")
    assert dp <= SOLVE_POSITION_LIMIT and ds <= SOLVE_SCALE_LIMIT, label
