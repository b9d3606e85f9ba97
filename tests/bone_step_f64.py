"""Float64 model of one bone-step of the solve, written from the reference's definitions
("The bone-step: what one step means").  Plain numpy, vectorised over the
skeletons of a batch; like geometry_f64.py it loads neither the library, the oracle nor any float32
recipe, so a misreading that those share cannot reach it.  Unconstrained rigs only: no snap runs,
the stale bone-direction cache never arises and every transform a step reads is the fresh forward
kinematics of the current pose.

What a step of bone b in segment g is (file:line of the reference in brackets):

- Segmentation [ik_bone_segment_3d.cpp:352-378]: a segment runs from its root bone down to the first
  bone with no child, several children or a pin; every child of that tip starts a segment, kept if it
  has a pinned descendant.  Steps run in post-order, children before their parent, each segment from
  its tip to its root [:56-72, :210-240]; the parentless segment runs last and translates.
- Effectors and weights [:74-88, :309-343]: a segment sees its own pin, then those of its children,
  unless its own pin's motion_propagation_factor is 0.  Each pin reached contributes weight*falloff,
  then weight*(priority/max priority)*falloff twice per positive priority (max priority counts as 1
  when all are 0); the falloff is multiplied by a pinned segment's factor on the way down and the
  descent stops at 0.
- Headings [ik_effector_3d.cpp:90-149]: with T the pin's target, E the effector bone's
  bone-direction global (FK global * D) and o the stepped bone's origin, the target headings are
  T.origin - E.origin and (T.origin +- T.column - E.origin) * w for each positive priority, w the
  pair's heading weight again; the tip headings are E.origin - o and
  (E.origin +- E.column * priority - o) * min(|T.origin - o|, 1).
- Fit [qcp.cpp:56-127, 162-218]: S = sum w target moved^T, lambda0 = (sum w |target|^2 + sum w
  |moved|^2) / 2, no Newton step; the quaternion (w, x, y, z) is the first row of the adjugate of
  (K - lambda0 I) with the vector part negated, K the 4x4 key matrix of S; the identity when its
  squared norm is below PRECISION.  With translate both sets are centred at their weighted centroids
  first and the translation is target centroid - moved centroid.  One heading [:59-78]: the axis is
  normalize(v x u) (v target, u moved), w = sqrt((1 + cos) / 2), the vector length 1 / (2 w |u||v|)
  before normalisation, so the angle is 2 atan2(1 / (2 w |u||v|), w); the weight is not read.
- Damp [ik_bone_segment_3d.cpp:97-112, 146-147, 227-240]: bone_damp[id] inside the array, else the
  default, and the default when that is smaller; pi in the parentless segment.  The rotation's angle
  is clamped to the damp about the fit's axis; the slerp that follows has weight 0.
- Application [:152-154]: new global basis = R * old global basis, origin + translation (zero
  outside the parentless segment), local = parent global^-1 * new global; children keep their locals.
- Stabilization [:114-127, 163-180], parentless segments only (child segments are built with 0
  passes, ik_bone_segment_3d.h:101): msd = sum w |target heading - tip heading after the step|^2 /
  (sum w)^2 with the target headings of before the step; accepted when msd <= previous * 1.0001,
  else the pre-step local is restored; a repeated pass recomputes the same step from the same pose,
  so the count of passes does not matter; previous is infinite after the segment's root bone.

Derived limit (CLAMP_ANGLE_BOUND): a clamped step's float32 quaternion is (v * fl(sqrt((1 - c^2) /
(1 - w^2))), fl(c)), c = cos(damp / 2) in double.  Its angle 2 acos(fl(c)) differs from the damp by at
most 2 u c / sin(damp / 2), u = 2^-24.  The check measures that angle as the rotation from the input
local to the output local, both float32 quaternions that went through Basis(q) (a rounding per
entry), the three 3x3 products of rotate_local_with_global, the affine inverse and product of
set_global_pose and the orthonormalising quaternion extraction: ten float32 stages, each moving an
entry of a rotation matrix by at most gamma_3 = 3u and so the angle by at most 3 sqrt(2) u.  Bound:
2 u c / sin(damp / 2) + 10 * 3 sqrt(2) u."""
import math
from dataclasses import dataclass, field

import numpy as np

from . import geometry_f64 as G

PRECISION = 1.0e-6        # ik_bone_segment_3d.h:85 evec_prec
ACCEPT_FACTOR = 1.0001    # ik_bone_segment_3d.cpp:166

# every misreading a shared restatement could carry: each is a switch of the model (negative controls)
MISREADINGS = ("swapped_sets", "target_origin_of_stepped_bone", "target_pairs_unweighted", "tip_without_priority",
               "no_distance_scale", "no_falloff", "clamp_cos_damp", "larger_damp", "root_damped",
               "translate_everywhere", "msd_divided_once", "previous_never_reset")


def clamp_angle_bound(damp):
    """The derived bound of the module docstring, rad."""
    return 2 * G.U32 / math.tan(damp / 2) + 10 * 3 * math.sqrt(2.0) * G.U32


@dataclass
class Rig:
    parents: np.ndarray
    pins: np.ndarray                  # [P] pinned bones
    pin_weight: np.ndarray            # [P]
    pin_priority: np.ndarray          # [P][3]
    pin_propagation: np.ndarray       # [P]
    rest_positions: np.ndarray        # [n][B][3] local positions of the setup pose (unit scales)
    default_damp: float = math.radians(5.0)
    bone_damp: tuple = ()
    stabilization_passes: int = 0


@dataclass
class Segment:
    root: int
    parent: int
    tip: int = -1
    bones: list = field(default_factory=list)        # tip first
    children: list = field(default_factory=list)     # kept child segments
    pinned_descendants: bool = False
    effectors: list = field(default_factory=list)    # pin indices
    weights: np.ndarray = None


@dataclass
class Topology:
    segments: list          # Segment, in post-order: index = the post-order number
    bone_list: list         # the order in which one iteration steps the bones
    table: tuple            # (root, tip, heading count) per segment, post-order


def topology(rig, misread=frozenset()):
    parents = [int(p) for p in rig.parents]
    B = len(parents)
    kids = [[c for c in range(B) if parents[c] == b] for b in range(B)]
    pin_of = {int(b): i for i, b in enumerate(rig.pins)}
    prio = np.asarray(rig.pin_priority, np.float64)

    def build(root, parent):
        seg = Segment(root, parent)
        b, bones = root, [root]
        while len(kids[b]) == 1 and b not in pin_of:
            b = kids[b][0]
            bones.append(b)
        seg.tip, seg.bones = b, bones[::-1]
        for c in kids[b]:
            child = build(c, seg)
            if child.pinned_descendants:
                seg.pinned_descendants = True
                seg.children.append(child)
        seg.pinned_descendants |= b in pin_of
        return seg

    def factor(seg):
        return min(max(float(rig.pin_propagation[pin_of[seg.tip]]), 0.0), 1.0) if seg.tip in pin_of else 1.0

    def effectors(seg):
        out = [pin_of[seg.tip]] if seg.tip in pin_of else []
        if factor(seg) > 0.0:
            for c in seg.children:
                out += effectors(c)
        return out

    def weights(seg, falloff, out):
        if falloff <= 0.0:
            return out
        if seg.tip in pin_of:
            i = pin_of[seg.tip]
            f = 1.0 if "no_falloff" in misread else falloff
            w, top = float(rig.pin_weight[i]), float(prio[i].max())
            top = 1.0 if top == 0.0 else top
            out.append(w * f)
            for a in range(3):
                if prio[i, a] > 0.0:
                    out += [w * (prio[i, a] / top) * f] * 2
        for c in seg.children:
            weights(c, falloff * factor(seg), out)
        return out

    order = []

    def post(seg):
        for c in seg.children:
            post(c)
        seg.effectors = effectors(seg)
        seg.weights = np.array(weights(seg, 1.0, []), np.float64)
        order.append(seg)

    for r in range(B):
        if parents[r] < 0:
            seg = build(r, None)
            if seg.pinned_descendants:
                post(seg)
    return Topology(order, [b for s in order for b in s.bones],
                    (np.array([s.root for s in order]), np.array([s.tip for s in order]), np.array([len(s.weights) for s in order])))


# --- batched rotations --------------------------------------------------------------------------
def quat_to_matrix(q):
    """geometry_f64.quat_to_matrix over leading axes, of the normalised quaternion (x, y, z, w)."""
    q = np.asarray(q, np.float64)
    x, y, z, w = np.moveaxis(q / np.linalg.norm(q, axis=-1, keepdims=True), -1, 0)
    return np.stack([np.stack([1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)], -1),
                     np.stack([2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)], -1),
                     np.stack([2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)], -1)], -2)


def axis_angle_matrix(axis, ang):
    """Rodrigues over leading axes; the identity where the axis is zero."""
    k = np.nan_to_num(axis / np.maximum(np.linalg.norm(axis, axis=-1, keepdims=True), 1e-300))
    K = np.zeros(k.shape[:-1] + (3, 3))
    K[..., 0, 1], K[..., 0, 2], K[..., 1, 0] = -k[..., 2], k[..., 1], k[..., 2]
    K[..., 1, 2], K[..., 2, 0], K[..., 2, 1] = -k[..., 0], -k[..., 1], k[..., 0]
    s, c = np.sin(ang)[..., None, None], np.cos(ang)[..., None, None]
    return np.eye(3) + s * K + (1 - c) * (K @ K)


def rotation_angle(A, B):
    """geometry_f64.rotation_angle over leading axes: the angle of A B^T."""
    M = A @ np.swapaxes(B, -1, -2)
    s = 0.5 * np.sqrt((M[..., 2, 1] - M[..., 1, 2]) ** 2 + (M[..., 0, 2] - M[..., 2, 0]) ** 2 + (M[..., 1, 0] - M[..., 0, 1]) ** 2)
    return np.arctan2(s, 0.5 * (np.trace(M, axis1=-2, axis2=-1) - 1.0))


def rotation_axis(M):
    """Unnormalised axis of a rotation matrix (its antisymmetric part)."""
    return np.stack([M[..., 2, 1] - M[..., 1, 2], M[..., 0, 2] - M[..., 2, 0], M[..., 1, 0] - M[..., 0, 1]], -1)


# --- state ----------------------------------------------------------------------------------------
class State:
    """Local bases [n][B][3][3] and origins [n][B][3] of a batch, and each segment's `previous`."""

    def __init__(self, pose):
        if isinstance(pose, State):
            self.basis, self.origin, self.previous = pose.basis.copy(), pose.origin.copy(), dict(pose.previous)
            return
        pose = np.asarray(pose, np.float64)
        self.basis = quat_to_matrix(pose[..., 0:4]) * pose[..., None, 7:10]     # Basis(q) * diag(scale)
        self.origin = pose[..., 4:7].copy()
        self.previous = {}

    def globals(self, parents):
        Gb, Go = np.empty_like(self.basis), np.empty_like(self.origin)
        done = set()

        def visit(b):
            if b in done:
                return
            p = int(parents[b])
            if p < 0:
                Gb[:, b], Go[:, b] = self.basis[:, b], self.origin[:, b]
            else:
                visit(p)
                Gb[:, b] = Gb[:, p] @ self.basis[:, b]
                Go[:, b] = Go[:, p] + np.einsum("nij,nj->ni", Gb[:, p], self.origin[:, b])
            done.add(b)

        for b in range(len(parents)):
            visit(b)
        return Gb, Go


def direction_frames(rig):
    """[n][B] bone-direction frames D of the setup pose (ik_bone_3d.cpp:57-93)."""
    inl = np.zeros(len(rig.parents), bool)
    for p in rig.pins:
        b = int(p)
        while b >= 0 and not inl[b]:
            inl[b] = True
            b = int(rig.parents[b])
    return np.stack([G.bone_direction_frames(rig.parents, pos, inl) for pos in np.asarray(rig.rest_positions, np.float64)])


# --- headings -----------------------------------------------------------------------------------
def headings(rig, seg, bone, Gb, Go, D, Tb, To, misread=frozenset()):
    """(target [n][H][3], tip [n][H][3]) of segment `seg` for the stepped bone."""
    prio = np.asarray(rig.pin_priority, np.float64)
    o = Go[:, bone]
    tgt, tip, i = [], [], 0
    for e in seg.effectors:
        eb = int(rig.pins[e])
        eo = o if "target_origin_of_stepped_bone" in misread else Go[:, eb]
        tip_basis, tip_o = Gb[:, eb] @ D[:, eb], Go[:, eb]
        tgt.append(To[:, e] - eo)
        tip.append(tip_o - o)
        i += 1
        scale = np.minimum(np.linalg.norm(To[:, e] - o, axis=-1), 1.0)[:, None]
        if "no_distance_scale" in misread:
            scale = 1.0
        for a in range(3):
            if prio[e, a] > 0.0:
                w = 1.0 if "target_pairs_unweighted" in misread else seg.weights[i]
                col = Tb[:, e, :, a]
                tgt += [(To[:, e] + col - eo) * w, (To[:, e] - col - eo) * w]
                tcol = tip_basis[:, :, a] * (1.0 if "tip_without_priority" in misread else prio[e, a])
                tip += [(tip_o + tcol - o) * scale, (tip_o - tcol - o) * scale]
                i += 2
    return np.stack(tgt, 1), np.stack(tip, 1)


# --- the fit ------------------------------------------------------------------------------------
def fit(moved, target, w, translate, misread=frozenset()):
    """(quaternion w >= 0 [n], vector part [n][3], squared norm against PRECISION [n] (inf on the
    one-point path), translation [n][3]) as the reference defines them."""
    n, H, _ = moved.shape
    translation = np.zeros((n, 3))
    if translate:
        total = w.sum()
        mc, tc = (w[:, None] * moved).sum(1), (w[:, None] * target).sum(1)
        if total > 0:
            mc, tc = mc / total, tc / total
        moved, target, translation = moved - mc[:, None], target - tc[:, None], tc - mc
    a, b = (moved, target) if "swapped_sets" in misread else (target, moved)     # coords1, coords2 (qcp.cpp:48)
    if H == 1:
        u, v = b[:, 0], a[:, 0]
        nu, nv = np.linalg.norm(u, axis=-1), np.linalg.norm(v, axis=-1)
        prod = nu * nv
        with np.errstate(invalid="ignore", divide="ignore"):
            cosang = np.sum(u * v, -1) / prod
            q0 = np.sqrt(0.5 * (1.0 + cosang))
            coeff = 1.0 / (2.0 * q0 * prod)
            cr = np.cross(v, u)
            axis = np.nan_to_num(cr / np.linalg.norm(cr, axis=-1, keepdims=True))    # normalized() of zero is zero
            vec = coeff[:, None] * axis
            opposite = np.sum(u * v, -1) < (2.0e-15 - 1.0) * prod
            vec = np.where(opposite[:, None], u / nu[:, None], vec)
            q0 = np.where(opposite, 0.0, q0)
        ident = prod == 0.0
        qw, qv = np.where(ident, 1.0, q0), np.where(ident[:, None], 0.0, vec)
        nsq = np.full(n, np.inf)
    else:
        S = np.einsum("h,nhi,nhj->nij", w, a, b)
        lam = 0.5 * (np.einsum("h,nhi,nhi->n", w, a, a) + np.einsum("h,nhi,nhi->n", w, b, b))
        xx, xy, xz, yx, yy, yz, zx, zy, zz = (S[:, i, j] for i in range(3) for j in range(3))
        K = np.empty((n, 4, 4))
        K[:, 0] = np.stack([xx + yy + zz, yz - zy, zx - xz, xy - yx], -1)
        K[:, 1] = np.stack([yz - zy, xx - yy - zz, xy + yx, xz + zx], -1)
        K[:, 2] = np.stack([zx - xz, xy + yx, yy - xx - zz, yz + zy], -1)
        K[:, 3] = np.stack([xy - yx, xz + zx, yz + zy, zz - xx - yy], -1)
        C = K - lam[:, None, None] * np.eye(4)
        cof = [(-1) ** j * np.linalg.det(C[:, 1:][:, :, [k for k in range(4) if k != j]]) for j in range(4)]
        qw, qv = cof[0], -np.stack(cof[1:], -1)
        nsq = qw * qw + np.sum(qv * qv, -1)
        ident = nsq < PRECISION
        qw, qv = np.where(ident, 1.0, qw), np.where(ident[:, None], 0.0, qv)
    norm = np.sqrt(qw * qw + np.sum(qv * qv, -1))
    qw, qv = qw / norm, qv / norm[:, None]
    flip = np.where(qw < 0, -1.0, 1.0)
    return qw * flip, qv * flip[:, None], nsq, translation


def damp_of(rig, topo_seg, bone, misread=frozenset()):
    """The angle a step of `bone` may turn by."""
    if topo_seg.parent is None and "root_damped" not in misread:
        return math.pi
    d = float(np.float32(rig.default_damp))
    if bone < len(rig.bone_damp):
        b = float(np.float32(rig.bone_damp[bone]))
        d = max(b, d) if "larger_damp" in misread else min(b, d)
    return d


# --- one step, a segment's pass, an iteration --------------------------------------------------
def msd(target, tip, w, misread=frozenset()):
    with np.errstate(invalid="ignore", divide="ignore"):
        s = np.einsum("h,nhi,nhi->n", w, target - tip, target - tip)
        return s / w.sum() if "msd_divided_once" in misread else s / w.sum() ** 2


def step(rig, state, seg, bone, D, Tb, To, iteration=0, misread=frozenset()):
    """Steps `bone` in place; returns the step's record (arrays over the skeletons)."""
    parents = rig.parents
    Gb, Go = state.globals(parents)
    target, tip = headings(rig, seg, bone, Gb, Go, D, Tb, To, misread)
    translate = seg.parent is None or "translate_everywhere" in misread
    qw, qv, nsq, translation = fit(tip, target, seg.weights, translate, misread)
    angle = 2.0 * np.arctan2(np.linalg.norm(qv, axis=-1), qw)
    damp = damp_of(rig, seg, bone, misread)
    limit = 2.0 * damp if "clamp_cos_damp" in misread else damp
    clamped = angle > limit
    R = axis_angle_matrix(qv, np.minimum(angle, limit))
    pre = (state.basis[:, bone].copy(), state.origin[:, bone].copy())
    new_b, new_o = R @ Gb[:, bone], Go[:, bone] + translation
    p = int(parents[bone])
    if p >= 0:
        inv = np.linalg.inv(Gb[:, p])
        new_b, new_o = inv @ new_b, np.einsum("nij,nj->ni", inv, new_o - Go[:, p])
    state.basis[:, bone], state.origin[:, bone] = new_b, new_o
    rec = dict(bone=bone, segment=seg, iteration=iteration, fit_angle=angle, axis=qv, damp=damp, limit=limit, clamped=clamped,
               nsq=nsq, pre=pre, post=(new_b.copy(), new_o.copy()), accepted=np.ones(len(angle), bool), margin=np.full(len(angle), -1.0))
    if rig.stabilization_passes > 0 and seg.parent is None:
        Gb2, Go2 = state.globals(parents)
        _, tip2 = headings(rig, seg, bone, Gb2, Go2, D, Tb, To, misread)
        now = msd(target, tip2, seg.weights, misread)
        prev = state.previous.get(id(seg), np.full(len(angle), np.inf))
        with np.errstate(invalid="ignore"):
            ok = now <= prev * ACCEPT_FACTOR
            rec["margin"] = np.where(np.isinf(prev), -1.0, now / (prev * ACCEPT_FACTOR) - 1.0)
        rec["accepted"], rec["msd"], rec["previous"] = ok, now, prev
        state.basis[:, bone] = np.where(ok[:, None, None], new_b, pre[0])
        state.origin[:, bone] = np.where(ok[:, None], new_o, pre[1])
        prev = np.where(ok, now, prev)
        if bone == seg.root and "previous_never_reset" not in misread:
            prev = np.full(len(angle), np.inf)
        state.previous[id(seg)] = prev
    return rec


def _targets(targets):
    t = np.asarray(targets, np.float64)
    return t[..., 0:9].reshape(t.shape[:-1] + (3, 3)), t[..., 9:12]


def segment_pass(rig, pose, targets, segment, misread=frozenset(), iteration=0, topo=None, D=None):
    """IKBoneSegment3D::segment_solver of post-order segment `segment`: its children's passes, then
    its own bones from the tip to the root.  Returns (State, step records in order)."""
    topo = topology(rig, misread) if topo is None else topo
    D = direction_frames(rig) if D is None else D
    state = State(pose)
    Tb, To = _targets(targets)
    records = []

    def run(seg):
        for c in seg.children:
            run(c)
        for b in seg.bones:
            records.append(step(rig, state, seg, b, D, Tb, To, iteration, misread))

    run(topo.segments[segment])
    return state, records


def iteration(rig, pose, targets, misread=frozenset(), iteration=0, topo=None, D=None):
    """One iteration: the pass of every parentless segment.  Returns (State, step records)."""
    topo = topology(rig, misread) if topo is None else topo
    D = direction_frames(rig) if D is None else D
    state, records = State(pose), []
    for k, seg in enumerate(topo.segments):
        if seg.parent is None:
            state, rec = segment_pass(rig, state, targets, k, misread, iteration, topo, D)
            records += rec
    return state, records
