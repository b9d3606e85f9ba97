"""Float64 models of the solve's two geometric building blocks, written from their mathematical
definitions: the weighted rigid fit (Kabsch, by SVD) and the Kusudama swing region on the unit
sphere (cones joined by paths that two tangent circles bound).  Plain numpy; nothing here loads
the oracle or the library, so a misreading that those two share cannot reach these models.

Definitions used:
- rotation from a unit quaternion (x, y, z, w): R = I + 2w[v]x + 2[v]x^2;
- Kabsch 1976 / Markley 1988: R = V diag(1, 1, det(V U^T)) U^T for the SVD U S V^T of the
  weighted covariance sum_i w_i (moved_i - mc)(target_i - tc)^T;
- a cone is the spherical cap {p : angle(p, c) <= r}; the two circles tangent to the caps
  (cA, rA) and (cB, rB) have radius tr = (pi - rA - rB) / 2 and centres t with
  angle(t, cA) = rA + tr and angle(t, cB) = rB + tr;
- the path between A and B is, on each side of the A-B great circle, the spherical triangle
  (A, t, B) minus the open tangent cap around t;
- the constraint frames of a Kusudama, its twist limit (swing-twist decomposition about +Y, the
  twist clamped to half the range either side of the centre) and the one-cone swing snap: the
  last section of this file.

The limits below are 4 x the worst value measured against the CPU oracle over the fixed seeds of
tests/test_geometry_cpu.py; DESIGN.md section 7a ("Float64 geometry") holds the table of measured
values, limits and the reference quirks that narrow an input class."""
import math

import numpy as np

# --- asserted limits: DESIGN.md section 7a, one row each (measured worst x 4) --------------------
QCP_UNIT_LIMIT = 4 * 1.34e-7           # | |q| - 1 |
QCP_DIRECTION_LIMIT_DEG = 4 * 1.16e-4  # angle(R (moved_i - mc), target_i - tc), non-zero weights
QCP_DIRECTION2_LIMIT_DEG = 4 * 1.68e-3  # the same for two points: their covariance can be far less balanced
QCP_KABSCH_LIMIT_DEG = 4 * 1.51e-4     # angle between the returned rotation and Kabsch's, n >= 3
QCP_TRANSLATION_LIMIT = 4 * 1.83e-7    # |translation - (tc - mc)|, relative to 1 + |tc| + |mc|
TANGENT_CENTRE_LIMIT = 4 * 7.21e-4     # Euclidean distance of unit vectors
TANGENT_RADIUS_LIMIT = 4 * 5.86e-8     # rad
SWING_UNCHANGED_LIMIT = 4 * 6.66e-8    # |result - normalised input| for an in-bounds point
SWING_UNIT_LIMIT = 4 * 2.16e-7         # | |result| - 1 | for an out-of-bounds point
SWING_BOUNDARY_LIMIT = 4 * 1.70e-4     # rad, result to the nearest cone or tangent circle
SWING_NEAREST_LIMIT = 4 * 1.24e-4      # rad, angle(result, query) - angle(lattice nearest, query)
SWING_REGION_LIMIT = 4 * 6.18e-3       # rad, result to the nearest member of the lattice

BOUNDARY_DELTA = 1.0e-3                # rad: classification is not asserted closer to a boundary
LEFT_OUT_CAP = 0.02                    # share of a chain class's points that may be left out
LATTICE_POINTS = 400_000               # spacing sqrt(4 pi / N) = 5.6e-3 rad


def unit(v):
    v = np.asarray(v, np.float64)
    return v / np.linalg.norm(v, axis=-1, keepdims=True)


def angle(a, b):
    """Angle between vectors (last axis), accurate near 0 and pi."""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return np.arctan2(np.linalg.norm(np.cross(a, b), axis=-1), np.sum(a * b, axis=-1))


# --- rotations ------------------------------------------------------------------------------
def quat_to_matrix(q):
    x, y, z, w = (float(c) for c in q)
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)],
                     [2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)],
                     [2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)]], np.float64)


def axis_angle_matrix(axis, ang):
    k = unit(axis)
    K = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]], np.float64)
    return np.eye(3) + math.sin(ang) * K + (1 - math.cos(ang)) * (K @ K)


def rotation_angle(Ra, Rb):
    """Angle of the rotation Ra Rb^T, from both its symmetric and antisymmetric parts."""
    M = Ra @ Rb.T
    s = 0.5 * math.sqrt((M[2, 1] - M[1, 2]) ** 2 + (M[0, 2] - M[2, 0]) ** 2 + (M[1, 0] - M[0, 1]) ** 2)
    return math.atan2(s, 0.5 * (np.trace(M) - 1.0))


# --- weighted Kabsch ------------------------------------------------------------------------
def kabsch(moved, target, weights, translate):
    """(R, singular values, target centroid - moved centroid, moved centroid, target centroid).
    R maps the (centred) moved points onto the (centred) targets.  The weights are rounded to
    float32 first, as the fitted code multiplies by (float)w."""
    m, t = np.asarray(moved, np.float64), np.asarray(target, np.float64)
    w = np.asarray(weights, np.float32).astype(np.float64)
    if translate:
        mc, tc = (w[:, None] * m).sum(0) / w.sum(), (w[:, None] * t).sum(0) / w.sum()
    else:
        mc = tc = np.zeros(3)
    H = ((m - mc) * w[:, None]).T @ (t - tc)
    U, S, Vt = np.linalg.svd(H)
    d = np.sign(np.linalg.det(Vt.T @ U.T))
    R = Vt.T @ np.diag([1.0, 1.0, d]) @ U.T
    return R, S * np.array([1.0, 1.0, d]), tc - mc, mc, tc


def qcp_eigenvector_norm_sq(R, S):
    """Squared norm of the unnormalised quaternion that an adjugate-column eigenvector solve of
    Horn's 4x4 matrix yields for the fit (R, signed singular values S).  The matrix has the
    eigenvalues s1+s2+s3, s1-s2-s3, -s1+s2-s3, -s1-s2+s3; the first-row cofactors of (K - l1 I)
    are prod(l_i - l1) * q_w * q, and q_w = cos(angle / 2)."""
    gaps = 2 * (S[1] + S[2]) * 2 * (S[0] + S[2]) * 2 * (S[0] + S[1])
    return (gaps * math.cos(rotation_angle(R, np.eye(3)) / 2)) ** 2


# --- Kusudama swing region ------------------------------------------------------------------
def tangent_circles(A, rA, B, rB):
    """(centre on the negative side of A x B, centre on the positive side, radius)."""
    A, B = unit(A), unit(B)
    tr = (math.pi - rA - rB) / 2
    cA, cB, d = math.cos(rA + tr), math.cos(rB + tr), float(A @ B)
    a, b = (cA - d * cB) / (1 - d * d), (cB - d * cA) / (1 - d * d)
    inplane = a * A + b * B
    h = math.sqrt(max(0.0, 1.0 - float(inplane @ inplane)))
    n = unit(np.cross(A, B))
    return inplane - h * n, inplane + h * n, tr


class SwingRegion:
    """The allowed region of cones [k][4] = (control point, radius): caps and paths."""

    def __init__(self, cones, swap_sides=False, tangent_radius_offset=0.0):
        cones = np.asarray(cones, np.float64)
        self.c = unit(cones[:, :3])
        self.r = cones[:, 3].copy()
        self.paths = []
        for i in range(len(cones) - 1):
            tn, tp, tr = tangent_circles(self.c[i], self.r[i], self.c[i + 1], self.r[i + 1])
            if swap_sides:          # negative control: a model with the centres on the wrong sides
                tn, tp = tp, tn
            self.paths.append((self.c[i], self.c[i + 1], tn, tp, tr + tangent_radius_offset))

    def circles(self):
        """Every circle that carries a piece of the region's boundary: (centre, radius, is_tangent)."""
        out = [(c, r, False) for c, r in zip(self.c, self.r)]
        for _, _, tn, tp, tr in self.paths:
            out += [(tn, tr, True), (tp, tr, True)]
        return out

    def member(self, p):
        """Membership of unit vectors p [m][3].  Angles are compared through their cosines, which
        is exact enough away from the boundary; points near it are left out by the callers."""
        p = unit(p)
        inside = np.zeros(p.shape[:-1], bool)
        for c, r in zip(self.c, self.r):
            inside |= p @ c >= math.cos(r)
        for A, B, tn, tp, tr in self.paths:
            for t, sign in ((tn, 1.0), (tp, -1.0)):
                tri = (sign * (p @ np.cross(A, t)) > 0) & (sign * (p @ np.cross(t, B)) > 0) & (sign * (p @ np.cross(B, A)) > 0)
                inside |= tri & (p @ t <= math.cos(tr))
        return inside

    def members_near_boundary(self, lattice, band):
        """The lattice members within `band` of a boundary-carrying circle.  The member nearest to
        a point outside the region, or to a point of its boundary, is one of them when band
        exceeds 2.5 covering radii of the lattice: a member deeper inside has a lattice point in
        a ball that lies wholly in the region and nearer to the query."""
        near = np.zeros(len(lattice), bool)
        for c, r, _ in self.circles():
            d = lattice @ c
            near |= (d < math.cos(max(r - band, 0.0))) & (d > math.cos(min(r + band, math.pi)))
        cand = lattice[near]
        return cand[self.member(cand)]

    def signed_circle_distances(self, p):
        """[circle][point]: angle(p, centre) - radius."""
        return np.stack([angle(p, c) - r for c, r, _ in self.circles()])

    def boundary_distance(self, p):
        """Distance to the nearest boundary-carrying circle: a lower bound on (and, on the
        boundary's own arcs, equal to) the distance to the region's boundary."""
        return np.abs(self.signed_circle_distances(p)).min(axis=0)

    def left_out(self, p, cap_slack=0.0):
        """Points whose classification is not asserted: within BOUNDARY_DELTA of a boundary circle,
        or less than cap_slack inside a tangent cap."""
        d = self.signed_circle_distances(p)
        tang = np.array([k for _, _, k in self.circles()])
        out = (np.abs(d) < BOUNDARY_DELTA).any(axis=0)
        if tang.any():
            out |= ((d[tang] < 0) & (d[tang] > -cap_slack)).any(axis=0)
        return out


def fibonacci_sphere(n=LATTICE_POINTS):
    i = np.arange(n, dtype=np.float64) + 0.5
    z = 1.0 - 2.0 * i / n
    phi = i * (math.pi * (3.0 - math.sqrt(5.0)))
    s = np.sqrt(1.0 - z * z)
    return np.stack([s * np.cos(phi), s * np.sin(phi), z], axis=1)


def nearest_members(members, queries):
    """For each query the lattice member with the largest dot product: (points, angles)."""
    q = unit(queries)
    idx = np.argmax(q @ members.T, axis=1)
    near = members[idx]
    return near, angle(near, q)


# --- Transform3D (rows r0 r1 r2 | origin), float64 values and rounding bounds ------------------
U32 = 2.0 ** -24


def _gamma(n):
    return n * U32 / (1 - n * U32)


def xform_split(x):
    x = np.asarray(x, np.float64)
    return x[:9].reshape(3, 3), x[9:]


def xform_mul_f64(a, b):
    """(value [12], bound [12]) of a * b: every entry is a dot product of at most four float32
    terms, |fl(s) - s| <= gamma_n sum |x_i y_i| (Higham, Accuracy and Stability, section 3.1)."""
    Ab, Ao = xform_split(a)
    Bb, Bo = xform_split(b)
    val = np.concatenate([(Ab @ Bb).reshape(-1), Ab @ Bo + Ao])
    bound = np.concatenate([(_gamma(3) * (np.abs(Ab) @ np.abs(Bb))).reshape(-1), _gamma(4) * (np.abs(Ab) @ np.abs(Bo) + np.abs(Ao))])
    return val, bound


def xform_affine_inverse_f64(a):
    """(value [12], bound [12]) of the affine inverse computed as adjugate * fl(1 / det) and
    -(inverse basis) * origin.  Rounding model: a 2x2 cofactor carries gamma_2 (|ab| + |cd|); the
    determinant is six triple products, gamma_5 of their absolute sum; the reciprocal and each
    product add one rounding; the origin is a three-term dot product of the computed entries."""
    Ab, Ao = xform_split(a)
    cof = np.zeros((3, 3))
    acof = np.zeros((3, 3))
    for i in range(3):
        for j in range(3):
            r = [k for k in range(3) if k != i]
            c = [k for k in range(3) if k != j]
            p, q = Ab[r[0], c[0]] * Ab[r[1], c[1]], Ab[r[0], c[1]] * Ab[r[1], c[0]]
            cof[i, j] = (-1) ** (i + j) * (p - q)
            acof[i, j] = abs(p) + abs(q)
    det = float(Ab[0] @ cof[0])
    ddet = _gamma(5) * float(np.abs(Ab[0]) @ acof[0])
    rel_s = (U32 + ddet / (abs(det) - ddet)) * (1 + U32)
    inv = cof.T / det
    dinv = (_gamma(2) * acof.T * (1 + rel_s) * (1 + U32) + np.abs(cof.T) * (rel_s + U32 + rel_s * U32)) / abs(det)
    org = -(inv @ Ao)
    dorg = (dinv @ np.abs(Ao)) * (1 + _gamma(3)) + _gamma(3) * (np.abs(inv) @ np.abs(Ao))
    return np.concatenate([inv.reshape(-1), org]), np.concatenate([dinv.reshape(-1), dorg])


# --- constraint frames and the two snaps of a Kusudama ---------------------
# Every rotation below is a 3x3 matrix in the constrained bone's parent frame.  L is the bone's local
# rotation, D its bone-direction frame (a child of the bone's own frame), Y = (0, 1, 0).
Y_AXIS = np.array([0.0, 1.0, 0.0])
ARC_DEADBAND = math.acos(1.0 - 1.0e-5)   # 4.47e-3 rad: Godot's Quaternion(v0, v1) is the identity below it
ARC_DEADBAND_MARGIN = 1.0e-4             # rad: arcs this close to the deadband are not asserted either way


def shortest_arc(a, b, deadband=True):
    """The rotation by angle(a, b) about a x b: it takes a to b along their great circle.  Every arc
    of the reference is a Godot Quaternion(v0, v1), which returns the identity when the vectors'
    cosine exceeds 1 - CMP_EPSILON (1e-5): arcs below ARC_DEADBAND are not made (section 7a's quirk
    table).  deadband=False gives the plain definition."""
    a, b = unit(a), unit(b)
    ang = float(angle(a, b))
    if ang < (ARC_DEADBAND if deadband else 1e-300):
        return np.eye(3)
    return axis_angle_matrix(np.cross(a, b), ang)


def near_deadband(ang):
    """True where an arc of this angle could fall on either side of the deadband in float32."""
    return np.abs(np.asarray(ang) - ARC_DEADBAND) < ARC_DEADBAND_MARGIN


def bone_direction_frame(child_positions):
    """A bone's bone-direction frame from the local positions of its children (unit scales).  The
    reference turns the frame by the arc from the children's centroid direction to the frame's own
    +Y (ik_bone_3d.cpp:91: Quaternion(child_centroid, bone_direction), applied on the left), so the
    frame's +Y ends mirrored through +Y, not on the centroid.  Identity for a childless bone and
    for a centroid on +Y."""
    c = np.asarray(child_positions, np.float64).reshape(-1, 3)
    if len(c) == 0:
        return np.eye(3)
    return shortest_arc(c.mean(axis=0), Y_AXIS)


def bone_direction_frames(parents, positions, in_list=None):
    """[bone] frames of one skeleton: positions [B][3] are the rest pose's local positions; a bone's
    children are its children among the solved bones (`in_list`, default all)."""
    parents = np.asarray(parents)
    B = len(parents)
    in_list = np.ones(B, bool) if in_list is None else np.asarray(in_list, bool)
    return np.stack([bone_direction_frame([positions[c] for c in range(B) if parents[c] == b and in_list[c]])
                     for b in range(B)])


def twist_direction(cones):
    """The direction the twist frame's +Y is taken to: the normalised mean of the points half way
    (along the great circle) between consecutive normalised control points of cones [k][4]; for
    one cone its control point; None without cones."""
    cones = np.asarray(cones, np.float64).reshape(-1, 4)
    if len(cones) == 0:
        return None
    c = unit(cones[:, :3])
    if len(c) == 1:
        return c[0]
    return unit(np.mean([unit(c[i] + c[i + 1]) for i in range(len(c) - 1)], axis=0))


def twist_frame(cones, reverse_arc=False):
    """The twist frame in the parent frame: the shortest arc that takes +Y to twist_direction(cones)
    (ik_kusudama_3d.cpp:37-89); the parent's frame without cones.  reverse_arc (negative control):
    the arc taken from that direction to +Y."""
    mean = twist_direction(cones)
    if mean is None:
        return np.eye(3)
    return shortest_arc(mean, Y_AXIS) if reverse_arc else shortest_arc(Y_AXIS, mean)


def twist_centre(min_angle, times=2):
    """+Z turned about +Y by min_angle twice (ik_kusudama_3d.cpp:108-111 applies twist_min_rot to
    +Z and then to the result), as the rotation about +Y.  times=1 is the negative control."""
    return axis_angle_matrix(Y_AXIS, times * float(min_angle))


def twist_angle(A):
    """The angle about +Y of the twist factor of A = swing * twist: for the quaternion (x, y, z, w)
    of A it is 2 atan2(y, w), and A[0,2] - A[2,0] = 4wy, A[0,0] + A[2,2] = 2(w^2 - y^2)."""
    return math.atan2(A[0, 2] - A[2, 0], A[0, 0] + A[2, 2])


def twist_offset(L, frame, centre):
    """The twist angle of the local rotation L away from the centre of the twist range."""
    return twist_angle(centre.T @ frame.T @ L)


def twist_limit(L, frame, centre, twist_range, half=0.5):
    """(expected rotation, twist angle before): frame * centre * swing * twist with the twist
    clamped to +-range/2 (ik_kusudama_3d.cpp:117-132).  half=1.0 is the negative control."""
    A = centre.T @ frame.T @ L
    t = twist_angle(A)
    swing = A @ axis_angle_matrix(Y_AXIS, -t)
    lim = half * float(twist_range)
    tc = t if lim >= math.pi else min(max(t, -lim), lim)
    return frame @ centre @ swing @ axis_angle_matrix(Y_AXIS, tc), t


def bone_direction(L, D, origin_offset=None):
    """The direction the swing limit judges, in the parent frame: L * D * (+Y), seen from the
    orientation frame's origin.  The ordinary solve keeps that origin on the bone's own
    (ik_bone_3d.cpp:145-151); constraint_mode never moves it off the parent's, so there the tip
    point is origin_offset (the bone's local position) + L * D * (+Y)."""
    tip = L @ D @ Y_AXIS
    if origin_offset is not None:
        tip = tip + np.asarray(origin_offset, np.float64)
    return tip


def swing_snap_one_cone(L, D, cone, origin_offset=None, radius_scale=1.0):
    """(expected rotation, angle of the direction beyond the cap, <= 0 inside).  Outside the cap
    {p : angle(p, c) <= r}, L is turned in the parent frame by the shortest arc from the
    direction to the point of the cap's circle on the great circle through c and the direction
    (ik_kusudama_3d.cpp:347-376, ik_open_cone_3d.cpp:358-381)."""
    cone = np.asarray(cone, np.float64)
    c, r = unit(cone[:3]), float(cone[3]) * radius_scale
    d = bone_direction(L, D, origin_offset)
    excess = float(angle(d, c)) - r
    if excess <= 0:
        return L, excess
    on_circle = axis_angle_matrix(np.cross(c, unit(d)), r) @ c
    return shortest_arc(d, on_circle) @ L, excess
