"""Float64 models of the four pose stages around the solve, written from what each operation means:
clip sampling (mbik_clip_sample steps 3 to 5), the modifier blend (mbik_pose_blend steps 2 to 5),
bone globals (mbik_pose_globals) and target capture (mbik_capture_targets).  Plain numpy; nothing
here loads the library, the oracle or the float32 recipes (clip_recipe, blend_recipe,
pose_globals_recipe), so a misreading that those share cannot reach these models.  Only the float64
Transform3D helpers of tests/geometry_f64.py are reused.  Every model returns the value and a bound
on the float32 result, as skin_cases.reference64 does; u = 2^-24, gamma_n = n u / (1 - n u).

Each model takes the switches of its wrong variants (the control tests of
tests/test_pose_meaning_cpu.py): long_arc, scale_first, child_first, wrap_pair, side, swapped.

Clip sampling, one tracked channel with keys (T, V) at raw time t in a clip of `length`:
    t' = clamp(t, 0, length) (LOOP_NONE) or fposmod(t, length) by math.fmod (LOOP_LINEAR);
    i = np.searchsorted(T, t', side="right") - 1, the last key <= t': discrete and exact, on the
        doubles the entry compares, so no time is left out for being close to a key;
    the pair (a, b) and the fraction c = from / delta in float64:
        interior     0 <= i < n-1              a = i, b = i+1   delta = T[b] - T[a]             from = t' - T[a]
        wrap after   wrap, i = n-1             a = n-1, b = 0   delta = (length - T[a]) + T[b]  from = t' - T[a]
        wrap before  wrap, i = -1              a = n-1, b = 0   the same delta                  from = (length - T[a]) + t'
        ends         no wrap, i = -1 / n-1, or one key:  the key itself
    (c = 0 when |delta| < 1e-5, Godot's is_zero_approx; a nearest track takes V[a]);
    positions and scales V[a] + (V[b] - V[a]) c; rotations the point at c of the shortest geodesic
    between the unit key quaternions.
  Bound of a lerped component.  The entry rounds from and delta to float32 (u each, relative: their
  double differences are the model's own) and divides (u): |c32 - c| <= gamma_3 |c|.  The lerp is one
  subtraction d = fl(V[b] - V[a]) (u |d|), one product p = fl(d c32) and one sum fl(V[a] + p): with
  D = |V[b] - V[a]| |c|, |p - (V[b] - V[a]) c| <= gamma_5 D and the sum adds u (|V[a]| + (1 + gamma_5) D):
      bound = gamma_5 D + u (|V[a]| + (1 + gamma_5) D).
  A copied key and an untracked channel (the rest pose) are exact: bound 0.  An interpolated rotation
  has no derived bound (the float32 slerp goes through acosf and sinf); it is judged by its angle to
  the model's, against a measured tolerance, and only where the arc between its two keys is below
  pi - ARC_MARGIN: towards pi the shortest arc's side flips with the last bit of the dot product.

Modifier blend of one bone, input pose a, modifier pose m, weight w:
    A = R(q_a / |q_a|) diag(s_a) with origin p_a, M likewise: Basis(rotation) * diag(scale);
    w >= 1, a NaN w or A == M (all 12 numbers): the modifier's pose stands, bit for bit;
    Godot's decomposition: scale S = sign(det A) * column norms, rotation R_A = A diag(1 / S);
    R_w = the point at w of the geodesic from R_A to R_M (R_A exp(w log(R_A^T R_M))),
    S_w = S_A + (S_M - S_A) w, o_w = p_a + (p_m - p_a) w (a negative w counts as 0);
    the blended transform is R_w diag(S_w) with origin o_w.
  The output pose is compared as a transform, R(q_out / |q_out|) diag(s_out) against R_w diag(S_w):
  that removes the quaternion's sign and the freedom of where a reflection is written.  The error is
  judged relative to max |S_w| against a measured tolerance, where the rotation from R_A to R_M is
  below pi - ARC_MARGIN and min |S_w| >= MIN_SCALE (with determinants of opposite sign the scale lerp
  passes through zero, where the decomposition of the result is undefined).  The origin's bound is
  the lerp bound above with c = w exact: gamma_2 D + u (|p_a| + (1 + gamma_2) D), D = |p_m - p_a| |w|.

Bone globals: global(b) = local(b) for a parentless bone, else global(parent(b)) * local(b), found by
walking up `parents` from each bone (no depth schedule); skin(b) = global(b) * inv_bind[b]; a pin's
distance |global(bone).origin - target.origin|.
  Bound.  geometry_f64.xform_mul_f64 bounds the rounding of one product entry by entry.  Carried
  down a chain entry by entry, an error bound is multiplied by |R| at every level, whose row sums
  reach sqrt(3): it would grow like 1.7^depth while the error itself does not.  So the error is
  carried in norms, and each level's fresh error is taken to the bone through the transforms that
  really lie between them.  Along a bone's ancestors c_0 (a root) ... c_m (the bone itself), level i
  adds the fresh basis error F_i = G(c_i-1) dL_i + rounding_i, with
      rho_i = |G(c_i-1)|_F e_l(c_i) + 1.01 |r_i|_F  >=  |F_i|_F,        rho_0 = e_l(c_0),
  r_i being xform_mul_f64's bound of that product (basis part) and e_l the local's own error
  (below); 1.01 covers r_i being taken at the float64 operands instead of the computed ones.  The
  later levels multiply F_i by L(c_i+1) ... L(c_m) = G(c_i)^-1 G(c_m) (bases), so to first order
      e_b(c_m) = 1.01 sum_i rho_i |G(c_i)^-1 G(c_m)|_F                  (|XY|_F <= |X|_F |Y|_F)
  bounds the Frobenius norm of the basis error (the outer 1.01: the second-order products of two
  errors).  An origin is a sum, origin(c_m) = sum_i G(c_i-1) p(c_i) with the exact positions p, so
  its errors only add:
      e_o(c_m) = e_o(c_m-1) + e_b(c_m-1) |p(c_m)| + 1.01 |r_m origin part|_2.
  Every entry of a global is then within e_b (basis) or e_o (origin).  The local's error: Basis(q)
  is built as 1 - (yy + zz), xy - wz, ... from s = 2 / (q . q): the dot product carries gamma_4, s
  one more rounding, each of xs = x s, xy = x ys one more, so a product term is within gamma_7 of
  itself, the sum or difference of two within gamma_8 (|xy| + |wz|), and a diagonal entry adds
  u |entry|; the product with diag(scale) is one rounding an entry (the other two terms are exact
  zeros).  The skin transform is one more product: e_b |inv_bind basis|_F + 1.01 |r|_F, and its
  origin e_b |inv_bind origin| + e_o + 1.01 |r origin part|; the distance is within e_o of the exact
  one plus gamma_4 (distance + e_o) for its subtraction, squares, sums and square root.

Target capture: affine_inverse(skeleton_global) * target_global by geometry_f64's
xform_affine_inverse_f64 and xform_mul_f64; the inverse's bound is carried through the product entry
by entry (one product: no growth), and the product's rounding bound is taken at |inverse| + its bound.
Hidden entries keep the previous target's bits."""
import math

import numpy as np

from . import geometry_f64 as G

U32 = G.U32
gamma = G._gamma
POSITION, ROTATION, SCALE = 0, 1, 2
SLICE = {POSITION: slice(4, 7), ROTATION: slice(0, 4), SCALE: slice(7, 10)}
CMP_EPSILON = 1e-5
ARC_MARGIN = 0.05    # rad: a rotation is judged only where its arc is below pi - ARC_MARGIN
MIN_SCALE = 0.1      # a blended bone is judged only where min |S_w| is at least this

UNTRACKED, SINGLE, CLAMP_FIRST, CLAMP_LAST, INTERIOR, WRAP_BEFORE, WRAP_AFTER = range(7)


# --- rotations --------------------------------------------------------------------------------
def unit_quats(q):
    q = np.asarray(q, np.float64)
    return q / np.linalg.norm(q, axis=-1, keepdims=True)


def rotations(q):
    """[..., 3, 3] rotation matrices of the normalised quaternions q [..., 4] (x, y, z, w)."""
    x, y, z, w = np.moveaxis(unit_quats(q), -1, 0)
    R = np.stack([1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y),
                  2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x),
                  2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)], axis=-1)
    return R.reshape(R.shape[:-1] + (3, 3))


def pose_basis(pose, scale_first=False):
    """[..., 3, 3]: R(q / |q|) diag(s) of poses [..., 10].  scale_first (wrong): diag(s) R."""
    pose = np.asarray(pose, np.float64)
    R, s = rotations(pose[..., 0:4]), pose[..., 7:10]
    return R * (s[..., :, None] if scale_first else s[..., None, :])


def rodrigues(axis, ang):
    """[m, 3, 3]: the rotations by ang [m] about the unit axes [m, 3]."""
    k = np.asarray(axis, np.float64)
    K = np.zeros(k.shape[:-1] + (3, 3))
    K[..., 0, 1], K[..., 0, 2], K[..., 1, 0] = -k[..., 2], k[..., 1], k[..., 2]
    K[..., 1, 2], K[..., 2, 0], K[..., 2, 1] = -k[..., 0], -k[..., 1], k[..., 0]
    s, c = np.sin(ang)[..., None, None], np.cos(ang)[..., None, None]
    return np.eye(3) + s * K + (1 - c) * (K @ K)


def quat_arc(qa, qb):
    """Rotation angle [m] in [0, pi] between the rotations of unit quaternions qa, qb [m, 4]."""
    half = np.arctan2(np.linalg.norm(qa - qb, axis=-1), np.linalg.norm(qa + qb, axis=-1))   # half the 4-D angle
    return 4.0 * np.minimum(half, math.pi / 2 - half)


def quat_angle(q, ref):
    """The same for any non-zero q against unit ref: the angle between the rotations they stand for."""
    return quat_arc(unit_quats(q), ref)


def quat_geodesic(qa, qb, c, long_arc=False):
    """The point at c [m] of the shortest geodesic from qa to qb (unit, [m, 4]); long_arc (wrong):
    from qa to qb as they stand, the long way round when their dot product is negative."""
    d = np.sum(qa * qb, axis=-1)
    if not long_arc:
        qb = np.where((d < 0)[:, None], -qb, qb)
    om = 2.0 * np.arctan2(np.linalg.norm(qa - qb, axis=-1), np.linalg.norm(qa + qb, axis=-1))   # angle on S^3
    s = np.sin(om)
    small = s < 1e-9
    ss = np.where(small, 1.0, s)
    k0 = np.where(small, 1.0 - c, np.sin((1.0 - c) * om) / ss)
    k1 = np.where(small, c, np.sin(c * om) / ss)
    return unit_quats(k0[:, None] * qa + k1[:, None] * qb)


def lerp_bound(a, b, c, c_roundings):
    """Bound [.., 3] of the float32 a + (b - a) c for float32 a, b and a c that carries c_roundings
    roundings (module docstring)."""
    D = np.abs(b - a) * np.abs(c)
    g = gamma(c_roundings + 2)
    return g * D + U32 * (np.abs(a) + (1 + g) * D) + 2.0 ** -148


# --- clip sampling ----------------------------------------------------------------------------
def clip_time(t, length, loop_mode):
    if loop_mode == 0:
        return min(max(t, 0.0), length)
    v = math.fmod(t, length)
    if v < 0:
        v += length
    return v + 0.0


def clip_track_f64(T, V, tp, length, linear, wrap, side="right", wrap_pair="last"):
    """One track at the mapped times tp [m]: (a, b, c, how), index arrays and the float64 fraction;
    b == a and c == 0 for a copy.  side="left" and wrap_pair="second" are the wrong variants."""
    n, m = T.shape[0], tp.shape[0]
    if n == 1:
        z = np.zeros(m, np.int64)
        return z, z, np.zeros(m), np.full(m, SINGLE, np.int8)
    i = np.searchsorted(T, tp, side=side) - 1
    interior = (i >= 0) & (i < n - 1)
    last = n - 1 if wrap_pair == "last" else 1
    a = np.where(interior, i, last)
    b = np.where(interior, i + 1, 0)
    how = np.where(interior, INTERIOR, np.where(i < 0, WRAP_BEFORE, WRAP_AFTER)).astype(np.int8)
    end = length - T[a]
    delta = np.where(interior, T[b] - T[a], end + T[b])
    frm = np.where(how == WRAP_BEFORE, end + tp, tp - T[a])
    c = np.where(np.abs(delta) < CMP_EPSILON, 0.0, frm / np.where(delta == 0, 1.0, delta))
    if not wrap:
        first, lastk = i < 0, i == n - 1
        a = np.where(first, 0, np.where(lastk, n - 1, a))
        how = np.where(first, CLAMP_FIRST, np.where(lastk, CLAMP_LAST, how)).astype(np.int8)
        b = np.where(first | lastk, a, b)
        c = np.where(first | lastk, 0.0, c)
    if not linear:
        b, c = a, np.zeros(m)
    return a, b, c, how


def clip_sample_f64(bone_count, rest, clips, time, clip_index, side="right", wrap_pair="last", long_arc=False):
    """Every bone of every skeleton at its finite time in its valid clip.  Returns a dict:
    value [n][B][10] float64; bound [n][B][10] (0 where the value is a copy, NaN on an interpolated
    rotation); how [n][B][3] (the case taken, UNTRACKED ... WRAP_AFTER); interp [n][B][3] (two keys
    were combined); arc [n][B] (rotation between an interpolated rotation's two keys, else 0);
    on_key [n][B][3] (the mapped time equals a key's)."""
    B = int(bone_count)
    rest = np.asarray(rest, np.float32).reshape(B, 10).astype(np.float64)
    time = np.asarray(time, np.float64).reshape(-1)
    ci = np.asarray(clip_index).reshape(-1)
    n = time.shape[0]
    assert np.isfinite(time).all() and ((ci >= 0) & (ci < len(clips))).all()
    value = np.broadcast_to(rest, (n, B, 10)).copy()
    bound = np.zeros((n, B, 10))
    how = np.full((n, B, 3), UNTRACKED, np.int8)
    interp = np.zeros((n, B, 3), bool)
    on_key = np.zeros((n, B, 3), bool)
    arc = np.zeros((n, B))
    for k, clip in enumerate(clips):
        sel = np.nonzero(ci == k)[0]
        if sel.size == 0:
            continue
        length = float(clip["length"])
        tp = np.array([clip_time(float(t), length, clip["loop_mode"]) for t in time[sel]])
        for tr in clip["tracks"]:
            T = np.asarray(tr["times"], np.float64).reshape(-1)
            if T.shape[0] == 0:
                continue
            bone, ch = int(tr["bone"]), int(tr["channel"])
            V = np.asarray(tr["values"], np.float32).reshape(T.shape[0], -1).astype(np.float64)
            wrap = clip["loop_mode"] == 1 and bool(tr["loop_wrap"])
            a, b, c, h = clip_track_f64(T, V, tp, length, tr["interpolation"] == 1, wrap, side, wrap_pair)
            two = a != b
            sl = SLICE[ch]
            how[sel, bone, ch], interp[sel, bone, ch] = h, two
            on_key[sel, bone, ch] = np.isin(tp, T)
            if ch == ROTATION:
                out = V[a]
                if two.any():
                    qa, qb = unit_quats(V[a[two]]), unit_quats(V[b[two]])
                    out[two] = quat_geodesic(qa, qb, c[two], long_arc)
                    arc[sel[two], bone] = quat_arc(qa, qb)
                value[sel, bone, sl] = out
                bound[sel, bone, sl] = np.where(two[:, None], np.nan, 0.0)
            else:
                cc = c[:, None]
                value[sel, bone, sl] = V[a] + (V[b] - V[a]) * cc
                bound[sel, bone, sl] = np.where(two[:, None], lerp_bound(V[a], V[b], cc, 3), 0.0)
    return dict(value=value, bound=bound, how=how, interp=interp, arc=arc, on_key=on_key)


# --- modifier blend ---------------------------------------------------------------------------
def godot_decompose(A):
    """Godot's convention for bases A [m, 3, 3]: (scale = sign(det) * column norms, rotation = A diag(1 / scale))."""
    sign = np.sign(np.linalg.det(A))
    scale = sign[:, None] * np.linalg.norm(A, axis=1)
    return scale, A / scale[:, None, :]


def blend_f64(pose_in, pose_mod, w, long_arc=False, scale_first=False):
    """The blend of bones pose_in / pose_mod [m][10] (float32) at weights w [m] (float32).  Returns a
    dict: early [m] (the modifier's bits stand); basis [m][3][3] = R_w diag(S_w); scale [m][3] = S_w;
    origin, origin_bound [m][3]; arc [m] (rotation from R_A to R_M); same_sign [m] (the two
    determinants' signs agree).  Rows with early set hold the modifier's own transform."""
    a = np.asarray(pose_in, np.float32).reshape(-1, 10).astype(np.float64)
    m = np.asarray(pose_mod, np.float32).reshape(-1, 10).astype(np.float64)
    w = np.asarray(w, np.float32).reshape(-1).astype(np.float64)
    A, M = pose_basis(a, scale_first), pose_basis(m, scale_first)
    same = (A == M).all(axis=(1, 2)) & (a[:, 4:7] == m[:, 4:7]).all(axis=1)
    early = ~(w < 1.0) | same
    w = np.where(early, 1.0, np.maximum(w, 0.0))
    sa, RA = godot_decompose(A)
    sm, RM = godot_decompose(M)
    D = np.swapaxes(RA, 1, 2) @ RM
    vee = 0.5 * np.stack([D[:, 2, 1] - D[:, 1, 2], D[:, 0, 2] - D[:, 2, 0], D[:, 1, 0] - D[:, 0, 1]], axis=1)
    s = np.linalg.norm(vee, axis=1)
    theta = np.arctan2(s, 0.5 * (np.trace(D, axis1=1, axis2=2) - 1.0))
    axis = np.where((s > 0)[:, None], vee / np.where(s > 0, s, 1.0)[:, None], np.array([1.0, 0.0, 0.0]))
    turn = -w * (2 * math.pi - theta) if long_arc else w * theta
    Rw = RA @ rodrigues(axis, turn)
    Sw = sa + (sm - sa) * w[:, None]
    basis = np.where(early[:, None, None], M, Rw * Sw[:, None, :])
    origin = a[:, 4:7] + (m[:, 4:7] - a[:, 4:7]) * w[:, None]
    return dict(early=early, basis=basis, scale=np.where(early[:, None], sm, Sw), origin=origin,
                origin_bound=lerp_bound(a[:, 4:7], m[:, 4:7], w[:, None], 0), arc=theta,
                same_sign=np.sign(sa[:, 0]) == np.sign(sm[:, 0]))


def blend_judged(model):
    """[m] bool: the blended bones whose transform error is judged (the module docstring's conditions)."""
    return ~model["early"] & (model["arc"] < math.pi - ARC_MARGIN) & (np.abs(model["scale"]).min(axis=1) >= MIN_SCALE)


def blend_transform_error(pose_out, model):
    """[m]: max |R(q_out) diag(s_out) - R_w diag(S_w)| over the nine entries, relative to max |S_w|."""
    T = pose_basis(np.asarray(pose_out, np.float32).reshape(-1, 10))
    return np.abs(T - model["basis"]).max(axis=(1, 2)) / np.abs(model["scale"]).max(axis=1)


# --- bone globals -----------------------------------------------------------------------------
def local_f64(pose10, scale_first=False):
    """(value [12], Frobenius bound of the basis error) of one bone's local transform from its
    float32 pose; the origin (the position) is exact."""
    p = np.asarray(pose10, np.float64)
    x, y, z, w = p[0:4] / np.linalg.norm(p[0:4])
    s = p[7:10]
    R = rotations(p[0:4])
    pairs = np.array([[y * y + z * z, abs(x * y) + abs(w * z), abs(x * z) + abs(w * y)],
                      [abs(x * y) + abs(w * z), x * x + z * z, abs(y * z) + abs(w * x)],
                      [abs(x * z) + abs(w * y), abs(y * z) + abs(w * x), x * x + y * y]])
    dR = gamma(8) * 2.0 * pairs + U32 * np.abs(R) * np.eye(3)
    if scale_first:
        basis, dB = R * s[:, None], dR * np.abs(s)[:, None] * (1 + U32) + U32 * np.abs(R * s[:, None])
    else:
        basis, dB = R * s[None, :], dR * np.abs(s)[None, :] * (1 + U32) + U32 * np.abs(R * s[None, :])
    return np.concatenate([basis.reshape(-1), p[4:7]]), float(np.linalg.norm(dB))


def ancestor_chains(parents):
    """Per bone the array of its ancestors from its root down to the bone itself, by walking up `parents`."""
    out = []
    for b in range(len(parents)):
        chain = []
        while b >= 0:
            chain.append(b)
            b = int(parents[b])
        out.append(np.array(chain[::-1]))
    return out


def globals_f64(parents, pins, pose, inv_bind=None, targets=None, child_first=False, scale_first=False):
    """Returns a dict: globals, globals_bound [n][B][12]; skin, skin_bound [n][B][12] when inv_bind
    [B][12] is given; dist, dist_bound [n][P] when targets [n][P][12] are.  child_first (wrong):
    local * global(parent); scale_first (wrong): diag(s) R for the local."""
    parents = [int(p) for p in parents]
    pose = np.asarray(pose, np.float32)
    n, B = pose.shape[:2]
    chains = ancestor_chains(parents)
    norm = np.linalg.norm
    out = dict(globals=np.zeros((n, B, 12)), globals_bound=np.zeros((n, B, 12)))
    if inv_bind is not None:
        ib = np.asarray(inv_bind, np.float32).astype(np.float64)
        out.update(skin=np.zeros((n, B, 12)), skin_bound=np.zeros((n, B, 12)))
    if targets is not None:
        tg = np.asarray(targets, np.float32).astype(np.float64)
        out.update(dist=np.zeros((n, len(pins))), dist_bound=np.zeros((n, len(pins))))
    for s in range(n):
        g = out["globals"][s]
        known = np.zeros(B, bool)
        rho, eb, eo, inv = np.zeros(B), np.zeros(B), np.zeros(B), np.zeros((B, 3, 3))

        def solve(b):
            path = []
            while b >= 0 and not known[b]:   # up to the first ancestor already known, or past a root
                path.append(b)
                b = parents[b]
            for c in reversed(path):
                lo, el = local_f64(pose[s, c], scale_first)
                p = parents[c]
                if p < 0:
                    g[c], rho[c] = lo, el
                else:
                    g[c], r = G.xform_mul_f64(lo, g[p]) if child_first else G.xform_mul_f64(g[p], lo)
                    rho[c] = norm(g[p, :9]) * el + 1.01 * norm(r[:9])
                    eo[c] = eo[p] + eb[p] * norm(lo[9:]) + 1.01 * norm(r[9:])
                basis = g[c, :9].reshape(3, 3)
                inv[c] = np.linalg.inv(basis)
                idx = chains[c]
                eb[c] = 1.01 * float(np.sum(rho[idx] * norm((inv[idx] @ basis).reshape(-1, 9), axis=1)))
                known[c] = True

        for b in range(B):
            solve(b)
        out["globals_bound"][s, :, :9], out["globals_bound"][s, :, 9:] = eb[:, None], eo[:, None]
        if inv_bind is not None:
            for b in range(B):
                out["skin"][s, b], r = G.xform_mul_f64(g[b], ib[b])
                out["skin_bound"][s, b, :9] = eb[b] * norm(ib[b, :9]) + 1.01 * norm(r[:9])
                out["skin_bound"][s, b, 9:] = eb[b] * norm(ib[b, 9:]) + eo[b] + 1.01 * norm(r[9:])
        if targets is not None:
            for e, pin in enumerate(pins):
                d = float(norm(g[int(pin), 9:] - tg[s, e, 9:]))
                out["dist"][s, e], out["dist_bound"][s, e] = d, eo[int(pin)] + gamma(4) * (d + eo[int(pin)])
    return out


# --- target capture ---------------------------------------------------------------------------
def capture_f64(skeleton_global, target_global, swapped=False):
    """(value [12], bound [12]) of affine_inverse(skeleton_global) * target_global for float32
    transforms [12]; swapped (wrong): affine_inverse(target_global) * skeleton_global."""
    sk, tg = np.asarray(skeleton_global, np.float64), np.asarray(target_global, np.float64)
    if swapped:
        sk, tg = tg, sk
    inv, dinv = G.xform_affine_inverse_f64(sk)
    val, _ = G.xform_mul_f64(inv, tg)
    _, r = G.xform_mul_f64(np.abs(inv) + dinv, tg)
    dB, dO = dinv[:9].reshape(3, 3), dinv[9:]
    tB, tO = np.abs(tg[:9].reshape(3, 3)), np.abs(tg[9:])
    carried = np.concatenate([(dB @ tB).reshape(-1), dB @ tO + dO])
    return val, carried + r
