"""Expected values for the root-motion tests (CPU and GPU): include/mbik.h's semantics of
mbik_clip_root_motion[_layers] and mbik_root_motion_apply -- the root_motion branches of Godot 4.3's
AnimationMixer::_blend_process and Transform3D::operator*= -- in float64 / float32 numpy scalars and
small arrays, one IEEE operation per element at a time:

    1. clip == -1: the layer is off; another clip outside the set: all 10 floats 0x7fc00000
    2. w, the contributing layers, totals and blend factors: tests/clip_layers_recipe.py's plan()
       for the root bone
    3. t0 = time_prev, t1 = time; both finite: p0, p1 by clip_recipe.sample_time (np.fmod);
       looped = linear loop and p0 > p1; segments (p0, p1), or (p0, L) then (+0.0, p1);
       a non-finite time: one segment of two NaN values
    4. X(u): np.searchsorted on the key times at the mapped time u, clip_recipe.pick, then the copy,
       the lerp or tests/blend_recipe.py's slerp
    5. from position 0, scale 0, rotation identity, layers ascending, segments in order:
       acc = acc + (X(u1) - X(u0)) * blend; acc = normalized(acc * slerp(identity, X(u0)^-1 X(u1), blend))
    6. an accumulated channel: acc, NaN as 0x7fc00000; any other: the start value
    7. pose: the rest pose's root record for every valid skeleton

    apply: G' = G * Transform3D(Basis(q), p): Basis::set_quaternion, Basis::operator*,
    Transform3D::xform, and with the flag Basis::orthonormalize, in Godot's operation order

Nothing here calls the code under test.  Comparisons are on uint32 views: every value, no tolerance.
`motion64` and `apply64` are the float64 meaning of the same steps for the geometry tests.
"""
import numpy as np

from . import blend_recipe as R
from . import clip_layers_recipe as LR
from . import clip_recipe as C

F, D = np.float32, np.float64
ORTHONORMALIZE = 1
NORMALIZE = LR.NORMALIZE
LAYER_DTYPE = LR.LAYER_DTYPE
START = np.array([0, 0, 0, 1, 0, 0, 0, 0, 0, 0], np.float32)
IDENT = np.array([[0, 0, 0, 1]], np.float32)

bits = R.bits
same_bits = R.same_bits
pack = LR.pack


def value_at(track, ch, u, length):
    """Step 4: the channel's value (float32 [3] or [4]) at the already mapped time u, and the branch."""
    T, V, linear, wrap = track
    n = T.shape[0]
    i = int(np.searchsorted(T, u, side="right")) - 1
    a, b, c, how = C.pick(T, n, i, wrap, linear, u, length)
    if b is None:
        return V[a].copy(), how
    if ch == C.ROTATION:
        return C._canon(R.slerp(V[a][None, :], V[b][None, :], np.array([c], np.float32)))[0], how
    r = V[a] + (V[b] - V[a]) * c
    assert r.dtype == np.float32
    return C._canon(r), how


def segments(t0, t1, length, loop_mode):
    """Step 3: the list of (u0, u1) float64 pairs, or None for a non-finite time."""
    if not (np.isfinite(t0) and np.isfinite(t1)):
        return None
    p0, p1 = C.sample_time(t0, length, loop_mode), C.sample_time(t1, length, loop_mode)
    if loop_mode == 1 and p0 > p1:
        return [(p0, D(length)), (D(0.0), p1)]
    return [(p0, p1)]


def expected(bone_count, rest, clips, layers, time_prev, root, flags=0):
    """(motion [count][10], stats) of the layer records `layers` [count][K] and `time_prev` [count][K]."""
    layers = np.asarray(layers)
    count, K = layers.shape
    time_prev = np.asarray(time_prev, np.float64).reshape(count, K)
    invalid, blend, acc, _ = LR.plan(bone_count, clips, layers, flags)
    tracks = C.index_tracks(clips)
    out = np.empty((count, 10), np.float32)
    stats = {"invalid_skeletons": int(invalid.sum()), "looped": 0, "segments": 0, "nonfinite": 0, "start_channels": 0, "on_key": 0}
    with np.errstate(all="ignore"):
        for s in range(count):
            if invalid[s]:
                out[s] = C.QNAN
                continue
            for ch in (C.POSITION, C.ROTATION, C.SCALE):
                sl = C.SLICE[ch]
                a = START[sl].copy()
                done = False
                for l in range(K):
                    if not acc[s, l, root, ch]:
                        continue
                    ci = int(layers["clip"][s, l])
                    length = D(clips[ci]["length"])
                    track = tracks[ci][root, ch]
                    b = blend[s, l, root, ch]
                    segs = segments(time_prev[s, l], layers["time"][s, l], length, clips[ci]["loop_mode"])
                    if segs is None:
                        stats["nonfinite"] += 1
                        nan = np.full(4 if ch == C.ROTATION else 3, C.QNAN, np.float32)
                        pairs = [(nan, nan)]
                    else:
                        stats["looped"] += len(segs) == 2
                        pairs = []
                        for u0, u1 in segs:
                            stats["on_key"] += int(u0 in track[0]) + int(u1 in track[0])
                            pairs.append((value_at(track, ch, u0, length)[0], value_at(track, ch, u1, length)[0]))
                    for x0, x1 in pairs:
                        stats["segments"] += 1
                        if ch == C.ROTATION:
                            d = LR.quat_mul(LR.inverse(x0[None, :]), x1[None, :])
                            e = R.slerp(IDENT.copy(), d, np.array([b], np.float32))
                            a = R.normalized(LR.quat_mul(a[None, :], e))[0]
                        else:
                            a = a + (x1 - x0) * b
                        assert a.dtype == np.float32
                    done = True
                out[s, sl] = C._canon(a) if done else START[sl]
                stats["start_channels"] += not done
    return out, stats


def expected_plain(bone_count, rest, clips, time_prev, time, root, clip_index=None, clip=0):
    """The plain call: one record (time, clip, 1.0f) a skeleton, flags 0 (so an index of -1 is a layer that is off)."""
    t = np.asarray(time, np.float64).reshape(-1)
    ci = np.full(t.shape, clip, np.int32) if clip_index is None else np.asarray(clip_index, np.int32)
    motion, stats = expected(bone_count, rest, clips, pack(t[:, None], ci[:, None], np.ones((t.shape[0], 1), np.float32)),
                             np.asarray(time_prev, np.float64).reshape(-1, 1), root, 0)
    return motion, stats


def expected_pose(pose, rest, clips, layers, root):
    """Step 7 on a copy of `pose` [count][bones][10]: every valid skeleton (step 1, from the records)
    gets the rest pose's root record.  Returns (pose, valid [count])."""
    out = np.array(pose, np.float32)
    clip = np.asarray(layers)["clip"].astype(np.int64)
    valid = ~((clip != LR.OFF) & ((clip < 0) | (clip >= len(clips)))).any(axis=1)
    out[valid, root] = np.asarray(rest, np.float32).reshape(-1, 10)[root]
    return out, valid


# ---------------------------------------------------------------- apply
def _sqrtf(x):
    return F(R.libm().sqrtf(float(x)))


def _dot3(a, b):
    return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]


def _normalized3(a):
    l = (a[0] * a[0] + a[1] * a[1]) + a[2] * a[2]
    if l == 0:
        return np.zeros(3, np.float32)
    return a / _sqrtf(l)


def basis_from_quat(q):
    """Basis::set_quaternion, float32 scalars; rows."""
    x, y, z, w = q
    d = ((x * x + y * y) + z * z) + w * w
    s = F(2) / d
    xs, ys, zs = x * s, y * s, z * s
    wx, wy, wz = w * xs, w * ys, w * zs
    xx, xy, xz = x * xs, x * ys, x * zs
    yy, yz, zz = y * ys, y * zs, z * zs
    one = F(1)
    return np.array([[one - (yy + zz), xy - wz, xz + wy], [xy + wz, one - (xx + zz), yz - wx], [xz - wy, yz + wx, one - (xx + yy)]],
                    np.float32)


def apply_one(m, G, flags):
    m = np.asarray(m, np.float32)
    A = np.asarray(G[0:9], np.float32).reshape(3, 3)
    o = np.asarray(G[9:12], np.float32)
    Bq = basis_from_quat(m[0:4])
    p = m[4:7]
    no = np.array([_dot3(A[i], p) + o[i] for i in range(3)], np.float32)
    nb = np.empty((3, 3), np.float32)
    for i in range(3):
        for j in range(3):
            nb[i, j] = (Bq[0, j] * A[i, 0] + Bq[1, j] * A[i, 1]) + Bq[2, j] * A[i, 2]
    if flags & ORTHONORMALIZE:
        x, y, z = nb[:, 0].copy(), nb[:, 1].copy(), nb[:, 2].copy()
        x = _normalized3(x)
        y = y - x * _dot3(x, y)
        y = _normalized3(y)
        z = (z - x * _dot3(x, z)) - y * _dot3(y, z)
        z = _normalized3(z)
        nb = np.stack([x, y, z], axis=1).astype(np.float32)
    out = np.concatenate([nb.reshape(9), no])
    assert out.dtype == np.float32
    return C._canon(out)


def expected_apply(motion, skeleton_global, flags=0):
    motion = np.asarray(motion, np.float32).reshape(-1, 10)
    G = np.asarray(skeleton_global, np.float32).reshape(-1, 12)
    with np.errstate(all="ignore"):
        return np.stack([apply_one(motion[s], G[s], flags) for s in range(G.shape[0])])


# ---------------------------------------------------------------- float64 meaning
def value64(T, V, u):
    """A linear track's value at mapped time u by np.interp, float64 (keys at 0 and at the length)."""
    return np.array([np.interp(u, T, V[:, k].astype(D)) for k in range(V.shape[1])])


def quat_to_matrix64(q):
    q = np.asarray(q, D)
    q = q / np.linalg.norm(q)
    x, y, z, w = q
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)],
                     [2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)],
                     [2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)]])


def apply64(q, p, basis, origin):
    """G * T(q, p) in float64: (basis', origin')."""
    return basis @ quat_to_matrix64(q), basis @ np.asarray(p, D) + origin


# ---------------------------------------------------------------- inputs
def random_frames(seed, n, K, clips, specials=True):
    """(layers [n][K], time_prev [n][K]): clip_layers_recipe.random_layers' crowd with a previous time
    a fraction of a clip length behind each layer's time -- so about a fifth of the looping layers
    cross the seam -- and, with specials, t0 == t1, t0 > t1, times exactly on 0 and on the length,
    and non-finite previous times scattered through the batch; the previous time of an off layer is NaN."""
    layers = LR.random_layers(seed, n, K, clips, specials=specials)
    rng = np.random.default_rng(seed + 77)
    ci = layers["clip"].astype(np.int64)
    L = np.array([c["length"] for c in clips])[np.clip(ci, 0, len(clips) - 1)]
    t1 = layers["time"].copy()
    t0 = t1 - rng.uniform(0.0, 0.4, (n, K)) * L
    if specials:
        k = rng.uniform(0.0, 1.0, (n, K))
        t0 = np.where(k < 0.05, t1, t0)                                         # a frame of no length
        t0 = np.where((k >= 0.05) & (k < 0.10), t1 + 0.1 * L, t0)                # backwards
        on0 = (k >= 0.10) & (k < 0.14)
        t0 = np.where(on0, 0.0, t0)
        t1 = np.where(on0, 0.25 * L, t1)
        onL = (k >= 0.14) & (k < 0.18)
        t0 = np.where(onL, 0.75 * L, t0)
        t1 = np.where(onL, L, t1)                                                # ends exactly on the length
        fromL = (k >= 0.18) & (k < 0.22)
        t0 = np.where(fromL, L, t0)
        t1 = np.where(fromL, 1.25 * L, t1)
        nf = (k >= 0.22) & (k < 0.25)
        t0 = np.where(nf, np.array([np.nan, np.inf, -np.inf])[rng.integers(0, 3, (n, K))], t0)
        t0 = np.where(ci == LR.OFF, np.nan, t0)
    out = layers.copy()
    out["time"] = t1
    return out, np.ascontiguousarray(t0, np.float64)
