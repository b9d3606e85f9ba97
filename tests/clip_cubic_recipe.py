"""Expected values for the cubic-interpolation tests (CPU and GPU): include/mbik.h's continuation of
mbik_clip_sample's step 5 for INTERPOLATION_CUBIC -- Godot 4.3's Animation::_interpolate,
Math::cubic_interpolate_in_time and Quaternion::spherical_cubic_interpolate_in_time -- in float64 /
float32 numpy scalars, one IEEE operation at a time, on top of tests/clip_recipe.py's time mapping,
key search and weight (sample_time, pick) and tests/clip_layers_recipe.py's layer plan:

    copies   n == 1, or not wrap and i < 0 or i == n-1: V[0] / V[n-1], as for every interpolation
    keys     not wrap: a = i, b = i+1, pre = max(i-1, 0), post = min(i+2, n-1);
             wrap: a = i or n-1, b = (a+1) mod n, pre = (a-1) mod n, post = (a+2) mod n
    times    pre_t, to_t, post_t relative to T[a], a key reached round the clip a length earlier or
             later; differences and sums in float64, rounded once to float32
    c        clip_recipe.pick's weight (its own delta); position, scale, shape at c == 0: V[a], copied
    cubic    t = lerp(0, to_t, c) and the six lerps of Barry-Goldman, lerp(a, b, w) = a + (b - a) * w
    rotation the four keys through the oracle's quat_to_basis / basis_to_quat, the three flips,
             log = get_axis * clamped angle, exp, the two expmap halves, tests/blend_recipe.py's slerp
    a NaN the arithmetic produced: 0x7fc00000

sinf, cosf, acosf and sqrtf are the platform glibc's through ctypes, as in tests/blend_recipe.py.
The layered calls, the shape calls and root motion restate their recipes' accumulation
(clip_layers_recipe, clip_shapes_recipe, root_motion_recipe) around this file's value of one channel
at one mapped time; a shape is sampled as the x component of a position channel, which is the same
sequence of operations.  Nothing here calls the code under test.  Comparisons are on uint32 views.
"""
import ctypes as C_

import numpy as np

from . import blend_recipe as R
from . import clip_layers_recipe as LR
from . import clip_recipe as C
from . import root_motion_recipe as RM

F, D = np.float32, np.float64
NEAREST, LINEAR, CUBIC = 0, 1, 2
POSITION, ROTATION, SCALE = C.POSITION, C.ROTATION, C.SCALE
QNAN = C.QNAN
EPS = R.CMP_EPSILON
UNIT_EPSILON = F(0.001)
PI_F = F(3.1415926535897932384626433833)
IDENT = np.array([[0, 0, 0, 1]], np.float32)

bits = R.bits
same_bits = R.same_bits


def libm():
    m = R.libm()
    m.cosf.restype, m.cosf.argtypes = C_.c_float, [C_.c_float]
    return m


def _sinf(x):
    return F(libm().sinf(float(x)))


def _cosf(x):
    return F(libm().cosf(float(x)))


def _acosf(x):
    return F(libm().acosf(float(x)))


def _sqrtf(x):
    return F(libm().sqrtf(float(x)))


# ---------------------------------------------------------------- the scalar cubic
def lerp(a, b, w):
    return a + (b - a) * w


def cubic_keys(n, i, a, wrap):
    """(pre, post) of a pick that is not a copy; a is clip_recipe.pick's."""
    if not wrap:
        return max(i - 1, 0), min(i + 2, n - 1)
    return (a - 1) % n, (a + 2) % n


def spans(T, a, b, pre, post, length):
    """(pre_t, to_t, post_t) float32: the one form of the wrap rules (a pick that does not wrap has
    pre <= a < b <= post)."""
    Ta = T[a]
    pre_t = F((-length + T[pre]) - Ta) if pre > a else F(T[pre] - Ta)
    to_t = F((length + T[b]) - Ta) if b < a else F(T[b] - Ta)
    post_t = F((length + T[post]) - Ta) if (b < a or post <= a) else F(T[post] - Ta)
    return pre_t, to_t, post_t


def cubic_weights(c, pre_t, to_t, post_t):
    zero, half, one = F(0), F(0.5), F(1)
    t = lerp(zero, to_t, c)
    a1 = zero if pre_t == 0 else (t - pre_t) / -pre_t
    a2 = half if to_t == 0 else t / to_t
    a3 = one if post_t - to_t == 0 else (t - to_t) / (post_t - to_t)
    b1 = zero if to_t - pre_t == 0 else (t - pre_t) / (to_t - pre_t)
    b2 = one if post_t == 0 else t / post_t
    for w in (t, a1, a2, a3, b1, b2):
        assert w.dtype == np.float32
    return a1, a2, a3, b1, b2


def cubic(frm, to, pre, post, w):
    """Math::cubic_interpolate_in_time on float32 scalars or arrays (per component)."""
    wa1, wa2, wa3, wb1, wb2 = w
    a1 = lerp(pre, frm, wa1)
    a2 = lerp(frm, to, wa2)
    a3 = lerp(to, post, wa3)
    b1 = lerp(a1, a2, wb1)
    b2 = lerp(a2, a3, wb2)
    r = lerp(b1, b2, wa2)
    assert r.dtype == np.float32
    return r


# ---------------------------------------------------------------- the spherical cubic
def _canon_rotation(po, q):
    """Basis(q).get_rotation_quaternion() by the oracle's exported primitives."""
    L = R._prims(po)
    q = np.ascontiguousarray(q, np.float32)
    b9, out = np.zeros(9, np.float32), np.zeros(4, np.float32)
    L.oracle_quat_to_basis(q.ctypes.data, b9.ctypes.data)
    L.oracle_basis_to_quat(b9.ctypes.data, out.ctypes.data)
    return out


def _dot4(a, b):
    return ((a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]) + a[3] * b[3]


def _length_sq3(v):
    return (v[0] * v[0] + v[1] * v[1]) + v[2] * v[2]


def _qmul(a, b):
    return LR.quat_mul(a[None, :], b[None, :])[0]


def _conj(q):
    return np.array([-q[0], -q[1], -q[2], q[3]], np.float32)


def quat_log(q):
    """Quaternion::log: get_axis() * get_angle(), Math::acos clamping."""
    w = q[3]
    if float(np.abs(w)) > 1 - 0.00001:
        axis = q[0:3].copy()
    else:
        r = F(1) / _sqrtf(F(1) - w * w)
        axis = q[0:3] * r
    ang = F(2) * (PI_F if w < F(-1) else (F(0) if w > F(1) else _acosf(w)))
    out = axis * ang
    assert out.dtype == np.float32
    return out


def quat_exp(v):
    """Quaternion::exp of (v, 0)."""
    ls = _length_sq3(v)
    theta = _sqrtf(ls)
    u = np.zeros(3, np.float32) if ls == 0 else v / _sqrtf(ls)
    lu = _length_sq3(u)
    unit = bool(lu == 1) or bool(np.abs(lu - F(1)) < UNIT_EPSILON)
    if bool(theta < EPS) or not unit:
        return IDENT[0].copy()
    d = _sqrtf(lu)
    if d == 0:
        return np.zeros(4, np.float32)
    half = theta * F(0.5)
    s = _sinf(half) / d
    out = np.array([u[0] * s, u[1] * s, u[2] * s, _cosf(half)], np.float32)
    return out


def _half(base, base_is_from, other, pre, post, w):
    inv = _conj(base)
    zero = np.zeros(3, np.float32)
    lo = quat_log(_qmul(inv, other))
    lf, lt = (zero, lo) if base_is_from else (lo, zero)
    lp, lq = quat_log(_qmul(inv, pre)), quat_log(_qmul(inv, post))
    return _qmul(base, quat_exp(cubic(lf, lt, lp, lq, w)))


def spherical_cubic(po, va, vb, vpre, vpost, c, w):
    frm, pre, to, post = (_canon_rotation(po, q) for q in (va, vpre, vb, vpost))
    if np.signbit(_dot4(frm, pre)):
        pre = -pre
    flip2 = bool(np.signbit(_dot4(frm, to)))
    if flip2:
        to = -to
    dp = _dot4(to, post)
    if (bool(dp <= 0) if flip2 else bool(np.signbit(dp))):
        post = -post
    q1 = _half(frm, True, to, pre, post, w)
    q2 = _half(to, False, frm, pre, post, w)
    return C._canon(R.slerp(q1[None, :], q2[None, :], np.array([c], np.float32)))[0]


# ---------------------------------------------------------------- one channel at one mapped time
def index_tracks(clips, key="tracks"):
    """Per clip: {(bone, channel): (T float64 [n], V float32 [n][3 or 4], interpolation, wrap)}."""
    out = []
    for clip in clips:
        d = {}
        for tr in clip.get(key, []):
            T = np.ascontiguousarray(tr["times"], np.float64).reshape(-1)
            if T.shape[0] == 0:
                continue
            V = np.ascontiguousarray(tr["values"], np.float32).reshape(T.shape[0], -1)
            assert (tr["bone"], tr["channel"]) not in d
            d[tr["bone"], tr["channel"]] = (T, V, int(tr["interpolation"]), clip["loop_mode"] == 1 and bool(tr["loop_wrap"]))
        out.append(d)
    return out


def value_at(po, track, ch, u, length, stats=None):
    """The channel's value (float32 [3] or [4]) at the already mapped time u."""
    T, V, interp, wrap = track
    n = T.shape[0]
    i = int(np.searchsorted(T, u, side="right")) - 1
    a, b, c, how = C.pick(T, n, i, wrap, interp != NEAREST, u, length)
    if stats is not None:
        k = ("nearest", "linear", "cubic")[interp] + ":" + how.split("+")[0]
        stats[k] = stats.get(k, 0) + 1
    if b is None:
        return V[a].copy()
    if interp == LINEAR:
        if ch == ROTATION:
            return C._canon(R.slerp(V[a][None, :], V[b][None, :], np.array([c], np.float32)))[0]
        return C._canon(V[a] + (V[b] - V[a]) * c)
    if ch != ROTATION and c == 0:   # on a key: the key's bits
        return V[a].copy()
    pre, post = cubic_keys(n, i, a, wrap)
    w = cubic_weights(c, *spans(T, a, b, pre, post, length))
    if stats is not None and (pre in (a, b) or post in (a, b)):
        stats["cubic:aliased"] = stats.get("cubic:aliased", 0) + 1
    if ch == ROTATION:
        return spherical_cubic(po, V[a], V[b], V[pre], V[post], c, w)
    return C._canon(cubic(V[a], V[b], V[pre], V[post], w))


def channel_sample(po, track, ch, t, clip, stats=None):
    """mbik_clip_sample's steps 2, 3, 5 and 6 for one tracked channel at the raw time t."""
    if not np.isfinite(t):
        return np.full(4 if ch == ROTATION else 3, QNAN, np.float32)
    length = D(clip["length"])
    return value_at(po, track, ch, C.sample_time(t, length, clip["loop_mode"]), length, stats)


# ---------------------------------------------------------------- the six calls
def expected(po, bone_count, rest, clips, time, clip_index=None, clip=0):
    """(poses [count][bones][10], stats) of the plain call."""
    rest = np.ascontiguousarray(rest, np.float32).reshape(bone_count, 10)
    time = np.ascontiguousarray(time, np.float64).reshape(-1)
    tracks = index_tracks(clips)
    out = np.empty((time.shape[0], bone_count, 10), np.float32)
    stats = {}
    with np.errstate(all="ignore"):
        for s in range(time.shape[0]):
            ci = int(clip if clip_index is None else clip_index[s])
            if not 0 <= ci < len(clips):
                out[s] = QNAN
                continue
            for bone in range(bone_count):
                for ch in (POSITION, ROTATION, SCALE):
                    tr = tracks[ci].get((bone, ch))
                    sl = C.SLICE[ch]
                    out[s, bone, sl] = rest[bone, sl] if tr is None else channel_sample(po, tr, ch, time[s], clips[ci], stats)
    return out, stats


def expected_layers(po, bone_count, rest, clips, layers, flags=0):
    """(poses [count][bones][10], stats): clip_layers_recipe's steps around this file's samples."""
    rest = np.ascontiguousarray(rest, np.float32).reshape(bone_count, 10)
    layers = np.asarray(layers)
    count, K = layers.shape
    invalid, blend, acc, stats = LR.plan(bone_count, clips, layers, flags)
    tracks = index_tracks(clips)
    out = np.empty((count, bone_count, 10), np.float32)
    with np.errstate(all="ignore"):
        for s in range(count):
            if invalid[s]:
                out[s] = QNAN
                continue
            for bone in range(bone_count):
                for ch in (POSITION, ROTATION, SCALE):
                    sl = C.SLICE[ch]
                    I = rest[bone, sl]
                    a, done = I.copy(), False
                    for l in range(K):
                        if not acc[s, l, bone, ch]:
                            continue
                        ci = int(layers["clip"][s, l])
                        x = channel_sample(po, tracks[ci][bone, ch], ch, layers["time"][s, l], clips[ci], stats)
                        b = blend[s, l, bone, ch]
                        if ch == ROTATION:
                            d = _qmul(_conj(I), x)
                            e = R.slerp(IDENT.copy(), d[None, :], np.array([b], np.float32))
                            a = R.normalized(LR.quat_mul(a[None, :], e))[0]
                        else:
                            a = a + (x - I) * b
                        assert a.dtype == np.float32
                        done = True
                    out[s, bone, sl] = C._canon(a) if done else I
    return out, stats


def expected_root(po, bone_count, rest, clips, layers, time_prev, root, flags=0):
    """(motion [count][10], stats): root_motion_recipe's steps around this file's X(u)."""
    layers = np.asarray(layers)
    count, K = layers.shape
    time_prev = np.asarray(time_prev, np.float64).reshape(count, K)
    invalid, blend, acc, _ = LR.plan(bone_count, clips, layers, flags)
    tracks = index_tracks(clips)
    out = np.empty((count, 10), np.float32)
    stats = {"looped": 0, "segments": 0}
    with np.errstate(all="ignore"):
        for s in range(count):
            if invalid[s]:
                out[s] = QNAN
                continue
            for ch in (POSITION, ROTATION, SCALE):
                sl = C.SLICE[ch]
                a, done = RM.START[sl].copy(), False
                for l in range(K):
                    if not acc[s, l, root, ch]:
                        continue
                    ci = int(layers["clip"][s, l])
                    length = D(clips[ci]["length"])
                    track = tracks[ci][root, ch]
                    b = blend[s, l, root, ch]
                    segs = RM.segments(time_prev[s, l], layers["time"][s, l], length, clips[ci]["loop_mode"])
                    if segs is None:
                        nan = np.full(4 if ch == ROTATION else 3, QNAN, np.float32)
                        pairs = [(nan, nan)]
                    else:
                        stats["looped"] += len(segs) == 2
                        pairs = [(value_at(po, track, ch, u0, length, stats), value_at(po, track, ch, u1, length, stats)) for u0, u1 in segs]
                    for x0, x1 in pairs:
                        stats["segments"] += 1
                        if ch == ROTATION:
                            d = _qmul(_conj(x0), x1)
                            e = R.slerp(IDENT.copy(), d[None, :], np.array([b], np.float32))
                            a = R.normalized(LR.quat_mul(a[None, :], e))[0]
                        else:
                            a = a + (x1 - x0) * b
                        assert a.dtype == np.float32
                    done = True
                out[s, sl] = C._canon(a) if done else RM.START[sl]
    return out, stats


def expected_root_plain(po, bone_count, rest, clips, time_prev, time, root, clip_index=None, clip=0):
    t = np.asarray(time, np.float64).reshape(-1)
    ci = np.full(t.shape, clip, np.int32) if clip_index is None else np.asarray(clip_index, np.int32)
    return expected_root(po, bone_count, rest, clips, LR.pack(t[:, None], ci[:, None], np.ones((t.shape[0], 1), np.float32)),
                         np.asarray(time_prev, np.float64).reshape(-1, 1), root, 0)


def shapes_as_pose(shape_count, clips, init=None):
    """(rest [P][10], clips): shape j as the position channel of bone j, its value in x (y = z = 0),
    init[j] the rest position's x -- the same operations on the x component, step for step."""
    P = int(shape_count)
    rest = np.zeros((P, 10), np.float32)
    rest[:, 3] = 1
    if init is not None:
        rest[:, 4] = np.asarray(init, np.float32).reshape(P)
    out = []
    for clip in clips:
        tracks = []
        for tr in clip.get("shape_tracks", []):
            v = np.ascontiguousarray(tr["values"], np.float32).reshape(-1)
            tracks.append(dict(bone=tr["shape"], channel=POSITION, interpolation=tr["interpolation"], loop_wrap=tr["loop_wrap"],
                               times=tr["times"], values=np.stack([v, np.zeros_like(v), np.zeros_like(v)], axis=1)))
        out.append(dict(length=clip["length"], loop_mode=clip["loop_mode"], tracks=tracks))
    return rest, out


def expected_shapes(po, shape_count, clips, time, clip_index=None, clip=0, init=None):
    rest, pc = shapes_as_pose(shape_count, clips, init)
    out, stats = expected(po, int(shape_count), rest, pc, time, clip_index, clip)
    return np.ascontiguousarray(out[:, :, 4]), stats


def expected_shapes_layers(po, shape_count, clips, layers, flags=0, init=None):
    rest, pc = shapes_as_pose(shape_count, clips, init)
    out, stats = expected_layers(po, int(shape_count), rest, pc, layers, flags)
    return np.ascontiguousarray(out[:, :, 4]), stats


# ---------------------------------------------------------------- inputs
def key_times(clip, key="tracks"):
    """Every key time of a clip's tracks, sorted, unique."""
    ts = [np.asarray(tr["times"], np.float64).reshape(-1) for tr in clip.get(key, [])]
    return np.unique(np.concatenate(ts)) if ts else np.zeros(0)


def times_of_interest(rng, clip, key="tracks", limit=40):
    """Exactly on up to `limit` keys and one ulp either side, before the first and after the last
    key, 0 and length, negative times, times past the length, the infinities and NaN."""
    L = clip["length"]
    ts = [0.0, -0.0, L, np.nextafter(L, 0.0), np.nextafter(L, np.inf), -0.3 * L, -L, -2.5 * L, 7.25 * L, 3.0 * L, 1e9, np.nan, np.inf,
          -np.inf]
    kt = key_times(clip, key)
    for x in kt[rng.permutation(kt.shape[0])[:limit]]:
        ts += [x, np.nextafter(x, -np.inf), np.nextafter(x, np.inf), x + L]
    if kt.shape[0]:
        ts += [kt[0] / 2.0, (kt[-1] + L) / 2.0]
    ts += list(rng.uniform(-L, 2.0 * L, 16))
    return np.array(ts, np.float64)
