"""Expected values for the layered clip-sampling tests (CPU and GPU): include/mbik.h's semantics of
mbik_clip_sample_layers -- Godot 4.3's AnimationMixer::_blend_process accumulation of each layer's
offset from the rest pose -- in float32 numpy operations, one IEEE operation per element at a time:

    1. clip == -1: the layer is off; another clip outside the set: every float of the skeleton 0x7fc00000
    2. w = weight; w < 0: 0; w > 1: 1 (a NaN passes both)
    3. a layer contributes to a (bone, channel) its clip has keys for
    4. blend = w, or (normalize) w / total with total = 0 + w_l + ... over the contributing layers,
       ascending; |total| < CMP_EPSILON: the channel receives nothing
    5. acc = I (the rest pose's channel); per contributing layer, ascending, unless |blend| < CMP_EPSILON:
       x = tests/clip_recipe.py's sample of (time_l, clip_l);
       position, scale: acc = acc + (x - I) * blend
       rotation: d = inverse(I) * x; e = slerp(identity, d, blend) (tests/blend_recipe.py);
                 acc = normalized(acc * e) (tests/blend_recipe.py)
    6. a channel with a layer accumulated: acc, NaN as 0x7fc00000; every other channel: the rest pose's bits

Nothing here calls the code under test.  Comparisons are on uint32 views: every value, no tolerance.
`model64` is the independent float64 meaning of steps 4 and 5 for the geometry tests.
"""
import numpy as np

from . import blend_recipe as R
from . import clip_recipe as C

F, D = np.float32, np.float64
EPS = R.CMP_EPSILON
OFF = -1
NORMALIZE = 1
LAYER_DTYPE = np.dtype([("time", "<f8"), ("clip", "<i4"), ("weight", "<f4")])
CHANNELS = (C.POSITION, C.ROTATION, C.SCALE)

bits = R.bits
same_bits = R.same_bits


def quat_mul(a, b):
    """Quaternion::operator* in gd_math.h's written order, rows of [N][4] float32 (x, y, z, w)."""
    ax, ay, az, aw = a[:, 0], a[:, 1], a[:, 2], a[:, 3]
    bx, by, bz, bw = b[:, 0], b[:, 1], b[:, 2], b[:, 3]
    x = aw * bx + ax * bw + ay * bz - az * by
    y = aw * by + ay * bw + az * bx - ax * bz
    z = aw * bz + az * bw + ax * by - ay * bx
    w = aw * bw - ax * bx - ay * by - az * bz
    out = np.stack([x, y, z, w], axis=1)
    assert out.dtype == np.float32
    return out


def inverse(q):
    return np.stack([-q[:, 0], -q[:, 1], -q[:, 2], q[:, 3]], axis=1)


def clamp_weight(w):
    """Step 2 on a float32 array."""
    w = np.array(w, np.float32)
    w = np.where(w < F(0), F(0), w)
    w = np.where(w > F(1), F(1), w)
    return w.astype(np.float32)


def tracked_table(bone_count, clips):
    """[clip][bone][channel] bool: the channel has at least one key."""
    t = np.zeros((len(clips), bone_count, 3), bool)
    for c, d in enumerate(C.index_tracks(clips)):
        for (bone, ch) in d:
            t[c, bone, ch] = True
    return t


def plan(bone_count, clips, layers, flags):
    """Steps 1 to 4 and 5's skip: per (skeleton, layer, bone, channel) the blend factor and whether
    the layer is accumulated, with the branch statistics."""
    layers = np.asarray(layers)
    count, K = layers.shape
    clip = layers["clip"].astype(np.int64)
    on = clip != OFF
    invalid = (on & ((clip < 0) | (clip >= len(clips)))).any(axis=1)
    live = on & ~invalid[:, None]
    w = clamp_weight(layers["weight"])
    tracked = tracked_table(bone_count, clips)
    contrib = np.zeros((count, K, bone_count, 3), bool)
    for s in range(count):
        for l in range(K):
            if live[s, l]:
                contrib[s, l] = tracked[clip[s, l]]
    wb = np.broadcast_to(w[:, :, None, None], contrib.shape)
    zero_total = np.zeros((count, bone_count, 3), bool)
    with np.errstate(all="ignore"):
        if flags & NORMALIZE:
            total = np.zeros((count, bone_count, 3), np.float32)
            for l in range(K):
                total = np.where(contrib[:, l], total + wb[:, l], total)
            assert total.dtype == np.float32
            zero_total = np.abs(total) < EPS
            blend = wb / total[:, None]
            assert blend.dtype == np.float32
        else:
            blend = np.array(wb, np.float32)
        small = np.abs(blend) < EPS
    has_layer = contrib.any(axis=1)
    acc = contrib & ~zero_total[:, None] & ~small
    valid = ~invalid
    stats = {
        "invalid_skeletons": int(invalid.sum()),
        "layers_off": int((~on & valid[:, None]).sum()),
        "untracked": int((live[:, :, None, None] & ~contrib).sum()),
        "zero_totals": int((zero_total & has_layer).sum()) if flags & NORMALIZE else 0,
        "skipped_by_weight": int((contrib & ~zero_total[:, None] & small).sum()),
        "accumulated": int(acc.sum()),
    }
    return invalid, blend, acc, stats


def samples(bone_count, rest, clips, layers, acc):
    """x [count][K][bones][10] float32: clip_recipe's sample of every layer some channel accumulates
    (the rest pose elsewhere, which nothing reads)."""
    layers = np.asarray(layers)
    count, K = layers.shape
    x = np.empty((count, K, bone_count, 10), np.float32)
    x[:] = np.asarray(rest, np.float32).reshape(bone_count, 10)
    for l in range(K):
        need = np.nonzero(acc[:, l].any(axis=(1, 2)))[0]
        if need.size:
            x[need, l], _ = C.expected(bone_count, rest, clips, layers["time"][need, l], layers["clip"][need, l])
    return x


def expected(bone_count, rest, clips, layers, flags=0):
    """(poses [count][bones][10], stats) of the layer records `layers` [count][K] (LAYER_DTYPE)."""
    rest = np.ascontiguousarray(rest, np.float32).reshape(bone_count, 10)
    layers = np.asarray(layers)
    count, K = layers.shape
    invalid, blend, acc, stats = plan(bone_count, clips, layers, flags)
    x = samples(bone_count, rest, clips, layers, acc)
    out = np.empty((count, bone_count, 10), np.float32)
    out[:] = rest
    stats["slerp"] = stats["slerp_trig"] = 0
    with np.errstate(all="ignore"):
        for ch in (C.POSITION, C.SCALE):
            sl = C.SLICE[ch]
            I = np.broadcast_to(rest[None, :, sl], (count, bone_count, 3))
            a = np.array(I, np.float32)
            for l in range(K):
                m = acc[:, l, :, ch]
                new = a + (x[:, l, :, sl] - I) * blend[:, l, :, ch, None]
                assert new.dtype == np.float32
                a = np.where(m[:, :, None], new, a)
            done = acc[:, :, :, ch].any(axis=1)
            out[:, :, sl][done] = C._canon(a[done])
        I = np.ascontiguousarray(np.broadcast_to(rest[None, :, 0:4], (count, bone_count, 4)))
        a = I.copy()
        ident = np.array([0, 0, 0, 1], np.float32)
        for l in range(K):
            m = acc[:, l, :, C.ROTATION]
            if not m.any():
                continue
            d = quat_mul(inverse(I[m]), x[:, l, :, 0:4][m])
            b = np.ascontiguousarray(blend[:, l, :, C.ROTATION][m])
            e = R.slerp(np.tile(ident, (d.shape[0], 1)), d, b)
            a[m] = R.normalized(quat_mul(a[m], e))
            stats["slerp"] += int(m.sum())
            stats["slerp_trig"] += int(((F(1) - np.abs(d[:, 3] * F(1))) > EPS).sum())
        done = acc[:, :, :, C.ROTATION].any(axis=1)
        out[:, :, 0:4][done] = C._canon(a[done])
    out[invalid] = C.QNAN
    assert out.dtype == np.float32
    return out, stats


def model64(bone_count, rest, clips, layers, flags=0):
    """The float64 meaning of steps 4 and 5, fed the float32 layer samples and the float32 blend
    factors: positions and scales by one weighted sum, rotations by exact unit-quaternion algebra
    (d = I^-1 x, e = the rotation a fraction `blend` of the way from identity to d along the
    shorter arc, acc = normalize(acc e)).  Returns (pose64 [count][bones][10], S [count][bones][10],
    blend, acc, x): S is the magnitude sum |I| + sum |blend| (|x| + |I|) of the position / scale
    floats (0 for the rotation floats)."""
    rest = np.ascontiguousarray(rest, np.float32).reshape(bone_count, 10)
    layers = np.asarray(layers)
    count, K = layers.shape
    invalid, blend, acc, _ = plan(bone_count, clips, layers, flags)
    x = samples(bone_count, rest, clips, layers, acc)
    r64, x64, b64 = rest.astype(D), x.astype(D), blend.astype(D)
    out = np.empty((count, bone_count, 10), D)
    out[:] = r64
    S = np.zeros((count, bone_count, 10), D)
    with np.errstate(all="ignore"):
        for ch in (C.POSITION, C.SCALE):
            sl = C.SLICE[ch]
            I = r64[None, :, sl]
            S[:, :, sl] = np.abs(I)
            for l in range(K):
                m = acc[:, l, :, ch][:, :, None]
                bl = b64[:, l, :, ch, None]
                out[:, :, sl] += np.where(m, (x64[:, l, :, sl] - I) * bl, 0.0)
                S[:, :, sl] += np.where(m, np.abs(bl) * (np.abs(x64[:, l, :, sl]) + np.abs(I)), 0.0)
        I = np.broadcast_to(r64[None, :, 0:4], (count, bone_count, 4))
        a = np.array(I)
        for l in range(K):
            m = acc[:, l, :, C.ROTATION]
            if not m.any():
                continue
            d = _qmul64(_qinv64(I[m]), x64[:, l, :, 0:4][m])
            e = _slerp64(d, b64[:, l, :, C.ROTATION][m])
            q = _qmul64(a[m], e)
            a[m] = q / np.linalg.norm(q, axis=1, keepdims=True)
        out[:, :, 0:4] = a
    return out, S, blend, acc, x


# ---------------------------------------------------------------- inputs
INT32_MIN = -2 ** 31
SPECIAL_WEIGHTS = np.array([-0.0, -1.0, 1e-6, 1.0, 2.0, np.nan, np.inf], np.float32)


def pack(time, clip, weight):
    t = np.asarray(time, np.float64)
    out = np.empty(t.shape, LAYER_DTYPE)
    out["time"], out["clip"], out["weight"] = t, np.asarray(clip, np.int32), np.asarray(weight, np.float32)
    return out


def random_layers(seed, n, K, clips, specials=True):
    """[n][K] layer records for a crowd in every state at once: a fifth of the layers off, a fifth
    weighted exactly 0 and a tenth below CMP_EPSILON, times from one loop before to two loops after
    the clip with a tenth exactly on a key.  specials: skeletons with an invalid clip index among
    valid ones, off layers with a NaN time and a NaN weight, the special weights and non-finite
    times scattered through the batch."""
    rng = np.random.default_rng(seed)
    ci = rng.integers(0, len(clips), (n, K)).astype(np.int32)
    L = np.array([c["length"] for c in clips])[ci]
    t = rng.uniform(-1.0, 3.0, (n, K)) * L
    for s, l in np.argwhere(rng.uniform(0.0, 1.0, (n, K)) < 0.1):
        tracks = clips[ci[s, l]]["tracks"]
        if tracks:
            T = tracks[rng.integers(0, len(tracks))]["times"]
            t[s, l] = T[rng.integers(0, len(T))]
    w = rng.uniform(0.0, 1.0, (n, K)).astype(np.float32)
    u = rng.uniform(0.0, 1.0, (n, K))
    w[u < 0.2] = 0.0
    w[(u >= 0.2) & (u < 0.3)] = rng.uniform(0.0, 9e-6, int(((u >= 0.2) & (u < 0.3)).sum())).astype(np.float32)
    ci[rng.uniform(0.0, 1.0, (n, K)) < 0.2] = OFF
    if specials:
        k = rng.uniform(0.0, 1.0, (n, K))
        sp = k < 0.06
        w[sp] = SPECIAL_WEIGHTS[rng.integers(0, len(SPECIAL_WEIGHTS), int(sp.sum()))]
        nf = (k >= 0.06) & (k < 0.08)
        t[nf] = np.array([np.nan, np.inf, -np.inf])[rng.integers(0, 3, int(nf.sum()))]
        off = ci == OFF
        poison = off & (rng.uniform(0.0, 1.0, (n, K)) < 0.5)
        t[poison], w[poison] = np.nan, np.nan
        bad = rng.uniform(0.0, 1.0, n) < 0.04
        for s in np.nonzero(bad)[0]:
            ci[s, rng.integers(0, K)] = np.array([len(clips), INT32_MIN, -2, 2 ** 31 - 1], np.int64)[rng.integers(0, 4)].astype(np.int32)
    return pack(t, ci, w)


def _qmul64(a, b):
    v = a[:, 3:4] * b[:, 0:3] + b[:, 3:4] * a[:, 0:3] + np.cross(a[:, 0:3], b[:, 0:3])
    w = a[:, 3] * b[:, 3] - np.sum(a[:, 0:3] * b[:, 0:3], axis=1)
    return np.concatenate([v, w[:, None]], axis=1)


def _qinv64(q):
    return q * np.array([-1.0, -1.0, -1.0, 1.0])


def _slerp64(d, t):
    """From identity towards d by the fraction t along the shorter arc, not renormalised (float64)."""
    d = np.where((d[:, 3] < 0)[:, None], -d, d)
    c = np.clip(d[:, 3], -1.0, 1.0)
    om = np.arccos(c)
    so = np.sin(om)
    lin = so < 1e-9
    so_ = np.where(lin, 1.0, so)
    s0 = np.where(lin, 1.0 - t, np.sin((1.0 - t) * om) / so_)
    s1 = np.where(lin, t, np.sin(t * om) / so_)
    ident = np.array([0.0, 0.0, 0.0, 1.0])
    return s0[:, None] * ident + s1[:, None] * d


def angle_between(q, p):
    """The rotation angle (radians) between rows of unit-ish quaternions, float64."""
    q = np.asarray(q, D)
    p = np.asarray(p, D)
    q = q / np.linalg.norm(q, axis=-1, keepdims=True)
    p = p / np.linalg.norm(p, axis=-1, keepdims=True)
    dq = q - p * np.sign(np.sum(q * p, axis=-1, keepdims=True))
    # 2 asin(|dq| / 2) is the half-angle; accurate for tiny angles where acos(dot) is not
    return 4.0 * np.arcsin(np.minimum(1.0, np.linalg.norm(dq, axis=-1) / 2.0))
