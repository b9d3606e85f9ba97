"""Expected values for the blend-shape track tests (CPU and GPU): include/mbik.h's semantics of
mbik_clip_sample_shapes and mbik_clip_sample_shapes_layers -- Godot 4.3's
Animation::blend_shape_track_interpolate and the TYPE_BLEND_SHAPE case of
AnimationMixer::_blend_process -- in float64 / float32 numpy scalars, one IEEE operation at a time,
on top of tests/clip_recipe.py's time mapping, key search and weight (sample_time, pick) and
tests/clip_layers_recipe.py's weight clamp:

    plain    1. clip index outside the set: every weight of the skeleton 0x7fc00000
             2. non-finite time: tracked shapes 0x7fc00000, untracked ones init[j]
             3. t' = clip_recipe.sample_time
             4. untracked shape: init[j]'s bits
             5. i = searchsorted(T, t', "right") - 1; clip_recipe.pick; V[a], or V[a] + (V[b] - V[a]) * c
             6. a NaN that 5's arithmetic produced: 0x7fc00000
    layered  clip == -1 off; another clip outside the set: the skeleton 0x7fc00000; w clamped;
             a layer contributes when its clip has keys for the shape; blend = w or w / total;
             acc = I; acc = acc + (x - I) * blend per contributing layer unless |blend| < CMP_EPSILON;
             acc (NaN as 0x7fc00000) when a layer was accumulated, else init[j]'s bits

Nothing here calls the code under test.  Comparisons are on uint32 views: every value, no tolerance.
"""
import numpy as np

from . import clip_layers_recipe as LR
from . import clip_recipe as C

F, D = np.float32, np.float64
EPS = LR.EPS
OFF = LR.OFF
NORMALIZE = LR.NORMALIZE
LAYER_DTYPE = LR.LAYER_DTYPE
QNAN = C.QNAN

bits = C.bits
same_bits = C.same_bits
pack = LR.pack

PLAIN_BRANCHES = ("untracked", "single", "clamp_first", "clamp_last", "interior_nearest", "interior_linear", "wrap_before",
                  "wrap_after", "nonfinite", "invalid_clip")
LAYER_BRANCHES = ("layers_off", "skipped_by_weight", "zero_totals", "accumulated")


def index_tracks(clips):
    """Per clip: {shape: (T float64 [n], V float32 [n], linear, wrap)} of the shape tracks with keys."""
    out = []
    for clip in clips:
        d = {}
        for tr in clip.get("shape_tracks", []):
            T = np.ascontiguousarray(tr["times"], np.float64).reshape(-1)
            if T.shape[0] == 0:
                continue
            V = np.ascontiguousarray(tr["values"], np.float32).reshape(-1)
            assert V.shape == T.shape and tr["shape"] not in d
            d[tr["shape"]] = (T, V, tr["interpolation"] == 1, clip["loop_mode"] == 1 and bool(tr["loop_wrap"]))
        out.append(d)
    return out


def init_of(shape_count, init):
    return np.zeros(shape_count, np.float32) if init is None else np.ascontiguousarray(init, np.float32).reshape(shape_count)


def _count(stats, key):
    stats[key] = stats.get(key, 0) + 1


def sample_tracked(tr, t, clip, stats):
    """Steps 2, 3, 5 and 6 for one tracked shape: a float32 scalar."""
    T, V, linear, wrap = tr
    if not np.isfinite(t):
        _count(stats, "nonfinite")
        return QNAN
    length = D(clip["length"])
    tp = C.sample_time(t, length, clip["loop_mode"])
    n = T.shape[0]
    i = int(np.searchsorted(T, tp, side="right")) - 1
    a, b, c, how = C.pick(T, n, i, wrap, linear, tp, length)
    for h in how.split("+"):
        _count(stats, h + ("_linear" if linear else "_nearest") if h == "interior" else h)
    if b is None:
        return V[a]
    r = V[a] + (V[b] - V[a]) * c
    assert r.dtype == np.float32
    return QNAN if np.isnan(r) else r


def expected(shape_count, clips, time, clip_index=None, clip=0, init=None):
    """(weights [count][P], stats) of the plain call."""
    P = int(shape_count)
    I = init_of(P, init)
    time = np.ascontiguousarray(time, np.float64).reshape(-1)
    tracks = index_tracks(clips)
    out = np.empty((time.shape[0], P), np.float32)
    stats = {k: 0 for k in PLAIN_BRANCHES}
    with np.errstate(all="ignore"):
        for s in range(time.shape[0]):
            ci = int(clip if clip_index is None else clip_index[s])
            if not 0 <= ci < len(clips):
                out[s] = QNAN
                stats["invalid_clip"] += 1
                continue
            for j in range(P):
                tr = tracks[ci].get(j)
                if tr is None:
                    out[s, j] = I[j]
                    stats["untracked"] += 1
                else:
                    out[s, j] = sample_tracked(tr, time[s], clips[ci], stats)
    return out, stats


def expected_layers(shape_count, clips, layers, flags=0, init=None):
    """(weights [count][P], stats) of the layered call; stats also counts the plain branches of the
    samples that were taken."""
    P = int(shape_count)
    I = init_of(P, init)
    layers = np.asarray(layers)
    count, K = layers.shape
    tracks = index_tracks(clips)
    out = np.empty((count, P), np.float32)
    stats = {k: 0 for k in PLAIN_BRANCHES + LAYER_BRANCHES + ("invalid_skeletons", "untracked_layers")}
    normalize = bool(flags & NORMALIZE)
    with np.errstate(all="ignore"):
        for s in range(count):
            clip = [int(c) for c in layers["clip"][s]]
            if any(c != OFF and not 0 <= c < len(clips) for c in clip):
                out[s] = QNAN
                stats["invalid_skeletons"] += 1
                continue
            w = LR.clamp_weight(layers["weight"][s])
            for j in range(P):
                trs = [None if c == OFF else tracks[c].get(j) for c in clip]
                stats["layers_off"] += sum(c == OFF for c in clip)
                stats["untracked_layers"] += sum(c != OFF and tr is None for c, tr in zip(clip, trs))
                total = F(0)
                for l in range(K):
                    if trs[l] is not None:
                        total = total + w[l]
                acc, done = I[j], False
                if normalize and np.abs(total) < EPS:
                    stats["zero_totals"] += any(tr is not None for tr in trs)
                else:
                    for l in range(K):
                        if trs[l] is None:
                            continue
                        blend = w[l] / total if normalize else w[l]
                        if np.abs(blend) < EPS:
                            stats["skipped_by_weight"] += 1
                            continue
                        x = sample_tracked(trs[l], layers["time"][s, l], clips[clip[l]], stats)
                        acc = acc + (x - I[j]) * blend
                        assert acc.dtype == np.float32
                        done = True
                        stats["accumulated"] += 1
                out[s, j] = (QNAN if np.isnan(acc) else acc) if done else I[j]
    return out, stats


# ---------------------------------------------------------------- inputs
def _as_pose_clips(clips):
    """`clips` with their shape tracks where clip_layers_recipe.random_layers looks for key times."""
    return [dict(length=c["length"], loop_mode=c["loop_mode"], tracks=c.get("shape_tracks", [])) for c in clips]


def random_layers(seed, n, K, clips, specials=True):
    """clip_layers_recipe.random_layers, with a tenth of the times exactly on a shape key."""
    return LR.random_layers(seed, n, K, _as_pose_clips(clips), specials=specials)


def random_times(seed, n, clips, specials=True):
    """(time [n], clip_index [n]): times from one loop before to two loops after the clip, a tenth
    exactly on a shape key; specials: non-finite times and invalid clip indices scattered through."""
    rng = np.random.default_rng(seed)
    ci = rng.integers(0, len(clips), n).astype(np.int32)
    t = rng.uniform(-1.0, 3.0, n) * np.array([c["length"] for c in clips])[ci]
    for s in np.nonzero(rng.uniform(0.0, 1.0, n) < 0.1)[0]:
        tracks = clips[ci[s]].get("shape_tracks", [])
        if tracks:
            T = tracks[rng.integers(0, len(tracks))]["times"]
            t[s] = T[rng.integers(0, len(T))]
    if specials:
        k = rng.uniform(0.0, 1.0, n)
        nf = k < 0.08
        t[nf] = np.array([np.nan, np.inf, -np.inf])[rng.integers(0, 3, int(nf.sum()))]
        bad = (k >= 0.08) & (k < 0.14)
        ci[bad] = np.array([len(clips), LR.INT32_MIN, -1, 2 ** 31 - 1], np.int64)[rng.integers(0, 4, int(bad.sum()))].astype(np.int32)
    return t, ci
