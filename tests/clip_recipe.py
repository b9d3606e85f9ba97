"""Expected values for the clip-sampling tests (CPU and GPU): Godot 4.3's Animation::_interpolate for
nearest / linear tracks, LOOP_NONE / LOOP_LINEAR, forward playback, as include/mbik.h (ABI 12)
states it, in float64 / float32 numpy scalars, one IEEE operation at a time:

    1. clip index outside the set: every float 0x7fc00000
    2. non-finite time: tracked channels 0x7fc00000, untracked ones the rest pose
    3. t' = clamp(t, 0, length) (LOOP_NONE) or fposmod(t, length) by np.fmod (LOOP_LINEAR)
    4. untracked channel: the rest pose's bits
    5. i = np.searchsorted(T, t', side="right") - 1; the keys a, b and the weight c = from / delta
       (differences and sums in float64, rounded once to float32, a float32 division; 0 when
       |delta| < CMP_EPSILON); V[a], V[a] + (V[b] - V[a]) * c, or tests/blend_recipe.py's slerp
    6. a NaN that 5's arithmetic produced: 0x7fc00000

Nothing here calls the code under test.  Comparisons are on uint32 views: every value, no tolerance.
"""
import numpy as np

from . import blend_recipe as R

F, D = np.float32, np.float64
NAN_BITS = np.uint32(0x7FC00000)
QNAN = NAN_BITS.view(np.float32)
POSITION, ROTATION, SCALE = 0, 1, 2
SLICE = {POSITION: slice(4, 7), ROTATION: slice(0, 4), SCALE: slice(7, 10)}

bits = R.bits
same_bits = R.same_bits


def sample_time(t, length, loop_mode):
    """Step 3: float64 in, float64 out."""
    t, length = D(t), D(length)
    if loop_mode == 0:
        return D(0.0) if t < 0 else (length if t > length else t)
    v = np.fmod(t, length)
    if v < 0:
        v = v + length
    return v + D(0.0)


def pick(T, n, i, wrap, linear, tp, length):
    """Step 5 up to the weight: (a, b or None for a copy of V[a], c float32, which branch)."""
    if n == 1:
        return 0, None, F(0), "single"
    if not wrap and i < 0:
        return 0, None, F(0), "clamp_first"
    if not wrap and i == n - 1:
        return n - 1, None, F(0), "clamp_last"
    if 0 <= i < n - 1:
        a, b, how = i, i + 1, "interior"
        delta = F(T[b] - T[a])
        frm = F(tp - T[a])
    else:
        a, b = n - 1, 0
        end = length - T[a]
        delta = F(end + T[0])
        if i < 0:
            frm, how = F(end + tp), "wrap_before"
        else:
            frm, how = F(tp - T[a]), "wrap_after"
    if not linear:
        return a, None, F(0), how
    if np.abs(delta) < R.CMP_EPSILON:
        return a, b, F(0), how + "+zero_delta"
    c = frm / delta
    assert c.dtype == np.float32
    return a, b, c, how


def _canon(x):
    x = np.array(x, np.float32)
    x.view(np.uint32)[np.isnan(x)] = NAN_BITS
    return x


def index_tracks(clips):
    """Per clip: {(bone, channel): (T float64 [n], V float32 [n][3 or 4], linear, wrap)} of the tracks with keys."""
    out = []
    for clip in clips:
        d = {}
        for tr in clip["tracks"]:
            T = np.ascontiguousarray(tr["times"], np.float64).reshape(-1)
            if T.shape[0] == 0:
                continue
            V = np.ascontiguousarray(tr["values"], np.float32).reshape(T.shape[0], -1)
            assert (tr["bone"], tr["channel"]) not in d
            d[tr["bone"], tr["channel"]] = (T, V, tr["interpolation"] == 1, clip["loop_mode"] == 1 and bool(tr["loop_wrap"]))
        out.append(d)
    return out


def expected(bone_count, rest, clips, time, clip_index=None, clip=0):
    """(poses [count][bones][10], stats): every sample of every skeleton; stats counts the branches
    taken, the slerps and how many of those took the trigonometric branch."""
    rest = np.ascontiguousarray(rest, np.float32).reshape(bone_count, 10)
    time = np.ascontiguousarray(time, np.float64).reshape(-1)
    count = time.shape[0]
    tracks = index_tracks(clips)
    out = np.empty((count, bone_count, 10), np.float32)
    stats = {"finite": 0, "evaluated": 0, "invalid_clip": 0, "nonfinite": 0}
    jobs = []   # (s, bone, qa, qb, c) of the linear rotation samples
    with np.errstate(all="ignore"):
        for s in range(count):
            ci = int(clip if clip_index is None else clip_index[s])
            if not 0 <= ci < len(clips):
                out[s] = QNAN
                stats["invalid_clip"] += 1
                continue
            t = time[s]
            finite = bool(np.isfinite(t))
            length = D(clips[ci]["length"])
            tp = sample_time(t, length, clips[ci]["loop_mode"]) if finite else None
            stats["finite" if finite else "nonfinite"] += bone_count
            for bone in range(bone_count):
                for ch in (POSITION, ROTATION, SCALE):
                    sl = SLICE[ch]
                    tr = tracks[ci].get((bone, ch))
                    if tr is None:
                        out[s, bone, sl] = rest[bone, sl]
                        continue
                    if not finite:
                        out[s, bone, sl] = QNAN
                        continue
                    T, V, linear, wrap = tr
                    n = T.shape[0]
                    i = int(np.searchsorted(T, tp, side="right")) - 1
                    a, b, c, how = pick(T, n, i, wrap, linear, tp, length)
                    stats["evaluated"] += 1
                    for h in how.split("+"):
                        stats[h] = stats.get(h, 0) + 1
                    if b is None:
                        out[s, bone, sl] = V[a]
                    elif ch == ROTATION:
                        jobs.append((s, bone, V[a], V[b], c))
                    else:
                        r = V[a] + (V[b] - V[a]) * c
                        assert r.dtype == np.float32
                        out[s, bone, sl] = _canon(r)
                        stats["lerp"] = stats.get("lerp", 0) + 1
        stats["slerp"] = len(jobs)
        stats["slerp_trig"] = 0
        if jobs:
            qa = np.array([j[2] for j in jobs], np.float32)
            qb = np.array([j[3] for j in jobs], np.float32)
            w = np.array([j[4] for j in jobs], np.float32)
            q = _canon(R.slerp(qa, qb, w))
            cosom = qa[:, 0] * qb[:, 0] + qa[:, 1] * qb[:, 1] + qa[:, 2] * qb[:, 2] + qa[:, 3] * qb[:, 3]
            stats["slerp_trig"] = int(((F(1) - np.abs(cosom)) > R.CMP_EPSILON).sum())
            for (s, bone, _, _, _), r in zip(jobs, q):
                out[s, bone, 0:4] = r
    return out, stats
