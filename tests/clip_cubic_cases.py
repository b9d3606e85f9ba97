"""Seeded inputs of the cubic-interpolation tests (CPU and GPU): clip sets whose tracks mix nearest,
linear and cubic interpolation with 0, 1, 2, 3, 4 and 17 keys, a walking root, key quaternions that
are not unit and some with |w| > 1, shape tracks of the same mix, and the mbik_clip_call_cpu calls
of the six kinds on them."""
import numpy as np

from many_bone_ik_amd import animation as A

from . import clip_cubic_recipe as Q
from . import clip_shapes_recipe as SR
from . import root_motion_recipe as RM

KEY_COUNTS = (0, 1, 2, 3, 4, 17)
KINDS = (A.NEAREST, A.LINEAR, A.CUBIC, A.CUBIC)   # half the tracks cubic
ROOT = 1


def cubic_set(seed, bone_count, shape_count=0, kinds=KINDS, root=ROOT):
    """(rest, clips): synthetic_walk_clips' set with `kinds` drawn per track; a fifth of the rotation
    tracks get keys scaled off the unit sphere by 0.5 .. 1.5 each, and a tenth a key with |w| > 1.
    With shape_count, shape tracks of the same mix."""
    root = min(root, bone_count - 1)
    rest, clips = A.synthetic_walk_clips(seed, bone_count, root, key_counts=KEY_COUNTS, walk_keys=(2, 3, 4, 9), interpolations=kinds)
    rng = np.random.default_rng(seed + 9)
    for clip in clips:
        for tr in clip["tracks"]:
            if tr["channel"] != A.ROTATION:
                continue
            u = rng.uniform()
            v = np.array(tr["values"], np.float32)
            if u < 0.2:
                v = (v * rng.uniform(0.5, 1.5, (v.shape[0], 1))).astype(np.float32)
            elif u < 0.3:
                k = int(np.argmax(np.abs(v[:, 3])))
                v[k] = (v[k] * (1.25 / max(abs(float(v[k, 3])), 0.1))).astype(np.float32)
                assert abs(v[k, 3]) > 1
            tr["values"] = v
    if shape_count:
        clips = A.synthetic_shape_tracks(seed + 5, shape_count, clips, key_counts=KEY_COUNTS, interpolations=kinds)
    return rest, clips


def plain_batch(seed, clips, key="tracks", limit=40):
    """(time [n], clip_index [n]): every clip at its times of interest, then invalid clip indices."""
    rng = np.random.default_rng(seed)
    t, ci = [], []
    for c, clip in enumerate(clips):
        x = Q.times_of_interest(rng, clip, key, limit)
        t.append(x)
        ci.append(np.full(x.shape[0], c, np.int32))
    t.append(np.array([0.5, 0.5], np.float64))
    ci.append(np.array([-1, len(clips)], np.int32))
    return np.concatenate(t), np.concatenate(ci)


def root_times(seed, clips, n):
    """(time_prev [n], time [n], clip_index [n]) of the plain root-motion call: frames a fraction of a
    clip behind, so that looping clips cross the seam, with frames on 0 and on the length."""
    layers, t0 = RM.random_frames(seed, n, 1, clips, specials=True)
    ci = layers["clip"][:, 0].copy()
    ci[ci == -1] = 0
    return np.ascontiguousarray(np.where(np.isnan(t0[:, 0]) & (layers["clip"][:, 0] == -1), 0.0, t0[:, 0])), \
        np.ascontiguousarray(np.where(np.isnan(layers["time"][:, 0]) & (layers["clip"][:, 0] == -1), 0.25, layers["time"][:, 0])), ci


def shape_layers(seed, n, K, clips):
    return SR.random_layers(seed, n, K, clips)
