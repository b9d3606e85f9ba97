"""mbik_clip_sample_cpu (Godot's Animation track interpolation for a batch of skeletons, host only)
against the recipe of tests/clip_recipe.py, bitwise: seeded clip sets of 1, 7 and 33 bones with
tracks of 0, 1, 2, 3 and 17 keys, both interpolations, both loop modes, loop_wrap on and off and
untracked channels, at times on, one ulp around, before and after the keys, 0, -0, length, negative
times, many loops ahead, NaN and the infinities; both wrap branches, a wrap pair closer than
CMP_EPSILON, invalid clip indices, both libm variants and every argument check."""
import ctypes as C

import numpy as np
import pytest

from many_bone_ik_amd import _lib
from many_bone_ik_amd import animation as A

from . import clip_recipe as R

BONE_COUNTS = (1, 7, 33)
INT32_MIN = -2 ** 31


def times_for(rng, clip, tracks_limit):
    """The times of interest of one clip: every key of up to `tracks_limit` of its tracks exactly and
    one ulp either side, half way to the first key and past the last one, and the specials."""
    L = clip["length"]
    ts = [0.0, -0.0, L, np.nextafter(L, 0.0), np.nextafter(L, np.inf), 5e-324, -5e-324, -0.3 * L, -L, -2.5 * L, -1e-300,
          7.25 * L, 3.0 * L, 1e9, -1e9, np.nan, np.inf, -np.inf]
    tracks = clip["tracks"]
    for k in rng.permutation(len(tracks))[:tracks_limit]:
        T = np.asarray(tracks[k]["times"], np.float64)
        for x in T:
            ts += [x, np.nextafter(x, -np.inf), np.nextafter(x, np.inf), x + L, x - 2.0 * L]
        ts += [T[0] / 2.0, (T[-1] + L) / 2.0]
    ts += list(rng.uniform(-L, 2.0 * L, 24))
    return np.array(ts, np.float64)


def batch_for(seed, B):
    """(rest, clips, time [n], clip_index [n]): every clip at its times of interest, then one skeleton
    per invalid clip index."""
    rest, clips = A.synthetic_clips(seed, B)
    rng = np.random.default_rng(seed + 1000)
    t, ci = [], []
    for c, clip in enumerate(clips):
        x = times_for(rng, clip, 8 if B > 7 else 1000)
        t.append(x)
        ci.append(np.full(x.shape[0], c, np.int32))
    t.append(np.array([0.5, 0.5, 0.5], np.float64))
    ci.append(np.array([-1, len(clips), INT32_MIN], np.int32))
    return rest, clips, np.concatenate(t), np.concatenate(ci)


@pytest.fixture(scope="module")
def cases(mbik):
    """Per bone count: (rest, clips, time, clip_index, expected, stats), computed once."""
    out = {}
    for B in BONE_COUNTS:
        rest, clips, t, ci = batch_for(40 + B, B)
        want, stats = R.expected(B, rest, clips, t, ci)
        for arr in (rest, t, ci, want):
            arr.setflags(write=False)
        out[B] = (rest, clips, t, ci, want, stats)
    return out


def assert_same(got, want, t, ci, what=""):
    bad = np.nonzero((R.bits(got) != R.bits(want)).any(axis=2))
    assert bad[0].size == 0, (f"{what}: {bad[0].size} bones differ; first: skeleton {bad[0][0]} bone {bad[1][0]} "
                              f"(t = {t[bad[0][0]]!r}, clip {ci[bad[0][0]]}): got {got[bad[0][0], bad[1][0]]}, "
                              f"want {want[bad[0][0], bad[1][0]]}")


@pytest.mark.parametrize("B", BONE_COUNTS)
def test_matches_recipe(cases, B):
    rest, clips, t, ci, want, stats = cases[B]
    got = A.clip_sample_cpu(B, rest, clips, t, ci)
    assert_same(got, want, t, ci, f"{B} bones")
    for c in range(len(clips)):   # the scalar `clip` instead of the index array
        sel = ci == c
        assert R.same_bits(A.clip_sample_cpu(B, rest, clips, t[sel], clip=c), want[sel])


def test_samples_reach_every_path(cases):
    """The recipe skipped no finite-time sample, the seeded sets hold what they are meant to hold and
    the times take every branch; at least 90 % of the slerps take the trigonometric branch."""
    total = {}
    samples = 0
    for B in BONE_COUNTS:
        rest, clips, t, ci, want, stats = cases[B]
        valid = (ci >= 0) & (ci < len(clips))
        assert stats["finite"] == int((np.isfinite(t) & valid).sum()) * B
        assert stats["nonfinite"] == 3 * len(clips) * B and stats["invalid_clip"] == 3
        tracked = sum(len(d) for d in R.index_tracks(clips))
        per_clip = [sum(1 for _ in d) for d in R.index_tracks(clips)]
        finite_per_clip = [int((np.isfinite(t) & (ci == c)).sum()) for c in range(len(clips))]
        assert stats["evaluated"] == sum(a * b for a, b in zip(per_clip, finite_per_clip)) and tracked > 0
        samples += stats["finite"]
        for k, v in stats.items():
            total[k] = total.get(k, 0) + v
    assert samples >= 3000
    for branch in ("single", "clamp_first", "clamp_last", "interior", "wrap_before", "wrap_after", "lerp", "slerp"):
        assert total.get(branch, 0) >= 50, (branch, total)
    assert total["slerp_trig"] >= 0.9 * total["slerp"], total
    # what the generator drew, over the 7- and 33-bone sets
    seen = set()
    for B in (7, 33):
        rest, clips, *_ = cases[B]
        tracked = set()
        for c, clip in enumerate(clips):
            for tr in clip["tracks"]:
                n = len(tr["times"])
                seen.add((n, tr["interpolation"], clip["loop_mode"], tr["loop_wrap"]))
                tracked.add((c, tr["bone"], tr["channel"]))
                if n > 1:
                    seen.add(("inside", tr["times"][0] > 0 and tr["times"][-1] < clip["length"]))
        assert len(tracked) < len(clips) * B * 3   # untracked channels
    for n in (1, 2, 3, 17):
        for interpolation in (0, 1):
            assert any(k[0] == n and k[1] == interpolation for k in seen if len(k) == 4), (n, interpolation)
    for loop_mode in (0, 1):
        for wrap in (0, 1):
            assert any(k[2] == loop_mode and k[3] == wrap for k in seen if len(k) == 4)
    assert ("inside", True) in seen and ("inside", False) in seen


def test_invalid_clip_and_non_finite_time(cases):
    rest, clips, t, ci, want, stats = cases[7]
    got = A.clip_sample_cpu(7, rest, clips, t, ci)
    bad = (ci < 0) | (ci >= len(clips))
    assert bad.sum() == 3 and (R.bits(got[bad]) == R.NAN_BITS).all()
    tracks = R.index_tracks(clips)
    for s in np.nonzero(~np.isfinite(t))[0]:
        for bone in range(7):
            for ch in (0, 1, 2):
                sl = R.SLICE[ch]
                if (bone, ch) in tracks[ci[s]]:
                    assert (R.bits(got[s, bone, sl]) == R.NAN_BITS).all()
                else:
                    assert R.same_bits(got[s, bone, sl], rest[bone, sl])


def _wrap_clips():
    """Two bones, LOOP_LINEAR, loop_wrap on: bone 0's keys lie strictly inside (0, length), so times
    before the first and after the last key interpolate across the loop; bone 1's last and first
    keys are 3e-6 s apart across the loop, below CMP_EPSILON."""
    rng = np.random.default_rng(5)
    L = 2.0
    tracks = []
    for bone, T in ((0, np.array([0.25, 0.75, 1.5])), (1, np.array([1e-6, 1.0, L - 2e-6]))):
        for ch in (0, 1, 2):
            V = A._key_rotations(rng, 3) if ch == 1 else rng.uniform(0.5, 1.5, (3, 3))
            tracks.append(dict(bone=bone, channel=ch, interpolation=1, loop_wrap=1, times=T, values=V.astype(np.float32)))
    rest = np.tile(np.array([0, 0, 0, 1, 0, 0, 0, 1, 1, 1], np.float32), (2, 1))
    return rest, [dict(length=L, loop_mode=1, tracks=tracks)]


def test_both_wrap_branches_and_a_zero_delta_pair(mbik):
    rest, clips = _wrap_clips()
    L = clips[0]["length"]
    t = np.array([0.0, 0.1, 0.2499, 0.25, 1.5, 1.6, 1.99, L, 2.1, -0.1, 5e-7, 1e-6, L - 2e-6, L - 1e-6, np.nextafter(L, 0.0),
                  4.0 + 5e-7, -1e-6], np.float64)
    want, stats = R.expected(2, rest, clips, t)
    assert stats["wrap_before"] >= 8 and stats["wrap_after"] >= 8 and stats["zero_delta"] >= 15
    got = A.clip_sample_cpu(2, rest, clips, t)
    assert_same(got, want, t, np.zeros(t.shape[0], np.int32))
    # c = 0 across the tiny pair: bone 1 holds its last key from there to its first key
    last = {ch: np.asarray(tr["values"])[-1] for tr in clips[0]["tracks"] if tr["bone"] == 1 for ch in [tr["channel"]]}
    for s in (10, 13, 14):   # 5e-7, L - 1e-6, just below L
        assert np.array_equal(got[s, 1, 4:7], last[0]) and np.array_equal(got[s, 1, 7:10], last[2])
        assert np.allclose(got[s, 1, 0:4], last[1], atol=1e-6)
    # and bone 0 really interpolates across the loop: between its last and first key values
    p = {ch: np.asarray(tr["values"]) for tr in clips[0]["tracks"] if tr["bone"] == 0 for ch in [tr["channel"]]}
    for s in (0, 1, 5, 6):
        lo, hi = np.minimum(p[0][-1], p[0][0]), np.maximum(p[0][-1], p[0][0])
        assert ((got[s, 0, 4:7] >= lo) & (got[s, 0, 4:7] <= hi)).all() and not np.array_equal(got[s, 0, 4:7], p[0][0])


def test_fposmod_is_exact(mbik):
    """One nearest track with a key every 1/64 s of an awkward length: the key a far-away time lands
    on is the one np.fmod says, for times up to 1e15 and of both signs."""
    L = 2.7182818284590452
    T = np.arange(0, 170, dtype=np.float64) / 64.0
    V = np.stack([np.arange(170), np.zeros(170), np.zeros(170)], axis=1).astype(np.float32)
    clips = [dict(length=L, loop_mode=1, tracks=[dict(bone=0, channel=0, interpolation=0, loop_wrap=1, times=T, values=V)])]
    rest = np.zeros((1, 10), np.float32)
    rng = np.random.default_rng(9)
    t = np.concatenate([rng.uniform(-1e3, 1e3, 300), rng.uniform(-1e9, 1e9, 300), rng.uniform(-1e15, 1e15, 300),
                        np.array([1e300, -1e300, 1.7976931348623157e308, L * 3, -L * 3, np.nextafter(L, 0) * 5])])
    want, _ = R.expected(1, rest, clips, t)
    got = A.clip_sample_cpu(1, rest, clips, t)
    assert_same(got, want, t, np.zeros(t.shape[0], np.int32))
    assert len(set(got[:, 0, 4].tolist())) > 150


def test_libm_variants_agree_off_their_few_inputs(cases):
    rest, clips, t, ci, want, stats = cases[7]
    assert_same(A.clip_sample_cpu(7, rest, clips, t, ci, libm_variant=1), want, t, ci, "variant 1")


def test_empty_tracks_and_empty_calls(cases):
    rest, clips, t, ci, want, stats = cases[7]
    # tracks without keys are no tracks: any number of them, next to a track with keys
    extra = [dict(c, tracks=c["tracks"] + [dict(bone=b, channel=ch, interpolation=1, loop_wrap=1, times=np.zeros(0), values=np.zeros((0, 3)))
                                           for b in (0, 0, 6) for ch in (0, 1, 2)]) for c in clips]
    assert R.same_bits(A.clip_sample_cpu(7, rest, extra, t[:50], ci[:50]), want[:50])
    assert A.clip_sample_cpu(7, rest, clips, np.zeros(0), np.zeros(0, np.int32)).shape == (0, 7, 10)
    assert A.clip_sample_cpu(0, np.zeros((0, 10), np.float32), [dict(length=1.0, loop_mode=0, tracks=[])], t[:5]).shape == (5, 0, 10)
    # a clip without tracks: the rest pose everywhere, NaN times included
    got = A.clip_sample_cpu(7, rest, [dict(length=1.0, loop_mode=1, tracks=[])], t[:40])
    assert R.same_bits(got, np.broadcast_to(rest, (40, 7, 10)))


# ---------------------------------------------------------------- argument checks
def _track(**k):
    d = dict(bone=0, channel=0, interpolation=1, loop_wrap=1, times=np.array([0.0, 0.5, 1.0]),
             values=np.arange(9, dtype=np.float32).reshape(3, 3))
    d.update(k)
    return d


def _clip(*tracks, **k):
    d = dict(length=1.0, loop_mode=0, tracks=list(tracks) or [_track()])
    d.update(k)
    return d


BAD_SETS = {
    "negative_bone_count": dict(B=-1),
    "no_clips": dict(clips=[]),
    "negative_clip_count": dict(clip_count=-1),
    "libm_variant": dict(lv=2),
    "channel_3": dict(clips=[_clip(_track(channel=3))]),
    "channel_negative": dict(clips=[_clip(_track(channel=-1))]),
    "interpolation_2": dict(clips=[_clip(_track(interpolation=2))]),
    "interpolation_on_an_empty_track": dict(clips=[_clip(_track(interpolation=5, times=np.zeros(0), values=np.zeros((0, 3))))]),
    "loop_mode_2": dict(clips=[_clip(loop_mode=2)]),
    "loop_mode_negative": dict(clips=[_clip(loop_mode=-1)]),
    "bone_too_large": dict(clips=[_clip(_track(bone=2))]),
    "bone_negative": dict(clips=[_clip(_track(bone=-1))]),
    "duplicate_track": dict(clips=[_clip(_track(), _track(interpolation=0))]),
    "duplicate_track_in_second_clip": dict(clips=[_clip(), _clip(_track(bone=1, channel=1, values=np.ones((3, 4), np.float32)),
                                                                 _track(bone=1, channel=1, values=np.ones((3, 4), np.float32)))]),
    "length_zero": dict(clips=[_clip(length=0.0)]),
    "length_negative": dict(clips=[_clip(length=-1.0)]),
    "length_nan": dict(clips=[_clip(length=float("nan"))]),
    "length_inf": dict(clips=[_clip(length=float("inf"))]),
    "times_equal": dict(clips=[_clip(_track(times=np.array([0.0, 0.5, 0.5])))]),
    "times_decreasing": dict(clips=[_clip(_track(times=np.array([0.0, 0.6, 0.5])))]),
    "time_nan": dict(clips=[_clip(_track(times=np.array([0.0, np.nan, 1.0])))]),
    "time_inf": dict(clips=[_clip(_track(times=np.array([0.0, 0.5, np.inf])))]),
    "time_negative": dict(clips=[_clip(_track(times=np.array([-0.1, 0.5, 1.0])))]),
    "time_past_length": dict(clips=[_clip(_track(times=np.array([0.0, 0.5, np.nextafter(1.0, 2.0)])))]),
    "null_times": dict(clips=[_clip(_track(times=None, key_count=3))]),
    "null_values": dict(clips=[_clip(_track(values=None, key_count=3))]),
    "negative_key_count": dict(clips=[_clip(_track(key_count=-1))]),
    "negative_track_count": dict(clips=[_clip(track_count=-1)]),
    "null_tracks": dict(clips=[dict(length=1.0, loop_mode=0, tracks=[], track_count=2)]),
}


def _raw_args(B=2, clips=None, clip_count=None, lv=0, rest=True):
    clips = [_clip()] if clips is None else clips
    descs, keep = A._descs(clips)
    rest_arr = np.zeros((max(B, 0), 10), np.float32)
    return (B, rest_arr.ctypes.data if rest else None, len(clips) if clip_count is None else clip_count, descs, lv), (keep, rest_arr)


@pytest.mark.parametrize("name", sorted(BAD_SETS))
def test_invalid_sets_are_rejected(mbik, name):
    """Every MBIK_EINVAL case of mbik_clipset_create, through create itself (the checks come before
    any device is looked for) and through the CPU entry, which shares them."""
    args, keep = _raw_args(**BAD_SETS[name])
    t, out, h = np.zeros(1, np.float64), np.zeros((1, 2, 10), np.float32), C.c_void_p()
    assert mbik.mbik_clipset_create(*args, 0, C.byref(h)) == _lib.MBIK_EINVAL and not h.value
    assert _lib.last_error()
    first = _lib.last_error()
    assert mbik.mbik_clip_sample_cpu(*args, 1, t.ctypes.data, None, 0, out.ctypes.data) == _lib.MBIK_EINVAL
    assert _lib.last_error() == first


def test_null_pointers_and_sample_arguments(mbik):
    args, keep = _raw_args()
    h = C.c_void_p()
    E = _lib.MBIK_EINVAL
    assert mbik.mbik_clipset_create(*args, 0, None) == E and "out" in _lib.last_error()
    null_rest, keep2 = _raw_args(rest=False)
    assert mbik.mbik_clipset_create(*null_rest, 0, C.byref(h)) == E and "rest_pose" in _lib.last_error()
    assert mbik.mbik_clipset_create(args[0], args[1], 1, None, 0, 0, C.byref(h)) == E and _lib.last_error()
    mbik.mbik_clipset_destroy(None)   # a no-op
    t, idx, out = np.zeros(4, np.float64), np.zeros(4, np.int32), np.zeros((4, 2, 10), np.float32)
    cpu = lambda *a: mbik.mbik_clip_sample_cpu(*args, *a)   # noqa: E731
    assert cpu(4, t.ctypes.data, idx.ctypes.data, 0, out.ctypes.data) == _lib.MBIK_OK
    assert cpu(4, None, idx.ctypes.data, 0, out.ctypes.data) == E and "time" in _lib.last_error()
    assert cpu(4, t.ctypes.data, idx.ctypes.data, 0, None) == E and "pose_out" in _lib.last_error()
    assert cpu(-1, t.ctypes.data, idx.ctypes.data, 0, out.ctypes.data) == E and _lib.last_error()
    for clip in (-1, 1, INT32_MIN):
        assert cpu(4, t.ctypes.data, None, clip, out.ctypes.data) == E and "clip" in _lib.last_error()
    assert cpu(4, t.ctypes.data, idx.ctypes.data, 7, out.ctypes.data) == _lib.MBIK_OK   # `clip` is unused with an index array
    assert cpu(0, None, None, 0, None) == _lib.MBIK_OK
    with pytest.raises(_lib.MbikError) as e:
        A.clip_sample_cpu(2, np.zeros((2, 10), np.float32), [_clip(length=0.0)], t)
    assert e.value.code == E
