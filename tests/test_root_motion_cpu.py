"""mbik_clip_root_motion_cpu, mbik_clip_root_motion_layers_cpu and mbik_root_motion_apply_cpu (the host
forms of the root-motion calls; the kernels run the same code) against tests/root_motion_recipe.py,
bitwise: seeded walking clip sets, bone counts 1 and 5, the root bone first and last, 1, 2, 3 and 8
layers in both modes, frames inside one pass, across the seam, on keys, on 0 and on the length, of no
length, backwards and non-finite, layers off, weighted zero and NaN, zero totals, invalid indices, the
pose fix-up, the apply with and without orthonormalisation, and every argument check."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from many_bone_ik_amd import _lib
from many_bone_ik_amd import animation as A

from . import root_motion_recipe as R

E = _lib.MBIK_EINVAL
RIGS = [(1, 0), (5, 0), (5, 4)]          # (bones, root bone)
LAYER_COUNTS = (1, 2, 3, 8)
IDENTITY = np.array([1, 0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0], np.float32)


def walk_set(B, root, seed=0):
    return A.synthetic_walk_clips(900 + 10 * B + root + seed, B, root)


def assert_same(got, want, what=""):
    bad = np.nonzero((R.bits(got) != R.bits(want)).any(axis=-1))[0]
    assert bad.size == 0, f"{what}: {bad.size} records differ; first {bad[0]}: got {got[bad[0]]}, want {want[bad[0]]}"


@pytest.mark.parametrize("B,root", RIGS, ids=str)
@pytest.mark.parametrize("K", LAYER_COUNTS)
def test_layers_match_the_recipe(mbik, B, root, K):
    rest, clips = walk_set(B, root)
    layers, t0 = R.random_frames(50 + K, 96, K, clips)
    for flags in (0, R.NORMALIZE):
        want, stats = R.expected(B, rest, clips, layers, t0, root, flags)
        got = A.clip_root_motion_layers_cpu(B, rest, clips, layers, t0, root, flags)
        assert_same(got, want, f"K={K} flags={flags}")
        for k in ("invalid_skeletons", "looped", "nonfinite", "start_channels", "on_key"):
            assert stats[k] >= 2, (k, stats)
        assert stats["segments"] >= 60, stats


def test_branch_statistics_of_a_batch(mbik):
    """The layered batches above hold what the issue lists: off, zero-weight and NaN-weight layers,
    zero totals, skipped weights and invalid indices (clip_layers_recipe's statistics of the records)."""
    from . import clip_layers_recipe as LR
    rest, clips = walk_set(5, 0)
    layers, t0 = R.random_frames(53, 160, 3, clips)
    _, _, _, stats = LR.plan(5, clips, layers, R.NORMALIZE)
    for k in ("layers_off", "skipped_by_weight", "untracked", "accumulated", "invalid_skeletons", "zero_totals"):
        assert stats[k] >= 1, (k, stats)
    assert np.isnan(layers["weight"]).any() and (layers["weight"] == 0).any()
    assert (t0 == layers["time"]).any() and (t0 > layers["time"]).any() and (~np.isfinite(t0)).any()


@pytest.mark.parametrize("B,root", RIGS, ids=str)
def test_plain_matches_the_recipe_and_the_one_layer_call(mbik, B, root):
    rest, clips = walk_set(B, root)
    layers, t0 = R.random_frames(7, 200, 1, clips)
    ci = layers["clip"][:, 0].copy()       # -1 among them: a layer that is off
    t1, t0 = layers["time"][:, 0], t0[:, 0]
    want, stats = R.expected_plain(B, rest, clips, t0, t1, root, ci)
    got = A.clip_root_motion_cpu(B, rest, clips, t0, t1, root, clip_index=ci)
    assert_same(got, want, "plain")
    assert stats["looped"] >= 5 and stats["invalid_skeletons"] >= 1
    one = A.clip_root_motion_layers_cpu(B, rest, clips, A.pack_layers(t1, ci, np.ones(t1.shape, np.float32)), t0[:, None], root, 0)
    assert R.same_bits(got, one), "plain call != one-layer call"
    for c in range(len(clips)):           # the one `clip` for every skeleton
        assert_same(A.clip_root_motion_cpu(B, rest, clips, t0, t1, root, clip=c), R.expected_plain(B, rest, clips, t0, t1, root, clip=c)[0],
                    f"clip={c}")


def test_plain_index_minus_one_is_a_layer_that_is_off(mbik):
    """The plain call is the one-layer call, so a clip_index of -1 is a layer that is off and gives
    the start values; any other index outside the set gives NaN."""
    rest, clips = walk_set(5, 0)
    got = A.clip_root_motion_cpu(5, rest, clips, [0.1], [0.2], 0, clip_index=[-1])
    assert R.same_bits(got[0], R.START)
    assert (R.bits(A.clip_root_motion_cpu(5, rest, clips, [0.1], [0.2], 0, clip_index=[-2])) == 0x7FC00000).all()


def test_times_exactly_on_keys_zero_and_length(mbik):
    """Frames whose ends are key times, 0 and the length, in every clip, each as one layer of weight 1."""
    B, root = 5, 0
    rest, clips = walk_set(B, root)
    t0, t1, ci = [], [], []
    for c, clip in enumerate(clips):
        L = clip["length"]
        marks = sorted({0.0, L, *[float(t) for tr in clip["tracks"] if tr["bone"] == root for t in tr["times"]]})
        for a in marks:
            for b in marks:
                for shift in (0.0, L, 2 * L):     # the same marks one and two loops on
                    t0.append(a + shift), t1.append(b + shift), ci.append(c)
        t0 += [0.75 * L, L, -0.0, 0.5 * L]
        t1 += [L, 1.25 * L, 0.0, 0.5 * L]
        ci += [c] * 4
    want, stats = R.expected_plain(B, rest, clips, t0, t1, root, ci)
    assert stats["on_key"] >= 100 and stats["looped"] >= 10
    assert_same(A.clip_root_motion_cpu(B, rest, clips, t0, t1, root, clip_index=ci), want)


def test_untracked_root_gives_the_start_values(mbik):
    B = 5
    rest, clips = A.synthetic_clips(12, B)
    clips = [dict(c, tracks=[t for t in c["tracks"] if t["bone"] != 2]) for c in clips]
    layers, t0 = R.random_frames(9, 60, 3, clips, specials=False)
    for flags in (0, R.NORMALIZE):
        got = A.clip_root_motion_layers_cpu(B, rest, clips, layers, t0, 2, flags)
        assert R.same_bits(got, np.tile(R.START, (60, 1)))
        assert_same(got, R.expected(B, rest, clips, layers, t0, 2, flags)[0])
    # one channel tracked only: the others keep their start bits
    rest, clips = walk_set(B, 0)
    last = len(clips) - 1                   # synthetic_walk_clips leaves the last clip's root untracked
    got = A.clip_root_motion_cpu(B, rest, clips, [0.1], [0.3], 0, clip=last)
    assert R.same_bits(got[0], R.START)
    got = A.clip_root_motion_cpu(B, rest, clips, [0.0], [clips[1]["length"]], 0, clip=1)    # position and rotation, no scale
    assert R.same_bits(got[0, 7:10], R.START[7:10]) and not R.same_bits(got[0, 4:7], R.START[4:7])


@pytest.mark.parametrize("B,root", RIGS, ids=str)
def test_pose_fix_up(mbik, B, root):
    rest, clips = walk_set(B, root)
    layers, t0 = R.random_frames(31, 90, 2, clips)
    sampled = A.clip_sample_layers_cpu(B, rest, clips, layers, R.NORMALIZE)
    pose = sampled.copy()
    motion = A.clip_root_motion_layers_cpu(B, rest, clips, layers, t0, root, R.NORMALIZE, pose=pose)
    want, valid = R.expected_pose(sampled, rest, clips, layers, root)
    assert R.same_bits(pose, want)
    invalid = ~valid
    assert (R.bits(motion[invalid]) == 0x7FC00000).all()
    assert invalid.any() and R.same_bits(pose[invalid], sampled[invalid]), "invalid skeletons are untouched"
    assert R.same_bits(pose[valid][:, root], np.tile(rest[root], (int(valid.sum()), 1)))
    others = [b for b in range(B) if b != root]
    assert R.same_bits(pose[:, others], sampled[:, others])
    assert (R.bits(sampled[valid][:, root]) != R.bits(rest[root])).any(), "the sampler had moved the root"
    # the plain form does the same
    t1 = layers["time"][:, 0]
    ci = layers["clip"][:, 0]
    pose = A.clip_sample_cpu(B, rest, clips, t1, clip_index=np.where(ci == -1, 0, ci))
    before = pose.copy()
    A.clip_root_motion_cpu(B, rest, clips, t0[:, 0], t1, root, clip_index=ci, pose=pose)
    want, valid = R.expected_pose(before, rest, clips, R.pack(t1[:, None], ci[:, None], np.ones((t1.shape[0], 1), np.float32)), root)
    assert R.same_bits(pose, want) and not valid.all()


def apply_inputs(seed, n):
    rng = np.random.default_rng(seed)
    rest, clips = walk_set(5, 0)
    layers, t0 = R.random_frames(seed, n, 2, clips)
    motion = A.clip_root_motion_layers_cpu(5, rest, clips, layers, t0, 0, R.NORMALIZE)
    q = rng.normal(0.0, 1.0, (n, 4))
    q /= np.linalg.norm(q, axis=1, keepdims=True)
    G = np.empty((n, 12), np.float32)
    for s in range(n):
        G[s, 0:9] = (R.quat_to_matrix64(q[s]) * rng.uniform(0.8, 1.2)).reshape(9)
    G[:, 9:12] = rng.uniform(-50.0, 50.0, (n, 3))
    motion[3], motion[5, 4] = np.nan, np.inf
    motion[7, 0:4] = 0.0                    # a zero quaternion: 2 / 0
    G[11, 2] = np.nan
    G[13, 0:9] = 0.0                        # a zero basis: the orthonormalisation's zero-length branch
    return motion, G


def test_apply_matches_the_recipe(mbik):
    motion, G = apply_inputs(4, 80)
    assert (R.bits(motion) == 0x7FC00000).all(axis=1).any()
    for flags in (0, R.ORTHONORMALIZE):
        got = A.root_motion_apply_cpu(motion, G, flags)
        assert_same(got, R.expected_apply(motion, G, flags), f"flags={flags}")
        nan = np.isnan(got)
        assert nan.any() and (R.bits(got)[nan] == 0x7FC00000).all()
    assert R.same_bits(A.root_motion_apply_cpu(np.tile(R.START, (3, 1)), np.tile(IDENTITY, (3, 1))), np.tile(IDENTITY, (3, 1)))


def _cpu(L, B, rest, clips, count, root, t0, t1, ci, clip, out, pose=None):
    descs, keep = A._descs(clips)
    p = lambda a: None if a is None else (a if isinstance(a, int) else a.ctypes.data)  # noqa: E731
    return L.mbik_clip_root_motion_cpu(B, rest.ctypes.data, len(clips), descs, 0, count, root, p(t0), p(t1), p(ci), clip, p(out), p(pose))


def _cpu_layers(L, B, rest, clips, count, K, root, layers, t0, flags, out, pose=None):
    descs, keep = A._descs(clips)
    p = lambda a: None if a is None else (a if isinstance(a, int) else a.ctypes.data)  # noqa: E731
    return L.mbik_clip_root_motion_layers_cpu(B, rest.ctypes.data, len(clips), descs, 0, count, K, root, p(layers), p(t0), flags, p(out), p(pose))


def test_argument_errors(mbik):
    L = _lib.load()
    B, n, K = 5, 6, 2
    rest, clips = walk_set(B, 0)
    layers, t0 = R.random_frames(1, n, K, clips, specials=False)
    t1 = np.ascontiguousarray(layers["time"][:, 0])
    tp = np.ascontiguousarray(t0[:, 0])
    ci = np.zeros(n, np.int32)
    out = np.zeros((n, 10), np.float32)
    pose = np.zeros((n, B, 10), np.float32)
    ok = lambda rc: rc == _lib.MBIK_OK      # noqa: E731
    bad = lambda rc: rc == E and _lib.last_error()  # noqa: E731
    # plain
    assert ok(_cpu(L, B, rest, clips, n, 0, tp, t1, ci, 0, out, pose))
    assert ok(_cpu(L, B, rest, clips, 0, 0, None, None, None, 0, None))              # count == 0
    assert bad(_cpu(L, B, rest, clips, -1, 0, tp, t1, ci, 0, out))
    for root in (-1, B):
        assert bad(_cpu(L, B, rest, clips, n, root, tp, t1, ci, 0, out))
        assert bad(_cpu(L, B, rest, clips, 0, root, tp, t1, ci, 0, out))
    assert bad(_cpu(L, B, rest, clips, n, 0, tp, t1, None, len(clips), out)) and bad(_cpu(L, B, rest, clips, n, 0, tp, t1, None, -1, out))
    assert ok(_cpu(L, B, rest, clips, n, 0, tp, t1, ci, len(clips), out))                # `clip` is not used with clip_index
    assert bad(_cpu(L, B, rest, clips, n, 0, None, t1, ci, 0, out)) and bad(_cpu(L, B, rest, clips, n, 0, tp, None, ci, 0, out))
    assert bad(_cpu(L, B, rest, clips, n, 0, tp, t1, ci, 0, None))
    assert bad(_cpu(L, B, rest, clips, n - 1, 0, tp.ctypes.data + 4, t1, ci, 0, out))    # time_prev not 8-byte aligned
    buf = np.zeros(n * 10 + 4, np.float64)
    o = buf.ctypes.data
    assert bad(_cpu(L, B, rest, clips, n, 0, o, t1, ci, 0, o)) and bad(_cpu(L, B, rest, clips, n, 0, tp, o + 8, ci, 0, o))
    assert bad(_cpu(L, B, rest, clips, n, 0, tp, t1, o + 16, 0, o)) and bad(_cpu(L, B, rest, clips, n, 0, tp, t1, ci, 0, o, o + 36))
    empty = np.zeros((0, 10), np.float32)
    assert bad(_cpu(L, 0, empty, [dict(length=1.0, loop_mode=0, tracks=[])], n, 0, tp, t1, ci, 0, out))   # a set without bones
    # layered
    assert ok(_cpu_layers(L, B, rest, clips, n, K, 0, layers, t0, 1, out, pose))
    assert ok(_cpu_layers(L, B, rest, clips, 0, K, 0, None, None, 0, None))
    assert bad(_cpu_layers(L, B, rest, clips, -1, K, 0, layers, t0, 0, out))
    for root in (-1, B):
        assert bad(_cpu_layers(L, B, rest, clips, n, K, root, layers, t0, 0, out))
    for k in (0, -1, 9):
        assert bad(_cpu_layers(L, B, rest, clips, n, k, 0, layers, t0, 0, out)) and bad(_cpu_layers(L, B, rest, clips, 0, k, 0, layers, t0, 0, out))
    assert bad(_cpu_layers(L, B, rest, clips, n, K, 0, layers, t0, 2, out)) and bad(_cpu_layers(L, B, rest, clips, 0, K, 0, layers, t0, 2, out))
    assert bad(_cpu_layers(L, B, rest, clips, n, K, 0, None, t0, 0, out)) and bad(_cpu_layers(L, B, rest, clips, n, K, 0, layers, None, 0, out))
    assert bad(_cpu_layers(L, B, rest, clips, n, K, 0, layers, t0, 0, None))
    assert bad(_cpu_layers(L, B, rest, clips, n - 1, K, 0, layers.ctypes.data + 4, t0, 0, out))
    assert bad(_cpu_layers(L, B, rest, clips, n - 1, K, 0, layers, t0.ctypes.data + 4, 0, out))
    assert bad(_cpu_layers(L, B, rest, clips, n, K, 0, o + 8, t0, 0, o)) and bad(_cpu_layers(L, B, rest, clips, n, K, 0, layers, o, 0, o + 8))
    assert bad(_cpu_layers(L, B, rest, clips, n, K, 0, layers, t0, 0, o, o + 4))
    # apply
    G = np.tile(IDENTITY, (n, 1))
    ap = L.mbik_root_motion_apply_cpu
    assert ok(ap(n, out.ctypes.data, 1, G.ctypes.data)) and ok(ap(0, None, 0, None))
    assert bad(ap(-1, out.ctypes.data, 0, G.ctypes.data)) and bad(ap(n, out.ctypes.data, 2, G.ctypes.data)) and bad(ap(0, None, 2, None))
    assert bad(ap(n, None, 0, G.ctypes.data)) and bad(ap(n, out.ctypes.data, 0, None))
    assert bad(ap(n, o, 0, o + 8)) and bad(ap(1, o + 48, 0, o + 4))
    # the device entries without a set
    assert bad(L.mbik_clip_root_motion(None, n, 0, tp.ctypes.data, t1.ctypes.data, None, 0, out.ctypes.data, None, None))
    assert bad(L.mbik_clip_root_motion_layers(None, n, K, 0, layers.ctypes.data, t0.ctypes.data, 0, out.ctypes.data, None, None))
    assert bad(L.mbik_root_motion_apply(None, n, out.ctypes.data, 0, G.ctypes.data, None))


def test_synthetic_walk_clips(mbik):
    """The generator: synthetic_clips' stream is untouched, the root walks from 0 at time 0 to a net
    displacement and turn at a key at the length, and the tracks mix interpolation and loop_wrap."""
    for B, root in RIGS:
        rest, clips = A.synthetic_walk_clips(40, B, root)
        rest0, clips0 = A.synthetic_clips(40, B)
        assert R.same_bits(rest, rest0) and len(clips) == len(clips0)
        for c, c0 in zip(clips, clips0):
            assert c["length"] == c0["length"] and c["loop_mode"] == c0["loop_mode"]
            other = lambda cl: [(t["bone"], t["channel"], t["times"].tobytes(), t["values"].tobytes()) for t in cl["tracks"] if t["bone"] != root]  # noqa: E731
            assert other(c) == other(c0)
    seen = set()
    for seed in range(6):
        _, clips = A.synthetic_walk_clips(seed, 5, 4)
        assert not [t for t in clips[-1]["tracks"] if t["bone"] == 4]
        for c in clips[:-1]:
            tr = {t["channel"]: t for t in c["tracks"] if t["bone"] == 4}
            assert A.POSITION in tr and A.ROTATION in tr
            for ch, t in tr.items():
                assert t["times"][0] == 0.0 and t["times"][-1] == c["length"] and len(t["times"]) >= 2
                seen.add((t["interpolation"], t["loop_wrap"]))
            assert np.array_equal(tr[A.POSITION]["values"][0], np.zeros(3, np.float32)) and np.abs(tr[A.POSITION]["values"][-1]).max() > 0
            q = tr[A.ROTATION]["values"]
            assert np.array_equal(q[0], np.array([0, 0, 0, 1], np.float32)) and q[-1][1] != 0 and q[-1][0] == 0 and q[-1][2] == 0
    assert seen == {(0, 0), (0, 1), (1, 0), (1, 1)}


def test_symbols_and_abi(mbik):
    header = open(os.path.join(os.path.dirname(os.path.dirname(__file__)), "include", "mbik.h")).read()
    assert re.search(r"^#define MBIK_ABI_VERSION 15$", header, re.M)
    assert re.search(r"^#define MBIK_ROOT_MOTION_ORTHONORMALIZE 1u$", header, re.M)
    lib = C.CDLL(_lib.LIB_PATH)
    for name in ("mbik_clip_root_motion", "mbik_clip_root_motion_layers", "mbik_root_motion_apply", "mbik_clip_root_motion_cpu",
                 "mbik_clip_root_motion_layers_cpu", "mbik_root_motion_apply_cpu"):
        assert name in _lib.EXPORTED_SYMBOLS and getattr(lib, name) and name + "(" in header
    assert A.ROOT_MOTION_ORTHONORMALIZE == 1
    for name in ("root_motion", "root_motion_layers", "apply_root_motion"):
        assert callable(getattr(A.ClipSet, name))
    assert "root motion, RESET" not in header
