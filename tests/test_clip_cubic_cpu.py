"""mbik_clip_call_cpu (the host twin of the six clip calls on a set that may hold cubic tracks)
against the recipe of tests/clip_cubic_recipe.py, bitwise: seeded sets whose tracks mix nearest,
linear and cubic interpolation within one bone, with 0, 1, 2, 3, 4 and 17 keys, loop_wrap on and off,
both loop modes, key quaternions off the unit sphere and with |w| > 1; times on every key and one ulp
either side, before the first and after the last key, 0, length, negative, past the length, NaN and
the infinities; 1, 2 and 8 layers with and without NORMALIZE; root-motion frames that cross the seam.
Then: a set without a cubic track gives the bits of the six older _cpu entries, and every refusal
the new entries add."""
import ctypes as C

import numpy as np
import pytest

from many_bone_ik_amd import _lib
from many_bone_ik_amd import animation as A

from . import clip_cubic_cases as K
from . import clip_cubic_recipe as Q
from . import clip_layers_recipe as LR
from . import root_motion_recipe as RM

B, P = 5, 3
ROOT = K.ROOT
LAYER_CASES = ((1, 0), (2, 0), (2, 1), (8, 0), (8, 1))   # (layer_count, flags)


@pytest.fixture(scope="module")
def cset(mbik):
    rest, clips = K.cubic_set(75, B, P)
    rest.setflags(write=False)
    return rest, clips


def assert_same(got, want, what):
    bad = np.argwhere(Q.bits(got) != Q.bits(want))
    assert bad.shape[0] == 0, f"{what}: {bad.shape[0]} floats differ; first at {tuple(bad[0])}: got {got[tuple(bad[0])]!r}, want {want[tuple(bad[0])]!r}"


def test_set_holds_what_it_should(cset):
    """Every key count with every interpolation kind, kinds mixed within one bone, wrapping and
    clamping cubic tracks, unnormalised keys and keys with |w| > 1."""
    rest, clips = cset
    seen, mixed, wraps, off_unit, big_w = set(), 0, set(), 0, 0
    for clip in clips:
        per_bone = {}
        for tr in clip["tracks"]:
            n = len(tr["times"])
            seen.add((n, tr["interpolation"]))
            per_bone.setdefault(tr["bone"], set()).add(tr["interpolation"])
            if tr["interpolation"] == A.CUBIC and n > 1:
                wraps.add((clip["loop_mode"], tr["loop_wrap"]))
            if tr["channel"] == A.ROTATION:
                norms = np.linalg.norm(np.asarray(tr["values"], np.float64), axis=1)
                off_unit += int((np.abs(norms - 1) > 0.05).any())
                big_w += int((np.abs(np.asarray(tr["values"])[:, 3]) > 1).any())
        mixed += sum(len(k) == 3 for k in per_bone.values())
    assert {n for n, k in seen if k == A.CUBIC} >= {1, 2, 3, 4, 17}
    assert mixed >= 1 and wraps == {(0, 0), (0, 1), (1, 0), (1, 1)} and off_unit >= 2 and big_w >= 1
    shape_kinds = {(len(tr["times"]), tr["interpolation"]) for clip in clips for tr in clip["shape_tracks"]}
    assert {k for _, k in shape_kinds} == {A.NEAREST, A.LINEAR, A.CUBIC}


def test_sample_matches_recipe(cset, oracle):
    rest, clips = cset
    t, ci = K.plain_batch(3, clips)
    want, stats = Q.expected(oracle, B, rest, clips, t, ci)
    assert_same(A.clip_sample_cpu(B, rest, clips, t, ci, cubic=True), want, "sample")
    for how in ("single", "clamp_first", "clamp_last", "interior", "wrap_before", "wrap_after"):
        assert stats.get("cubic:" + how, 0) > 0, (how, stats)
    assert stats["cubic:aliased"] > 0 and stats.get("linear:interior", 0) > 0 and stats.get("nearest:interior", 0) > 0
    sel = ci == 1   # the scalar `clip` instead of the index array
    assert Q.same_bits(A.clip_sample_cpu(B, rest, clips, t[sel], clip=1, cubic=True), want[sel])


@pytest.mark.parametrize("libm_variant", (0, 1))
def test_sample_other_libm_variant_runs(cset, libm_variant):
    """Both variants take a cubic set; they agree wherever no sine or cosine is evaluated (copies)."""
    rest, clips = cset
    t = np.array([0.0, 0.3, 0.9], np.float64)
    out = A.clip_sample_cpu(B, rest, clips, t, clip=0, libm_variant=libm_variant, cubic=True)
    assert out.shape == (3, B, 10) and np.isfinite(out).all()


@pytest.mark.parametrize("layer_count,flags", LAYER_CASES)
def test_sample_layers_matches_recipe(cset, oracle, layer_count, flags):
    rest, clips = cset
    layers = LR.random_layers(70 + layer_count, 24, layer_count, clips)
    want, stats = Q.expected_layers(oracle, B, rest, clips, layers, flags)
    assert_same(A.clip_sample_layers_cpu(B, rest, clips, layers, flags, cubic=True), want, f"layers K={layer_count} flags={flags}")
    assert stats["accumulated"] > 0 and any(k.startswith("cubic:") for k in stats)


def test_shapes_match_recipe(cset, oracle):
    rest, clips = cset
    init = np.array([0.0, 0.25, -0.5], np.float32)
    t, ci = K.plain_batch(5, clips, "shape_tracks")
    want, stats = Q.expected_shapes(oracle, P, clips, t, ci, init=init)
    assert_same(A.clip_sample_shapes_cpu(P, clips, t, ci, shape_init=init, cubic=True), want, "shapes")
    assert stats.get("cubic:interior", 0) > 0 and stats.get("cubic:aliased", 0) > 0


@pytest.mark.parametrize("layer_count,flags", LAYER_CASES)
def test_shapes_layers_match_recipe(cset, oracle, layer_count, flags):
    rest, clips = cset
    init = np.array([0.0, 0.25, -0.5], np.float32)
    layers = K.shape_layers(90 + layer_count, 40, layer_count, clips)
    want, stats = Q.expected_shapes_layers(oracle, P, clips, layers, flags, init=init)
    assert_same(A.clip_sample_shapes_layers_cpu(P, clips, layers, flags, shape_init=init, cubic=True), want,
                f"shape layers K={layer_count} flags={flags}")
    assert stats["accumulated"] > 0


def test_root_motion_matches_recipe(cset, oracle):
    rest, clips = cset
    t0, t1, ci = K.root_times(21, clips, 120)
    want, stats = Q.expected_root_plain(oracle, B, rest, clips, t0, t1, ROOT, ci)
    pose = np.zeros((t1.shape[0], B, 10), np.float32)
    got = A.clip_root_motion_cpu(B, rest, clips, t0, t1, ROOT, ci, pose=pose, cubic=True)
    assert_same(got, want, "root motion")
    assert stats["looped"] > 0 and stats.get("cubic:interior", 0) > 0
    valid = (ci >= -1) & (ci < len(clips))   # (-1: the one layer of the plain form is off, a valid skeleton)
    assert valid.sum() > 100 and Q.same_bits(pose[valid][:, ROOT], np.broadcast_to(rest[ROOT], (int(valid.sum()), 10)).copy())
    assert not pose[~valid].any()


@pytest.mark.parametrize("layer_count,flags", LAYER_CASES)
def test_root_motion_layers_matches_recipe(cset, oracle, layer_count, flags):
    rest, clips = cset
    layers, t0 = RM.random_frames(30 + layer_count, 40, layer_count, clips)
    want, stats = Q.expected_root(oracle, B, rest, clips, layers, t0, ROOT, flags)
    got = A.clip_root_motion_layers_cpu(B, rest, clips, layers, t0, ROOT, flags, cubic=True)
    assert_same(got, want, f"root layers K={layer_count} flags={flags}")
    assert stats["looped"] > 0


def test_set_without_cubic_gives_the_older_entries_bits(mbik):
    """mbik_clipset_desc + mbik_clip_call_cpu on nearest / linear tracks: the six older _cpu entries' bits."""
    rest, clips = K.cubic_set(62, B, P, kinds=(A.NEAREST, A.LINEAR))
    t, ci = K.plain_batch(4, clips)
    assert Q.same_bits(A.clip_sample_cpu(B, rest, clips, t, ci, cubic=True), A.clip_sample_cpu(B, rest, clips, t, ci))
    ts, cs = K.plain_batch(6, clips, "shape_tracks")
    assert Q.same_bits(A.clip_sample_shapes_cpu(P, clips, ts, cs, cubic=True), A.clip_sample_shapes_cpu(P, clips, ts, cs))
    t0, t1, cr = K.root_times(22, clips, 64)
    assert Q.same_bits(A.clip_root_motion_cpu(B, rest, clips, t0, t1, ROOT, cr, cubic=True), A.clip_root_motion_cpu(B, rest, clips, t0, t1, ROOT, cr))
    for layer_count, flags in ((2, 0), (8, 1)):
        layers, prev = RM.random_frames(40 + layer_count, 48, layer_count, clips)
        assert Q.same_bits(A.clip_sample_layers_cpu(B, rest, clips, layers, flags, cubic=True), A.clip_sample_layers_cpu(B, rest, clips, layers, flags))
        assert Q.same_bits(A.clip_root_motion_layers_cpu(B, rest, clips, layers, prev, ROOT, flags, cubic=True),
                           A.clip_root_motion_layers_cpu(B, rest, clips, layers, prev, ROOT, flags))
        sl = K.shape_layers(50 + layer_count, 48, layer_count, clips)
        assert Q.same_bits(A.clip_sample_shapes_layers_cpu(P, clips, sl, flags, cubic=True), A.clip_sample_shapes_layers_cpu(P, clips, sl, flags))


# ---------------------------------------------------------------- refusals
def _desc(clips, shapes=None, bone_count=2):
    rest = np.zeros((bone_count, 10), np.float32)
    rest[:, 3] = 1
    return A._set_desc(bone_count, rest, clips, 0, shapes)


def _call(kind, n=1, **kw):
    t = np.zeros(n, np.float64)
    out = np.zeros((n, 2, 10), np.float32)
    c = _lib.MbikClipCall()
    c.struct_size, c.kind, c.count, c.layer_count = C.sizeof(_lib.MbikClipCall), kind, n, 1
    c.time, c.time_prev, c.out = t.ctypes.data, t.ctypes.data, out.ctypes.data
    for k, v in kw.items():
        setattr(c, k, v)
    return c, (t, out)


def _track(interpolation=A.CUBIC, **kw):
    return dict(dict(bone=0, channel=A.POSITION, interpolation=interpolation, loop_wrap=1, times=[0.0, 0.5], values=np.zeros((2, 3), np.float32)), **kw)


def _refused(rc, word):
    assert rc == _lib.MBIK_EINVAL, rc
    assert word in _lib.last_error(), _lib.last_error()


def test_new_refusals(mbik):
    good, keep = _desc([dict(length=1.0, loop_mode=0, tracks=[_track()])])
    call, keep_c = _call(_lib.CLIP_CALL_SAMPLE)
    assert mbik.mbik_clip_call_cpu(C.byref(good), C.byref(call)) == 0
    _refused(mbik.mbik_clip_call_cpu(None, C.byref(call)), "null mbik_clipset_desc")
    _refused(mbik.mbik_clip_call_cpu(C.byref(good), None), "null mbik_clip_call")
    h = C.c_void_p()
    _refused(mbik.mbik_clipset_create_desc(None, 0, C.byref(h)), "null mbik_clipset_desc")
    for fn in (lambda d: mbik.mbik_clip_call_cpu(C.byref(d), C.byref(call)), lambda d: mbik.mbik_clipset_create_desc(C.byref(d), 0, C.byref(h))):
        d, k = _desc([dict(length=1.0, loop_mode=0, tracks=[_track()])])
        d.struct_size -= 1
        _refused(fn(d), "struct_size")
        d, k = _desc([dict(length=1.0, loop_mode=0, tracks=[_track()])])
        d.flags = 1
        _refused(fn(d), "flags")
    small, k = _call(_lib.CLIP_CALL_SAMPLE)
    small.struct_size -= 1
    _refused(mbik.mbik_clip_call_cpu(C.byref(good), C.byref(small)), "struct_size")
    for kind in (-1, 6):
        bad, k = _call(kind)
        _refused(mbik.mbik_clip_call_cpu(C.byref(good), C.byref(bad)), "unknown mbik_clip_call.kind")
    # a shape kind on a set described without shapes
    sh, k = _call(_lib.CLIP_CALL_SHAPES)
    _refused(mbik.mbik_clip_call_cpu(C.byref(good), C.byref(sh)), "null shapes")


@pytest.mark.parametrize("interpolation", (3, 4, -1))
def test_other_interpolations_stay_refused(mbik, interpolation):
    call, keep_c = _call(_lib.CLIP_CALL_SAMPLE)
    d, keep = _desc([dict(length=1.0, loop_mode=0, tracks=[_track(interpolation)])])
    _refused(mbik.mbik_clip_call_cpu(C.byref(d), C.byref(call)), f"unknown interpolation {interpolation}")
    h = C.c_void_p()
    _refused(mbik.mbik_clipset_create_desc(C.byref(d), 0, C.byref(h)), f"unknown interpolation {interpolation}")
    shape = dict(shape=0, interpolation=interpolation, loop_wrap=1, times=[0.0], values=[0.0])
    d, keep = _desc([dict(length=1.0, loop_mode=0, tracks=[], shape_tracks=[shape])], shapes=(1, None))
    _refused(mbik.mbik_clip_call_cpu(C.byref(d), C.byref(call)), f"unknown interpolation {interpolation}")


def test_ping_pong_stays_refused(mbik):
    call, keep_c = _call(_lib.CLIP_CALL_SAMPLE)
    d, keep = _desc([dict(length=1.0, loop_mode=2, tracks=[_track()])])
    _refused(mbik.mbik_clip_call_cpu(C.byref(d), C.byref(call)), "unknown loop_mode 2")
    h = C.c_void_p()
    _refused(mbik.mbik_clipset_create_desc(C.byref(d), 0, C.byref(h)), "unknown loop_mode 2")


def test_older_entries_still_refuse_cubic(mbik):
    """Without cubic=True the Python calls go through the older entries, which refuse interpolation 2."""
    rest = np.zeros((2, 10), np.float32)
    with pytest.raises(_lib.MbikError, match="unknown interpolation 2"):
        A.clip_sample_cpu(2, rest, [dict(length=1.0, loop_mode=0, tracks=[_track()])], [0.0])


def test_call_checks_are_the_older_entries(mbik):
    """A kind's call checks come from its older _cpu entry: the same text."""
    good, keep = _desc([dict(length=1.0, loop_mode=0, tracks=[_track()])])
    c, k = _call(_lib.CLIP_CALL_SAMPLE, clip=7)
    _refused(mbik.mbik_clip_call_cpu(C.byref(good), C.byref(c)), "outside the set's 1 clips")
    c, k = _call(_lib.CLIP_CALL_SAMPLE_LAYERS, layer_count=9)
    _refused(mbik.mbik_clip_call_cpu(C.byref(good), C.byref(c)), "layer_count 9 outside")
    c, k = _call(_lib.CLIP_CALL_ROOT_MOTION, root_bone=5)
    _refused(mbik.mbik_clip_call_cpu(C.byref(good), C.byref(c)), "root_bone 5 outside")
    c, k = _call(_lib.CLIP_CALL_SAMPLE, count=-1)
    assert mbik.mbik_clip_call_cpu(C.byref(good), C.byref(c)) == _lib.MBIK_EINVAL


def test_symbols_and_header(mbik):
    header = open(_lib.LIB_PATH.replace("many_bone_ik_amd/libmbik.so", "include/mbik.h")).read()
    for name in ("mbik_clipset_create_desc", "mbik_clip_call_cpu"):
        assert name in _lib.EXPORTED_SYMBOLS and getattr(mbik, name) and name + "(" in header
    assert "#define MBIK_ABI_VERSION 15" in header
