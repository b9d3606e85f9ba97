"""Animation clip sampling for crowds (include/mbik.h, ABI 12).

`ClipSet` owns one `mbik_clipset`: several clips for one rig, resident on one GPU, bound to a bone
count and a libm_variant.  `ClipSet.sample()` takes device pointers -- one time (float64) and one
clip index (int32) per skeleton -- and writes the poses `Plan.solve()` reads; it is asynchronous on
the given HIP stream.  `clip_sample_cpu()` runs the same code on numpy arrays without a device, and
`synthetic_clips()` is the seeded clip generator the tests and tools/clip_bench.py use.
`ClipSet.sample_layers()` blends up to MAX_LAYERS (time, clip, weight) records a skeleton
(`pack_layers()`, LAYER_DTYPE) as Godot's AnimationMixer does; `clip_sample_layers_cpu()` is its
host form.

A clip is a dict: {"length": seconds, "loop_mode": 0 none | 1 linear, "tracks": [track, ...]}; a
track is a dict: {"bone", "channel": 0 position | 1 rotation | 2 scale, "interpolation": 0 nearest |
1 linear, "loop_wrap": 0 | 1, "times": [keys] float64, "values": [keys][3 or 4] float32}.

A clip may also carry blend-shape tracks: "shape_tracks": [{"shape", "interpolation",
"loop_wrap", "times": [keys] float64, "values": [keys] float32}, ...].  A `ClipSet` made with
`shape_count` > 0 holds them; `ClipSet.sample_shapes()` and `ClipSet.sample_shapes_layers()` write
the [count][shape_count] weights `Mesh.skin(..., shape_weights_ptr=...)` reads, from the same times,
clip indices and layer records as the poses.  `clip_sample_shapes_cpu()` and
`clip_sample_shapes_layers_cpu()` are the host forms, `synthetic_shape_tracks()` the seeded generator.

Root motion: `ClipSet.root_motion()` / `ClipSet.root_motion_layers()` write one
motion record [10] (rotation delta xyzw, position delta, scale delta of the root bone over the frame,
the loop seam handled) per skeleton and hold the root bone at rest in the sampled poses;
`ClipSet.apply_root_motion()` composes the records into skeleton_global [count][12] in place.
`clip_root_motion_cpu()`, `clip_root_motion_layers_cpu()` and `root_motion_apply_cpu()` are the host
forms, `synthetic_walk_clips()` the seeded generator of clips whose root bone walks and turns.

Playback: `Playback` owns one `mbik_playback`, the per-skeleton playback state of a
crowd on a `ClipSet`'s device -- AnimationPlayer's current animation, cross-fades and
animation_set_next.  `Playback.advance()` moves it one frame on and writes the layer records and
previous times `sample_layers()` and `root_motion_layers()` read, from a device array of commands
(`pack_commands()`, CMD_DTYPE) or none; `Playback.write()` / `read()` exchange state (SLOT_DTYPE
records and flag words) with the host.  `playback_advance_cpu()` is the host form.

Cubic interpolation: a track's "interpolation" may be CUBIC in a set made with
`ClipSet(..., cubic=True)` (mbik_clipset_create_desc) and in the six `*_cpu` functions called with
`cubic=True` (mbik_clip_call_cpu).  Without `cubic=True` every call is what it was and refuses CUBIC.
The generators take `interpolations=`, the kinds their tracks draw from.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib
from ._lib import check

POSITION, ROTATION, SCALE = 0, 1, 2
NEAREST, LINEAR, CUBIC = 0, 1, 2  # CUBIC: only through the `cubic=True` forms (mbik_clipset_create_desc, mbik_clip_call_cpu)
LOOP_NONE, LOOP_LINEAR = 0, 1
# floats of a pose record [10] that a channel owns (quaternion xyzw | position | scale)
CHANNEL_SLICE = {POSITION: slice(4, 7), ROTATION: slice(0, 4), SCALE: slice(7, 10)}
# mbik_clip_layer: one (time, clip, weight) record of mbik_clip_sample_layers, 16 bytes
LAYER_DTYPE = np.dtype([("time", "<f8"), ("clip", "<i4"), ("weight", "<f4")])
MAX_LAYERS = _lib.CLIP_MAX_LAYERS
LAYERS_NORMALIZE = _lib.CLIP_LAYERS_NORMALIZE
LAYER_OFF = -1
ROOT_MOTION_ORTHONORMALIZE = _lib.ROOT_MOTION_ORTHONORMALIZE
# mbik_playback_slot and mbik_playback_cmd, 24 bytes each
SLOT_DTYPE = np.dtype([("pos", "<f8"), ("clip", "<i4"), ("speed", "<f4"), ("blend_left", "<f4"), ("blend_time", "<f4")])
CMD_DTYPE = np.dtype([("start", "<f8"), ("skeleton", "<i4"), ("clip", "<i4"), ("blend_time", "<f4"), ("speed", "<f4")])
# a skeleton's flag bits (the first two) and the event bits of an advance
PLAYBACK_STARTED, PLAYBACK_ENDED, PLAYBACK_LOOPED = _lib.PLAYBACK_STARTED, _lib.PLAYBACK_ENDED, _lib.PLAYBACK_LOOPED
PLAYBACK_TRANSITIONED, PLAYBACK_BAD_COMMAND, PLAYBACK_FADE_DROPPED = _lib.PLAYBACK_TRANSITIONED, _lib.PLAYBACK_BAD_COMMAND, _lib.PLAYBACK_FADE_DROPPED
PLAYBACK_STOP = -1  # a command's clip that stops its skeleton


def _ptr(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def _set_tracks(d, clip, key, record, place, floats_per_key):
    """Fills a per-clip record's track_count / tracks from the track dicts clip[key] (`record`: their ctypes type, `place`:
    the fields that name a track's place); the objects its pointers refer to.  A dict's "key_count", and the clip's
    "<key>_count" (with no tracks: a null pointer), override what the arrays give: how the tests build invalid sets."""
    tracks, count_key = clip.get(key, []), key[:-1] + "_count"
    arr = (record * max(len(tracks), 1))()
    keep = [arr]
    for t, tr in zip(arr, tracks):
        times = None if tr.get("times") is None else np.ascontiguousarray(tr["times"], np.float64).reshape(-1)
        values = None if tr.get("values") is None else np.ascontiguousarray(tr["values"], np.float32)
        n = tr.get("key_count", 0 if times is None else times.shape[0])
        if values is not None and times is not None and "key_count" not in tr:
            assert values.size == n * floats_per_key(tr), (values.shape, n)
        keep += [times, values]
        for f in place:
            setattr(t, f, int(tr[f]))
        t.interpolation, t.loop_wrap, t.key_count = int(tr.get("interpolation", LINEAR)), int(tr.get("loop_wrap", 1)), int(n)
        t.times = None if times is None else times.ctypes.data
        t.values = None if values is None else values.ctypes.data
    d.track_count = int(clip.get(count_key, len(tracks)))
    d.tracks = C.cast(arr, C.POINTER(record)) if tracks or count_key not in clip else None
    return keep


def _descs(clips):
    """(array of mbik_clip_desc, the objects its pointers refer to)."""
    keep = []
    descs = (_lib.MbikClipDesc * max(len(clips), 1))()
    for d, clip in zip(descs, clips):
        keep += _set_tracks(d, clip, "tracks", _lib.MbikClipTrack, ("bone", "channel"), lambda tr: 4 if tr["channel"] == ROTATION else 3)
        d.length, d.loop_mode = float(clip["length"]), int(clip.get("loop_mode", LOOP_NONE))
    return descs, keep


def _shape_descs(shape_count, clips, shape_init):
    """(mbik_clipset_shapes, the objects its pointers refer to) from the clips' "shape_tracks"."""
    keep = []
    per_clip = (_lib.MbikClipShapeTracks * max(len(clips), 1))()
    for d, clip in zip(per_clip, clips):
        keep += _set_tracks(d, clip, "shape_tracks", _lib.MbikShapeTrack, ("shape",), lambda tr: 1)
    init = None if shape_init is None else np.ascontiguousarray(shape_init, np.float32).reshape(-1)
    assert init is None or init.shape == (shape_count,), init.shape
    sh = _lib.MbikClipsetShapes()
    sh.struct_size, sh.shape_count = C.sizeof(_lib.MbikClipsetShapes), int(shape_count)
    sh.init = None if init is None else init.ctypes.data
    sh.clips = C.cast(per_clip, C.POINTER(_lib.MbikClipShapeTracks))
    keep += [per_clip, init]
    return sh, keep


def _rest(bone_count, rest_pose):
    rest = np.ascontiguousarray(rest_pose, np.float32)
    assert rest.shape == (bone_count, 10), rest.shape
    return rest


def _set_args(bone_count, rest_pose, clips, libm_variant, shapes=None):
    """The arguments every entry that takes a set's description starts with -- (bone_count, rest_pose, clip_count, clips[,
    shapes], libm_variant); shapes: (shape_count, shape_init) -- and the objects their pointers refer to."""
    rest = _rest(bone_count, rest_pose)
    descs, keep = _descs(clips)
    args = [int(bone_count), _ptr(rest), len(clips), descs]
    if shapes is not None:
        sh, keep_sh = _shape_descs(shapes[0], clips, shapes[1])
        args.append(C.byref(sh))
        keep += [sh, keep_sh]
    return args + [libm_variant], keep + [rest]


def _set_desc(bone_count, rest_pose, clips, libm_variant, shapes=None):
    """(mbik_clipset_desc, the objects its pointers refer to) from _set_args' arguments."""
    rest = _rest(bone_count, rest_pose)
    descs, keep = _descs(clips)
    d = _lib.MbikClipsetDesc()
    d.struct_size, d.bone_count, d.clip_count, d.libm_variant, d.flags = C.sizeof(_lib.MbikClipsetDesc), int(bone_count), len(clips), libm_variant, 0
    d.rest_pose = rest.ctypes.data
    d.clips = C.cast(descs, C.POINTER(_lib.MbikClipDesc))
    if shapes is not None:
        sh, keep_sh = _shape_descs(shapes[0], clips, shapes[1])
        d.shapes = C.pointer(sh)
        keep += [sh, keep_sh]
    return d, keep + [rest, descs]


def _call_cpu(desc, kind, **fields):
    """mbik_clip_call_cpu of `kind` on `desc`; fields: mbik_clip_call's, arrays for its pointers."""
    c = _lib.MbikClipCall()
    c.struct_size, c.kind = C.sizeof(_lib.MbikClipCall), kind
    for k, v in fields.items():
        setattr(c, k, (None if v is None else v.ctypes.data) if k in ("time", "time_prev", "clip_index", "layers", "out", "pose") else v)
    check(_lib.load().mbik_clip_call_cpu(C.byref(desc), C.byref(c)))


class ClipSet:
    """Several clips of one rig on one GPU (mbik_clipset_create).  Immutable; close() frees it.
    cubic=True: made by mbik_clipset_create_desc, which takes tracks with interpolation CUBIC."""

    def __init__(self, bone_count: int, rest_pose, clips, libm_variant: int = 0, device: int = 0, shape_count: int = 0,
                 shape_init=None, cubic: bool = False):
        self._L = _lib.load()
        self.bone_count, self.clip_count, self.libm_variant, self.device = int(bone_count), len(clips), libm_variant, device
        self.shape_count = int(shape_count)
        shapes = (self.shape_count, shape_init) if self.shape_count else None
        h = C.c_void_p()
        if cubic:
            desc, keep = _set_desc(bone_count, rest_pose, clips, libm_variant, shapes)
            check(self._L.mbik_clipset_create_desc(C.byref(desc), device, C.byref(h)))
        else:
            args, keep = _set_args(bone_count, rest_pose, clips, libm_variant, shapes)
            create = self._L.mbik_clipset_create_shaped if self.shape_count else self._L.mbik_clipset_create
            check(create(*args, device, C.byref(h)))
        del keep
        self.h = h

    def sample(self, time_ptr: int, pose_out_ptr: int, count: int, clip_index_ptr: int = 0, clip: int = 0, stream: int = 0) -> None:
        """mbik_clip_sample: pose_out [count][bones][10] from the device arrays time [count] (float64)
        and clip_index [count] (int32; or the one `clip` for every skeleton); asynchronous on `stream`."""
        check(self._L.mbik_clip_sample(self.h, count, C.c_void_p(time_ptr or None), C.c_void_p(clip_index_ptr or None), clip,
                                       C.c_void_p(pose_out_ptr or None), C.c_void_p(stream or None)))

    def sample_layers(self, layers_ptr: int, pose_out_ptr: int, count: int, layer_count: int, flags: int = 0, stream: int = 0) -> None:
        """mbik_clip_sample_layers: pose_out [count][bones][10] from the device array layers
        [count][layer_count] of LAYER_DTYPE records, blended as AnimationMixer blends them (flags:
        LAYERS_NORMALIZE for AnimationPlayer's cross-fade); asynchronous on `stream`."""
        check(self._L.mbik_clip_sample_layers(self.h, count, layer_count, C.c_void_p(layers_ptr or None), flags,
                                              C.c_void_p(pose_out_ptr or None), C.c_void_p(stream or None)))

    def sample_shapes(self, time_ptr: int, weights_out_ptr: int, count: int, clip_index_ptr: int = 0, clip: int = 0,
                      stream: int = 0) -> None:
        """mbik_clip_sample_shapes: weights_out [count][shape_count] (float32, what Mesh.skin's
        shape_weights_ptr reads) from the device arrays sample() takes; asynchronous on `stream`."""
        check(self._L.mbik_clip_sample_shapes(self.h, count, C.c_void_p(time_ptr or None), C.c_void_p(clip_index_ptr or None), clip,
                                              C.c_void_p(weights_out_ptr or None), C.c_void_p(stream or None)))

    def sample_shapes_layers(self, layers_ptr: int, weights_out_ptr: int, count: int, layer_count: int, flags: int = 0,
                             stream: int = 0) -> None:
        """mbik_clip_sample_shapes_layers: weights_out [count][shape_count] from the layer records
        sample_layers() takes, blended as AnimationMixer blends blend-shape tracks; asynchronous on `stream`."""
        check(self._L.mbik_clip_sample_shapes_layers(self.h, count, layer_count, C.c_void_p(layers_ptr or None), flags,
                                                     C.c_void_p(weights_out_ptr or None), C.c_void_p(stream or None)))

    def root_motion(self, time_prev_ptr: int, time_ptr: int, motion_out_ptr: int, count: int, root_bone: int, clip_index_ptr: int = 0,
                    clip: int = 0, pose_ptr: int = 0, stream: int = 0) -> None:
        """mbik_clip_root_motion: motion_out [count][10] -- the root bone's rotation, position and scale
        deltas from time_prev [count] to time [count] (float64) in clip_index [count] (or the one
        `clip`); with pose_ptr the root bone of the sampled poses [count][bones][10] is put back to
        rest.  Asynchronous on `stream`, behind the sample call that wrote the poses."""
        check(self._L.mbik_clip_root_motion(self.h, count, root_bone, C.c_void_p(time_prev_ptr or None), C.c_void_p(time_ptr or None),
                                            C.c_void_p(clip_index_ptr or None), clip, C.c_void_p(motion_out_ptr or None),
                                            C.c_void_p(pose_ptr or None), C.c_void_p(stream or None)))

    def root_motion_layers(self, layers_ptr: int, time_prev_ptr: int, motion_out_ptr: int, count: int, layer_count: int, root_bone: int,
                           flags: int = 0, pose_ptr: int = 0, stream: int = 0) -> None:
        """mbik_clip_root_motion_layers: the same from this frame's layer records [count][layer_count]
        (what sample_layers() took) and each layer's previous time [count][layer_count] (float64),
        blended with sample_layers()' factors (flags: LAYERS_NORMALIZE)."""
        check(self._L.mbik_clip_root_motion_layers(self.h, count, layer_count, root_bone, C.c_void_p(layers_ptr or None),
                                                   C.c_void_p(time_prev_ptr or None), flags, C.c_void_p(motion_out_ptr or None),
                                                   C.c_void_p(pose_ptr or None), C.c_void_p(stream or None)))

    def apply_root_motion(self, motion_ptr: int, skeleton_global_ptr: int, count: int, flags: int = 0, stream: int = 0) -> None:
        """mbik_root_motion_apply: skeleton_global [count][12] (basis rows, then origin) times each
        record's Transform3D(Basis(rotation), position), in place (flags: ROOT_MOTION_ORTHONORMALIZE)."""
        check(self._L.mbik_root_motion_apply(self.h, count, C.c_void_p(motion_ptr or None), flags, C.c_void_p(skeleton_global_ptr or None),
                                             C.c_void_p(stream or None)))

    def close(self) -> None:
        if getattr(self, "h", None):
            self._L.mbik_clipset_destroy(self.h)
            self.h = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def clip_sample_cpu(bone_count: int, rest_pose, clips, time, clip_index=None, clip: int = 0, libm_variant: int = 0, cubic: bool = False):
    """mbik_clip_sample_cpu (host only): `time` [count] seconds and `clip_index` [count] (or the one
    `clip`) -> poses [count][bones][10].  cubic=True (here and in the five functions below): through
    mbik_clip_call_cpu, which takes tracks with interpolation CUBIC."""
    L = _lib.load()
    t = np.ascontiguousarray(time, np.float64).reshape(-1)
    idx = None if clip_index is None else np.ascontiguousarray(clip_index, np.int32).reshape(-1)
    assert idx is None or idx.shape == t.shape, (idx.shape, t.shape)
    out = np.empty((t.shape[0], bone_count, 10), np.float32)
    if cubic:
        desc, keep = _set_desc(bone_count, rest_pose, clips, libm_variant)
        _call_cpu(desc, _lib.CLIP_CALL_SAMPLE, count=t.shape[0], time=t, clip_index=idx, clip=clip, out=out)
        return out
    args, keep = _set_args(bone_count, rest_pose, clips, libm_variant)
    check(L.mbik_clip_sample_cpu(*args, t.shape[0], _ptr(t), _ptr(idx), clip,
                                 _ptr(out)))
    del keep
    return out


def pack_layers(time, clip, weight):
    """Layer records [count][K] of LAYER_DTYPE from three arrays of that shape (a 1-D array is one
    layer a skeleton).  clip == LAYER_OFF switches a layer off."""
    t = np.asarray(time, np.float64)
    if t.ndim == 1:
        t = t[:, None]
    assert t.ndim == 2, t.shape
    out = np.empty(t.shape, LAYER_DTYPE)
    out["time"] = t
    out["clip"] = np.asarray(clip, np.int32).reshape(t.shape)
    out["weight"] = np.asarray(weight, np.float32).reshape(t.shape)
    return out


def clip_sample_layers_cpu(bone_count: int, rest_pose, clips, layers, flags: int = 0, libm_variant: int = 0, cubic: bool = False):
    """mbik_clip_sample_layers_cpu (host only): `layers` [count][K] of LAYER_DTYPE (pack_layers) ->
    poses [count][bones][10]."""
    L = _lib.load()
    rec = np.ascontiguousarray(layers, LAYER_DTYPE)
    assert rec.ndim == 2, rec.shape
    out = np.empty((rec.shape[0], bone_count, 10), np.float32)
    if cubic:
        desc, keep = _set_desc(bone_count, rest_pose, clips, libm_variant)
        _call_cpu(desc, _lib.CLIP_CALL_SAMPLE_LAYERS, count=rec.shape[0], layer_count=rec.shape[1], layers=rec, flags=flags, out=out)
        return out
    args, keep = _set_args(bone_count, rest_pose, clips, libm_variant)
    check(L.mbik_clip_sample_layers_cpu(*args, rec.shape[0], rec.shape[1], _ptr(rec), flags, _ptr(out)))
    del keep
    return out


def _pose_arg(pose, count, bone_count):
    if pose is None:
        return None
    assert isinstance(pose, np.ndarray) and pose.dtype == np.float32 and pose.flags["C_CONTIGUOUS"], "pose is changed in place"
    assert pose.shape == (count, bone_count, 10), pose.shape
    return pose


def clip_root_motion_cpu(bone_count: int, rest_pose, clips, time_prev, time, root_bone: int, clip_index=None, clip: int = 0, pose=None,
                         libm_variant: int = 0, cubic: bool = False):
    """mbik_clip_root_motion_cpu (host only): `time_prev` and `time` [count] seconds and `clip_index`
    [count] (or the one `clip`) -> motion records [count][10].  `pose` (float32 [count][bones][10],
    optional) gets the rest pose's root record in place."""
    L = _lib.load()
    args, keep = _set_args(bone_count, rest_pose, clips, libm_variant)
    t0 = np.ascontiguousarray(time_prev, np.float64).reshape(-1)
    t1 = np.ascontiguousarray(time, np.float64).reshape(-1)
    idx = None if clip_index is None else np.ascontiguousarray(clip_index, np.int32).reshape(-1)
    assert t0.shape == t1.shape and (idx is None or idx.shape == t1.shape), (t0.shape, t1.shape)
    out = np.empty((t1.shape[0], 10), np.float32)
    if cubic:
        desc, keep_d = _set_desc(bone_count, rest_pose, clips, libm_variant)
        _call_cpu(desc, _lib.CLIP_CALL_ROOT_MOTION, count=t1.shape[0], root_bone=root_bone, time_prev=t0, time=t1, clip_index=idx, clip=clip,
                  out=out, pose=_pose_arg(pose, t1.shape[0], bone_count))
        return out
    check(L.mbik_clip_root_motion_cpu(*args, t1.shape[0], root_bone, _ptr(t0), _ptr(t1), _ptr(idx), clip, _ptr(out),
                                      _ptr(_pose_arg(pose, t1.shape[0], bone_count))))
    del keep
    return out


def clip_root_motion_layers_cpu(bone_count: int, rest_pose, clips, layers, time_prev, root_bone: int, flags: int = 0, pose=None,
                                libm_variant: int = 0, cubic: bool = False):
    """mbik_clip_root_motion_layers_cpu (host only): `layers` [count][K] of LAYER_DTYPE and
    `time_prev` [count][K] seconds -> motion records [count][10]; `pose` as in clip_root_motion_cpu."""
    L = _lib.load()
    args, keep = _set_args(bone_count, rest_pose, clips, libm_variant)
    rec = np.ascontiguousarray(layers, LAYER_DTYPE)
    assert rec.ndim == 2, rec.shape
    t0 = np.ascontiguousarray(time_prev, np.float64).reshape(rec.shape)
    out = np.empty((rec.shape[0], 10), np.float32)
    if cubic:
        desc, keep_d = _set_desc(bone_count, rest_pose, clips, libm_variant)
        _call_cpu(desc, _lib.CLIP_CALL_ROOT_MOTION_LAYERS, count=rec.shape[0], layer_count=rec.shape[1], root_bone=root_bone, layers=rec,
                  time_prev=t0, flags=flags, out=out, pose=_pose_arg(pose, rec.shape[0], bone_count))
        return out
    check(L.mbik_clip_root_motion_layers_cpu(*args, rec.shape[0], rec.shape[1], root_bone, _ptr(rec), _ptr(t0), flags, _ptr(out),
                                             _ptr(_pose_arg(pose, rec.shape[0], bone_count))))
    del keep
    return out


def root_motion_apply_cpu(motion, skeleton_global, flags: int = 0):
    """mbik_root_motion_apply_cpu (host only): a new skeleton_global [count][12] = each transform
    times its record's Transform3D(Basis(rotation), position)."""
    L = _lib.load()
    m = np.ascontiguousarray(motion, np.float32).reshape(-1, 10)
    g = np.array(skeleton_global, np.float32, order="C").reshape(-1, 12)
    assert g.shape[0] == m.shape[0], (g.shape, m.shape)
    check(L.mbik_root_motion_apply_cpu(m.shape[0], _ptr(m), flags, _ptr(g)))
    return g


def _playback_desc(clip_count, next, blend_times, default_blend_time):
    """(mbik_playback_desc or None, the objects its pointers refer to)."""
    if next is None and blend_times is None and default_blend_time == 0.0:
        return None, []
    nx = None if next is None else np.ascontiguousarray(next, np.int32).reshape(-1)
    bt = None if blend_times is None else np.ascontiguousarray(blend_times, np.float32)
    assert nx is None or nx.shape == (clip_count,), nx.shape
    assert bt is None or bt.shape == (clip_count, clip_count), bt.shape
    d = _lib.MbikPlaybackDesc()
    d.struct_size, d.default_blend_time = C.sizeof(_lib.MbikPlaybackDesc), float(default_blend_time)
    d.next = None if nx is None else nx.ctypes.data
    d.blend_times = None if bt is None else bt.ctypes.data
    return d, [nx, bt]


def empty_state(count: int, layer_count: int):
    """(slots [count][K] of SLOT_DTYPE, flags [count] uint32) with every slot off: a new object's state."""
    slots = np.zeros((count, layer_count), SLOT_DTYPE)
    slots["clip"] = LAYER_OFF
    return slots, np.zeros(count, np.uint32)


class Playback:
    """The playback state of `capacity` skeletons with `layer_count` slots each on `clipset`'s GPU
    (mbik_playback_create).  `next` [clips] (-1: none) is animation_set_next, `blend_times`
    [clips][clips] (from, to) set_blend_time.  The set may be closed before the object."""

    def __init__(self, clipset: ClipSet, capacity: int, layer_count: int, next=None, blend_times=None, default_blend_time: float = 0.0):
        self._L = _lib.load()
        self.capacity, self.layer_count, self.clip_count = int(capacity), int(layer_count), clipset.clip_count
        desc, keep = _playback_desc(clipset.clip_count, next, blend_times, default_blend_time)
        h = C.c_void_p()
        check(self._L.mbik_playback_create(clipset.h, self.capacity, self.layer_count, None if desc is None else C.byref(desc), C.byref(h)))
        del keep
        self.h = h

    def advance(self, delta: float, layers_ptr: int, time_prev_ptr: int, count: int, speed_scale: float = 1.0, cmds_ptr: int = 0,
                cmd_count: int = 0, events_ptr: int = 0, stream: int = 0) -> None:
        """mbik_playback_advance: the first `count` skeletons one frame of `delta` seconds on, after
        the `cmd_count` commands of the device array cmds (CMD_DTYPE, sorted by skeleton); writes the
        device arrays layers [count][K] (LAYER_DTYPE), time_prev [count][K] (float64) and, when
        given, events [count] (uint8).  Asynchronous on `stream`."""
        check(self._L.mbik_playback_advance(self.h, count, delta, speed_scale, C.c_void_p(cmds_ptr or None), cmd_count,
                                            C.c_void_p(layers_ptr or None), C.c_void_p(time_prev_ptr or None), C.c_void_p(events_ptr or None),
                                            C.c_void_p(stream or None)))

    def read(self, first: int = 0, n: int | None = None):
        """mbik_playback_read: (slots [n][K] of SLOT_DTYPE, flags [n] uint32) of skeletons [first, first + n)."""
        n = self.capacity - first if n is None else n
        slots, flags = np.empty((max(n, 0), self.layer_count), SLOT_DTYPE), np.empty(max(n, 0), np.uint32)
        check(self._L.mbik_playback_read(self.h, first, n, _ptr(slots), _ptr(flags)))
        return slots, flags

    def write(self, slots, flags, first: int = 0) -> None:
        """mbik_playback_write: the state of skeletons [first, first + len(flags)) from host records."""
        f = np.ascontiguousarray(flags, np.uint32).reshape(-1)
        rec = np.ascontiguousarray(slots, SLOT_DTYPE).reshape(f.shape[0], self.layer_count)
        check(self._L.mbik_playback_write(self.h, first, f.shape[0], _ptr(rec), _ptr(f)))

    def close(self) -> None:
        if getattr(self, "h", None):
            self._L.mbik_playback_destroy(self.h)
            self.h = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def pack_commands(skeleton, clip, start=np.nan, blend_time=-1.0, speed=1.0):
    """Command records of CMD_DTYPE from arrays (or scalars) of one length, sorted by skeleton,
    stably: commands for one skeleton keep their order.  clip == PLAYBACK_STOP stops a skeleton; a
    start that is not finite is the clip's start; a negative blend_time is the object's."""
    sk = np.asarray(skeleton, np.int32).reshape(-1)
    out = np.empty(sk.shape, CMD_DTYPE)
    out["skeleton"] = sk
    out["clip"] = np.broadcast_to(np.asarray(clip, np.int32), sk.shape)
    out["start"] = np.broadcast_to(np.asarray(start, np.float64), sk.shape)
    out["blend_time"] = np.broadcast_to(np.asarray(blend_time, np.float32), sk.shape)
    out["speed"] = np.broadcast_to(np.asarray(speed, np.float32), sk.shape)
    return out[np.argsort(sk, kind="stable")]


def playback_advance_cpu(clips, state, flags, delta: float, speed_scale: float = 1.0, cmds=None, next=None, blend_times=None,
                         default_blend_time: float = 0.0, events: bool = True):
    """mbik_playback_advance_cpu (host only): `state` [count][K] of SLOT_DTYPE and `flags` [count]
    one frame on -> (state, flags, layers [count][K] of LAYER_DTYPE, time_prev [count][K], events
    [count] uint8 or None), all new arrays.  `cmds` is used as it is given (pack_commands sorts)."""
    L = _lib.load()
    descs, keep = _descs([dict(length=c["length"], loop_mode=c.get("loop_mode", LOOP_NONE), tracks=[]) for c in clips])
    desc, keep_d = _playback_desc(len(clips), next, blend_times, default_blend_time)
    st = np.array(state, SLOT_DTYPE, order="C")
    assert st.ndim == 2, st.shape
    fl = np.array(flags, np.uint32, order="C").reshape(-1)
    assert fl.shape[0] == st.shape[0], (fl.shape, st.shape)
    cm = None if cmds is None else np.ascontiguousarray(cmds, CMD_DTYPE).reshape(-1)
    layers, prev = np.empty(st.shape, LAYER_DTYPE), np.empty(st.shape, np.float64)
    ev = np.empty(st.shape[0], np.uint8) if events else None
    check(L.mbik_playback_advance_cpu(len(clips), descs, None if desc is None else C.byref(desc), st.shape[0], st.shape[1], _ptr(st), _ptr(fl),
                                      delta, speed_scale, _ptr(cm), 0 if cm is None else cm.shape[0], _ptr(layers), _ptr(prev), _ptr(ev)))
    del keep, keep_d
    return st, fl, layers, prev, ev


# the host forms of the shape calls need no rig: the pose tracks of `clips` are left out
_NO_REST = np.zeros((1, 10), np.float32)


def _shape_only(clips):
    return [dict(length=c["length"], loop_mode=c.get("loop_mode", LOOP_NONE), tracks=[],
                 **{k: c[k] for k in ("shape_tracks", "shape_track_count") if k in c}) for c in clips]


def clip_sample_shapes_cpu(shape_count: int, clips, time, clip_index=None, clip: int = 0, shape_init=None, cubic: bool = False):
    """mbik_clip_sample_shapes_cpu (host only): `time` [count] seconds and `clip_index` [count] (or
    the one `clip`) -> weights [count][shape_count]."""
    L = _lib.load()
    args, keep = _set_args(0, _NO_REST[:0], _shape_only(clips), 0, (shape_count, shape_init))
    t = np.ascontiguousarray(time, np.float64).reshape(-1)
    idx = None if clip_index is None else np.ascontiguousarray(clip_index, np.int32).reshape(-1)
    assert idx is None or idx.shape == t.shape, (idx.shape, t.shape)
    out = np.empty((t.shape[0], max(int(shape_count), 0)), np.float32)
    if cubic:
        desc, keep_d = _set_desc(0, _NO_REST[:0], _shape_only(clips), 0, (shape_count, shape_init))
        _call_cpu(desc, _lib.CLIP_CALL_SHAPES, count=t.shape[0], time=t, clip_index=idx, clip=clip, out=out)
        return out
    check(L.mbik_clip_sample_shapes_cpu(*args, t.shape[0], _ptr(t), _ptr(idx), clip, _ptr(out)))
    del keep
    return out


def clip_sample_shapes_layers_cpu(shape_count: int, clips, layers, flags: int = 0, shape_init=None, cubic: bool = False):
    """mbik_clip_sample_shapes_layers_cpu (host only): `layers` [count][K] of LAYER_DTYPE
    (pack_layers) -> weights [count][shape_count]."""
    L = _lib.load()
    args, keep = _set_args(0, _NO_REST[:0], _shape_only(clips), 0, (shape_count, shape_init))
    rec = np.ascontiguousarray(layers, LAYER_DTYPE)
    assert rec.ndim == 2, rec.shape
    out = np.empty((rec.shape[0], max(int(shape_count), 0)), np.float32)
    if cubic:
        desc, keep_d = _set_desc(0, _NO_REST[:0], _shape_only(clips), 0, (shape_count, shape_init))
        _call_cpu(desc, _lib.CLIP_CALL_SHAPES_LAYERS, count=rec.shape[0], layer_count=rec.shape[1], layers=rec, flags=flags, out=out)
        return out
    check(L.mbik_clip_sample_shapes_layers_cpu(*args, rec.shape[0], rec.shape[1], _ptr(rec), flags, _ptr(out)))
    del keep
    return out


def _unit_quats(rng, n):
    q = rng.normal(0.0, 1.0, (n, 4))
    return q / np.linalg.norm(q, axis=1, keepdims=True)


def _quat_mul(a, b):
    x = a[..., 3] * b[..., 0] + a[..., 0] * b[..., 3] + a[..., 1] * b[..., 2] - a[..., 2] * b[..., 1]
    y = a[..., 3] * b[..., 1] + a[..., 1] * b[..., 3] + a[..., 2] * b[..., 0] - a[..., 0] * b[..., 2]
    z = a[..., 3] * b[..., 2] + a[..., 2] * b[..., 3] + a[..., 0] * b[..., 1] - a[..., 1] * b[..., 0]
    w = a[..., 3] * b[..., 3] - a[..., 0] * b[..., 0] - a[..., 1] * b[..., 1] - a[..., 2] * b[..., 2]
    return np.stack([x, y, z, w], axis=-1)


def _key_rotations(rng, n):
    """n unit quaternions, each 10..120 degrees from the one before it and the last at least 10
    degrees from the first (the pair a wrapping track interpolates)."""
    q = np.empty((n, 4))
    q[0] = _unit_quats(rng, 1)[0]
    k = 1
    while k < n:
        ax = rng.normal(0.0, 1.0, 3)
        ax /= np.linalg.norm(ax)
        ang = np.radians(rng.uniform(10.0, 120.0))
        cand = _quat_mul(q[k - 1], np.concatenate([ax * np.sin(ang / 2), [np.cos(ang / 2)]]))
        if k == n - 1 and 2.0 * np.degrees(np.arccos(min(1.0, abs(float(cand @ q[0]))))) < 10.0:
            continue
        q[k] = cand
        k += 1
    return q


def _draw_interpolation(rng, interpolations):
    """One draw of the stream either way: 0 or 1 as ever, or one of `interpolations`."""
    if interpolations is None:
        return int(rng.integers(0, 2))
    return int(interpolations[rng.integers(0, len(interpolations))])


def synthetic_clips(seed: int, bone_count: int, clip_count: int = 3, key_counts=(0, 1, 2, 3, 17), lengths=(1.0, 3.0), interpolations=None):
    """A seeded clip set for a rig of `bone_count` bones: (rest_pose [bones][10], clips).

    Every (clip, bone, channel) draws its key count from `key_counts` (0: untracked, no track), its
    interpolation and its loop_wrap at random; clips alternate LOOP_LINEAR and LOOP_NONE, starting
    with LOOP_LINEAR, with lengths drawn from `lengths`.  A third of the tracks keep their keys
    strictly inside (0, length), a third have keys exactly at 0 and at length, and a third a key at
    0 only.  Key rotations are unit quaternions at least 10 degrees apart (the wrap pair included),
    positions lie in [-1, 1] and scales in [0.5, 1.5].  interpolations: the kinds a track draws its
    interpolation from, e.g. (NEAREST, LINEAR, CUBIC); None: NEAREST or LINEAR, the stream as it always was."""
    rng = np.random.default_rng(seed)
    B = int(bone_count)
    rest = np.concatenate([_unit_quats(rng, B), rng.uniform(-1.0, 1.0, (B, 3)), rng.uniform(0.5, 1.5, (B, 3))], axis=1).astype(np.float32)
    clips = []
    for c in range(clip_count):
        length = float(rng.uniform(lengths[0], lengths[1]))
        tracks = []
        for bone in range(B):
            for channel in (POSITION, ROTATION, SCALE):
                n = int(key_counts[rng.integers(0, len(key_counts))])
                interpolation, loop_wrap, edge = _draw_interpolation(rng, interpolations), int(rng.integers(0, 2)), int(rng.integers(0, 3))
                if n == 0:
                    continue
                times = np.sort(rng.uniform(0.05 * length, 0.95 * length, n))
                while n > 1 and np.min(np.diff(times)) <= 0.0:
                    times = np.sort(rng.uniform(0.05 * length, 0.95 * length, n))
                if edge >= 1:
                    times[0] = 0.0
                if edge == 1 and n > 1:
                    times[-1] = length
                if channel == ROTATION:
                    values = _key_rotations(rng, n)
                elif channel == POSITION:
                    values = rng.uniform(-1.0, 1.0, (n, 3))
                else:
                    values = rng.uniform(0.5, 1.5, (n, 3))
                tracks.append(dict(bone=bone, channel=channel, interpolation=interpolation, loop_wrap=loop_wrap,
                                   times=times.astype(np.float64), values=values.astype(np.float32)))
        clips.append(dict(length=length, loop_mode=LOOP_LINEAR if c % 2 == 0 else LOOP_NONE, tracks=tracks))
    return rest, clips


def synthetic_walk_clips(seed: int, bone_count: int, root_bone: int, clip_count: int = 3, key_counts=(0, 1, 2, 3, 17),
                         lengths=(1.0, 3.0), walk_keys=(2, 3, 9), interpolations=None):
    """synthetic_clips' set with a walking root: (rest_pose, clips).

    The tracks of `root_bone` are replaced, from a random stream of their own (seed + 1): in every
    clip but the last a position track and a yaw-rotation track whose keys run from key 0 at time 0
    (position 0, no turn) to a key at time `length` holding the net displacement (up to 2 units a
    loop) and the net turn (up to 100 degrees about y); key counts come from `walk_keys`, and each
    track draws its interpolation and its loop_wrap at random.  The first clip has a scale track of
    the same shape as well.  The last clip leaves the root untracked.  Every other bone is
    synthetic_clips' own."""
    rest, clips = synthetic_clips(seed, bone_count, clip_count, key_counts, lengths, interpolations)
    rng = np.random.default_rng(seed + 1)
    out = []
    for c, clip in enumerate(clips):
        length = float(clip["length"])
        tracks = [t for t in clip["tracks"] if t["bone"] != root_bone]
        if c < max(1, len(clips) - 1):
            for channel in (POSITION, ROTATION, SCALE)[:3 if c == 0 else 2]:
                n = int(walk_keys[rng.integers(0, len(walk_keys))])
                times = np.concatenate([[0.0], np.sort(rng.uniform(0.05 * length, 0.95 * length, n - 2)), [length]])
                f = times / length + np.concatenate([[0.0], rng.uniform(-0.3, 0.3, n - 2) / n, [0.0]])   # uneven pace
                if channel == ROTATION:
                    ang = np.radians(rng.uniform(-100.0, 100.0)) * f
                    values = np.stack([np.zeros(n), np.sin(ang / 2), np.zeros(n), np.cos(ang / 2)], axis=1)
                elif channel == POSITION:
                    values = f[:, None] * rng.uniform(-2.0, 2.0, 3)[None, :]
                else:
                    values = 1.0 + f[:, None] * rng.uniform(-0.25, 0.25, 3)[None, :]
                tracks.append(dict(bone=int(root_bone), channel=channel, interpolation=_draw_interpolation(rng, interpolations),
                                   loop_wrap=int(rng.integers(0, 2)), times=times.astype(np.float64), values=values.astype(np.float32)))
        out.append(dict(clip, tracks=tracks))
    return rest, out


def synthetic_shape_tracks(seed: int, shape_count: int, clips, key_counts=(0, 1, 2, 3, 17), interpolations=None):
    """Copies of `clips` with seeded "shape_tracks" for `shape_count` blend shapes added.

    synthetic_clips' mix: every (clip, shape) draws its key count from `key_counts` (0: untracked),
    its interpolation and its loop_wrap at random; a third of the tracks keep their keys strictly
    inside (0, length), a third have keys exactly at 0 and at length, and a third a key at 0 only.
    Values lie in [-0.25, 1.25]; about a tenth of them are exactly 0 and a tenth exactly 1."""
    rng = np.random.default_rng(seed)
    out = []
    for clip in clips:
        length = float(clip["length"])
        tracks = []
        for shape in range(int(shape_count)):
            n = int(key_counts[rng.integers(0, len(key_counts))])
            interpolation, loop_wrap, edge = _draw_interpolation(rng, interpolations), int(rng.integers(0, 2)), int(rng.integers(0, 3))
            if n == 0:
                continue
            times = np.sort(rng.uniform(0.05 * length, 0.95 * length, n))
            while n > 1 and np.min(np.diff(times)) <= 0.0:
                times = np.sort(rng.uniform(0.05 * length, 0.95 * length, n))
            if edge >= 1:
                times[0] = 0.0
            if edge == 1 and n > 1:
                times[-1] = length
            values = rng.uniform(-0.25, 1.25, n)
            u = rng.uniform(0.0, 1.0, n)
            values[u < 0.1] = 0.0
            values[u > 0.9] = 1.0
            tracks.append(dict(shape=shape, interpolation=interpolation, loop_wrap=loop_wrap, times=times.astype(np.float64),
                               values=values.astype(np.float32)))
        out.append(dict(clip, shape_tracks=tracks))
    return out
