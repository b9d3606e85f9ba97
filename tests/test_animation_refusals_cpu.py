"""The refusal ledger of the animation front end (clip sets, sampling, root motion, playback).

Every way these entries refuse a call without needing a device, as (return code, exact text of
mbik_last_error()), pinned in tests/golden/animation_refusals.json.  The other animation suites look
for a word in the text; this one pins the whole text and, through calls with two faults at once,
which refusal comes first.  A case is a named set of changes to one valid call (B = 2, two clips, one
3-key pose track and one 3-key shape track, P = 1, count = 4, K = 2) through the raw ctypes entries.

SET_CASES change what a clip set (or a playback object's description and state) is made from,
CALL_CASES the arguments of a call on a good one; tests/test_gpu_animation_refusals.py runs the
latter through the device entries as well.  `python -m tests.test_animation_refusals_cpu` records
the golden file anew from the library in the tree.
"""
import ctypes as C
import json
import os

import numpy as np
import pytest

from many_bone_ik_amd import _lib
from many_bone_ik_amd import animation as A

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "animation_refusals.json")
B, COUNT, K, P = 2, 4, 2, 1
BUF_BYTES = 1024   # every buffer of a call: above any size a call names, so a refusal that went missing writes inside it
UNWRITTEN = 0xA5   # the byte every output buffer is filled with
INT32_MAX = 2**31 - 1
REST_BONE = np.array([0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 1.0, 1.0, 1.0], np.float32)


def _tr(**over):
    q = np.array([[0.0, 0.0, 0.0, 1.0]] * 3, np.float32)
    return dict(dict(bone=0, channel=A.ROTATION, interpolation=1, loop_wrap=1, times=[0.0, 0.5, 1.0], values=q), **over)


def _st(**over):
    return dict(dict(shape=0, interpolation=1, loop_wrap=1, times=[0.0, 0.5, 1.0], values=[0.0, 0.5, 1.0]), **over)


def default_args():
    """One valid call of every entry: scalars, the set's description, and for each pointer the name of
    a buffer (None: a null pointer; "name+4": four bytes in; another argument's name: an alias)."""
    return dict(
        bone_count=B, rest="rest", clip_count=None, libm=0, shapes=dict(struct_size=None, shape_count=P, init=None, clips=True),
        clips=[dict(length=1.0, loop_mode=1, tracks=[_tr()], shape_tracks=[_st()]), dict(length=2.0, loop_mode=0, tracks=[], shape_tracks=[])],
        handle=None, out=True, capacity=COUNT, first=0, n=COUNT,
        count=COUNT, layer_count=K, root_bone=0, clip=0, flags=0, time="time", time_prev="time_prev", clip_index=None, pose_out="pose_out",
        layers="layers", weights_out="weights_out", motion_out="motion_out", pose=None, motion="motion", skeleton_global="skeleton_global",
        desc=None, state={}, pflag={}, slots="slots", pflags="pflags", delta=0.1, speed_scale=1.0, cmds=None, cmd_count=0,
        layers_out="layers_out", time_prev_out="time_prev_out", events_out="events_out")


POINTERS = ("time", "time_prev", "clip_index", "pose_out", "layers", "weights_out", "motion_out", "pose", "motion", "skeleton_global",
            "slots", "pflags", "cmds", "layers_out", "time_prev_out", "events_out")
NO_POINTERS = {k: None for k in POINTERS}


def _set(a, path, value):
    *head, last = path.split(".")
    for k in head:
        a = a[int(k)] if isinstance(a, list) else a[k]
    if isinstance(a, list):
        a[int(last)] = value
    else:
        a[last] = value


def host_alloc(content):
    """(keep-alive, address) of a 16-byte aligned host copy of `content` (uint8)."""
    raw = np.zeros(content.size + 16, np.uint8)
    off = (-raw.ctypes.data) % 16
    raw[off:off + content.size] = content
    return raw, raw.ctypes.data + off


class Call:
    """The arguments of one call, marshalled: buffers allocated through `alloc`, descs built."""

    def __init__(self, overrides, alloc=host_alloc):
        a = default_args()
        for path, value in overrides.items():
            _set(a, path, value)
        self.a, self.keep, self.addr = a, [], {}
        n = BUF_BYTES // 8
        layers = np.zeros(BUF_BYTES // 16, A.LAYER_DTYPE)
        layers["time"], layers["clip"], layers["weight"] = 0.125 + 0.25 * np.arange(layers.size), np.arange(layers.size) % 2, 0.75
        slots = np.zeros(BUF_BYTES // 24, A.SLOT_DTYPE)
        slots["clip"] = A.LAYER_OFF
        for (sk, j), fields in a["state"].items():
            for f, v in fields.items():
                slots[sk * a["layer_count"] + j][f] = v
        pflags = np.zeros(BUF_BYTES // 4, np.uint32)
        for sk, v in a["pflag"].items():
            pflags[sk] = v
        motion = np.tile(np.array([0.0, 0.0, 0.0, 1.0, 0.1, 0.2, 0.3, 1.0, 1.0, 1.0], np.float32), BUF_BYTES // 40)
        inputs = dict(layers=layers, slots=slots, pflags=pflags, cmds=np.zeros(BUF_BYTES // 24, A.CMD_DTYPE), rest=np.tile(REST_BONE, BUF_BYTES // 40),
                      time=0.3 * np.arange(n), time_prev=0.3 * np.arange(n) - 0.05, clip_index=(np.arange(2 * n) % 2).astype(np.int32), motion=motion,
                      skeleton_global=np.tile(np.array([1, 0, 0, 0, 1, 0, 0, 0, 1, 2, 3, 4], np.float32), BUF_BYTES // 48))
        for name in POINTERS + ("rest",):
            content = np.full(BUF_BYTES, 0 if name in inputs else UNWRITTEN, np.uint8)
            if name in inputs:
                content[:inputs[name].nbytes] = np.frombuffer(inputs[name].tobytes(), np.uint8)
            keep, self.addr[name] = alloc(content)
            self.keep.append(keep)

    def p(self, key):
        v = self.a[key]
        if v is None:
            return None
        name, _, off = v.partition("+")
        return self.addr[name] + int(off or 0)

    def set_args(self, shaped=False):
        """(bone_count, rest_pose, clip_count, clips[, shapes], libm_variant)."""
        a = self.a
        descs, keep = (None, None) if a["clips"] is None else A._descs(a["clips"])
        self.keep.append(keep)
        args = [a["bone_count"], self.p("rest"), len(a["clips"]) if a["clip_count"] is None else a["clip_count"], descs]
        if shaped:
            args.append(self.shapes())
        return args + [a["libm"]]

    def shapes(self):
        s = self.a["shapes"]
        if s is None:
            return None
        sh, keep = A._shape_descs(s["shape_count"], self.a["clips"], s["init"])
        if s["struct_size"] is not None:
            sh.struct_size = s["struct_size"]
        if not s["clips"]:
            sh.clips = None
        self.keep += [keep, sh]
        return C.byref(sh)

    def playback_desc(self):
        d = self.a["desc"]
        if d is None:
            return None
        nx = None if d.get("next") is None else np.asarray(d["next"], np.int32)
        bt = None if d.get("blend_times") is None else np.asarray(d["blend_times"], np.float32)
        desc = _lib.MbikPlaybackDesc()
        desc.struct_size = d.get("struct_size", C.sizeof(_lib.MbikPlaybackDesc))
        desc.default_blend_time = d.get("default_blend_time", 0.0)
        desc.next = None if nx is None else nx.ctypes.data
        desc.blend_times = None if bt is None else bt.ctypes.data
        self.keep += [nx, bt, desc]
        return C.byref(desc)


def _create(L, c, shaped):
    h = C.c_void_p()
    f = L.mbik_clipset_create_shaped if shaped else L.mbik_clipset_create
    rc = f(*c.set_args(shaped), 0, C.byref(h) if c.a["out"] else None)
    assert rc != _lib.MBIK_OK and not h.value, "a ledger case made a set"
    return rc


def _playback_create(L, c):
    h = C.c_void_p()
    rc = L.mbik_playback_create(c.a["handle"], c.a["capacity"], c.a["layer_count"], c.playback_desc(), C.byref(h) if c.a["out"] else None)
    assert rc != _lib.MBIK_OK and not h.value, "a ledger case made a playback object"
    return rc


# entry name -> the call, from (library, Call); a device entry takes its handle and its stream (none) from the arguments
ENTRIES = {
    "clipset_create": lambda L, c: _create(L, c, False),
    "clipset_create_shaped": lambda L, c: _create(L, c, True),
    "sample": lambda L, c: L.mbik_clip_sample(c.a["handle"], c.a["count"], c.p("time"), c.p("clip_index"), c.a["clip"], c.p("pose_out"), None),
    "sample_cpu": lambda L, c: L.mbik_clip_sample_cpu(*c.set_args(), c.a["count"], c.p("time"), c.p("clip_index"), c.a["clip"], c.p("pose_out")),
    "sample_layers": lambda L, c: L.mbik_clip_sample_layers(c.a["handle"], c.a["count"], c.a["layer_count"], c.p("layers"), c.a["flags"],
                                                            c.p("pose_out"), None),
    "sample_layers_cpu": lambda L, c: L.mbik_clip_sample_layers_cpu(*c.set_args(), c.a["count"], c.a["layer_count"], c.p("layers"),
                                                                    c.a["flags"], c.p("pose_out")),
    "sample_shapes": lambda L, c: L.mbik_clip_sample_shapes(c.a["handle"], c.a["count"], c.p("time"), c.p("clip_index"), c.a["clip"],
                                                            c.p("weights_out"), None),
    "sample_shapes_cpu": lambda L, c: L.mbik_clip_sample_shapes_cpu(*c.set_args(True), c.a["count"], c.p("time"), c.p("clip_index"),
                                                                    c.a["clip"], c.p("weights_out")),
    "sample_shapes_layers": lambda L, c: L.mbik_clip_sample_shapes_layers(c.a["handle"], c.a["count"], c.a["layer_count"], c.p("layers"),
                                                                          c.a["flags"], c.p("weights_out"), None),
    "sample_shapes_layers_cpu": lambda L, c: L.mbik_clip_sample_shapes_layers_cpu(*c.set_args(True), c.a["count"], c.a["layer_count"],
                                                                                  c.p("layers"), c.a["flags"], c.p("weights_out")),
    "root_motion": lambda L, c: L.mbik_clip_root_motion(c.a["handle"], c.a["count"], c.a["root_bone"], c.p("time_prev"), c.p("time"),
                                                        c.p("clip_index"), c.a["clip"], c.p("motion_out"), c.p("pose"), None),
    "root_motion_cpu": lambda L, c: L.mbik_clip_root_motion_cpu(*c.set_args(), c.a["count"], c.a["root_bone"], c.p("time_prev"), c.p("time"),
                                                                c.p("clip_index"), c.a["clip"], c.p("motion_out"), c.p("pose")),
    "root_motion_layers": lambda L, c: L.mbik_clip_root_motion_layers(c.a["handle"], c.a["count"], c.a["layer_count"], c.a["root_bone"],
                                                                      c.p("layers"), c.p("time_prev"), c.a["flags"], c.p("motion_out"),
                                                                      c.p("pose"), None),
    "root_motion_layers_cpu": lambda L, c: L.mbik_clip_root_motion_layers_cpu(*c.set_args(), c.a["count"], c.a["layer_count"],
                                                                              c.a["root_bone"], c.p("layers"), c.p("time_prev"), c.a["flags"],
                                                                              c.p("motion_out"), c.p("pose")),
    "root_apply": lambda L, c: L.mbik_root_motion_apply(c.a["handle"], c.a["count"], c.p("motion"), c.a["flags"], c.p("skeleton_global"), None),
    "root_apply_cpu": lambda L, c: L.mbik_root_motion_apply_cpu(c.a["count"], c.p("motion"), c.a["flags"], c.p("skeleton_global")),
    "playback_create": _playback_create,
    "playback_write": lambda L, c: L.mbik_playback_write(c.a["handle"], c.a["first"], c.a["n"], c.p("slots"), c.p("pflags")),
    "playback_read": lambda L, c: L.mbik_playback_read(c.a["handle"], c.a["first"], c.a["n"], c.p("slots"), c.p("pflags")),
    "advance": lambda L, c: L.mbik_playback_advance(c.a["handle"], c.a["count"], c.a["delta"], c.a["speed_scale"], c.p("cmds"),
                                                    c.a["cmd_count"], c.p("layers_out"), c.p("time_prev_out"), c.p("events_out"), None),
    "advance_cpu": lambda L, c: L.mbik_playback_advance_cpu(
        len(c.a["clips"]) if c.a["clip_count"] is None else c.a["clip_count"], c.set_args()[3], c.playback_desc(), c.a["count"],
        c.a["layer_count"], c.p("slots"), c.p("pflags"), c.a["delta"], c.a["speed_scale"], c.p("cmds"), c.a["cmd_count"], c.p("layers_out"),
        c.p("time_prev_out"), c.p("events_out")),
}
POSE_CPU = ("sample_cpu", "sample_layers_cpu", "root_motion_cpu", "root_motion_layers_cpu")
SHAPE_CPU = ("sample_shapes_cpu", "sample_shapes_layers_cpu")
NAN, INF = float("nan"), float("inf")

# ---- what a set is made from: (entry, name, changes) -------------------------------------------------------------------------
_BAD_POSE_SETS = {
    "negative bone_count": {"bone_count": -1},
    "negative clip_count": {"clip_count": -1},
    "null rest_pose": {"rest": None},
    "no clips": {"clips": []},
    "null clips": {"clips": None, "clip_count": 1},
    "unknown libm_variant": {"libm": 2},
    "too many headers": {"bone_count": 2**30},
    "zero length": {"clips.0.length": 0.0},
    "nan length": {"clips.1.length": NAN},
    "unknown loop_mode": {"clips.1.loop_mode": 2},
    "negative track_count": {"clips.1.track_count": -1},
    "null tracks": {"clips.1.track_count": 1},
    "bone outside": {"clips.0.tracks": [_tr(bone=B)]},
    "unknown channel": {"clips.0.tracks": [_tr(channel=3, key_count=3)]},
    "unknown interpolation": {"clips.0.tracks": [_tr(), _tr(bone=1, interpolation=2)]},
    "negative key_count": {"clips.0.tracks": [_tr(key_count=-1)]},
    "null times": {"clips.0.tracks": [_tr(times=None, key_count=3)]},
    "null values": {"clips.0.tracks": [_tr(values=None, key_count=3)]},
    "second track": {"clips.0.tracks": [_tr(), _tr(key_count=0), _tr()]},
    "key time past length": {"clips.0.tracks": [_tr(times=[0.0, 0.5, 1.5])]},
    "key time negative": {"clips.0.tracks": [_tr(times=[-0.5, 0.5, 1.0])]},
    "key time nan": {"clips.0.tracks": [_tr(times=[0.0, NAN, 1.0])]},
    "key times equal": {"clips.0.tracks": [_tr(times=[0.0, 0.5, 0.5])]},
    # two faults: the clip's own before its tracks', an earlier track's before a later one's
    "zero length and a bad track": {"clips.0.length": 0.0, "clips.0.tracks": [_tr(bone=B)]},
    "bad bone and bad channel": {"clips.0.tracks": [_tr(bone=-1, channel=7, key_count=3)]},
    "bad interpolation before null times": {"clips.0.tracks": [_tr(interpolation=-1, times=None, key_count=3)]},
    "unordered and outside": {"clips.0.tracks": [_tr(times=[0.5, 0.25, 7.0])]},
}
_BAD_SHAPE_SETS = {
    "null shapes": {"shapes": None},
    "small struct_size": {"shapes.struct_size": 8},
    "zero shape_count": {"shapes.shape_count": 0},
    "null shapes clips": {"shapes.clips": False},
    "too many shape headers": {"shapes.shape_count": INT32_MAX, "clips.0.shape_tracks": []},
    "negative shape track_count": {"clips.1.shape_track_count": -1},
    "null shape tracks": {"clips.1.shape_track_count": 1},
    "shape outside": {"clips.0.shape_tracks": [_st(shape=P)]},
    "unknown shape interpolation": {"clips.0.shape_tracks": [_st(interpolation=2)]},
    "negative shape key_count": {"clips.0.shape_tracks": [_st(key_count=-1)]},
    "null shape times": {"clips.0.shape_tracks": [_st(times=None, key_count=3)]},
    "null shape values": {"clips.0.shape_tracks": [_st(values=None, key_count=3)]},
    "second shape track": {"clips.0.shape_tracks": [_st(), _st()]},
    "shape key time past length": {"clips.0.shape_tracks": [_st(times=[0.0, 0.5, 1.5])]},
    "shape key times equal": {"clips.0.shape_tracks": [_st(times=[0.0, 0.0, 1.0])]},
    # two faults: the pose tracks' before the shapes'
    "bad pose track and null shapes": {"clips.0.tracks": [_tr(channel=3, key_count=3)], "shapes": None},
    "small struct_size and zero shape_count": {"shapes.struct_size": 8, "shapes.shape_count": 0},
}
_BAD_PLAYBACK = {
    "no clips": {"clips": []},
    "null clips": {"clips": None, "clip_count": 1},
    "zero length": {"clips.1.length": 0.0},
    "unknown loop_mode": {"clips.0.loop_mode": -1},
    "small desc": {"desc": dict(struct_size=8)},
    "negative default_blend_time": {"desc": dict(default_blend_time=-1.0)},
    "nan default_blend_time": {"desc": dict(default_blend_time=NAN)},
    "next outside": {"desc": dict(next=[1, 2])},
    "next below -1": {"desc": dict(next=[-2, 0])},
    "negative blend_times": {"desc": dict(blend_times=[[0.0, 0.0], [-1.0, 0.0]])},
    "inf blend_times": {"desc": dict(blend_times=[[0.0, INF], [0.0, 0.0]])},
    "unknown flag bits": {"pflag": {1: 4}},
    "slot clip outside": {"state": {(0, 0): dict(clip=2)}},
    "on slot behind off slot": {"state": {(2, 1): dict(clip=0, blend_time=1.0)}},
    "pos outside": {"state": {(0, 0): dict(clip=0, pos=1.5)}},
    "speed not finite": {"state": {(0, 0): dict(clip=0, speed=INF)}},
    "fade without blend_time": {"state": {(0, 0): dict(clip=0), (0, 1): dict(clip=1)}},
    # two faults: the clips before the desc, the desc before the count, the state before the call
    "bad clip and bad desc": {"clips.0.length": -1.0, "desc": dict(struct_size=8)},
    "bad desc and negative count": {"desc": dict(next=[5, 0]), "count": -1},
    "negative count and bad layer_count": {"count": -1, "layer_count": 9},
    "bad layer_count and null slots": {"layer_count": 0, "slots": None},
    "null flags": {"pflags": None},
    "bad state and bad delta": {"pflag": {0: 8}, "delta": NAN},
}
SET_CASES = (
    [(e, n, ch) for e in ("clipset_create", "sample_cpu") for n, ch in _BAD_POSE_SETS.items()]
    + [(e, n, ch) for e in ("clipset_create_shaped", "sample_shapes_cpu") for n, ch in _BAD_SHAPE_SETS.items()]
    + [(e, "zero length", {"clips.0.length": 0.0}) for e in POSE_CPU[1:] + SHAPE_CPU[1:]]
    + [("advance_cpu", n, ch) for n, ch in _BAD_PLAYBACK.items()]
    + [("clipset_create", "null out", {"out": False}), ("clipset_create_shaped", "null out", {"out": False}),
       ("clipset_create", "null out and a bad set", {"out": False, "clips": []}),
       ("playback_create", "null out", {"out": False}), ("playback_create", "null clip set", {}),
       ("playback_create", "null clip set and bad layer_count", {"layer_count": 0, "capacity": -1})]
    # a bad set with bad call arguments: the set's refusal comes first
    + [(e, "bad set and bad call", {"clips.0.length": 0.0, "count": -1, "layer_count": 0, "flags": 2, "root_bone": -1}) for e in POSE_CPU + SHAPE_CPU]
    # B == 0: the pose forms have nothing to do before they look at a pointer; the shape forms have no such exit
    + [(e, "no bones and no pointers", {"bone_count": 0, "clips.0.tracks": [], **NO_POINTERS, "rest": "rest"}) for e in POSE_CPU + SHAPE_CPU]
)

# ---- the arguments of a call on a good set: (entry of the _cpu form, name, changes) -------------------------------------------
_LAYERED = {
    "negative count": {"count": -1},
    "layer_count 0": {"layer_count": 0},
    "layer_count 9": {"layer_count": 9},
    "unknown flags": {"flags": 2},
    "null layers": {"layers": None},
    "layers misaligned": {"layers": "layers+4"},
    "negative count and bad layer_count": {"count": -1, "layer_count": 0},
    "bad layer_count and bad flags": {"layer_count": 9, "flags": 4},
    "bad flags and null layers": {"flags": 2, "layers": None},
    "count 0 and no pointers": {"count": 0, **NO_POINTERS},
    "count 0 and bad flags": {"count": 0, "flags": 2, **NO_POINTERS},
}
_PLAIN = {
    "negative count": {"count": -1},
    "null time": {"time": None},
    "clip -1": {"clip": -1},
    "clip 2": {"clip": 2},
    "clip unused with an index": {"clip": 7, "clip_index": "clip_index"},
    "count 0 and no pointers": {"count": 0, **NO_POINTERS},
}
_ROOT = {
    "root_bone -1": {"root_bone": -1},
    "root_bone B": {"root_bone": B},
    "null time_prev": {"time_prev": None},
    "null motion_out": {"motion_out": None},
    "time_prev misaligned": {"time_prev": "time_prev+4"},
    "motion_out overlaps time_prev": {"motion_out": "time_prev"},
    "motion_out overlaps pose": {"pose": "motion_out"},
    "negative count and bad root_bone": {"count": -1, "root_bone": B},
    "null time_prev and null motion_out": {"time_prev": None, "motion_out": None},
    "count 0 and bad root_bone": {"count": 0, "root_bone": -1, **NO_POINTERS},
}
CALL_CASES = (
    [("sample_cpu", n, ch) for n, ch in _PLAIN.items()]
    + [("sample_cpu", "null pose_out", {"pose_out": None}), ("sample_cpu", "null time and null pose_out", {"time": None, "pose_out": None}),
       ("sample_cpu", "null pose_out and bad clip", {"pose_out": None, "clip": 2}),
       # (mbik.h promises no overlap test for pose_out of the plain form)
       ("sample_cpu", "count 0 and bad clip", {"count": 0, "clip": 2})]
    + [("sample_layers_cpu", n, ch) for n, ch in _LAYERED.items()]
    + [("sample_layers_cpu", "null pose_out", {"pose_out": None}), ("sample_layers_cpu", "pose_out overlaps layers", {"pose_out": "layers"}),
       ("sample_layers_cpu", "null layers and null pose_out", {"layers": None, "pose_out": None}),
       ("sample_layers_cpu", "null pose_out and layers misaligned", {"pose_out": None, "layers": "layers+4"})]
    + [("sample_shapes_cpu", n, ch) for n, ch in _PLAIN.items()]
    + [("sample_shapes_cpu", "null weights_out", {"weights_out": None}), ("sample_shapes_cpu", "weights_out overlaps time", {"weights_out": "time"}),
       ("sample_shapes_cpu", "weights_out overlaps clip_index", {"clip_index": "clip_index", "weights_out": "clip_index"}),
       ("sample_shapes_cpu", "bad clip and overlap", {"clip": 2, "weights_out": "time"}),
       ("sample_shapes_cpu", "count 0 and bad clip", {"count": 0, "clip": 2})]
    + [("sample_shapes_layers_cpu", n, ch) for n, ch in _LAYERED.items()]
    + [("sample_shapes_layers_cpu", "null weights_out", {"weights_out": None}),
       ("sample_shapes_layers_cpu", "weights_out overlaps layers", {"weights_out": "layers"}),
       ("sample_shapes_layers_cpu", "null weights_out and layers misaligned", {"weights_out": None, "layers": "layers+4"})]
    + [("root_motion_cpu", n, ch) for n, ch in {**_PLAIN, **_ROOT}.items()]
    + [("root_motion_cpu", "time misaligned", {"time": "time+4"}), ("root_motion_cpu", "motion_out overlaps time", {"motion_out": "time"}),
       ("root_motion_cpu", "motion_out overlaps clip_index", {"clip_index": "clip_index", "motion_out": "clip_index"}),
       ("root_motion_cpu", "bad root_bone and bad clip", {"root_bone": B, "clip": 2}),
       ("root_motion_cpu", "count 0 and bad clip", {"count": 0, "clip": 2, **NO_POINTERS}),
       ("root_motion_cpu", "null time_prev and time misaligned", {"time_prev": None, "time": "time+4"})]
    + [("root_motion_layers_cpu", n, ch) for n, ch in {**_LAYERED, **_ROOT}.items()]
    + [("root_motion_layers_cpu", "motion_out overlaps layers", {"motion_out": "layers"}),
       ("root_motion_layers_cpu", "bad root_bone and bad layer_count", {"root_bone": B, "layer_count": 0}),
       ("root_motion_layers_cpu", "null time_prev and layers misaligned", {"time_prev": None, "layers": "layers+4"}),
       ("root_motion_layers_cpu", "layers misaligned and time_prev misaligned", {"layers": "layers+4", "time_prev": "time_prev+4"})]
    + [("root_apply_cpu", n, ch) for n, ch in {
        "negative count": {"count": -1}, "unknown flags": {"flags": 2}, "null motion": {"motion": None},
        "null skeleton_global": {"skeleton_global": None}, "skeleton_global overlaps motion": {"skeleton_global": "motion"},
        "negative count and bad flags": {"count": -1, "flags": 2}, "bad flags and null motion": {"flags": 2, "motion": None},
        "count 0 and no pointers": {"count": 0, **NO_POINTERS}}.items()]
    + [("advance_cpu", n, ch) for n, ch in {
        "nan delta": {"delta": NAN}, "inf speed_scale": {"speed_scale": INF}, "negative cmd_count": {"cmd_count": -1},
        "null layers_out": {"layers_out": None}, "null time_prev_out": {"time_prev_out": None}, "null cmds": {"cmd_count": 1},
        "layers_out misaligned": {"layers_out": "layers_out+4"}, "time_prev_out misaligned": {"time_prev_out": "time_prev_out+4"},
        "cmds misaligned": {"cmds": "cmds+4", "cmd_count": 1}, "cmds unused without a count": {"cmds": "cmds+4"},
        "time_prev_out overlaps layers_out": {"time_prev_out": "layers_out"}, "events_out overlaps layers_out": {"events_out": "layers_out"},
        "events_out overlaps time_prev_out": {"events_out": "time_prev_out"}, "layers_out overlaps cmds": {"cmds": "layers_out", "cmd_count": 1},
        "time_prev_out overlaps cmds": {"cmds": "time_prev_out", "cmd_count": 1}, "events_out overlaps cmds": {"cmds": "events_out", "cmd_count": 1},
        "no events_out": {"events_out": None},
        "bad delta and bad speed_scale": {"delta": INF, "speed_scale": NAN}, "bad cmd_count and null layers_out": {"cmd_count": -1, "layers_out": None},
        "null layers_out and misaligned time_prev_out": {"layers_out": None, "time_prev_out": "time_prev_out+4"},
        "count 0 and no pointers": {"count": 0, **NO_POINTERS}, "count 0 and bad delta": {"count": 0, "delta": NAN, **NO_POINTERS}}.items()]
)
# the device entries with a null handle: their first refusal, whatever else is wrong
NULL_HANDLE_CASES = [(e, "null handle", {"count": -1, "n": -1}) for e in
                     ("sample", "sample_layers", "sample_shapes", "sample_shapes_layers", "root_motion", "root_motion_layers", "root_apply",
                      "advance", "playback_write", "playback_read")]
CASES = SET_CASES + CALL_CASES + NULL_HANDLE_CASES


def case_id(case):
    return f"{case[0]}: {case[1]}"


def run_case(L, entry, changes, alloc=host_alloc):
    """(return code, text) of one call; the text of a call that succeeds is empty."""
    call = Call(changes, alloc)
    rc = ENTRIES[entry](L, call)
    return [rc, _lib.last_error() if rc < 0 else ""]


def record(L):
    """Every case's outcome, as the golden file holds it."""
    return {case_id(c): run_case(L, c[0], c[2]) for c in CASES}


@pytest.fixture(scope="module")
def golden():
    with open(GOLDEN) as fh:
        return json.load(fh)


def test_the_table_and_the_golden_file_name_the_same_cases(golden):
    ids = [case_id(c) for c in CASES]
    assert len(set(ids)) == len(ids)
    assert sorted(ids) == sorted(golden)


@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_refusal_code_and_text(mbik, golden, case):
    assert run_case(mbik, case[0], case[2]) == golden[case_id(case)]


def test_every_reachable_text_is_covered(golden):
    """The ledger holds each refusal family of the two host files at least once (by a word of its text)."""
    texts = " | ".join(t for _, t in golden.values())
    for word in ("negative count", "null rest_pose", "at least one clip", "null clips", "libm_variant", "(clip, bone, channel) headers",
                 "length must be", "loop_mode", "negative track_count", "null tracks", "bone 2 outside", "unknown channel", "unknown interpolation",
                 "negative key_count", "null times or values", "a second track with keys for bone", "not finite or outside", "strictly increasing",
                 "null time", "null pose_out", "outside the set's", "layer_count 0 outside", "unknown flags", "null layers", "layers is not 8-byte",
                 "pose_out overlaps layers", "root_bone", "null time_prev", "null motion_out", "time is not 8-byte", "time_prev is not 8-byte",
                 "motion_out overlaps layers", "motion_out overlaps time", "motion_out overlaps time_prev", "motion_out overlaps clip_index",
                 "motion_out overlaps pose", "null motion", "null skeleton_global", "skeleton_global overlaps motion", "null shapes",
                 "shapes->struct_size", "shape_count must", "null shapes->clips", "(clip, shape) headers", "negative shape track_count",
                 "null shape tracks", "shape 1 outside", "for shape 0", "null weights_out", "weights_out overlaps time",
                 "weights_out overlaps clip_index", "weights_out overlaps layers", "null out", "null clip set", "null playback object",
                 "mbik_playback_desc.struct_size", "default_blend_time", "next[0]", "blend_times[1][0]", "unknown flag bits", "slot 0: clip 2",
                 "behind an off slot", "pos is not finite", "speed is not finite", "a fade needs", "delta is not finite",
                 "speed_scale is not finite", "negative cmd_count", "null layers_out", "null time_prev_out", "null cmds",
                 "layers_out is not 8-byte", "time_prev_out is not 8-byte", "cmds is not 8-byte", "time_prev_out overlaps layers_out",
                 "events_out overlaps layers_out", "events_out overlaps time_prev_out", "layers_out overlaps cmds", "time_prev_out overlaps cmds",
                 "events_out overlaps cmds", "null slots or flags"):
        assert word in texts, word


if __name__ == "__main__":
    with open(GOLDEN, "w") as fh:
        json.dump(record(_lib.load()), fh, indent=1, sort_keys=True)
        fh.write("\n")
