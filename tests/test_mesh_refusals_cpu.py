"""The refusal ledger of the mesh front end (mesh creation, skinning, bounds, culling, LOD lists).

Every way these entries refuse a call without needing a device, as (return code, exact text of
mbik_last_error(), the buffers the call wrote), pinned in tests/golden/mesh_refusals.json, in the shape
tests/test_animation_refusals_cpu.py gives its ledger and with its helpers.  A case is a named set of
changes to one valid call through the raw ctypes entries: B = 2, V = 3, K = 4, normals and tangents, P = 1
relative shape with normals and tangents, count = 4, max_list = 4, list_count = 2, one plane, two LOD
ranges.  Calls with two faults pin which refusal comes first; the empty calls pin that they succeed and
write nothing (every output buffer is filled with 0xA5), or zero their counts and nothing else.

MESH_CASES change what a mesh is made from, CALL_CASES the arguments of a call on a good one;
tests/test_gpu_mesh_refusals.py runs the latter through the device entries as well.  The old entries and
the struct call reach the same checks by different routes, so each entry has its own cases.
`python -m tests.test_mesh_refusals_cpu` records the golden file anew from the library in the tree
(MBIK_LIB_OVERRIDE: from another one).
"""
import ctypes as C
import json
import os

import numpy as np
import pytest

from many_bone_ik_amd import _lib

from .test_animation_refusals_cpu import BUF_BYTES, UNWRITTEN, _set, host_alloc

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "mesh_refusals.json")
B, V, K, P, COUNT, MAX_LIST, LIST_COUNT, PLANES, RANGES = 2, 3, 4, 1, 4, 4, 2, 1, 2
NAN, INF = float("nan"), float("inf")

INPUTS = ("positions", "normals", "tangents", "bone_indices", "weights", "shape_positions", "shape_normals", "shape_tangents", "skin",
          "shape_weights", "indices", "list_count", "bone_boxes", "used", "boxes", "skeleton_global", "planes", "camera", "ranges", "state")
OUTPUTS = ("out_positions", "out_normals", "out_tangents", "boxes_out", "used_out", "visible", "cull_indices", "visible_count", "level",
           "lod_indices", "list_counts")
CALL_POINTERS = ("skin", "shape_weights", "indices", "list_count", "out_positions", "out_normals", "out_tangents")


def default_args():
    """One valid call of every entry: scalars, the structs' own fields, and for each pointer the name of a
    buffer (None: a null pointer; "name+4": four bytes in; another argument's name: an alias)."""
    a = dict(bone_count=B, vertex_count=V, influences=K, bad_index=None, handle=None, out=True, desc={}, call={},
             shapes=dict(struct_size=None, shape_count=P, mode=0, positions="shape_positions", normals="shape_normals"),
             count=COUNT, max_list=MAX_LIST, flags=0, margin=0.25, plane_count=PLANES, range_count=RANGES, lod_flags=0,
             camera_data=[0.5, 0.0, -1.0], ranges_data=[[0.0, 2.0, 0.1, 0.2], [2.0, 0.0, 0.2, 0.0]])
    a.update({name: name for name in INPUTS + OUTPUTS})
    return a


def _contents(a):
    k = a["influences"] if a["influences"] in (4, 8) else 4
    idx = (np.arange(V)[:, None] + np.arange(k)[None, :]).astype(np.int32) % B
    if a["bad_index"]:
        v, s, value = a["bad_index"]
        idx[v, s] = value
    unit = np.array([[1, 0, 0], [0, 1, 0], [0.6, 0.8, 0]], np.float32)
    skin = np.tile(np.array([1, 0, 0, 0, 0, 1, 0, -1, 0, 0.5, 0.25, -0.5], np.float32), (COUNT, B, 1))
    skin[:, :, 9] += 0.5 * np.arange(COUNT, dtype=np.float32)[:, None]
    boxes = np.tile(np.array([-0.5, -0.5, -0.5, 1, 1, 1], np.float32), (COUNT, 1))
    boxes[:, 0] += 1.5 * np.arange(COUNT, dtype=np.float32)
    return dict(
        positions=np.array([[0, 0, 0], [1, 0.5, 0], [0.25, 1, -1]], np.float32), normals=unit,
        tangents=np.array([[0, 1, 0, 1], [0, 0, 1, -1], [0, 0, 1, 1]], np.float32), bone_indices=idx,
        weights=np.full((V, k), 1.0 / k, np.float32), shape_positions=np.full((P, V, 3), 0.125, np.float32),
        shape_normals=np.full((P, V, 3), 0.0625, np.float32), shape_tangents=np.full((P, V, 3), 0.03125, np.float32), skin=skin,
        shape_weights=np.linspace(0.0, 1.0, COUNT * P, dtype=np.float32), indices=np.array([1, 3, 0, 2], np.int32),
        list_count=np.array([LIST_COUNT], np.int32), bone_boxes=np.tile(np.array([-1, -1, -1, 2, 2, 2], np.float32), (B, 1)),
        used=np.ones(B, np.uint8), boxes=boxes, skeleton_global=np.tile(np.array([1, 0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0.5], np.float32), (COUNT, 1)),
        planes=np.array([[1, 0, 0, 2.0]], np.float32), camera=np.asarray(a["camera_data"], np.float32),
        ranges=np.asarray(a["ranges_data"], np.float32), state=np.zeros(COUNT, np.uint8))


class Call:
    """The arguments of one call, marshalled: buffers allocated through `alloc`, structs built."""

    def __init__(self, overrides, alloc=host_alloc):
        a = default_args()
        for path, value in overrides.items():
            _set(a, path, value)
        self.a, self.keep, self.addr, self.initial = a, [], {}, {}
        inputs = _contents(a)
        for name in INPUTS + OUTPUTS:
            content = np.full(BUF_BYTES, 0 if name in inputs else UNWRITTEN, np.uint8)
            if name in inputs:
                content[:inputs[name].nbytes] = np.frombuffer(inputs[name].tobytes(), np.uint8)
            keep, self.addr[name] = alloc(content)
            self.keep.append(keep)
            self.initial[name] = content

    def at(self, v):
        if v is None:
            return None
        name, _, off = v.partition("+")
        return self.addr[name] + int(off or 0)

    def p(self, key):
        return self.at(self.a[key])

    def mesh_args(self):
        a = self.a
        return [a["bone_count"], a["vertex_count"], a["influences"], self.p("positions"), self.p("normals"), self.p("bone_indices"),
                self.p("weights")]

    def shapes(self):
        s = self.a["shapes"]
        if s is None:
            return None
        sh = _lib.MbikMeshShapes(C.sizeof(_lib.MbikMeshShapes) if s["struct_size"] is None else s["struct_size"], s["shape_count"], s["mode"],
                                 self.at(s["positions"]), self.at(s["normals"]))
        self.keep.append(sh)
        return C.pointer(sh)

    def desc(self):
        a, d = self.a, self.a["desc"]
        if d is None:
            return None
        desc = _lib.MbikMeshDesc(d.get("struct_size", C.sizeof(_lib.MbikMeshDesc)), a["bone_count"], a["vertex_count"], a["influences"],
                                 self.p("positions"), self.p("normals"), self.p("tangents"), self.p("bone_indices"), self.p("weights"),
                                 self.shapes(), self.p("shape_tangents"))
        self.keep.append(desc)
        return C.byref(desc)

    def call(self):
        a, c = self.a, self.a["call"]
        if c is None:
            return None
        call = _lib.MbikSkinCall(c.get("struct_size", C.sizeof(_lib.MbikSkinCall)), a["count"], self.p("skin"), self.p("shape_weights"),
                                 self.p("indices"), self.p("list_count"), a["max_list"], a["flags"], self.p("out_positions"),
                                 self.p("out_normals"), self.p("out_tangents"))
        self.keep.append(call)
        return C.byref(call)

    def cull_args(self):
        a = self.a
        return [a["count"], self.p("boxes"), self.p("skeleton_global"), a["margin"], a["plane_count"], self.p("planes")]

    def lod_args(self):
        a = self.a
        return self.cull_args() + [self.p("camera"), a["range_count"], self.p("ranges"), a["lod_flags"], self.p("state"), self.p("level"),
                                       self.p("lod_indices"), self.p("list_counts")]


def _create(L, c, form):
    h = C.c_void_p()
    out = C.byref(h) if c.a["out"] else None
    if form == "desc":
        rc = L.mbik_mesh_create_desc(c.desc(), 0, out)
    elif form == "shaped":
        rc = L.mbik_mesh_create_shaped(*c.mesh_args(), c.shapes(), 0, out)
    else:
        rc = L.mbik_mesh_create(*c.mesh_args(), 0, out)
    assert rc != _lib.MBIK_OK and not h.value, "a ledger case made a mesh"
    return rc


PLAIN_FORM = {"shape_weights": None, "indices": None, "list_count": None}
SHAPED_FORM = {"indices": None, "list_count": None}
_skin_ptrs = lambda c: [c.p("skin"), c.p("out_positions"), c.p("out_normals")]   # noqa: E731
_shaped_ptrs = lambda c: [c.p("skin"), c.p("shape_weights"), c.p("out_positions"), c.p("out_normals")]   # noqa: E731
_listed_args = lambda c: [c.a["count"], c.p("indices"), c.p("list_count"), c.a["max_list"], c.p("skin"), c.p("shape_weights"), c.a["flags"],   # noqa: E731
                          c.p("out_positions"), c.p("out_normals")]
_cull_outs = lambda c: [c.p("visible"), c.p("cull_indices"), c.p("visible_count")]   # noqa: E731
# entry name -> (the call, from (library, Call); the changes that make the valid call this entry's form)
ENTRIES = {
    "create": (lambda L, c: _create(L, c, "plain"), {}),
    "create_shaped": (lambda L, c: _create(L, c, "shaped"), {}),
    "create_desc": (lambda L, c: _create(L, c, "desc"), {}),
    "skin_cpu": (lambda L, c: L.mbik_skin_vertices_cpu(*c.mesh_args(), c.a["count"], *_skin_ptrs(c)), {}),
    "shaped_cpu": (lambda L, c: L.mbik_skin_vertices_shaped_cpu(*c.mesh_args(), c.shapes(), c.a["count"], *_shaped_ptrs(c)), {}),
    "listed_cpu": (lambda L, c: L.mbik_skin_vertices_listed_cpu(*c.mesh_args(), c.shapes(), *_listed_args(c)), {}),
    "call_plain_cpu": (lambda L, c: L.mbik_skin_vertices_call_cpu(c.desc(), c.call()), PLAIN_FORM),
    "call_shaped_cpu": (lambda L, c: L.mbik_skin_vertices_call_cpu(c.desc(), c.call()), SHAPED_FORM),
    "call_listed_cpu": (lambda L, c: L.mbik_skin_vertices_call_cpu(c.desc(), c.call()), {}),
    "bone_boxes_cpu": (lambda L, c: L.mbik_bone_boxes_cpu(*c.mesh_args()[:4], *c.mesh_args()[5:], c.p("boxes_out"), c.p("used_out")), {}),
    "bounds_cpu": (lambda L, c: L.mbik_skin_bounds_cpu(c.a["bone_count"], c.p("bone_boxes"), c.p("used"), c.a["count"], c.p("skin"),
                                                       c.p("boxes_out")), {}),
    "cull_cpu": (lambda L, c: L.mbik_cull_boxes_cpu(*c.cull_args(), *_cull_outs(c)), {}),
    "lod_cpu": (lambda L, c: L.mbik_cull_lod_cpu(*c.lod_args()), {}),
    # the device entries: their handle and their stream (none) from the arguments
    "skin": (lambda L, c: L.mbik_skin_vertices(c.a["handle"], c.a["count"], *_skin_ptrs(c), None), {}),
    "shaped": (lambda L, c: L.mbik_skin_vertices_shaped(c.a["handle"], c.a["count"], *_shaped_ptrs(c), None), {}),
    "listed": (lambda L, c: L.mbik_skin_vertices_listed(c.a["handle"], *_listed_args(c), None), {}),
    "call_plain": (lambda L, c: L.mbik_skin_vertices_call(c.a["handle"], c.call(), None), PLAIN_FORM),
    "call_shaped": (lambda L, c: L.mbik_skin_vertices_call(c.a["handle"], c.call(), None), SHAPED_FORM),
    "call_listed": (lambda L, c: L.mbik_skin_vertices_call(c.a["handle"], c.call(), None), {}),
    "mesh_bone_boxes": (lambda L, c: L.mbik_mesh_bone_boxes(c.a["handle"], c.p("boxes_out"), c.p("used_out")), {}),
    "launch_shape": (lambda L, c: L.mbik_mesh_launch_shape(c.a["handle"], c.a["count"], None, None), {}),
    "bounds": (lambda L, c: L.mbik_skin_bounds(c.a["handle"], c.a["count"], c.p("skin"), c.p("boxes_out"), None), {}),
    "cull": (lambda L, c: L.mbik_cull_boxes(c.a["handle"], *c.cull_args(), *_cull_outs(c), None), {}),
    "lod": (lambda L, c: L.mbik_cull_lod(c.a["handle"], *c.lod_args(), None), {}),
}
OLD_CPU, CALL_CPU = ("skin_cpu", "shaped_cpu", "listed_cpu"), ("call_plain_cpu", "call_shaped_cpu", "call_listed_cpu")
SKIN_CPU = OLD_CPU + CALL_CPU
SHAPED_ENTRIES, LISTED_ENTRIES = ("shaped_cpu", "call_shaped_cpu"), ("listed_cpu", "call_listed_cpu")

# ---- what a mesh is made from -----------------------------------------------------------------------------------------------
_BAD_MESH = {
    "influences 5": {"influences": 5},
    "negative B": {"bone_count": -1},
    "negative V": {"vertex_count": -1},
    "null positions": {"positions": None},
    "null bone_indices": {"bone_indices": None},
    "null weights": {"weights": None},
    "bone index B": {"bad_index": (2, 1, B)},
    "bone index -1": {"bad_index": (0, 3, -1)},
    "eight influences, bone index B": {"influences": 8, "bad_index": (1, 7, B)},
    # two faults
    "bad influences and negative B": {"influences": 0, "bone_count": -1},
    "negative V and null positions": {"vertex_count": -1, "positions": None},
    "null weights and a bad index": {"weights": None, "bad_index": (0, 0, 7)},
    "two bad indices": {"bad_index": (1, 2, -5), "bone_count": 1},
}
_BAD_SHAPES = {
    "small shapes struct_size": {"shapes.struct_size": 8},
    "shape_count 0": {"shapes.shape_count": 0},
    "shape mode 2": {"shapes.mode": 2},
    "null shape positions": {"shapes.positions": None},
    "shape normals missing": {"shapes.normals": None},
    "shape normals without mesh normals": {"normals": None, "tangents": None, "shape_tangents": None, "out_normals": None, "out_tangents": None},
    "small shapes struct_size and shape_count 0": {"shapes.struct_size": 8, "shapes.shape_count": 0},
    "shape_count 0 and bad mode": {"shapes.shape_count": 0, "shapes.mode": -1},
    "bad mode and null shape positions": {"shapes.mode": 3, "shapes.positions": None},
    "null shape positions and normals mismatch": {"shapes.positions": None, "shapes.normals": None},
    "bad shapes and bad call": {"shapes.mode": 2, "count": -1, "flags": 2},
}
_BAD_TANGENTS = {
    "tangents without normals": {"normals": None, "shapes.normals": None, "out_normals": None, "out_tangents": None},
    "shape_tangents missing": {"shape_tangents": None},
    "shape_tangents without tangents": {"tangents": None, "out_tangents": None},
    "shape_tangents without shapes": {"shapes": None, "shape_weights": None},
    "null desc": {"desc": None},
    "small desc struct_size": {"desc.struct_size": 8},
    "small desc struct_size and a bad mesh": {"desc.struct_size": 8, "influences": 5},
    "bad shapes and a tangent mismatch": {"shapes.shape_count": 0, "shape_tangents": None},
    "tangent mismatch and a bad index": {"shape_tangents": None, "bad_index": (0, 0, B)},
    "tangents without normals and shape_tangents missing": {"normals": None, "shapes.normals": None, "shape_tangents": None},
}
_CREATE_ONLY = {
    "null out": {"out": False},
    "null out and a bad mesh": {"out": False, "influences": 5},
    "too many bones": {"bone_count": 4000},
    "negative V and too many bones": {"vertex_count": -1, "bone_count": 4000},
}
MESH_CASES = (
    [(e, n, ch) for e in ("create", "create_shaped", "create_desc", "bone_boxes_cpu") + SKIN_CPU for n, ch in _BAD_MESH.items()]
    + [(e, n, ch) for e in ("create", "create_shaped", "create_desc") for n, ch in _CREATE_ONLY.items()]
    + [(e, n, ch) for e in ("create_shaped", "create_desc", "shaped_cpu", "listed_cpu") + CALL_CPU for n, ch in _BAD_SHAPES.items()]
    + [(e, "null shapes", {"shapes": None}) for e in ("create_shaped", "shaped_cpu")]
    + [(e, "null shapes and a bad index", {"shapes": None, "bad_index": (0, 0, B)}) for e in ("create_shaped", "shaped_cpu")]
    + [(e, "bad index and bad shapes", {"shapes.shape_count": 0, "bad_index": (0, 0, B)}) for e in ("create_shaped", "create_desc", "shaped_cpu", "call_shaped_cpu")]
    + [(e, "shapes too large for the LDS", {"bone_count": 3000, "shapes.shape_count": 10000}) for e in ("create_shaped", "create_desc")]
    + [(e, n, ch) for e in ("create_desc",) + CALL_CPU for n, ch in _BAD_TANGENTS.items()]
    + [(e, "bad mesh and bad call", {"influences": 5, "count": -1, "flags": 2, "max_list": -1, "skin": None}) for e in SKIN_CPU]
)

# ---- the arguments of a call on a good mesh ---------------------------------------------------------------------------------
NO_NORMALS = {"normals": None, "shapes.normals": None, "tangents": None, "shape_tangents": None, "out_tangents": None}
NO_TANGENTS = {"tangents": None, "shape_tangents": None}
NO_SHAPES = {"shapes": None, "shape_tangents": None}
NO_CALL_POINTERS = {k: None for k in CALL_POINTERS}
COMPACT = {"flags": 1, "max_list": 2}   # the outputs are 2 rows of 36 (48) bytes: 72 (96); in place 4 rows: 144 (192)
_COMMON = {
    "valid": {},
    "negative count": {"count": -1},
    "out_normals for a mesh without normals": dict(NO_NORMALS),
    "null skin": {"skin": None},
    "null out_positions": {"out_positions": None},
    "no out_normals": {"out_normals": None, "out_tangents": None},
    "out_positions overlaps skin": {"out_positions": "skin+380"},
    "out_positions behind skin": {"out_positions": "skin+384"},
    "out_normals overlaps skin": {"out_normals": "skin+380"},
    "out_normals overlaps out_positions": {"out_normals": "out_positions+140"},
    "out_positions overlaps out_normals from below": {"out_positions": "out_normals+140"},
    # the empty calls
    "count 0 and no pointers": {"count": 0, **NO_CALL_POINTERS},
    "V 0 and no pointers": {"vertex_count": 0, **NO_CALL_POINTERS},
    "count 0 and out_normals for a mesh without normals": {"count": 0, **NO_NORMALS},
    # two faults
    "negative count and out_normals for a mesh without normals": {"count": -1, **NO_NORMALS},
    "out_normals for a mesh without normals and null skin": {**NO_NORMALS, "skin": None},
    "null skin and null out_positions": {"skin": None, "out_positions": None},
    "null out_positions and out_normals overlaps skin": {"out_positions": None, "out_normals": "skin"},
    "both outputs overlap skin": {"out_positions": "skin", "out_normals": "skin+200"},
    "out_normals overlaps skin and out_positions": {"out_normals": "skin+300", "out_positions": "skin+400"},
}
_SHAPED = {
    "null shape_weights": {"shape_weights": None},
    "count 0 and null shape_weights": {"count": 0, **NO_CALL_POINTERS},
    "no shapes": dict(NO_SHAPES),
    "no shapes and negative count": {**NO_SHAPES, "count": -1},
    "out_positions overlaps shape_weights": {"out_positions": "shape_weights+12"},
    "out_positions behind shape_weights": {"out_positions": "shape_weights+16"},
    "out_normals overlaps shape_weights": {"out_normals": "shape_weights+12"},
    "out_normals overlaps out_positions and null shape_weights": {"out_normals": "out_positions", "shape_weights": None},
    "null shape_weights and null skin": {"shape_weights": None, "skin": None},
    "both outputs overlap shape_weights": {"out_positions": "shape_weights", "out_normals": "shape_weights+200"},
}
_LISTED = {
    "unknown flag bits": {"flags": 2},
    "negative max_list": {"max_list": -1},
    "no shapes": dict(NO_SHAPES),
    "no shapes and no shape_weights": {**NO_SHAPES, "shape_weights": None},
    "no shape_weights": {"shape_weights": None},
    "null indices": {"indices": None},
    "null list_count": {"list_count": None},
    "out_positions overlaps indices": {"out_positions": "indices+12"},
    "out_positions behind indices": {"out_positions": "indices+16"},
    "out_normals overlaps indices": {"out_normals": "indices+12"},
    "out_positions overlaps list_count": {"out_positions": "list_count"},
    "out_normals overlaps list_count": {"out_normals": "list_count+3"},
    "out_positions overlaps shape_weights": {"out_positions": "shape_weights+12"},
    "out_normals overlaps shape_weights": {"out_normals": "shape_weights+12"},
    "compact": dict(COMPACT),
    "compact: out_normals overlaps out_positions": {**COMPACT, "out_normals": "out_positions+68"},
    "compact: out_normals behind out_positions": {**COMPACT, "out_normals": "out_positions+72"},
    "in place: out_normals 72 bytes behind out_positions": {"max_list": 2, "out_normals": "out_positions+72"},
    "compact: out_positions overlaps skin from below": {**COMPACT, "skin": "out_positions+68"},
    "compact: skin behind out_positions": {**COMPACT, "skin": "out_positions+72"},
    "compact: out_normals overlaps shape_weights from below": {**COMPACT, "shape_weights": "out_normals+68"},
    "compact: indices behind out_positions": {**COMPACT, "indices": "out_positions+72"},
    "compact: indices sized by max_list": {**COMPACT, "out_positions": "indices+8"},
    "compact: list_count overlaps out_normals from below": {**COMPACT, "list_count": "out_normals+71"},
    # the empty calls
    "max_list 0 and no pointers": {"max_list": 0, **NO_CALL_POINTERS},
    "max_list 0, compact, and no pointers": {"flags": 1, "max_list": 0, **NO_CALL_POINTERS},
    "max_list 0 and unknown flag bits": {"max_list": 0, "flags": 4, **NO_CALL_POINTERS},
    "count 0 and negative max_list": {"count": 0, "max_list": -1},
    "count 0 and no shapes": {"count": 0, **NO_SHAPES},
    # two faults
    "unknown flag bits and negative max_list": {"flags": 2, "max_list": -1},
    "negative max_list and no shapes": {"max_list": -1, **NO_SHAPES},
    "no shapes and negative count": {**NO_SHAPES, "count": -1},
    "negative count and unknown flag bits": {"count": -1, "flags": 2},
    "null shape_weights overlap and null indices": {"out_positions": "shape_weights", "indices": None},
    "null indices and outputs that overlap": {"indices": None, "out_normals": "out_positions"},
    "null indices and out_positions overlaps list_count": {"indices": None, "out_positions": "list_count"},
    "null indices and null list_count": {"indices": None, "list_count": None},
    "out_positions overlaps list_count and out_normals overlaps indices": {"out_positions": "list_count", "out_normals": "indices"},
    "out_positions overlaps indices and list_count": {"list_count": "indices+4", "out_positions": "indices"},
}
_TANGENTS = {
    "no out_tangents": {"out_tangents": None},
    "out_tangents for a mesh without tangents": dict(NO_TANGENTS),
    "out_tangents without out_normals": {"out_normals": None},
    "out_tangents overlaps skin": {"out_tangents": "skin+380"},
    "out_tangents overlaps out_positions": {"out_tangents": "out_positions+140"},
    "out_tangents behind out_positions": {"out_tangents": "out_positions+144"},
    "out_tangents overlaps out_normals": {"out_tangents": "out_normals+140"},
    "out_positions overlaps out_tangents from below": {"out_positions": "out_tangents+188"},
    "out_positions behind out_tangents": {"out_positions": "out_tangents+192"},
    "indices without list_count": {"indices": "indices", "list_count": None},
    "list_count without indices": {"indices": None, "list_count": "list_count"},
    "count 0, no pointers but out_tangents": {"count": 0, **NO_CALL_POINTERS, "out_tangents": "out_tangents"},
    # two faults
    "a lone list_count and out_tangents for a mesh without tangents": {"indices": None, "list_count": "list_count", **NO_TANGENTS},
    "out_tangents for a mesh without tangents and without out_normals": {**NO_TANGENTS, "out_normals": None},
    "out_tangents without out_normals and negative count": {"out_normals": None, "count": -1},
    "out_tangents for a mesh without tangents and negative count": {**NO_TANGENTS, "count": -1},
    "out_normals overlaps out_positions and out_tangents overlaps skin": {"out_normals": "out_positions", "out_tangents": "skin"},
    "out_tangents overlaps skin and out_positions": {"out_tangents": "skin+300", "out_positions": "skin+400"},
    "out_tangents overlaps out_positions and out_normals": {"out_positions": "out_tangents+100", "out_normals": "out_tangents+150"},
}
_TANGENTS_SHAPED = {
    "out_tangents overlaps shape_weights": {"out_tangents": "shape_weights+12"},
    "out_tangents overlaps skin and shape_weights": {"shape_weights": "skin+400", "out_tangents": "skin+300"},
}
_TANGENTS_LISTED = {
    "out_tangents overlaps indices": {"out_tangents": "indices+12"},
    "out_tangents overlaps list_count": {"out_tangents": "list_count"},
    "out_tangents overlaps shape_weights and indices": {"indices": "shape_weights+8", "out_tangents": "shape_weights"},
    "out_tangents overlaps indices and list_count": {"list_count": "indices+4", "out_tangents": "indices"},
    "out_tangents overlaps list_count and out_positions": {"out_positions": "out_tangents+100", "list_count": "out_tangents+300"},
    "compact: out_tangents overlaps out_normals from below": {**COMPACT, "out_normals": "out_tangents+92"},
    "compact: out_normals behind out_tangents": {**COMPACT, "out_normals": "out_tangents+96"},
    "compact: out_tangents overlaps out_positions": {**COMPACT, "out_tangents": "out_positions+68"},
    "compact: out_tangents behind out_positions": {**COMPACT, "out_tangents": "out_positions+72"},
}
_BOUNDS = {
    "valid": {},
    "negative bone count": {"bone_count": -1},
    "null bone_boxes": {"bone_boxes": None},
    "null used": {"used": None},
    "no bones and no boxes": {"bone_count": 0, "bone_boxes": None, "used": None},
    "negative count": {"count": -1},
    "null skin": {"skin": None},
    "null boxes": {"boxes_out": None},
    "boxes overlaps skin": {"boxes_out": "skin+380"},
    "boxes behind skin": {"boxes_out": "skin+384"},
    "skin overlaps boxes from below": {"skin": "boxes_out+92"},
    "count 0 and no pointers": {"count": 0, "skin": None, "boxes_out": None},
    "negative bone count and negative count": {"bone_count": -1, "count": -1},
    "null bone_boxes and negative count": {"bone_boxes": None, "count": -1},
    "negative count and null skin": {"count": -1, "skin": None},
    "null skin and null boxes": {"skin": None, "boxes_out": None},
    "null boxes and an overlap": {"boxes_out": None, "skin": "boxes_out"},
}
_PLANES = {
    "negative count": {"count": -1},
    "plane_count -1": {"plane_count": -1},
    "plane_count 17": {"plane_count": 17},
    "null planes": {"planes": None},
    "no planes": {"plane_count": 0, "planes": None},
    "null boxes": {"boxes": None},
    "no skeleton_global": {"skeleton_global": None},
    "negative count and bad plane_count": {"count": -1, "plane_count": 17},
    "bad plane_count and null planes": {"plane_count": -1, "planes": None},
    "bad plane_count and null boxes": {"plane_count": 17, "boxes": None},
    "null planes and null boxes": {"planes": None, "boxes": None},
}
_CULL_IN, _CULL_OUT = ("boxes", "skeleton_global"), ("visible", "cull_indices", "visible_count")
_LOD_IN, _LOD_OUT = ("boxes", "skeleton_global", "planes", "camera", "ranges"), ("state", "level", "lod_indices", "list_counts")


def _overlaps(ins, outs):
    """Each output on each input, then on each earlier output: the pairs in the order the check visits them; then, two at
    once, each pair against the one the check visits next."""
    pairs = [(o, i) for n, o in enumerate(outs) for i in ins + outs[:n]]
    cases = {f"{o} overlaps {i}": {o: i} for o, i in pairs}
    for (o, i), (o2, i2) in zip(pairs, pairs[1:]):
        if o2 != o and o2 != i and i2 != o:
            cases[f"{o} overlaps {i} and {o2} overlaps {i2}"] = {o: i, o2: i2}
        elif o2 == o and i2 in ins:
            cases[f"{o} overlaps {i} and {i2}"] = {i2: i + "+1", o: i}
    return cases


_CULL = {
    "valid": {},
    "both visible and indices null": {"visible": None, "cull_indices": None},
    "indices without visible_count": {"visible_count": None},
    "verdicts only": {"cull_indices": None, "visible_count": None},
    "count only": {"visible": None, "cull_indices": None, "visible_count": "visible_count"},
    "list only": {"visible": None},
    "visible behind boxes": {"visible": "boxes+96"},
    "boxes behind visible": {"boxes": "visible+4"},
    "visible_count overlaps indices from above": {"visible_count": "cull_indices+15"},
    "visible_count behind indices": {"visible_count": "cull_indices+16"},
    "count 0": {"count": 0},
    "count 0 and no boxes": {"count": 0, "boxes": None, "skeleton_global": None},
    "count 0 and no visible_count": {"count": 0, "cull_indices": None, "visible_count": None},
    "count 0 and both outputs null": {"count": 0, "visible": None, "cull_indices": None},
    "null planes and both outputs null": {"planes": None, "visible": None, "cull_indices": None},
    "both outputs null and no visible_count": {"visible": None, "cull_indices": None, "visible_count": None},
    "indices without visible_count and null boxes": {"visible_count": None, "boxes": None},
    "null boxes and an overlap": {"boxes": None, "visible": "skeleton_global"},
}
_LOD = {
    "valid": {},
    "exclusive": {"lod_flags": 1},
    "no level": {"level": None},
    "range_count 0": {"range_count": 0},
    "range_count 9": {"range_count": 9},
    "null ranges": {"ranges": None},
    "null camera": {"camera": None},
    "camera nan": {"camera_data": [0.0, NAN, 0.0]},
    "camera inf": {"camera_data": [0.0, 0.0, -INF]},
    "range 0 negative begin": {"ranges_data.0.0": -1.0},
    "range 1 end inf": {"ranges_data.1.1": INF},
    "range 1 begin_margin nan": {"ranges_data.1.2": NAN},
    "range 0 negative end_margin": {"ranges_data.0.3": -0.5},
    "range 0 begins behind its end": {"ranges_data.0.0": 3.0},
    "range 1 unused": {"range_count": 1, "ranges_data.1.0": NAN},
    "unknown flag bits": {"lod_flags": 2},
    "null state": {"state": None},
    "null indices": {"lod_indices": None},
    "null list_counts": {"list_counts": None},
    "indices sized by the range count": {"list_counts": "lod_indices+31"},
    "list_counts behind indices": {"list_counts": "lod_indices+32"},
    "count 0": {"count": 0},
    "count 0 and no pointers": {"count": 0, "boxes": None, "skeleton_global": None, "state": None, "level": None, "lod_indices": None},
    "count 0 and no list_counts": {"count": 0, "list_counts": None},
    "count 0 and bad flags": {"count": 0, "lod_flags": 2},
    # two faults, each line against the next
    "null planes and bad range_count": {"planes": None, "range_count": 0},
    "bad range_count and null ranges": {"range_count": 9, "ranges": None},
    "null ranges and null camera": {"ranges": None, "camera": None},
    "null camera and a bad range": {"camera": None, "ranges_data.0.0": -1.0},
    "camera nan and a bad range": {"camera_data": [NAN, 0.0, 0.0], "ranges_data.0.0": -1.0},
    "two bad ranges": {"ranges_data.0.0": 3.0, "ranges_data.1.3": -1.0},
    "a bad range and bad flags": {"ranges_data.1.0": -2.0, "lod_flags": 2},
    "bad flags and null boxes": {"lod_flags": 4, "boxes": None},
    "null boxes and null state": {"boxes": None, "state": None},
    "null state and null indices": {"state": None, "lod_indices": None},
    "null indices and null list_counts": {"lod_indices": None, "list_counts": None},
    "null list_counts and an overlap": {"list_counts": None, "state": "boxes"},
}
CALL_CASES = (
    [(e, n, ch) for e in SKIN_CPU for n, ch in _COMMON.items()]
    + [(e, n, ch) for e in SHAPED_ENTRIES for n, ch in _SHAPED.items()]
    + [(e, n, ch) for e in LISTED_ENTRIES for n, ch in _LISTED.items()]
    + [(e, n, ch) for e in CALL_CPU for n, ch in _TANGENTS.items()]
    + [(e, n, ch) for e in CALL_CPU[1:] for n, ch in _TANGENTS_SHAPED.items()]
    + [("call_listed_cpu", n, ch) for n, ch in _TANGENTS_LISTED.items()]
    + [("call_plain_cpu", "null call", {"call": None}), ("call_plain_cpu", "small call struct_size", {"call.struct_size": 8}),
       ("call_plain_cpu", "null desc and null call", {"desc": None, "call": None}),
       ("call_plain_cpu", "small call struct_size and a bad mesh", {"call.struct_size": 8, "influences": 5}),
       ("call_plain_cpu", "shape_weights on a mesh without shapes", {**NO_SHAPES, "shape_weights": "shape_weights"})]
    + [("bone_boxes_cpu", n, ch) for n, ch in {
        "valid": {}, "null boxes": {"boxes_out": None}, "null used": {"used_out": None},
        "no bones and no outputs": {"bone_count": 0, "vertex_count": 0, "boxes_out": None, "used_out": None},
        "bad mesh and null boxes": {"influences": 5, "boxes_out": None}}.items()]
    + [("bounds_cpu", n, ch) for n, ch in _BOUNDS.items()]
    + [("cull_cpu", n, ch) for n, ch in {**_PLANES, **_CULL, **_overlaps(_CULL_IN, _CULL_OUT)}.items()]
    + [("lod_cpu", n, ch) for n, ch in {**_PLANES, **_LOD, **_overlaps(_LOD_IN, _LOD_OUT)}.items()]
)
# the device entries with a null mesh: their first refusal whatever else is wrong, but for the two whose call check comes first
NULL_MESH_CASES = (
    [(e, "null mesh", {"count": -1, "flags": 2, "plane_count": -1}) for e in
     ("skin", "shaped", "listed", "call_plain", "call_listed", "mesh_bone_boxes", "launch_shape", "bounds", "cull")]
    + [("call_plain", "null call and null mesh", {"call": None}), ("call_plain", "small call struct_size and null mesh", {"call.struct_size": 8}),
       ("lod", "null mesh", {}), ("lod", "negative count and null mesh", {"count": -1}),
       ("lod", "an overlap and null mesh", {"list_counts": "lod_indices"}), ("lod", "count 0 and null mesh", {"count": 0})]
)
CASES = MESH_CASES + CALL_CASES + NULL_MESH_CASES


def case_id(case):
    return f"{case[0]}: {case[1]}"


def make_call(entry, changes, alloc=host_alloc):
    return Call({**ENTRIES[entry][1], **changes}, alloc)


def written(call, read=None):
    """The buffers whose bytes are no longer what the call was given."""
    read = read or (lambda addr: np.frombuffer((C.c_uint8 * BUF_BYTES).from_address(addr), np.uint8))
    return sorted(name for name, was in call.initial.items() if not np.array_equal(read(call.addr[name]), was))


def run_case(L, entry, changes):
    """(return code, text, written buffers) of one call; the text of a call that succeeds is empty."""
    call = make_call(entry, changes)
    rc = ENTRIES[entry][0](L, call)
    return [rc, _lib.last_error() if rc < 0 else "", written(call)]


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


def test_a_refused_call_writes_nothing_and_an_empty_call_only_its_counts(golden):
    for name, (rc, _, wrote) in golden.items():
        changes = next(c[2] for c in CASES if case_id(c) == name)
        empty = changes.get("count") == 0 or changes.get("vertex_count") == 0 or changes.get("max_list") == 0
        if rc < 0 or (empty and not name.startswith(("cull_cpu", "lod_cpu"))):
            assert wrote == [], name
        elif empty:
            assert wrote in ([], ["visible_count"], ["list_counts"]), name


def test_every_reachable_text_is_covered(golden):
    """The ledger holds each refusal family of the three host files at least once (by a word of its text)."""
    texts = " | ".join(t for _, t, _ in golden.values())
    words = ("null out_mesh", "influences must be 4 or 8", "negative bone or vertex count", "null mesh array", "vertex 2 influence 1: bone index 2 outside [0, 2)",
                 "vertex 1 influence 7", "a mesh supports at most", "null shapes", "mbik_mesh_shapes.struct_size", "shape_count must be at least 1",
                 "shape mode must be", "null shape positions", "both have normals or both have none", "exceeds 160 KiB", "tangents given for a mesh without normals",
                 "shape_tangents must be given exactly", "null desc", "mbik_mesh_desc.struct_size", "null call", "mbik_skin_call.struct_size",
                 "negative count", "out_normals given for a mesh without normals", "null skin", "null out_positions", "out_positions overlaps skin",
                 "out_normals overlaps skin", "out_normals overlaps out_positions", "null shape_weights", "the mesh has no shapes (mbik_mesh_create_shaped)",
                 "out_positions overlaps shape_weights", "out_normals overlaps shape_weights", "unknown flag bits", "negative max_list",
                 "shape_weights given for a mesh without shapes", "null indices", "null list_count", "out_positions overlaps indices",
                 "out_normals overlaps indices", "out_positions overlaps list_count", "out_normals overlaps list_count",
                 "indices and list_count must be given together", "out_tangents given for a mesh without tangents", "out_tangents given without out_normals",
                 "out_tangents overlaps skin", "out_tangents overlaps shape_weights", "out_tangents overlaps indices", "out_tangents overlaps list_count",
                 "out_tangents overlaps out_positions", "out_tangents overlaps out_normals", "null mesh", "null boxes or used", "negative bone count",
                 "null bone_boxes or used", "null boxes", "boxes overlaps skin", "plane_count outside", "null planes", "both visible and indices are null",
                 "indices without visible_count", "range_count outside", "null ranges", "null camera", "camera is not finite",
                 "range 0 has a negative or non-finite field", "range 1 has a negative", "range 0 begins behind its end", "null state", "null list_counts")
    pairs = tuple(f"{o} overlaps {i}" for o, i in [("visible", "boxes"), ("visible", "skeleton_global"), ("indices", "boxes"), ("indices", "visible"),
                                                      ("visible_count", "indices"), ("state", "planes"), ("state", "camera"), ("level", "ranges"),
                                                      ("level", "state"), ("indices", "level"), ("list_counts", "indices"), ("list_counts", "ranges")])
    for word in words + pairs:
        assert word in texts, word


if __name__ == "__main__":
    with open(GOLDEN, "w") as fh:
        json.dump(record(_lib.load()), fh, indent=1, sort_keys=True)
        fh.write("\n")
