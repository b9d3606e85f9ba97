"""Linear blend skinning of meshes from skin transforms (include/mbik.h, ABI 10).

`Mesh` owns one `mbik_mesh`: the mesh arrays of one surface (positions, optional normals, 4 or 8
bone indices and weights a vertex) resident on one GPU, bound to a bone count.  `Mesh.skin()`
takes device pointers -- the skin transforms are `Plan.pose_globals(..., inv_bind_ptr=...)`'s
output -- and is asynchronous on the given HIP stream.  `skin_vertices_cpu()` runs the same code
on numpy arrays without a device, and `synthetic_mesh()` is the seeded mesh generator the tests
and tools/skin_bench.py use.

Blend shapes (ABI 13): a `Mesh` created with `shape_positions` carries P shapes
shared by every skeleton, `Mesh.skin(..., shape_weights_ptr=...)` morphs each skeleton by its own P
weights in front of the skinning (mbik_skin_vertices_shaped), `skin_vertices_cpu(...,
shape_weights=...)` is the host side and `synthetic_shapes()` the seeded generator.

Bounds and culling (ABI 14): a `Mesh` carries one box per bone (`Mesh.bone_boxes()`),
`Mesh.bounds()` merges them, moved by each skeleton's skin transforms, into one box per skeleton
(mbik_skin_bounds), and `Mesh.cull()` tests those boxes against frustum planes and writes the
verdicts and the ascending list of visible skeletons (mbik_cull_boxes), all on the device.
`bone_boxes_cpu()`, `skin_bounds_cpu()` and `cull_boxes_cpu()` are the host sides.

List-driven skinning (ABI 15): `Mesh.skin_listed()` skins the skeletons a device list
names -- `Mesh.cull()`'s indices and visible_count, on the same stream and never read by the host --
in place or compacted (mbik_skin_vertices_listed); `skin_vertices_listed_cpu()` is the host side.

Distance LOD lists: `Mesh.cull_lod()` writes one such list per visibility range
(mbik_cull_lod: Godot's visibility_range_begin / _end with their margins as hysteresis, in front of the
plane test), `cull_lod_cpu()` is the host side, and `MeshLod` holds one mesh per level of detail:
`select()` makes the lists and `skin()` skins each level's mesh over its own.

Tangents: a `Mesh` created with `tangents` [V][4] (xyz and the binormal sign; with
`shape_tangents` [P][V][3] on a shaped mesh) goes through mbik_mesh_create_desc, and `out_tangents_ptr` on
`Mesh.skin()`, `Mesh.skin_listed()` and `MeshLod.skin()` writes the third stream [rows][V][4] through
mbik_skin_vertices_call, the one struct-based call over the three forms (`Mesh.skin_call()` is that call
as it is).  `skin_vertices_cpu(..., tangents=...)` and `skin_vertices_listed_cpu(..., tangents=...)` are
the host sides; `synthetic_tangents()` and `synthetic_shape_tangents()` the seeded generators.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib
from ._lib import check


def _ptr(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def _mesh_arrays(positions, bone_indices, weights, normals):
    pos = np.ascontiguousarray(positions, np.float32)
    idx = np.ascontiguousarray(bone_indices, np.int32)
    wgt = np.ascontiguousarray(weights, np.float32)
    nrm = None if normals is None else np.ascontiguousarray(normals, np.float32)
    V = pos.shape[0]
    assert pos.shape == (V, 3), pos.shape
    assert idx.ndim == 2 and idx.shape[0] == V and wgt.shape == idx.shape, (idx.shape, wgt.shape)
    assert nrm is None or nrm.shape == (V, 3), nrm.shape
    return pos, idx, wgt, nrm


def _shape_arrays(V, shape_positions, shape_normals, shape_mode):
    """-> (MbikMeshShapes, the arrays it points into), or (None, ()) without shapes."""
    if shape_positions is None:
        if shape_normals is not None:
            raise ValueError("shape_normals without shape_positions")
        return None, ()
    if shape_mode not in _lib.SHAPE_MODES:
        raise ValueError("shape_mode must be 'relative' or 'normalized'")
    sp = np.ascontiguousarray(shape_positions, np.float32)
    sn = None if shape_normals is None else np.ascontiguousarray(shape_normals, np.float32)
    P = sp.shape[0]
    assert sp.shape == (P, V, 3), sp.shape
    assert sn is None or sn.shape == (P, V, 3), sn.shape
    sh = _lib.MbikMeshShapes(C.sizeof(_lib.MbikMeshShapes), P, _lib.SHAPE_MODES[shape_mode], _ptr(sp), _ptr(sn))
    return sh, (sp, sn)


def _tangent_arrays(V, nrm, tangents, shapes, shape_tangents):
    """-> (tangents [V][4] or None, shape_tangents [P][V][3] or None), contiguous float32."""
    tan = None if tangents is None else np.ascontiguousarray(tangents, np.float32)
    stan = None if shape_tangents is None else np.ascontiguousarray(shape_tangents, np.float32)
    assert tan is None or tan.shape == (V, 4), tan.shape
    assert stan is None or shapes is None or stan.shape == (shapes.shape_count, V, 3), stan.shape
    return tan, stan


def _mesh_desc(bone_count, pos, idx, wgt, nrm, tan, shapes, stan):
    """mbik_mesh_desc over arrays the caller keeps alive."""
    return _lib.MbikMeshDesc(C.sizeof(_lib.MbikMeshDesc), int(bone_count), pos.shape[0], idx.shape[1], _ptr(pos), _ptr(nrm), _ptr(tan),
                             _ptr(idx), _ptr(wgt), None if shapes is None else C.pointer(shapes), _ptr(stan))


def _skin_call(count, skin, out_positions, out_normals=None, out_tangents=None, shape_weights=None, indices=None, list_count=None,
               max_list=0, flags=0):
    """mbik_skin_call from addresses (ints, c_void_p or None)."""
    vp = lambda x: x if isinstance(x, C.c_void_p) else C.c_void_p(x or None)
    return _lib.MbikSkinCall(C.sizeof(_lib.MbikSkinCall), count, vp(skin), vp(shape_weights), vp(indices), vp(list_count), max_list, flags,
                             vp(out_positions), vp(out_normals), vp(out_tangents))


def _marshal_mesh(bone_count, positions, bone_indices, weights, normals=None, shape_positions=None, shape_normals=None,
                  shape_mode="relative", tangents=None, shape_tangents=None):
    """The mesh arguments every entry takes -> (mbik_mesh_desc, what it points into: keep it alive as long)."""
    pos, idx, wgt, nrm = _mesh_arrays(positions, bone_indices, weights, normals)
    shapes, keep = _shape_arrays(pos.shape[0], shape_positions, shape_normals, shape_mode)
    tan, stan = _tangent_arrays(pos.shape[0], nrm, tangents, shapes, shape_tangents)
    return _mesh_desc(bone_count, pos, idx, wgt, nrm, tan, shapes, stan), (pos, idx, wgt, nrm, shapes, keep, tan, stan)


def _shape_count(desc):
    return desc.shapes.contents.shape_count if desc.shapes else 0


def _out(given, wanted, shape):
    """An output array of a host call: `given` as it is (float32, `shape`, contiguous; written in place), else NaN-filled when
    the mesh has the stream (`wanted`), else None."""
    if given is None:
        given = np.full(shape, np.nan, np.float32) if wanted else None
    assert given is None or (given.dtype == np.float32 and given.shape == shape and given.flags.c_contiguous)
    return given


def _skin_inputs(desc, bone_count, skin, shape_weights):
    """-> (skin [count][bones][12], shape_weights [count][P] or None), contiguous float32."""
    sk = np.ascontiguousarray(skin, np.float32)
    assert sk.shape == (sk.shape[0], bone_count, 12), sk.shape
    cw = None if shape_weights is None else np.ascontiguousarray(shape_weights, np.float32)
    assert cw is None or not desc.shapes or cw.shape == (sk.shape[0], _shape_count(desc)), cw.shape
    return sk, cw


class Mesh:
    """One mesh surface on one GPU (mbik_mesh_create_desc).  Immutable; close() frees it."""

    def __init__(self, bone_count: int, positions, bone_indices, weights, normals=None, device: int = 0,
                 shape_positions=None, shape_normals=None, shape_mode: str = "relative", tangents=None, shape_tangents=None):
        """shape_positions [P][V][3] (and shape_normals, exactly when `normals` is given) make a
        shaped mesh; shape_mode is 'relative' or 'normalized'.  tangents [V][4] (xyz and the binormal
        sign; needs normals; with shape_tangents [P][V][3] exactly when the mesh is shaped) make a
        mesh with tangents.  Every form is one mbik_mesh_create_desc."""
        self._L = _lib.load()
        desc, _keep = _marshal_mesh(bone_count, positions, bone_indices, weights, normals, shape_positions, shape_normals, shape_mode,
                                    tangents, shape_tangents)
        self.bone_count, self.vertex_count, self.influences = int(bone_count), desc.vertex_count, desc.influences
        self.has_normals, self.has_tangents, self.shape_count = bool(desc.normals), bool(desc.tangents), _shape_count(desc)
        self.device = device
        h = C.c_void_p()
        check(self._L.mbik_mesh_create_desc(C.byref(desc), device, C.byref(h)))
        self.h = h

    def skin_call(self, skin_ptr: int, out_positions_ptr: int, count: int, out_normals_ptr: int = 0, out_tangents_ptr: int = 0,
                  shape_weights_ptr: int = 0, indices_ptr: int = 0, list_count_ptr: int = 0, max_list: int | None = None,
                  compact: bool = False, stream: int = 0) -> None:
        """mbik_skin_vertices_call: the plain (no list, no shape weights), the shaped or, with indices_ptr and
        list_count_ptr, the listed form; out_tangents [rows][vertices][4] is the third stream of a mesh with
        tangents, and without it the call is the existing entry of its form."""
        call = _skin_call(count, skin_ptr, out_positions_ptr, out_normals_ptr, out_tangents_ptr, shape_weights_ptr, indices_ptr,
                          list_count_ptr, count if max_list is None else max_list, _lib.SKIN_LIST_COMPACT if compact else 0)
        check(self._L.mbik_skin_vertices_call(self.h, C.byref(call), C.c_void_p(stream or None)))

    def skin(self, skin_ptr: int, out_positions_ptr: int, count: int, out_normals_ptr: int = 0, stream: int = 0,
             shape_weights_ptr: int = 0, out_tangents_ptr: int = 0) -> None:
        """skin_call()'s plain and shaped forms (what mbik_skin_vertices and mbik_skin_vertices_shaped do):
        out_positions [count][vertices][3] (and out_normals) from the device skin transforms
        [count][bones][12]; asynchronous on `stream`.  With shape_weights_ptr (device, [count][shapes])
        each skeleton is morphed by its own weights first; without it a shaped mesh skins its base
        arrays.  With out_tangents_ptr ([count][vertices][4]) the tangents are written as well."""
        self.skin_call(skin_ptr, out_positions_ptr, count, out_normals_ptr, out_tangents_ptr, shape_weights_ptr, stream=stream)

    def bone_boxes(self):
        """mbik_mesh_bone_boxes: (boxes [bones][6] position then size, used [bones] uint8); an unused
        bone's box is six zeros."""
        boxes = np.zeros((self.bone_count, 6), np.float32)
        used = np.zeros((self.bone_count,), np.uint8)
        check(self._L.mbik_mesh_bone_boxes(self.h, _ptr(boxes), _ptr(used)))
        return boxes, used

    def bounds(self, skin_ptr: int, boxes_ptr: int, count: int, stream: int = 0) -> None:
        """mbik_skin_bounds: boxes [count][6] from the device skin transforms [count][bones][12];
        asynchronous on `stream`."""
        check(self._L.mbik_skin_bounds(self.h, count, C.c_void_p(skin_ptr or None), C.c_void_p(boxes_ptr or None),
                                       C.c_void_p(stream or None)))

    def cull(self, boxes_ptr: int, count: int, planes, skeleton_global_ptr: int = 0, margin: float = 0.0, visible_ptr: int = 0,
             indices_ptr: int = 0, visible_count_ptr: int = 0, stream: int = 0) -> None:
        """mbik_cull_boxes: the device boxes [count][6] (moved by skeleton_global [count][12] and grown
        by `margin` when given) against `planes`, a host array [n][4] of outward normals and distances.
        visible [count] uint8, indices [count] int32 (the visible skeletons, ascending) and
        visible_count [1] int32 are device pointers; asynchronous on `stream`."""
        pl = np.ascontiguousarray(planes, np.float32).reshape(-1, 4)
        check(self._L.mbik_cull_boxes(self.h, count, C.c_void_p(boxes_ptr or None), C.c_void_p(skeleton_global_ptr or None), margin,
                                      pl.shape[0], _ptr(pl) if pl.shape[0] else None, C.c_void_p(visible_ptr or None),
                                      C.c_void_p(indices_ptr or None), C.c_void_p(visible_count_ptr or None), C.c_void_p(stream or None)))

    def cull_lod(self, boxes_ptr: int, count: int, planes, camera, ranges, state_ptr: int, indices_ptr: int, list_counts_ptr: int,
                 level_ptr: int = 0, skeleton_global_ptr: int = 0, margin: float = 0.0, flags: int = 0, stream: int = 0) -> None:
        """mbik_cull_lod: cull()'s plane test behind a distance test against `ranges` (host, LOD_RANGE_DTYPE
        or [n][4]: begin, end, begin_margin, end_margin; 0 = no limit) from `camera` (host, [3]).  state
        [count] uint8 is read and written (bit r: in range r; the hysteresis; keep it from frame to
        frame), level [count] uint8 (the least range seen, or LOD_NONE) is optional, indices [n][count]
        int32 holds list r in row r and list_counts [n] int32 its length: device pointers; asynchronous
        on `stream`.  flags: _lib.LOD_EXCLUSIVE lists a skeleton under its level only."""
        pl = np.ascontiguousarray(planes, np.float32).reshape(-1, 4)
        cam = np.ascontiguousarray(camera, np.float32).reshape(3)
        rg = lod_ranges(ranges)
        check(self._L.mbik_cull_lod(self.h, count, C.c_void_p(boxes_ptr or None), C.c_void_p(skeleton_global_ptr or None), margin,
                                    pl.shape[0], _ptr(pl) if pl.shape[0] else None, _ptr(cam), rg.shape[0], _ptr(rg) if rg.shape[0] else None,
                                    flags, C.c_void_p(state_ptr or None), C.c_void_p(level_ptr or None), C.c_void_p(indices_ptr or None),
                                    C.c_void_p(list_counts_ptr or None), C.c_void_p(stream or None)))

    def skin_listed(self, skin_ptr: int, out_positions_ptr: int, count: int, indices_ptr: int, list_count_ptr: int,
                    max_list: int | None = None, compact: bool = False, out_normals_ptr: int = 0, shape_weights_ptr: int = 0,
                    stream: int = 0, out_tangents_ptr: int = 0) -> None:
        """mbik_skin_vertices_listed: skin() for the skeletons the device list indices [max_list] int32
        names, its length read from list_count [1] int32 on the device (cull()'s indices and
        visible_count on the same stream are such a list); max_list defaults to `count`.  An entry
        outside [0, count) is skipped.  In place the outputs are [count][vertices][3] and unlisted rows
        are not touched; compact they are [max_list][vertices][3] and row r belongs to indices[r].
        out_tangents_ptr: the same rows of [vertices][4] (mbik_skin_vertices_call)."""
        if out_tangents_ptr or (indices_ptr and list_count_ptr):
            self.skin_call(skin_ptr, out_positions_ptr, count, out_normals_ptr, out_tangents_ptr, shape_weights_ptr, indices_ptr,
                           list_count_ptr, max_list, compact, stream)
            return
        # (a call without its list is the struct call's plain form, or refused there in other words: the listed entry says what
        # it has always said, in the place among its checks where it has always said it)
        check(self._L.mbik_skin_vertices_listed(self.h, count, C.c_void_p(indices_ptr or None), C.c_void_p(list_count_ptr or None),
                                                count if max_list is None else max_list, C.c_void_p(skin_ptr or None),
                                                C.c_void_p(shape_weights_ptr or None), _lib.SKIN_LIST_COMPACT if compact else 0,
                                                C.c_void_p(out_positions_ptr or None), C.c_void_p(out_normals_ptr or None),
                                                C.c_void_p(stream or None)))

    def launch_shape(self, count: int) -> tuple[int, int]:
        """(skeletons per block, vertex chunks) of a skin() call for `count` skeletons; of the shaped
        call when the mesh has shapes."""
        s, c = C.c_int32(0), C.c_int32(0)
        check(self._L.mbik_mesh_launch_shape(self.h, count, C.byref(s), C.byref(c)))
        return s.value, c.value

    def close(self) -> None:
        if getattr(self, "h", None):
            self._L.mbik_mesh_destroy(self.h)
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


def skin_vertices_cpu(bone_count: int, positions, bone_indices, weights, skin, normals=None, shape_positions=None,
                      shape_normals=None, shape_mode: str = "relative", shape_weights=None, tangents=None, shape_tangents=None):
    """mbik_skin_vertices_cpu (host only): `skin` [count][bones][12] -> (positions [count][V][3],
    normals [count][V][3] or None when the mesh has none).  With shape_positions [P][V][3] (and
    shape_normals) and shape_weights [count][P]: mbik_skin_vertices_shaped_cpu.  With tangents [V][4]
    (and shape_tangents [P][V][3] on a shaped mesh): mbik_skin_vertices_call_cpu, and a third array,
    tangents [count][V][4]."""
    desc, _keep = _marshal_mesh(bone_count, positions, bone_indices, weights, normals, shape_positions, shape_normals, shape_mode,
                                tangents, shape_tangents)
    with_tangents = tangents is not None or shape_tangents is not None
    if not with_tangents and bool(desc.shapes) != (shape_weights is not None):
        raise ValueError("shape_positions without shape_weights" if desc.shapes else "shape_weights without shape_positions")
    sk, cw = _skin_inputs(desc, bone_count, skin, shape_weights)
    rows = (sk.shape[0], desc.vertex_count)
    outs = [_out(None, True, rows + (3,)), _out(None, desc.normals, rows + (3,)), _out(None, desc.tangents, rows + (4,))]
    call = _skin_call(sk.shape[0], _ptr(sk), *map(_ptr, outs), _ptr(cw))
    check(_lib.load().mbik_skin_vertices_call_cpu(C.byref(desc), C.byref(call)))
    return tuple(outs) if with_tangents else tuple(outs[:2])


def skin_vertices_listed_cpu(bone_count: int, positions, bone_indices, weights, skin, indices, list_count, max_list=None,
                             compact: bool = False, normals=None, shape_positions=None, shape_normals=None,
                             shape_mode: str = "relative", shape_weights=None, out_positions=None, out_normals=None, tangents=None,
                             shape_tangents=None, out_tangents=None):
    """mbik_skin_vertices_listed_cpu (host only): the skeletons indices[0 .. min(max(list_count, 0),
    max_list)) of `skin` [count][bones][12] -> (positions, normals or None when the mesh has none),
    [max_list][V][3] when compact and [count][V][3] otherwise.  max_list defaults to len(indices).  Rows
    the call does not write keep what out_positions / out_normals (float32 arrays of that shape, written
    in place) held; NaN when they are not given.  shape_weights [count][P] with shape_positions: the
    shaped bits; shape_positions alone: the base arrays.  With tangents [V][4] (and shape_tangents on a
    shaped mesh): mbik_skin_vertices_call_cpu, and a third array, tangents [rows][V][4] (out_tangents
    as the other two)."""
    desc, _keep = _marshal_mesh(bone_count, positions, bone_indices, weights, normals, shape_positions, shape_normals, shape_mode,
                                tangents, shape_tangents)
    with_tangents = tangents is not None or shape_tangents is not None
    sk, cw = _skin_inputs(desc, bone_count, skin, shape_weights)
    ind = np.ascontiguousarray(indices, np.int32).reshape(-1)
    cnt = np.asarray([int(list_count)], np.int32)
    max_list = ind.shape[0] if max_list is None else int(max_list)
    assert 0 <= max_list <= ind.shape[0], max_list
    rows = (max_list if compact else sk.shape[0], desc.vertex_count)
    outs = [_out(out_positions, True, rows + (3,)), _out(out_normals, desc.normals, rows + (3,)),
            _out(out_tangents, desc.tangents, rows + (4,)) if with_tangents else None]
    call = _skin_call(sk.shape[0], _ptr(sk), *map(_ptr, outs), _ptr(cw), _ptr(ind), _ptr(cnt), max_list, _lib.SKIN_LIST_COMPACT if compact else 0)
    check(_lib.load().mbik_skin_vertices_call_cpu(C.byref(desc), C.byref(call)))
    return tuple(outs) if with_tangents else tuple(outs[:2])


def bone_boxes_cpu(bone_count: int, positions, bone_indices, weights):
    """mbik_bone_boxes_cpu (host only): (boxes [bones][6], used [bones] uint8) of a mesh."""
    d, _keep = _marshal_mesh(bone_count, positions, bone_indices, weights)
    boxes = np.zeros((bone_count, 6), np.float32)
    used = np.zeros((bone_count,), np.uint8)
    check(_lib.load().mbik_bone_boxes_cpu(bone_count, d.vertex_count, d.influences, d.positions, d.bone_indices, d.weights, _ptr(boxes),
                                          _ptr(used)))
    return boxes, used


def skin_bounds_cpu(bone_boxes, used, skin):
    """mbik_skin_bounds_cpu (host only): `skin` [count][bones][12] -> boxes [count][6]."""
    L = _lib.load()
    bb = np.ascontiguousarray(bone_boxes, np.float32)
    us = np.ascontiguousarray(used, np.uint8)
    sk = np.ascontiguousarray(skin, np.float32)
    B, count = us.shape[0], sk.shape[0]
    assert bb.shape == (B, 6) and sk.shape == (count, B, 12), (bb.shape, sk.shape)
    out = np.empty((count, 6), np.float32)
    check(L.mbik_skin_bounds_cpu(B, _ptr(bb), _ptr(us), count, _ptr(sk), _ptr(out)))
    return out


def cull_boxes_cpu(boxes, planes, skeleton_global=None, margin: float = 0.0):
    """mbik_cull_boxes_cpu (host only): boxes [count][6] against planes [n][4] ->
    (visible [count] uint8, indices [visible count] int32 ascending)."""
    L = _lib.load()
    bx = np.ascontiguousarray(boxes, np.float32)
    pl = np.ascontiguousarray(planes, np.float32).reshape(-1, 4)
    sg = None if skeleton_global is None else np.ascontiguousarray(skeleton_global, np.float32)
    count = bx.shape[0]
    assert bx.shape == (count, 6) and (sg is None or sg.shape == (count, 12)), bx.shape
    visible = np.zeros((count,), np.uint8)
    indices = np.full((count,), -1, np.int32)
    n = np.full((1,), -1, np.int32)
    check(L.mbik_cull_boxes_cpu(count, _ptr(bx), _ptr(sg), margin, pl.shape[0], _ptr(pl) if pl.shape[0] else None, _ptr(visible),
                                _ptr(indices), _ptr(n)))
    assert (indices[n[0]:] == -1).all()
    return visible, indices[:n[0]].copy()


LOD_RANGE_DTYPE = np.dtype([("begin", np.float32), ("end", np.float32), ("begin_margin", np.float32), ("end_margin", np.float32)])  # mbik_lod_range


def lod_ranges(ranges):
    """-> a contiguous LOD_RANGE_DTYPE array [n] from one, or from rows of (begin, end, begin_margin, end_margin)."""
    a = np.asarray(ranges)
    if a.dtype == LOD_RANGE_DTYPE:
        return np.ascontiguousarray(a).reshape(-1)
    return np.ascontiguousarray(np.asarray(ranges, np.float32).reshape(-1, 4)).view(LOD_RANGE_DTYPE).reshape(-1)


def cull_lod_cpu(boxes, planes, camera, ranges, state, skeleton_global=None, margin: float = 0.0, flags: int = 0):
    """mbik_cull_lod_cpu (host only): boxes [count][6] against planes [n][4] and `ranges` seen from
    `camera`, with the previous `state` [count] uint8 (not modified) ->
    (state [count] uint8, level [count] uint8, lists: one ascending int32 array per range)."""
    L = _lib.load()
    bx = np.ascontiguousarray(boxes, np.float32)
    pl = np.ascontiguousarray(planes, np.float32).reshape(-1, 4)
    cam = np.ascontiguousarray(camera, np.float32).reshape(3)
    rg = lod_ranges(ranges)
    sg = None if skeleton_global is None else np.ascontiguousarray(skeleton_global, np.float32)
    count, R = bx.shape[0], rg.shape[0]
    assert bx.shape == (count, 6) and (sg is None or sg.shape == (count, 12)), bx.shape
    st = np.array(state, np.uint8).reshape(count)
    level = np.full((count,), 0xEE, np.uint8)
    indices = np.full((max(R, 1), count), -1, np.int32)
    n = np.full((max(R, 1),), -1, np.int32)
    check(L.mbik_cull_lod_cpu(count, _ptr(bx), _ptr(sg), margin, pl.shape[0], _ptr(pl) if pl.shape[0] else None, _ptr(cam), R,
                              _ptr(rg) if R else None, flags, _ptr(st), _ptr(level), _ptr(indices), _ptr(n)))
    assert all((indices[r, n[r]:] == -1).all() for r in range(R))
    return st, level, [indices[r, :n[r]].copy() for r in range(R)]


class MeshLod:
    """One character at several levels of detail: `meshes[r]` is the mesh of range `ranges[r]`, all on
    one rig and one device.  select() writes one list per range and skin() skins each mesh over its own
    list; both are asynchronous on `stream` and the host reads nothing in between.  The meshes stay the
    caller's (close them there)."""

    def __init__(self, meshes, ranges):
        self.meshes, self.ranges = list(meshes), lod_ranges(ranges)
        if not self.meshes or len(self.meshes) != self.ranges.shape[0]:
            raise ValueError("one mesh per range, at least one")
        if len({m.bone_count for m in self.meshes}) != 1 or len({m.device for m in self.meshes}) != 1:
            raise ValueError("the meshes of a LOD set share their bone count and their device")

    def select(self, boxes_ptr: int, count: int, planes, camera, state_ptr: int, indices_ptr: int, list_counts_ptr: int,
               level_ptr: int = 0, skeleton_global_ptr: int = 0, margin: float = 0.0, exclusive: bool = True, stream: int = 0) -> None:
        """meshes[0].cull_lod(...) with this set's ranges (the first mesh gives the device and the
        scratch).  exclusive (the default): a skeleton is in the list of its level only, so that
        overlapping ranges do not skin it twice."""
        self.meshes[0].cull_lod(boxes_ptr, count, planes, camera, self.ranges, state_ptr, indices_ptr, list_counts_ptr,
                                level_ptr=level_ptr, skeleton_global_ptr=skeleton_global_ptr, margin=margin,
                                flags=_lib.LOD_EXCLUSIVE if exclusive else 0, stream=stream)

    def skin(self, skin_ptr: int, out_positions_ptrs, count: int, indices_ptr: int, list_counts_ptr: int, max_lists=None,
             compact: bool = False, out_normals_ptrs=None, stream: int = 0, out_tangents_ptrs=None) -> None:
        """skin_listed() once per level: meshes[r] over row r of select()'s indices ([ranges][count] int32)
        with list_counts[r], into out_positions_ptrs[r] (and out_normals_ptrs[r]).  max_lists[r] is the
        caller's bound on list r's length (it sizes that launch); `count` where not given.
        out_tangents_ptrs[r]: level r's tangents (its mesh has tangents), or 0 / None for none."""
        for r, mesh in enumerate(self.meshes):
            bound = count if max_lists is None else int(max_lists[r])
            mesh.skin_listed(skin_ptr, out_positions_ptrs[r], count, indices_ptr + 4 * r * count, list_counts_ptr + 4 * r,
                             max_list=bound, compact=compact, out_normals_ptr=0 if out_normals_ptrs is None else out_normals_ptrs[r],
                             stream=stream, out_tangents_ptr=0 if out_tangents_ptrs is None else (out_tangents_ptrs[r] or 0))


def synthetic_mesh(parents, rest_globals, vertex_count: int, influences: int, seed: int):
    """A seeded mesh around a rig: (positions [V][3], normals [V][3], bone_indices [V][K], weights [V][K]).

    Vertices are scattered around the bone origins of `rest_globals` [bones][12] in bone order
    (vertex v belongs to bone v * bones // V), so neighbouring vertices share bones.  A vertex is
    bound to its bone, then to that bone's ancestors from the parent upwards, then (K = 8) to its
    descendants breadth first; a rig too small to fill the K slots repeats the vertex's own bone.
    Weights are positive, fall off along the list and sum to 1 in float32 arithmetic; normals are
    unit vectors."""
    if influences not in (4, 8):
        raise ValueError("influences must be 4 or 8")
    parents = [int(p) for p in parents]
    B = len(parents)
    rest = np.asarray(rest_globals, np.float32).reshape(B, 12)
    rng = np.random.default_rng(seed)
    children = [[] for _ in range(B)]
    for b, p in enumerate(parents):
        if p >= 0:
            children[p].append(b)
    lists = []
    for b in range(B):
        seq, a = [b], parents[b]
        while a >= 0 and len(seq) < influences and a not in seq:
            seq.append(a)
            a = parents[a]
        queue = list(children[b])
        while queue and len(seq) < influences:
            c = queue.pop(0)
            if c not in seq:
                seq.append(c)
                queue.extend(children[c])
        lists.append(seq + [b] * (influences - len(seq)))
    lists = np.asarray(lists, np.int32).reshape(B, influences)
    V = int(vertex_count)
    bone = (np.arange(V, dtype=np.int64) * B // max(V, 1)).astype(np.int64)
    positions = (rest[bone, 9:12] + rng.normal(0.0, 0.1, (V, 3))).astype(np.float32)
    normals = rng.normal(0.0, 1.0, (V, 3))
    normals = (normals / np.maximum(np.linalg.norm(normals, axis=1, keepdims=True), 1e-12)).astype(np.float32)
    raw = rng.uniform(0.25, 1.0, (V, influences)) * 0.5 ** np.arange(influences)
    weights = (raw / raw.sum(axis=1, keepdims=True)).astype(np.float32)
    return positions, normals, lists[bone], weights


def synthetic_shapes(positions, normals, shape_count: int, seed: int):
    """Seeded dense blend shapes for a mesh: (shape_positions [P][V][3], shape_normals [P][V][3], or
    None when `normals` is None).  Position offsets are smooth in the vertex order (a few sine waves
    of amplitude up to 0.05 per shape, as a body-shape or face slider moves neighbouring vertices
    together) plus a little noise; normal offsets have magnitude at most 0.1."""
    pos = np.asarray(positions, np.float32)
    V, P = pos.shape[0], int(shape_count)
    rng = np.random.default_rng(seed)
    t = np.arange(V, dtype=np.float64)[None, :, None] / max(V, 1)
    freq = rng.uniform(1.0, 8.0, (P, 1, 3))
    phase = rng.uniform(0.0, 2.0 * np.pi, (P, 1, 3))
    amp = rng.uniform(0.01, 0.05, (P, 1, 3))
    sp = (amp * np.sin(2.0 * np.pi * freq * t + phase) + rng.normal(0.0, 0.002, (P, V, 3))).astype(np.float32)
    if normals is None:
        return sp, None
    d = rng.normal(0.0, 1.0, (P, V, 3))
    d /= np.maximum(np.linalg.norm(d, axis=2, keepdims=True), 1e-12)
    sn = (d * rng.uniform(0.0, 0.1, (P, V, 1))).astype(np.float32)
    return sp, sn


def synthetic_tangents(positions, normals, seed: int):
    """Seeded tangents for a mesh: [V][4], xyz a unit vector perpendicular to the vertex's normal (a random
    direction with its normal component removed) and w the binormal sign, +1 or -1."""
    nrm = np.asarray(normals, np.float64)
    V = np.asarray(positions).shape[0]
    assert nrm.shape == (V, 3), nrm.shape
    rng = np.random.default_rng(seed)
    n = nrm / np.maximum(np.linalg.norm(nrm, axis=1, keepdims=True), 1e-12)
    d = rng.normal(0.0, 1.0, (V, 3))
    t = d - n * (d * n).sum(axis=1, keepdims=True)
    # (a direction along the normal leaves nothing: take the normal's cross product with its least axis instead)
    axis = np.eye(3)[np.argmin(np.abs(n), axis=1)] if V else np.zeros((0, 3))
    t = np.where(np.linalg.norm(t, axis=1, keepdims=True) < 1e-6, np.cross(n, axis), t)
    t /= np.maximum(np.linalg.norm(t, axis=1, keepdims=True), 1e-12)
    sign = np.where(rng.uniform(0.0, 1.0, (V, 1)) < 0.5, -1.0, 1.0)
    return np.concatenate([t, sign], axis=1).astype(np.float32)


def synthetic_shape_tangents(tangents, shape_count: int, seed: int):
    """Seeded tangent offsets of dense blend shapes: [P][V][3], magnitude at most 0.1 as synthetic_shapes' normals."""
    V, P = np.asarray(tangents).shape[0], int(shape_count)
    rng = np.random.default_rng(seed)
    d = rng.normal(0.0, 1.0, (P, V, 3))
    d /= np.maximum(np.linalg.norm(d, axis=2, keepdims=True), 1e-12)
    return (d * rng.uniform(0.0, 0.1, (P, V, 1))).astype(np.float32)
