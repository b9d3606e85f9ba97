"""Linear blend skinning of meshes from skin transforms (include/mbik.h, ABI 10).

`Mesh` owns one `mbik_mesh`: the mesh arrays of one surface (positions, optional normals, 4 or 8
bone indices and weights a vertex) resident on one GPU, bound to a bone count.  `Mesh.skin()`
takes device pointers -- the skin transforms are `Plan.pose_globals(..., inv_bind_ptr=...)`'s
output -- and is asynchronous on the given HIP stream.  `skin_vertices_cpu()` runs the same code
on numpy arrays without a device, and `synthetic_mesh()` is the seeded mesh generator the tests
and tools/skin_bench.py use.
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


class Mesh:
    """One mesh surface on one GPU (mbik_mesh_create).  Immutable; close() frees it."""

    def __init__(self, bone_count: int, positions, bone_indices, weights, normals=None, device: int = 0):
        self._L = _lib.load()
        pos, idx, wgt, nrm = _mesh_arrays(positions, bone_indices, weights, normals)
        self.bone_count, self.vertex_count, self.influences = int(bone_count), pos.shape[0], idx.shape[1]
        self.has_normals = nrm is not None
        self.device = device
        h = C.c_void_p()
        check(self._L.mbik_mesh_create(self.bone_count, self.vertex_count, self.influences, _ptr(pos), _ptr(nrm), _ptr(idx),
                                       _ptr(wgt), device, C.byref(h)))
        self.h = h

    def skin(self, skin_ptr: int, out_positions_ptr: int, count: int, out_normals_ptr: int = 0, stream: int = 0) -> None:
        """mbik_skin_vertices: out_positions [count][vertices][3] (and out_normals) from the device
        skin transforms [count][bones][12]; asynchronous on `stream`."""
        check(self._L.mbik_skin_vertices(self.h, count, C.c_void_p(skin_ptr or None), C.c_void_p(out_positions_ptr or None),
                                         C.c_void_p(out_normals_ptr or None), C.c_void_p(stream or None)))

    def launch_shape(self, count: int) -> tuple[int, int]:
        """(skeletons per block, vertex chunks) of a skin() call for `count` skeletons."""
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


def skin_vertices_cpu(bone_count: int, positions, bone_indices, weights, skin, normals=None):
    """mbik_skin_vertices_cpu (host only): `skin` [count][bones][12] -> (positions [count][V][3],
    normals [count][V][3] or None when the mesh has none)."""
    L = _lib.load()
    pos, idx, wgt, nrm = _mesh_arrays(positions, bone_indices, weights, normals)
    sk = np.ascontiguousarray(skin, np.float32)
    count, V = sk.shape[0], pos.shape[0]
    assert sk.shape == (count, bone_count, 12), sk.shape
    out_p = np.empty((count, V, 3), np.float32)
    out_n = None if nrm is None else np.empty((count, V, 3), np.float32)
    check(L.mbik_skin_vertices_cpu(bone_count, V, idx.shape[1], _ptr(pos), _ptr(nrm), _ptr(idx), _ptr(wgt), count, _ptr(sk),
                                   _ptr(out_p), _ptr(out_n)))
    return out_p, out_n


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
