"""Inputs and references shared by the list-driven skinning tests (tests/test_skin_list_cpu.py,
tests/test_gpu_skin_list.py).

The reference of a listed call is never the listed code: `expected` takes the rows the EXISTING
entries mbik_skin_vertices_cpu / mbik_skin_vertices_shaped_cpu computed for the whole batch and puts
them where include/mbik.h says a listed call writes them, over a buffer of sentinels.  Comparing a
whole output buffer with it (skin_cases.same_bits) checks the listed rows and that every other row
still holds the sentinel in one go.
"""
import numpy as np

from many_bone_ik_amd import workloads as W
from many_bone_ik_amd.skinning import bone_boxes_cpu, cull_boxes_cpu, skin_bounds_cpu, skin_vertices_cpu, synthetic_mesh
from many_bone_ik_amd.solver import pose_globals_cpu

from . import morph_recipe as MR
from . import skin_cases as S

F = np.float32
SENTINEL = -12345.678
PAD = 16


def list_length(list_count, max_list):
    return min(max(int(list_count), 0), int(max_list))


def expected(full, indices, list_count, max_list, compact):
    """full [count][V][3]: the existing call's output for every skeleton.  -> the listed call's whole
    output, [max_list][V][3] compact or [count][V][3] in place, SENTINEL where nothing is written."""
    count = full.shape[0]
    out = np.full(((max_list if compact else count),) + full.shape[1:], SENTINEL, F)
    for r in range(list_length(list_count, max_list)):
        s = int(indices[r])
        if 0 <= s < count:
            out[r if compact else s] = full[s]
    return out


def guarded(rows, V):
    """A float32 output [rows][V][3] of sentinels with PAD sentinel floats in front and behind: (flat buffer, view)."""
    flat = np.full(PAD + rows * V * 3 + PAD, SENTINEL, F)
    return flat, flat[PAD:PAD + rows * V * 3].reshape(rows, V, 3)


def guards_intact(flat):
    return bool((flat[:PAD] == F(SENTINEL)).all() and (flat[-PAD:] == F(SENTINEL)).all())


class Case:
    """A random mesh, optionally shaped, with the existing calls' outputs for `count` skeletons."""

    def __init__(self, seed, B, V, K, count, normals=True, P=0, mode="relative", special_weights=False):
        self.B, self.V, self.K, self.count, self.P, self.mode = B, V, K, count, P, mode
        self.pos, nrm, self.idx, self.w = S.random_mesh(seed, B, V, K)
        self.nrm = nrm if normals else None
        self.skin = S.random_skin(seed + 1, count, B)
        self.sp = self.sn = self.cw = None
        if P:
            self.sp, sn = MR.random_shapes(seed + 2, P, V)
            self.sn = sn if normals else None
            self.cw = MR.random_shape_weights(seed + 3, count, P, 0 if mode == "relative" else 1).astype(F)
            if special_weights:
                # below the shader's threshold, and NaN: both are skipped; on every third and every fifth skeleton,
                # so that any list of some length names such skeletons and leaves others out
                self.cw[::3, 0] = 0.00005
                self.cw[1::5, P - 1] = np.nan
        self.plain_p, self.plain_n = skin_vertices_cpu(B, self.pos, self.idx, self.w, self.skin, normals=self.nrm)
        self.shaped_p = self.shaped_n = None
        if P:
            self.shaped_p, self.shaped_n = skin_vertices_cpu(B, self.pos, self.idx, self.w, self.skin, normals=self.nrm,
                                                             shape_positions=self.sp, shape_normals=self.sn, shape_mode=mode,
                                                             shape_weights=self.cw)

    def mesh_kw(self):
        kw = dict(normals=self.nrm)
        if self.P:
            kw.update(shape_positions=self.sp, shape_normals=self.sn, shape_mode=self.mode)
        return kw

    def full(self, shaped):
        return (self.shaped_p, self.shaped_n) if shaped else (self.plain_p, self.plain_n)


def cull_chain(n=64, K=4, V=300, seed=3):
    """The C2 rig with `n` skeletons and a mesh around it: dict(wl, parents, pins, B, inv_bind, pos, nrm, idx, w).
    chain_reference runs the host chain on poses of it."""
    wl = W.generate(2, n)
    parents, pins = wl.topo.parents.tolist(), wl.topo.pins.tolist()
    B = len(parents)
    rest, _ = pose_globals_cpu(parents, [], wl.pose[:1])
    inv_bind = np.random.default_rng(25).uniform(-1.0, 1.0, (B, 12)).astype(F)
    pos, nrm, idx, w = synthetic_mesh(parents, rest[0], V, K, seed=seed)
    return dict(wl=wl, parents=parents, pins=pins, B=B, inv_bind=inv_bind, pos=pos, nrm=nrm, idx=idx, w=w)


def chain_reference(c, pose):
    """The host chain from `pose` on: (skin, planes 1, planes 2, list 1, list 2), with the asserts on the
    reference lists themselves."""
    skin, _ = pose_globals_cpu(c["parents"], c["pins"], pose, inv_bind=c["inv_bind"])
    bb, used = bone_boxes_cpu(c["B"], c["pos"], c["idx"], c["w"])
    boxes = skin_bounds_cpu(bb, used, skin)
    planes1, planes2 = chain_planes(boxes)
    l1, l2 = cull_boxes_cpu(boxes, planes1)[1], cull_boxes_cpu(boxes, planes2)[1]
    count = skin.shape[0]
    assert 0 < len(l2) < len(l1) < count, (len(l1), len(l2), count)
    assert len(set(l1.tolist()) - set(l2.tolist())) > 0          # visible first, culled second
    return skin, planes1, planes2, l1, l2


def chain_planes(boxes):
    """Two one-plane frusta x <= d: a box is visible when its least x is at most d (include/mbik.h), so with d the
    2/3 and the 1/3 quantile of the boxes' least x the first list keeps about two thirds of the skeletons and the
    second about one third (derived from the data, so the lists are neither empty nor full; chain_reference asserts it)."""
    cx = np.sort(boxes[:, 0])
    d1, d2 = float(cx[(2 * len(cx)) // 3]), float(cx[len(cx) // 3])
    return np.array([[1, 0, 0, d1]], F), np.array([[1, 0, 0, d2]], F)
