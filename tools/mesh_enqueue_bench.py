"""Host-side cost of a call of the mesh entries and their two neighbours on the plan: back-to-back enqueues at
the smallest launch, no synchronisation inside the loop and one at the end (tools/enqueue_bench.py's method).

    [MBIK_LIB_OVERRIDE=other/libmbik.so] python tools/mesh_enqueue_bench.py [CALLS [REPEATS]]

The mesh is the refusal ledger's (tests/test_mesh_refusals_cpu.py): B = 2, V = 3, K = 4, normals, tangents, one
relative shape; count = 4, max_list = 4, one plane, two LOD ranges.  The plan is C1's rig, count = 4.  Entries:
mbik_skin_vertices, mbik_skin_vertices_listed, mbik_skin_vertices_call (listed, shaped, with tangents),
mbik_skin_bounds, mbik_cull_boxes, mbik_cull_lod, mbik_pose_globals, mbik_pose_blend, through raw ctypes.  Per
entry and repeat, microseconds per call up to the loop's return.  Prints one JSON line; compare libraries in
alternating fresh processes.
"""
import ctypes as C
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from many_bone_ik_amd import _lib  # noqa: E402
from many_bone_ik_amd import workloads as W  # noqa: E402
from many_bone_ik_amd.skinning import Mesh  # noqa: E402
from many_bone_ik_amd.solver import Plan  # noqa: E402

B, V, K, P, COUNT = 2, 3, 4, 1, 4


def main(calls=2000, repeats=3):
    dev = torch.device("cuda", 0)
    L = _lib.load()
    idx = ((np.arange(V)[:, None] + np.arange(K)[None, :]) % B).astype(np.int32)
    nrm = np.array([[1, 0, 0], [0, 1, 0], [0.6, 0.8, 0]], np.float32)
    tan = np.array([[0, 1, 0, 1], [0, 0, 1, -1], [0, 0, 1, 1]], np.float32)
    mesh = Mesh(B, np.array([[0, 0, 0], [1, 0.5, 0], [0.25, 1, -1]], np.float32), idx, np.full((V, K), 1.0 / K, np.float32), nrm,
                shape_positions=np.full((P, V, 3), 0.125, np.float32), shape_normals=np.full((P, V, 3), 0.0625, np.float32), tangents=tan,
                shape_tangents=np.full((P, V, 3), 0.03125, np.float32))
    keep = []

    def d(a):
        keep.append(torch.from_numpy(np.ascontiguousarray(a)).to(dev))
        return C.c_void_p(keep[-1].data_ptr())

    skin = d(np.tile(np.array([1, 0, 0, 0, 0, 1, 0, -1, 0, 0.5, 0.25, -0.5], np.float32), (COUNT, B, 1)))
    weights, indices, list_count = d(np.linspace(0, 1, COUNT * P, dtype=np.float32)), d(np.array([1, 3, 0, 2], np.int32)), d(np.array([2], np.int32))
    out_p, out_n, out_t = (d(np.zeros((COUNT, V, w), np.float32)) for w in (3, 3, 4))
    boxes, glob = d(np.tile(np.array([-0.5, -0.5, -0.5, 1, 1, 1], np.float32), (COUNT, 1))), d(np.tile(np.array([1, 0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0], np.float32), (COUNT, 1)))
    visible, cull_idx, visible_count, state, level = d(np.zeros(COUNT, np.uint8)), d(np.zeros(COUNT, np.int32)), d(np.zeros(1, np.int32)), d(np.zeros(COUNT, np.uint8)), d(np.zeros(COUNT, np.uint8))
    lod_idx, list_counts = d(np.zeros((2, COUNT), np.int32)), d(np.zeros(2, np.int32))
    planes, camera = np.array([[1, 0, 0, 2.0]], np.float32), np.array([0.5, 0.0, -1.0], np.float32)
    ranges = np.array([[0.0, 2.0, 0.1, 0.2], [2.0, 0.0, 0.2, 0.0]], np.float32)
    hp = lambda a: C.c_void_p(a.ctypes.data)   # noqa: E731
    call = _lib.MbikSkinCall(C.sizeof(_lib.MbikSkinCall), COUNT, skin, weights, indices, list_count, COUNT, 0, out_p, out_n, out_t)
    wl = W.generate(1, COUNT)
    plan = Plan.from_workload(wl)
    pose, pose_mod = d(wl.pose), d(wl.pose)
    pose_out, globs = d(np.zeros_like(wl.pose)), d(np.zeros(wl.pose.shape[:2] + (12,), np.float32))
    h = mesh.h
    entries = {
        "skin_vertices": lambda: L.mbik_skin_vertices(h, COUNT, skin, out_p, out_n, None),
        "skin_vertices_listed": lambda: L.mbik_skin_vertices_listed(h, COUNT, indices, list_count, COUNT, skin, weights, 0, out_p, out_n, None),
        "skin_vertices_call": lambda: L.mbik_skin_vertices_call(h, C.byref(call), None),
        "skin_bounds": lambda: L.mbik_skin_bounds(h, COUNT, skin, boxes, None),
        "cull_boxes": lambda: L.mbik_cull_boxes(h, COUNT, boxes, glob, 0.25, 1, hp(planes), visible, cull_idx, visible_count, None),
        "cull_lod": lambda: L.mbik_cull_lod(h, COUNT, boxes, glob, 0.25, 1, hp(planes), hp(camera), 2, hp(ranges), 0, state, level, lod_idx,
                                            list_counts, None),
        "pose_globals": lambda: L.mbik_pose_globals(plan.h, COUNT, pose, None, globs, None, None, None),
        "pose_blend": lambda: L.mbik_pose_blend(plan.h, COUNT, pose, pose_mod, 0.5, None, pose_out, None),
    }
    out = {"lib": _lib.LIB_PATH, "calls": calls, "enqueue_us": {}}
    for name, f in entries.items():
        for _ in range(200):
            assert f() == _lib.MBIK_OK, (name, _lib.last_error())
        torch.cuda.synchronize()
        rounds = []
        for _ in range(repeats):
            t0 = time.perf_counter()
            for _ in range(calls):
                f()
            t1 = time.perf_counter()
            torch.cuda.synchronize()
            rounds.append(round((t1 - t0) / calls * 1e6, 3))
        out["enqueue_us"][name] = rounds
    plan.close()
    mesh.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main(*(int(a) for a in sys.argv[1:3]))
