"""mbik_skin_vertices_call on the GPU against mbik_skin_vertices_call_cpu, bitwise (two NaNs count as equal;
the sign w bit for bit): every output is compared whole, listed rows with the host's bits and every other row with its
sentinel, behind guards of a row and more.  The range call plain and shaped over tile ends, vertex lanes and chunks; lists
with duplicates, out-of-range entries and clamped counts; float-aligned out_tangents; offsets past 2^31; out_tangents NULL
against the existing device entries; the existing device kernels fed the tangents as normals; the chain pose_globals ->
bounds -> LOD lists -> listed skinning of three meshes with tangents; the refusals with the host entry's texts."""
import ctypes as C

import numpy as np
import pytest

from many_bone_ik_amd import _lib
from many_bone_ik_amd import workloads as W
from many_bone_ik_amd.skinning import (Mesh, MeshLod, _skin_call, bone_boxes_cpu, cull_lod_cpu, skin_bounds_cpu, skin_vertices_listed_cpu,
                                       synthetic_mesh, synthetic_tangents)
from many_bone_ik_amd.solver import Plan, pose_globals_cpu

from . import skin_cases as S
from . import tangent_recipe as T
from .test_gpu_parity import torch_dev  # noqa: F401 (fixture)
from .test_gpu_skin_list import DeviceCase, list_buffers

pytestmark = pytest.mark.gpu

F = np.float32
SENTINEL = T.SENTINEL
PAD = 16
MODES = [None, "relative", "normalized"]
MODE_IDS = ["plain", "relative", "normalized"]


class Out:
    """One output buffer of `width` floats a vertex: `off` floats of shift, a guard of one row + PAD, the rows, the same guard."""

    def __init__(self, torch, dev, rows, V, width, off=0):
        self.off, self.guard, self.rows, self.V, self.width = off, V * width + PAD, rows, V, width
        self.t = torch.full((off + 2 * self.guard + rows * V * width,), SENTINEL, dtype=torch.float32, device=dev)
        self.ptr = self.t[off + self.guard:].data_ptr()

    def read(self):
        h = self.t.cpu().numpy()
        a, b = self.off + self.guard, self.off + self.guard + self.rows * self.V * self.width
        assert (h[:a] == F(SENTINEL)).all() and (h[b:] == F(SENTINEL)).all()
        return h[a:b].reshape(self.rows, self.V, self.width)


def bits_equal(a, b):
    return np.array_equal(np.ascontiguousarray(a, F).view(np.uint32), np.ascontiguousarray(b, F).view(np.uint32))


def check_call(torch, dev, mesh, d, shaped, indices=None, list_count=0, max_list=0, compact=False, off_t=0, stream=0):
    """One device call with all three outputs, compared whole with the host entry's; -> the tangents."""
    case = d.case
    listed = indices is not None
    rows = max_list if listed and compact else case.count
    outs = [Out(torch, dev, rows, case.V, 3), Out(torch, dev, rows, case.V, 3), Out(torch, dev, rows, case.V, 4, off_t)]
    kw = {}
    if listed:
        t_ind, p_ind, t_cnt = list_buffers(torch, dev, indices, list_count, max_list)
        kw = dict(indices_ptr=p_ind, list_count_ptr=t_cnt[1:].data_ptr(), max_list=max_list, compact=compact)
    torch.cuda.synchronize()
    mesh.skin_call(d.skin_ptr, outs[0].ptr, case.count, outs[1].ptr, outs[2].ptr, shape_weights_ptr=d.w_ptr if shaped else 0, stream=stream, **kw)
    torch.cuda.synchronize()
    desc, _keep = case.desc()
    ckw = dict(indices=indices[:max_list], list_count=list_count, max_list=max_list, compact=compact) if listed else {}
    rc, ref_p, ref_n, ref_t = T.call_cpu(desc, case.count, case.skin, case.V, shape_weights=case.cw if shaped else None, **ckw)
    assert rc == 0, T.last_error()
    got = [o.read() for o in outs]
    tag = (case.B, case.V, case.K, case.count, case.P, shaped, list_count, max_list, compact, off_t)
    assert S.same_bits(got[0], ref_p) and S.same_bits(got[1], ref_n) and S.same_bits(got[2], ref_t), tag
    assert bits_equal(got[2][..., 3], ref_t[..., 3]), tag
    return got[2]


# ---------------- the range call, plain and shaped ----------------
@pytest.mark.parametrize("mode", MODES, ids=MODE_IDS)
@pytest.mark.parametrize("K", [4, 8])
@pytest.mark.parametrize("B", [1, 32, 200])
def test_range(mbik, torch_dev, B, K, mode):
    """V 1, 63, 65, 257 (64, 128 and 256 vertex lanes) and 1000 (more than one chunk); counts 1, 17 and 33, which end in a short
    tile for S = 16 (B = 1), 13 (B = 32) and 2 (B = 200); P 3 and 17; weights under the threshold, NaN weights and skeletons
    with every weight skipped inside one tile."""
    torch, dev = torch_dev
    for i, (V, count) in enumerate(((1, 33), (63, 17), (65, 1), (257, 33), (1000, 17))):
        P = (3, 17)[i % 2] if mode else 0
        case = T.Case(1000 + 10 * B + K + i, B, V, K, count, P=P, mode=mode or "relative", special_weights=bool(mode))
        if mode and count > 2:
            assert (np.abs(np.nan_to_num(case.cw[2])) <= 0.0001).all() and np.isnan(case.cw).any()
        d = DeviceCase(torch, dev, case)
        with Mesh(B, case.pos, case.idx, case.w, **case.mesh_kw()) as mesh:
            assert mesh.has_tangents
            Sx, chunks = mesh.launch_shape(count)
            assert count in (1, Sx) or count % Sx != 0
            assert V != 1000 or B == 200 or chunks > 1
            check_call(torch, dev, mesh, d, bool(mode))
            if mode and i == 1:
                check_call(torch, dev, mesh, d, False)            # the base tangents of a shaped mesh, not renormalised


# ---------------- lists ----------------
@pytest.mark.parametrize("compact", [False, True], ids=["in_place", "compact"])
@pytest.mark.parametrize("mode", MODES, ids=MODE_IDS)
@pytest.mark.parametrize("K", [4, 8])
def test_listed(mbik, torch_dev, K, mode, compact):
    """Duplicates, -1 and count among valid entries over more than one tile; list_count 0, negative and above max_list; max_list
    above count; unlisted rows keep their sentinel (the whole-buffer compare)."""
    torch, dev = torch_dev
    B, V, count = 32, 129, 20
    case = T.Case(2000 + K, B, V, K, count, P=3 if mode else 0, mode=mode or "relative", special_weights=bool(mode))
    d = DeviceCase(torch, dev, case)
    long_list = np.array([4, -1, 9, count, 0, count - 1, -1, 2, 11, 19, count, 7, -1, 4, 4, 9,
                          count, 3, 8, 1, -1, 6, 10, 12, 14, 16, 18, 0, count, 5], np.int32)
    assert len(long_list) > count and len(long_list) > 2 * 13        # max_list above count, and more than two tiles of 13
    with Mesh(B, case.pos, case.idx, case.w, **case.mesh_kw()) as mesh:
        for indices, list_count, max_list in ((long_list, len(long_list), len(long_list)), (long_list, 17, len(long_list)),
                                              (long_list, 0, len(long_list)), (long_list, -3, 14), (long_list, 2 ** 31 - 1, 14),
                                              (np.array([7, 7, 7], np.int32), 3, 3)):
            got = check_call(torch, dev, mesh, d, bool(mode), indices, list_count, max_list, compact)
            n = T.list_length(list_count, max_list)
            valid = [(r, int(s)) for r, s in enumerate(indices[:n]) if 0 <= s < count]
            written = int((got[:, 0, 3] != F(SENTINEL)).sum())
            assert written == (len(valid) if compact else len({s for _, s in valid}))


@pytest.mark.parametrize("V", [1, 63, 65, 257, 1000])
def test_listed_vertex_lanes_and_chunks(mbik, torch_dev, V):
    torch, dev = torch_dev
    case = T.Case(2500 + V, 32, V, 8, 31, P=17, mode="normalized", special_weights=True)
    d = DeviceCase(torch, dev, case)
    indices = np.random.default_rng(V).permutation(31).astype(np.int32)[:29]
    indices[[3, 17]] = [-1, 31]
    with Mesh(case.B, case.pos, case.idx, case.w, **case.mesh_kw()) as mesh:
        for compact in (False, True):
            check_call(torch, dev, mesh, d, True, indices, 29, 29, compact)
            check_call(torch, dev, mesh, d, False, indices, 14, 29, compact)


# ---------------- float alignment ----------------
@pytest.mark.parametrize("shift", [1, 2, 3])
def test_float_aligned_out_tangents(mbik, torch_dev, shift):
    torch, dev = torch_dev
    case = T.Case(3000, 32, 65, 4, 20, P=4, special_weights=True)
    d = DeviceCase(torch, dev, case)
    indices = np.array([19, 0, 7, 7, -1, 3, 12, 20, 5, 1, 18, 2, 9, 4, 11], np.int32)
    with Mesh(case.B, case.pos, case.idx, case.w, **case.mesh_kw()) as mesh:
        for shaped in (False, True):
            check_call(torch, dev, mesh, d, shaped, off_t=shift)
            for compact in (False, True):
                check_call(torch, dev, mesh, d, shaped, indices, len(indices), len(indices), compact, off_t=shift)


# ---------------- offsets past 2^31 ----------------
def test_offsets_past_2_31(mbik, torch_dev):
    """count x V x 4 > 2^31 floats (8.6 GB of tangents, 6.4 GB each of positions and normals), in place, the list [0, count-1]:
    the two rows against a two-skeleton range call of the same matrices on the device and against the host entry; the rows next
    to them keep their sentinel."""
    torch, dev = torch_dev
    B, V, K, count = 2, 65537, 4, 8193
    assert count * V * 4 > 2 ** 31 > count * V * 3
    free, _ = torch.cuda.mem_get_info(dev)
    if free < 26 * 10 ** 9:
        pytest.skip(f"the three outputs need 21.5 GB of device memory and 26 GB free are asked for, {free / 1e9:.1f} GB free")
    case = T.Case(18, B, V, K, 2)
    skin = S.random_skin(19, count, B)
    case.skin = np.ascontiguousarray(skin[[0, count - 1]])
    d_skin = torch.from_numpy(skin).to(dev)
    d_two = torch.from_numpy(case.skin).to(dev)
    big = [torch.empty((count, V, w), dtype=torch.float32, device=dev) for w in (3, 3, 4)]
    small = [torch.full((2, V, w), SENTINEL, dtype=torch.float32, device=dev) for w in (3, 3, 4)]
    for b in big:
        b[1], b[-2] = SENTINEL, SENTINEL
    d_ind = torch.tensor([0, count - 1], dtype=torch.int32, device=dev)
    d_cnt = torch.tensor([2], dtype=torch.int32, device=dev)
    with Mesh(B, case.pos, case.idx, case.w, **case.mesh_kw()) as mesh:
        mesh.skin_listed(d_skin.data_ptr(), big[0].data_ptr(), count, d_ind.data_ptr(), d_cnt.data_ptr(), max_list=2,
                         out_normals_ptr=big[1].data_ptr(), out_tangents_ptr=big[2].data_ptr())
        mesh.skin(d_two.data_ptr(), small[0].data_ptr(), 2, out_normals_ptr=small[1].data_ptr(), out_tangents_ptr=small[2].data_ptr())
        torch.cuda.synchronize()
    for b, s in zip(big, small):
        assert torch.equal(b[0].view(torch.int32), s[0].view(torch.int32)) and torch.equal(b[-1].view(torch.int32), s[1].view(torch.int32))
        assert bool((b[1] == SENTINEL).all()) and bool((b[-2] == SENTINEL).all())
    desc, _keep = case.desc()
    rc, ref_p, ref_n, ref_t = T.call_cpu(desc, 2, case.skin, V)
    assert rc == 0
    assert S.same_bits(small[0].cpu().numpy(), ref_p) and S.same_bits(small[1].cpu().numpy(), ref_n) and S.same_bits(small[2].cpu().numpy(), ref_t)
    del big


# ---------------- out_tangents NULL: the existing device entries ----------------
@pytest.mark.parametrize("mode", MODES, ids=MODE_IDS)
@pytest.mark.parametrize("K", [4, 8])
def test_without_out_tangents_it_is_the_existing_entry(mbik, torch_dev, K, mode):
    """The new call without out_tangents against mbik_skin_vertices / _shaped / _listed on the same mesh (with tangents) and the
    same buffers, device with device, bitwise, with normals and positions only."""
    torch, dev = torch_dev
    B, V, count = 32, 700, 27
    case = T.Case(4000 + K, B, V, K, count, P=3 if mode else 0, mode=mode or "relative", special_weights=bool(mode))
    d = DeviceCase(torch, dev, case)
    indices = np.array([26, 3, 3, -1, 14, 27, 0, 9, 21, 5, 12, 13, 1, 2, 8, 25], np.int32)
    t_ind, p_ind, t_cnt = list_buffers(torch, dev, indices, len(indices), len(indices))
    w = d.w_ptr if mode else 0
    with Mesh(B, case.pos, case.idx, case.w, **case.mesh_kw()) as mesh:
        assert mesh.launch_shape(count)[1] > 1
        for normals in (True, False):
            for form in ("range", "in_place", "compact"):
                rows = len(indices) if form == "compact" else count
                new, old = [[Out(torch, dev, rows, V, 3), Out(torch, dev, rows, V, 3)] for _ in range(2)]
                lkw = {} if form == "range" else dict(indices_ptr=p_ind, list_count_ptr=t_cnt[1:].data_ptr(), max_list=len(indices),
                                                      compact=form == "compact")
                mesh.skin_call(d.skin_ptr, new[0].ptr, count, new[1].ptr if normals else 0, 0, shape_weights_ptr=w, **lkw)
                if form == "range":
                    mesh.skin(d.skin_ptr, old[0].ptr, count, out_normals_ptr=old[1].ptr if normals else 0, shape_weights_ptr=w)
                else:
                    mesh.skin_listed(d.skin_ptr, old[0].ptr, count, p_ind, t_cnt[1:].data_ptr(), max_list=len(indices),
                                     compact=form == "compact", out_normals_ptr=old[1].ptr if normals else 0, shape_weights_ptr=w)
                torch.cuda.synchronize()
                for a, b in zip(new, old):
                    assert torch.equal(a.t.view(torch.int32), b.t.view(torch.int32)), (form, normals)
                assert bool((new[0].t != SENTINEL).any()) and (normals or bool((new[1].t == SENTINEL).all()))


# ---------------- the existing kernels fed the tangents as normals ----------------
@pytest.mark.parametrize("mode", MODES, ids=MODE_IDS)
@pytest.mark.parametrize("K", [4, 8])
def test_tangents_as_normals_on_the_device(mbik, torch_dev, K, mode):
    """A second mesh carries the tangents' xyz as its normals and the shape tangents as its shape normals; the EXISTING device
    entries on it write, as normals, out_tangents.xyz of the new call, in the range and in both listed forms."""
    torch, dev = torch_dev
    B, V, count = 32, 300, 17
    case = T.Case(5000 + K, B, V, K, count, P=17 if mode else 0, mode=mode or "relative", special_weights=bool(mode))
    d = DeviceCase(torch, dev, case)
    indices = np.array([16, 3, 3, -1, 14, 17, 0, 9], np.int32)
    t_ind, p_ind, t_cnt = list_buffers(torch, dev, indices, len(indices), len(indices))
    w = d.w_ptr if mode else 0
    as_kw = dict(normals=np.ascontiguousarray(case.tan[:, :3]))
    if mode:
        as_kw.update(shape_positions=case.sp, shape_normals=case.st, shape_mode=case.mode)
    with Mesh(B, case.pos, case.idx, case.w, **case.mesh_kw()) as mesh, Mesh(B, case.pos, case.idx, case.w, **as_kw) as as_mesh:
        assert not as_mesh.has_tangents
        for form in ("range", "in_place", "compact"):
            rows = len(indices) if form == "compact" else count
            got_t = check_call(torch, dev, mesh, d, bool(mode), *(() if form == "range" else (indices, len(indices), len(indices), form == "compact")))
            o_p, o_n = Out(torch, dev, rows, V, 3), Out(torch, dev, rows, V, 3)
            if form == "range":
                as_mesh.skin(d.skin_ptr, o_p.ptr, count, out_normals_ptr=o_n.ptr, shape_weights_ptr=w)
            else:
                as_mesh.skin_listed(d.skin_ptr, o_p.ptr, count, p_ind, t_cnt[1:].data_ptr(), max_list=len(indices), compact=form == "compact",
                                    out_normals_ptr=o_n.ptr, shape_weights_ptr=w)
            torch.cuda.synchronize()
            assert S.same_bits(o_n.read(), got_t[..., :3]), form


# ---------------- the full chain ----------------
@pytest.mark.parametrize("compact", [False, True], ids=["in_place", "compact"])
def test_chain_pose_globals_bounds_lod_skin_with_tangents(mbik, torch_dev, compact):
    """pose_globals(inv_bind) -> bounds -> LOD lists -> listed skinning with tangents of three meshes (K = 8, 4, 4) on one side
    stream with nothing in between, on the C2 rig, against the host chain.  The ranges are cut at the terciles of the reference
    boxes' distance from the camera, so that no list is empty (asserted on the reference lists)."""
    torch, dev = torch_dev
    n, Vs, Ks = 96, (300, 65, 9), (8, 4, 4)
    wl = W.generate(2, n)
    parents, pins = wl.topo.parents.tolist(), wl.topo.pins.tolist()
    B = len(parents)
    rest, _ = pose_globals_cpu(parents, [], wl.pose[:1])
    inv_bind = np.random.default_rng(25).uniform(-1.0, 1.0, (B, 12)).astype(F)
    arrays = []
    for V, K in zip(Vs, Ks):
        pos, nrm, idx, w = synthetic_mesh(parents, rest[0], V, K, seed=60 + V)
        arrays.append((pos, nrm, idx, w, synthetic_tangents(pos, nrm, seed=61 + V)))
    # the host chain
    skin, _ = pose_globals_cpu(parents, pins, wl.pose, inv_bind=inv_bind)
    bb, used = bone_boxes_cpu(B, arrays[0][0], arrays[0][2], arrays[0][3])
    boxes = skin_bounds_cpu(bb, used, skin)
    camera = np.array([40.0, 3.0, -2.0], F)
    dist = np.linalg.norm(boxes[:, :3].astype(np.float64) + 0.5 * boxes[:, 3:] - camera, axis=1)
    q1, q2 = np.sort(dist)[[n // 3, (2 * n) // 3]]
    ranges = np.array([[0, q1, 0, 0], [q1, q2, 0, 0], [q2, 0, 0, 0]], F)
    planes = np.zeros((0, 4), F)
    state = np.zeros(n, np.uint8)
    ref_state, ref_level, lists = cull_lod_cpu(boxes, planes, camera, ranges, state, flags=_lib.LOD_EXCLUSIVE)
    assert all(len(l) >= 5 for l in lists) and sum(len(l) for l in lists) <= n
    want = []
    for (pos, nrm, idx, w, tan), lst, V in zip(arrays, lists, Vs):
        padded = np.concatenate([lst, np.full(n - len(lst), -1, np.int32)])
        want.append(skin_vertices_listed_cpu(B, pos, idx, w, skin, padded, len(lst), max_list=n, compact=compact, normals=nrm, tangents=tan,
                                             out_positions=np.full((n, V, 3), F(SENTINEL), F), out_normals=np.full((n, V, 3), F(SENTINEL), F),
                                             out_tangents=np.full((n, V, 4), F(SENTINEL), F)))
    # the device chain
    plan = Plan.from_workload(wl)
    d_pose, d_ib = torch.from_numpy(wl.pose).to(dev), torch.from_numpy(inv_bind).to(dev)
    d_g = torch.empty((n, B, 12), dtype=torch.float32, device=dev)
    d_b = torch.zeros(n * 6, dtype=torch.float32, device=dev)
    d_state = torch.zeros(n, dtype=torch.uint8, device=dev)
    d_ind = torch.full((3 * n,), -777, dtype=torch.int32, device=dev)
    d_cnt = torch.full((3,), 123456789, dtype=torch.int32, device=dev)
    outs = [[Out(torch, dev, n, V, width) for width in (3, 3, 4)] for V in Vs]
    meshes = [Mesh(B, pos, idx, w, normals=nrm, tangents=tan) for pos, nrm, idx, w, tan in arrays]
    try:
        lod = MeshLod(meshes, ranges)
        torch.cuda.synchronize()
        st = torch.cuda.Stream(device=dev)
        plan.pose_globals(d_pose.data_ptr(), d_g.data_ptr(), n, inv_bind_ptr=d_ib.data_ptr(), stream=st.cuda_stream)
        meshes[0].bounds(d_g.data_ptr(), d_b.data_ptr(), n, stream=st.cuda_stream)
        lod.select(d_b.data_ptr(), n, planes, camera, d_state.data_ptr(), d_ind.data_ptr(), d_cnt.data_ptr(), stream=st.cuda_stream)
        lod.skin(d_g.data_ptr(), [o[0].ptr for o in outs], n, d_ind.data_ptr(), d_cnt.data_ptr(), compact=compact,
                 out_normals_ptrs=[o[1].ptr for o in outs], out_tangents_ptrs=[o[2].ptr for o in outs], stream=st.cuda_stream)
        st.synchronize()
    finally:
        for m in meshes:
            m.close()
        plan.close()
    assert S.same_bits(d_g.cpu().numpy(), skin) and np.array_equal(d_state.cpu().numpy(), ref_state)
    assert d_cnt.cpu().tolist() == [len(l) for l in lists]
    ind = d_ind.cpu().numpy().reshape(3, n)
    for r in range(3):
        assert np.array_equal(ind[r, :len(lists[r])], lists[r])
        for o, ref in zip(outs[r], want[r]):
            assert S.same_bits(o.read(), ref), r
        assert bits_equal(outs[r][2].read()[..., 3], want[r][2][..., 3])


# ---------------- refusals ----------------
def test_refusals_through_the_device_entry(mbik, torch_dev):
    """tests/tangent_recipe.py's table through mbik_skin_vertices_call, with the texts mbik_skin_vertices_call_cpu gives for the
    same calls on host buffers; nothing is launched by a refused call."""
    torch, dev = torch_dev
    L = _lib.load()
    B, V, P, n, M = 5, 9, 2, 3, 4
    lay = T.RefusalLayout(B, V, P, n, M)
    case, plain_case = T.Case(500, B, V, 4, n, P=P), T.Case(500, B, V, 4, n)
    buf = torch.zeros(lay.words, dtype=torch.float32, device=dev)
    hbuf = np.zeros(lay.words, F)
    meshes = {"tan": Mesh(B, plain_case.pos, plain_case.idx, plain_case.w, **plain_case.mesh_kw()),
              "shaped_tan": Mesh(B, case.pos, case.idx, case.w, **case.mesh_kw()),
              "normals": Mesh(B, plain_case.pos, plain_case.idx, plain_case.w, normals=plain_case.nrm),
              "plain": Mesh(B, plain_case.pos, plain_case.idx, plain_case.w)}
    descs = {"tan": plain_case.desc(), "shaped_tan": case.desc(), "normals": plain_case.desc(tangents=False)}
    d = plain_case.desc(tangents=False)
    d[0].normals = None
    descs["plain"] = d
    refused = []

    def make(base, skin, cw, ind, cnt, p, q, t, count, max_list, flags, struct_size):
        at = lambda o: None if o is None else base + 4 * o
        call = _skin_call(count, at(skin), at(p), at(q), at(t), at(cw), at(ind), at(cnt), max_list, flags)
        if struct_size is not None:
            call.struct_size = struct_size
        return call

    def run_device(mesh, **f):
        call = make(buf.data_ptr(), **f)
        rc = L.mbik_skin_vertices_call(meshes[mesh].h, C.byref(call), None)
        if rc != 0:
            refused.append(1)
            torch.cuda.synchronize()
            assert not bool(buf.any())                             # (before anything ran: nothing was launched)
        return rc, T.last_error()

    def run_host(mesh, **f):
        call = make(hbuf.ctypes.data, **f)
        return L.mbik_skin_vertices_call_cpu(C.byref(descs[mesh][0]), C.byref(call)), T.last_error()

    try:
        seen = T.call_refusals(lay, run_device)
        assert seen == T.call_refusals(lay, run_host) and len(refused) == len(seen)
        good = make(buf.data_ptr(), skin=lay.at["skin"], cw=None, ind=None, cnt=None, p=lay.at["p"], q=lay.at["q"], t=lay.at["t"], count=n,
                    max_list=0, flags=0, struct_size=None)
        assert L.mbik_skin_vertices_call(None, C.byref(good), None) == _lib.MBIK_EINVAL and T.last_error() == "null mesh"
        # nothing to do: OK without a launch
        for f in (dict(count=0), dict(ind=lay.at["ind"], cnt=lay.at["cnt"], max_list=0, flags=1)):
            call = make(buf.data_ptr(), **dict(dict(skin=None, cw=None, ind=None, cnt=None, p=None, q=None, t=None, count=n, max_list=0,
                                                    flags=0, struct_size=None), **f))
            assert L.mbik_skin_vertices_call(meshes["tan"].h, C.byref(call), None) == _lib.MBIK_OK
        with Mesh(B, plain_case.pos[:0], plain_case.idx[:0], plain_case.w[:0], normals=plain_case.nrm[:0], tangents=plain_case.tan[:0]) as empty:
            call = make(buf.data_ptr(), skin=None, cw=None, ind=None, cnt=None, p=None, q=None, t=None, count=n, max_list=0, flags=0, struct_size=None)
            assert L.mbik_skin_vertices_call(empty.h, C.byref(call), None) == _lib.MBIK_OK
        # the descriptor's refusals through mbik_mesh_create_desc with a device present
        def create(dsc):
            h = C.c_void_p(1)
            rc = L.mbik_mesh_create_desc(None if dsc is None else C.byref(dsc), 0, C.byref(h))
            assert h.value is None
            return rc, T.last_error()
        assert len(T.desc_refusals(case, create)) >= 6
        torch.cuda.synchronize()
    finally:
        for m in meshes.values():
            m.close()
