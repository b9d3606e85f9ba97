"""mbik_skin_bounds and mbik_cull_boxes on the GPU against mbik_skin_bounds_cpu and
mbik_cull_boxes_cpu, bitwise (two NaNs count as equal), with sentinels in front of and behind every
output: rig sizes and used-bone tables over skeleton counts that end inside a wave, a block and a
skeleton tile; a NaN beside finite neighbours; float-aligned buffers; the largest rig; shaped meshes;
stream order; the visible list across the scan's second level; every output combination; error codes."""
import ctypes as C

import numpy as np
import pytest

from many_bone_ik_amd import _lib
from many_bone_ik_amd import workloads as W
from many_bone_ik_amd.skinning import Mesh, bone_boxes_cpu, cull_boxes_cpu, skin_bounds_cpu, synthetic_mesh
from many_bone_ik_amd.solver import Plan, pose_globals_cpu

from . import bounds_recipe as R
from . import morph_recipe as MR
from . import skin_cases as S
from .test_gpu_parity import torch_dev  # noqa: F401 (fixture)

pytestmark = pytest.mark.gpu

F = np.float32
SENTINEL = -12345.678
BYTE_SENTINEL = 0xAB
INT_SENTINEL = -777
PAD = 16
MAX_BONES = 3413   # MBIK_SKIN_MAX_BONES
# A bounds block takes min(20 KiB / (48 B a bone), 64) skeletons (host_bounds.cpp): 64 for B = 1, 13 for
# B = 32, 2 for B = 200, 1 at MAX_BONES.  A cull block takes 256 skeletons and the scan 256 blocks a pass.
TILE = {1: 64, 32: 13, 200: 2}


def table_mesh(seed, B, V, K, table):
    pos, nrm, idx, w = S.random_mesh(seed, B, V, K)
    if table == "full":
        idx[:, 0] = np.arange(V) % B          # (V >= B: every bone is named with a weight above 0)
    if table == "sparse":
        idx = (idx // 3 * 3).astype(np.int32)
    if table == "empty":
        w = np.zeros_like(w)
    return pos, nrm, idx, w


def run_bounds(torch, dev, mesh, skin, off_skin=0, off_b=0, stream=0):
    """Launches mbik_skin_bounds on device copies; `off` sentinel floats in front of the output (the
    buffer is shifted by that many floats) and PAD behind must come back untouched.  -> boxes [n][6]"""
    n = skin.shape[0]
    d_skin = torch.zeros(skin.size + off_skin, dtype=torch.float32, device=dev)
    d_skin[off_skin:] = torch.from_numpy(skin.reshape(-1)).to(dev)
    d_b = torch.full((off_b + n * 6 + PAD,), SENTINEL, dtype=torch.float32, device=dev)
    torch.cuda.synchronize()
    mesh.bounds(d_skin[off_skin:].data_ptr(), d_b[off_b:].data_ptr(), n, stream=stream)
    torch.cuda.synchronize()
    h = d_b.cpu().numpy()
    assert (h[:off_b] == F(SENTINEL)).all() and (h[off_b + n * 6:] == F(SENTINEL)).all()
    return h[off_b:off_b + n * 6].reshape(n, 6)


class CullBuffers:
    """Device outputs of one cull with sentinels around each and garbage in visible_count."""

    def __init__(self, torch, dev, n):
        self.n, self.front = n, 8
        self.visible = torch.full((self.front + n + PAD,), BYTE_SENTINEL, dtype=torch.uint8, device=dev)
        self.indices = torch.full((self.front + n + PAD,), INT_SENTINEL, dtype=torch.int32, device=dev)
        self.count = torch.full((self.front + 1 + PAD,), INT_SENTINEL, dtype=torch.int32, device=dev)
        self.count[self.front] = 123456789   # garbage: the call must not rely on a cleared count

    def ptrs(self, visible, indices, count):
        f = self.front
        return dict(visible_ptr=self.visible[f:].data_ptr() if visible else 0, indices_ptr=self.indices[f:].data_ptr() if indices else 0,
                    visible_count_ptr=self.count[f:].data_ptr() if count else 0)

    def check(self, ref_vis, visible, indices, count):
        f, n = self.front, self.n
        v, i, c = self.visible.cpu().numpy(), self.indices.cpu().numpy(), self.count.cpu().numpy()
        ref_ind = np.flatnonzero(ref_vis)
        assert (v[:f] == BYTE_SENTINEL).all() and (v[f + n:] == BYTE_SENTINEL).all()
        assert (i[:f] == INT_SENTINEL).all() and (i[f + n:] == INT_SENTINEL).all()
        assert (c[:f] == INT_SENTINEL).all() and (c[f + 1:] == INT_SENTINEL).all()
        assert np.array_equal(v[f:f + n], ref_vis) if visible else (v[f:f + n] == BYTE_SENTINEL).all()
        if indices:
            assert np.array_equal(i[f:f + len(ref_ind)], ref_ind)
            assert (i[f + len(ref_ind):f + n] == INT_SENTINEL).all()        # indices[n:] is not touched
        else:
            assert (i[f:f + n] == INT_SENTINEL).all()
        assert c[f] == (len(ref_ind) if count else 123456789)


def random_boxes(seed, n):
    rng = np.random.default_rng(seed)
    return np.concatenate([rng.uniform(-4.0, 4.0, (n, 3)), rng.uniform(0.0, 1.5, (n, 3))], axis=1).astype(F)


@pytest.fixture(scope="module")
def small_mesh(mbik, torch_dev):
    pos, _, idx, w = S.random_mesh(3, 3, 9, 4)
    with Mesh(3, pos, idx, w) as mesh:
        yield mesh


# ---------------- bounds ----------------
@pytest.mark.parametrize("table", ["full", "sparse", "empty"])
@pytest.mark.parametrize("B", [1, 32, 200])
def test_bounds_match_cpu(mbik, torch_dev, B, table):
    """Counts 1, 63, 65, 257 and one that ends one skeleton into a tile; the mesh's readback equals mbik_bone_boxes_cpu."""
    torch, dev = torch_dev
    K = 4 if B != 32 else 8
    pos, _, idx, w = table_mesh(100 + B, B, 250, K, table)
    boxes, used = bone_boxes_cpu(B, pos, idx, w)
    assert {"full": used.all(), "sparse": B == 1 or (not used.all() and used.any()), "empty": not used.any()}[table]
    counts = (1, 63, 65, 257, 5 * TILE[B] + 1)
    skin = S.random_skin(101 + B, max(counts), B)
    ref = skin_bounds_cpu(boxes, used, skin)
    with Mesh(B, pos, idx, w) as mesh:
        got_boxes, got_used = mesh.bone_boxes()
        assert S.same_bits(got_boxes, boxes) and np.array_equal(got_used, used)
        for count in counts:
            assert S.same_bits(run_bounds(torch, dev, mesh, skin[:count]), ref[:count]), count
    if table == "empty":
        assert not ref.any()


def test_bounds_largest_rig(mbik, torch_dev):
    """MBIK_SKIN_MAX_BONES bones: one skeleton a block, the matrices fill the LDS, the item loop runs 14 passes."""
    torch, dev = torch_dev
    B, V, K = MAX_BONES, 3000, 4
    pos, _, idx, w = S.random_mesh(5, B, V, K)
    idx[0, 0], idx[1, 1], idx[V - 1, 3] = 0, B - 1, B - 1
    boxes, used = bone_boxes_cpu(B, pos, idx, w)
    assert used[0] and used[B - 1] and not used.all()
    skin = S.random_skin(6, 2, B)
    with Mesh(B, pos, idx, w) as mesh:
        assert S.same_bits(run_bounds(torch, dev, mesh, skin), skin_bounds_cpu(boxes, used, skin))
    # every bone used: the last item's box lands on the last matrix's floats
    idx2 = (np.arange(V * K, dtype=np.int64).reshape(V, K) % B).astype(np.int32)
    boxes2, used2 = bone_boxes_cpu(B, pos, idx2, w)
    assert used2.all()
    with Mesh(B, pos, idx2, w) as mesh:
        assert S.same_bits(run_bounds(torch, dev, mesh, skin), skin_bounds_cpu(boxes2, used2, skin))


def test_bounds_nan_stays_in_its_skeleton(mbik, torch_dev):
    torch, dev = torch_dev
    B, count, bad = 32, 40, 14          # (skeleton 14 is the second of the second tile)
    pos, _, idx, w = S.random_mesh(7, B, 300, 4)
    boxes, used = bone_boxes_cpu(B, pos, idx, w)
    skin = S.random_skin(8, count, B)
    clean = skin_bounds_cpu(boxes, used, skin)
    skin[bad, B - 1, 5] = np.nan
    with Mesh(B, pos, idx, w) as mesh:
        got = run_bounds(torch, dev, mesh, skin)
    assert S.same_bits(got, skin_bounds_cpu(boxes, used, skin))
    others = np.arange(count) != bad
    assert S.same_bits(got[others], clean[others]) and np.isnan(got[bad]).any() and np.isfinite(got[others]).all()


@pytest.mark.parametrize("shift", [1, 2, 3])
@pytest.mark.parametrize("which", ["skin", "boxes"])
def test_bounds_float_aligned_buffers(mbik, torch_dev, which, shift):
    torch, dev = torch_dev
    B = 32
    pos, _, idx, w = S.random_mesh(9, B, 200, 4)
    boxes, used = bone_boxes_cpu(B, pos, idx, w)
    skin = S.random_skin(10, 27, B)
    with Mesh(B, pos, idx, w) as mesh:
        got = run_bounds(torch, dev, mesh, skin, **({"skin": dict(off_skin=shift), "boxes": dict(off_b=shift)}[which]))
    assert S.same_bits(got, skin_bounds_cpu(boxes, used, skin))


def test_bounds_on_a_shaped_mesh(mbik, torch_dev):
    """Blend shapes do not enter the boxes: the shaped mesh gives the plain mesh's."""
    torch, dev = torch_dev
    B, V, K, P = 32, 500, 4, 3
    pos, nrm, idx, w = S.random_mesh(11, B, V, K)
    sp, sn = MR.random_shapes(12, P, V)
    boxes, used = bone_boxes_cpu(B, pos, idx, w)
    skin = S.random_skin(13, 30, B)
    with Mesh(B, pos, idx, w, normals=nrm, shape_positions=sp, shape_normals=sn) as mesh:
        got_boxes, got_used = mesh.bone_boxes()
        got = run_bounds(torch, dev, mesh, skin)
    assert S.same_bits(got_boxes, boxes) and np.array_equal(got_used, used)
    assert S.same_bits(got, skin_bounds_cpu(boxes, used, skin))


def test_bounds_and_cull_in_stream_order_after_pose_globals(mbik, torch_dev):
    """pose_globals(inv_bind) -> bounds -> cull on one side stream, nothing in between."""
    torch, dev = torch_dev
    wl = W.generate(2, 64)
    parents, pins = wl.topo.parents.tolist(), wl.topo.pins.tolist()
    n, B, K, V = wl.n, len(parents), 4, 600
    rest, _ = pose_globals_cpu(parents, [], wl.pose[:1])
    inv_bind = np.random.default_rng(25).uniform(-1.0, 1.0, (B, 12)).astype(F)
    pos, _, idx, w = synthetic_mesh(parents, rest[0], V, K, seed=3)
    planes = R.frustum_planes(4)
    plan = Plan.from_workload(wl)
    d_pose, d_ib = torch.from_numpy(wl.pose).to(dev), torch.from_numpy(inv_bind).to(dev)
    d_g = torch.empty((n, B, 12), dtype=torch.float32, device=dev)
    d_b = torch.full((n * 6 + PAD,), SENTINEL, dtype=torch.float32, device=dev)
    out = CullBuffers(torch, dev, n)
    with Mesh(B, pos, idx, w) as mesh:
        torch.cuda.synchronize()
        st = torch.cuda.Stream(device=dev)
        plan.pose_globals(d_pose.data_ptr(), d_g.data_ptr(), n, inv_bind_ptr=d_ib.data_ptr(), stream=st.cuda_stream)
        mesh.bounds(d_g.data_ptr(), d_b.data_ptr(), n, stream=st.cuda_stream)
        mesh.cull(d_b.data_ptr(), n, planes, stream=st.cuda_stream, **out.ptrs(True, True, True))
        st.synchronize()
    plan.close()
    skinned, _ = pose_globals_cpu(parents, pins, wl.pose, inv_bind=inv_bind)
    boxes, used = bone_boxes_cpu(B, pos, idx, w)
    ref = skin_bounds_cpu(boxes, used, skinned)
    h = d_b.cpu().numpy()
    assert (h[n * 6:] == F(SENTINEL)).all() and S.same_bits(h[:n * 6].reshape(n, 6), ref) and np.isfinite(ref).all()
    out.check(cull_boxes_cpu(ref, planes)[0], True, True, True)


def test_bounds_error_codes(mbik, torch_dev):
    torch, dev = torch_dev
    L = _lib.load()
    B, n = 5, 3
    pos, _, idx, w = S.random_mesh(1, B, 9, 4)
    skin = S.random_skin(2, n, B)
    buf = torch.zeros(n * B * 12 + n * 6, dtype=torch.float32, device=dev)
    buf[:n * B * 12] = torch.from_numpy(skin.reshape(-1)).to(dev)
    a = n * B * 12
    at = lambda i: buf[i:].data_ptr()
    vp = lambda x: C.c_void_p(x or None)
    with Mesh(B, pos, idx, w) as mesh:
        call = lambda m, count, p_skin, p_out: L.mbik_skin_bounds(m, count, vp(p_skin), vp(p_out), None)
        E = _lib.MBIK_EINVAL
        assert call(None, n, at(0), at(a)) == E            # null mesh
        assert call(mesh.h, n, 0, at(a)) == E              # null skin
        assert call(mesh.h, n, at(0), 0) == E              # null boxes
        assert call(mesh.h, -1, at(0), at(a)) == E         # negative count
        assert call(mesh.h, n, at(0), at(a - 1)) == E      # boxes overlaps skin
        assert call(mesh.h, 0, 0, 0) == _lib.MBIK_OK       # count == 0: OK, no launch
        torch.cuda.synchronize()
        assert not bool(buf[a:].any())                     # nothing was launched
        assert call(mesh.h, n, at(0), at(a)) == _lib.MBIK_OK    # adjacent, not overlapping
        torch.cuda.synchronize()
    boxes, used = bone_boxes_cpu(B, pos, idx, w)
    assert S.same_bits(buf[a:].cpu().numpy().reshape(n, 6), skin_bounds_cpu(boxes, used, skin))


# ---------------- culling ----------------
@pytest.mark.parametrize("outputs", ["visible", "indices", "both"])
@pytest.mark.parametrize("count", [1, 63, 64, 65, 257, 65537])
def test_cull_matches_cpu(mbik, torch_dev, small_mesh, count, outputs):
    """65,537 skeletons are 257 blocks: the scan's second pass, and a last block of one skeleton."""
    torch, dev = torch_dev
    boxes, planes = random_boxes(200 + count, count), R.frustum_planes(5)
    ref_vis, _ = cull_boxes_cpu(boxes, planes)
    assert count < 63 or 0 < ref_vis.sum() < count
    d_boxes = torch.from_numpy(boxes).to(dev)
    want_v, want_i = outputs != "indices", outputs != "visible"
    out = CullBuffers(torch, dev, count)
    small_mesh.cull(d_boxes.data_ptr(), count, planes, **out.ptrs(want_v, want_i, want_i))
    torch.cuda.synchronize()
    out.check(ref_vis, want_v, want_i, want_i)


@pytest.mark.parametrize("count", [257, 65537])
def test_cull_all_none_and_last(mbik, torch_dev, small_mesh, count):
    torch, dev = torch_dev
    boxes = random_boxes(300 + count, count)
    boxes[-1, :3] = [50.0, 0.0, 0.0]
    d_boxes = torch.from_numpy(boxes).to(dev)
    cases = {"no planes": np.zeros((0, 4), F), "far planes": np.array([[1, 0, 0, 1000], [0, -1, 0, 1000]], F),
             "none": np.array([[1, 0, 0, -100]], F), "only the last": np.array([[-1, 0, 0, -40]], F)}
    for name, planes in cases.items():
        ref_vis, _ = cull_boxes_cpu(boxes, planes)
        assert ref_vis.sum() == {"no planes": count, "far planes": count, "none": 0, "only the last": 1}[name] and (name != "only the last" or ref_vis[-1])
        out = CullBuffers(torch, dev, count)
        small_mesh.cull(d_boxes.data_ptr(), count, planes, **out.ptrs(True, True, True))
        torch.cuda.synchronize()
        out.check(ref_vis, True, True, True)
    out = CullBuffers(torch, dev, count)                     # visible_count alone beside visible
    small_mesh.cull(d_boxes.data_ptr(), count, cases["only the last"], **out.ptrs(True, False, True))
    torch.cuda.synchronize()
    out.check(cull_boxes_cpu(boxes, cases["only the last"])[0], True, False, True)


def test_cull_twice_on_one_stream(mbik, torch_dev, small_mesh):
    """Two calls back to back share the mesh's scratch; the stream orders them."""
    torch, dev = torch_dev
    count = 5000
    boxes = random_boxes(400, count)
    d_boxes = torch.from_numpy(boxes).to(dev)
    p1, p2 = R.frustum_planes(6), R.frustum_planes(7)[:3]
    o1, o2 = CullBuffers(torch, dev, count), CullBuffers(torch, dev, count)
    torch.cuda.synchronize()
    st = torch.cuda.Stream(device=dev)
    small_mesh.cull(d_boxes.data_ptr(), count, p1, stream=st.cuda_stream, **o1.ptrs(True, True, True))
    small_mesh.cull(d_boxes.data_ptr(), count, p2, stream=st.cuda_stream, **o2.ptrs(True, True, True))
    st.synchronize()
    r1, r2 = cull_boxes_cpu(boxes, p1)[0], cull_boxes_cpu(boxes, p2)[0]
    assert not np.array_equal(r1, r2)
    o1.check(r1, True, True, True), o2.check(r2, True, True, True)


@pytest.mark.parametrize("margin", [0.0, 0.6, -0.2])
def test_cull_world_transform_and_margin(mbik, torch_dev, small_mesh, margin):
    torch, dev = torch_dev
    count = 1000
    boxes, planes = random_boxes(500, count), R.frustum_planes(8)
    boxes[7, 1], boxes[8, 4] = np.nan, np.inf
    sg = S.random_skin(501, count, 1).reshape(count, 12)
    d_boxes = torch.from_numpy(boxes).to(dev)
    d_sg = torch.zeros(count * 12 + 1, dtype=torch.float32, device=dev)       # (float-aligned)
    d_sg[1:] = torch.from_numpy(sg.reshape(-1)).to(dev)
    ref_vis, _ = cull_boxes_cpu(boxes, planes, skeleton_global=sg, margin=margin)
    assert not np.array_equal(ref_vis, cull_boxes_cpu(boxes, planes, margin=margin)[0]) and ref_vis[7] == 1
    out = CullBuffers(torch, dev, count)
    small_mesh.cull(d_boxes.data_ptr(), count, planes, skeleton_global_ptr=d_sg[1:].data_ptr(), margin=margin, **out.ptrs(True, True, True))
    torch.cuda.synchronize()
    out.check(ref_vis, True, True, True)


def test_cull_error_codes(mbik, torch_dev, small_mesh):
    torch, dev = torch_dev
    L = _lib.load()
    n = 8
    boxes = random_boxes(600, n)
    buf = torch.zeros(n * 6 + n * 12, dtype=torch.float32, device=dev)
    buf[:n * 6] = torch.from_numpy(boxes.reshape(-1)).to(dev)
    out = torch.zeros(256, dtype=torch.uint8, device=dev)
    p_boxes, p_sg = buf.data_ptr(), buf[n * 6:].data_ptr()
    p_vis, p_ind, p_cnt = out.data_ptr(), out[64:].data_ptr(), out[128:].data_ptr()
    planes = np.array([[1, 0, 0, 0.5], [0, 1, 0, 2.0]], F)
    planes17 = np.tile(planes[:1], (17, 1))
    vp = lambda x: C.c_void_p(x or None)

    def call(mesh=small_mesh.h, count=n, b=p_boxes, g=p_sg, pc=2, pl=planes, v=p_vis, i=p_ind, c=p_cnt):
        return L.mbik_cull_boxes(mesh, count, vp(b), vp(g), 0.0, pc, S.ptr(pl), vp(v), vp(i), vp(c), None)

    E = _lib.MBIK_EINVAL
    assert call(mesh=None) == E and call(b=0) == E and call(count=-1) == E
    assert call(pc=17, pl=planes17) == E and call(pc=-1) == E and call(pl=None) == E
    assert call(v=0, i=0) == E and call(v=0, i=0, c=0) == E        # both outputs null
    assert call(c=0) == E                                          # indices without visible_count
    assert call(v=p_boxes + n * 24 - 1) == E                       # visible overlaps boxes
    assert call(i=p_sg + n * 48 - 4) == E                          # indices overlaps skeleton_global
    assert call(c=p_boxes) == E                                    # visible_count overlaps boxes
    assert call(i=p_vis + 4) == E                                  # indices overlaps visible
    assert call(c=p_ind + 4 * (n - 1)) == E                        # visible_count overlaps indices
    assert call(c=p_vis + n - 1) == E                              # visible_count overlaps visible
    torch.cuda.synchronize()
    assert not bool(out.any())                                     # nothing was launched
    out[128:132] = 0x55
    assert call(count=0) == _lib.MBIK_OK                           # count == 0: the count is written, nothing else
    torch.cuda.synchronize()
    assert not bool(out.any())
    assert call(pc=16, pl=planes17) == _lib.MBIK_OK and call(g=0) == _lib.MBIK_OK
    assert call(v=p_vis, i=p_vis + n, c=p_vis + 5 * n) == _lib.MBIK_OK      # adjacent, not overlapping
    torch.cuda.synchronize()
    h = out.cpu().numpy()
    ref_vis, ref_ind = cull_boxes_cpu(boxes, planes, skeleton_global=np.zeros((n, 12), F))
    assert np.array_equal(h[:n], ref_vis) and h[5 * n:5 * n + 4].view(np.int32)[0] == len(ref_ind)
    assert np.array_equal(h[n:n + 4 * len(ref_ind)].view(np.int32), ref_ind)
