"""mbik_cull_lod on the GPU against mbik_cull_lod_cpu, bitwise, with sentinels in the list
rows and behind every output: the seeded crowds of tests/test_cull_lod_cpu.py over counts that end inside
a wave and a block, 65,793 skeletons (257 blocks and one more: the scan's carry and a last partial
block), four frames with the state kept on the device, a side stream right behind mbik_skin_bounds, the
chain bounds -> cull_lod -> listed skinning of three meshes, a NaN box, no planes, mbik_cull_boxes
around the call on the same mesh, and the refusals with a mesh in hand."""
import ctypes as C

import numpy as np
import pytest

from many_bone_ik_amd import _lib
from many_bone_ik_amd.skinning import (Mesh, MeshLod, bone_boxes_cpu, cull_boxes_cpu, cull_lod_cpu, lod_ranges, skin_bounds_cpu,
                                       skin_vertices_listed_cpu, synthetic_mesh)

from . import lod_recipe as LR
from . import skin_cases as S
from .test_cull_lod_cpu import BYTE_SENTINEL, CASES, INT_SENTINEL, case_inputs, run_cpu, sequence_inputs
from .test_gpu_parity import torch_dev  # noqa: F401 (fixture)

pytestmark = pytest.mark.gpu

F = np.float32
PAD = 16
BIG = 257 * 256 + 1


@pytest.fixture(scope="module")
def small_mesh(mbik, torch_dev):
    pos, _, idx, w = S.random_mesh(3, 3, 9, 4)
    with Mesh(3, pos, idx, w) as mesh:
        yield mesh


def crowd_skin(seed, n, B):
    """Skin transforms [n][B][12] of a crowd: small bases, every skeleton's bones around a place of its own within 20 units."""
    rng = np.random.default_rng(seed)
    skin = rng.uniform(-0.5, 0.5, (n, B, 12)).astype(F)
    skin[..., 9:] += rng.uniform(-20.0, 20.0, (n, 1, 3)).astype(F)
    return skin


class LodBuffers:
    """Device outputs of one call: sentinels in the rows and behind each output, garbage in list_counts."""

    def __init__(self, torch, dev, n, R, state):
        self.n, self.R = n, R
        self.state = torch.full((n + PAD,), BYTE_SENTINEL, dtype=torch.uint8, device=dev)
        self.state[:n] = torch.from_numpy(np.array(state, np.uint8)).to(dev)
        self.level = torch.full((n + PAD,), BYTE_SENTINEL, dtype=torch.uint8, device=dev)
        self.indices = torch.full((R * n + PAD,), INT_SENTINEL, dtype=torch.int32, device=dev)
        self.counts = torch.full((R + PAD,), INT_SENTINEL, dtype=torch.int32, device=dev)
        self.counts[:R] = 123456789

    def ptrs(self, level=True):
        return dict(state_ptr=self.state.data_ptr(), level_ptr=self.level.data_ptr() if level else 0, indices_ptr=self.indices.data_ptr(),
                    list_counts_ptr=self.counts.data_ptr())

    def read(self):
        """-> (state, level, indices [R][n], counts), the pads checked."""
        n, R = self.n, self.R
        st, lv, ind, cnt = (t.cpu().numpy() for t in (self.state, self.level, self.indices, self.counts))
        assert (st[n:] == BYTE_SENTINEL).all() and (lv[n:] == BYTE_SENTINEL).all()
        assert (ind[R * n:] == INT_SENTINEL).all() and (cnt[R:] == INT_SENTINEL).all()
        return st[:n], lv[:n], ind[:R * n].reshape(R, n), cnt[:R]


def same_outputs(got, ref):
    """Everything bitwise: state, level, the counts and the whole rows, so the lists and their untouched tails."""
    return all(np.array_equal(g, r) for g, r in zip(got, ref))


def run_gpu(torch, dev, mesh, boxes, planes, camera, ranges, state, sg=None, margin=0.0, flags=0, stream=0):
    n = boxes.shape[0]
    d_boxes = torch.from_numpy(np.ascontiguousarray(boxes)).to(dev)
    d_sg = None if sg is None else torch.from_numpy(np.ascontiguousarray(sg)).to(dev)
    out = LodBuffers(torch, dev, n, lod_ranges(ranges).shape[0], state)
    torch.cuda.synchronize()
    mesh.cull_lod(d_boxes.data_ptr() if n else 0, n, planes, camera, ranges, skeleton_global_ptr=0 if d_sg is None else d_sg.data_ptr(),
                  margin=margin, flags=flags, stream=stream, **out.ptrs())
    torch.cuda.synchronize()
    return out.read()


@pytest.mark.parametrize("range_count,with_global,margin", CASES)
def test_device_matches_cpu(mbik, torch_dev, small_mesh, range_count, with_global, margin):
    torch, dev = torch_dev
    c = case_inputs(range_count, with_global, margin)
    for count in LR.COUNTS:
        for flags in (0, _lib.LOD_EXCLUSIVE):
            sg = None if c["sg"] is None else c["sg"][:count]
            args = (c["boxes"][:count], c["planes"], c["camera"], c["ranges"], c["state"][:count], sg, margin, flags)
            ref = run_cpu(*args)
            assert count < 63 or 0 < ref[3].sum()
            assert same_outputs(run_gpu(torch, dev, small_mesh, *args), ref), (count, flags)


@pytest.mark.parametrize("flags", [0, 1], ids=["overlapping", "exclusive"])
@pytest.mark.parametrize("range_count", [3, 8])
def test_across_the_scans_second_pass(mbik, torch_dev, small_mesh, range_count, flags):
    """65,793 skeletons: 258 blocks, so every row's scan carries into a second pass, and the last block holds one skeleton."""
    torch, dev = torch_dev
    boxes, planes, state = LR.crowd(70 + range_count, BIG, nan_every=9973), LR.planes(71), LR.states(72, BIG)
    boxes[-1, :3] = [0.5, 0.5, 0.5]                                      # the last skeleton is seen and near
    args = (boxes, planes, LR.CAMERA, LR.RANGES[range_count], state, None, 0.0, flags)
    ref = run_cpu(*args)
    assert ref[1][-1] == 0 and ref[2][0, ref[3][0] - 1] == BIG - 1 and (ref[3][:3] > 256).all()
    assert same_outputs(run_gpu(torch, dev, small_mesh, *args), ref)


@pytest.mark.parametrize("range_count", [3, 8])
def test_four_frames_with_the_state_on_the_device(mbik, torch_dev, small_mesh, range_count):
    """The state buffer stays on the device from frame to frame and is never given back by the host: every frame's
    lists come from the state the frame before left there."""
    torch, dev = torch_dev
    boxes, planes, cams, ranges = sequence_inputs(range_count)
    n, R = boxes.shape[0], range_count
    d_boxes = torch.from_numpy(boxes).to(dev)
    d_state = torch.zeros(n, dtype=torch.uint8, device=dev)
    state = np.zeros(n, np.uint8)
    for f, cam in enumerate(cams):
        ref = run_cpu(boxes, planes, cam, ranges, state, None, 0.25, 0)
        out = LodBuffers(torch, dev, n, R, state)
        mesh_args = dict(out.ptrs(), state_ptr=d_state.data_ptr())
        small_mesh.cull_lod(d_boxes.data_ptr(), n, planes, cam, ranges, margin=0.25, **mesh_args)
        torch.cuda.synchronize()
        _, lv, ind, cnt = out.read()
        assert same_outputs((d_state.cpu().numpy(), lv, ind, cnt), ref), f
        assert f == 0 or not np.array_equal(ref[0], run_cpu(boxes, planes, cam, ranges, np.zeros(n, np.uint8), None, 0.25, 0)[0])
        state = ref[0]


def test_on_a_side_stream_right_behind_bounds(mbik, torch_dev):
    torch, dev = torch_dev
    B, n = 5, 700
    pos, _, idx, w = S.random_mesh(41, B, 60, 4)
    skin = crowd_skin(42, n, B)
    bb, used = bone_boxes_cpu(B, pos, idx, w)
    boxes = skin_bounds_cpu(bb, used, skin)
    planes, ranges, state = LR.planes(43), LR.RANGES[3], LR.states(44, n)
    ref = run_cpu(boxes, planes, LR.CAMERA, ranges, state, None, 0.1, 0)
    assert (ref[3] > 0).all()
    d_skin = torch.from_numpy(skin).to(dev)
    d_b = torch.zeros(n * 6, dtype=torch.float32, device=dev)
    out = LodBuffers(torch, dev, n, 3, state)
    with Mesh(B, pos, idx, w) as mesh:
        torch.cuda.synchronize()
        st = torch.cuda.Stream(device=dev)
        mesh.bounds(d_skin.data_ptr(), d_b.data_ptr(), n, stream=st.cuda_stream)
        mesh.cull_lod(d_b.data_ptr(), n, planes, LR.CAMERA, ranges, margin=0.1, stream=st.cuda_stream, **out.ptrs())
        st.synchronize()
    assert S.same_bits(d_b.cpu().numpy().reshape(n, 6), boxes) and same_outputs(out.read(), ref)


@pytest.mark.parametrize("compact", [False, True], ids=["in_place", "compact"])
def test_chain_bounds_lod_listed_skin(mbik, torch_dev, compact):
    """Three meshes of 64, 16 and 4 vertices on one 5-bone rig: bounds of the first, one list per mesh, each mesh
    skinned over its own list, on one stream with nothing in between, against the _cpu chain."""
    torch, dev = torch_dev
    parents, B, n, Vs = [-1, 0, 1, 2, 3], 5, 300, (64, 16, 4)
    rest = np.zeros((B, 12), F)
    rest[:, [0, 4, 8]] = 1.0
    rest[:, 10] = np.arange(B) * 0.4
    arrays = [synthetic_mesh(parents, rest, V, 4, seed=50 + V) for V in Vs]
    skin = crowd_skin(51, n, B)
    planes, state = LR.planes(52), LR.states(53, n)
    ranges = np.array([[0, 10, 0, 1], [10, 14, 1, 1], [14, 0, 1, 0]], F)
    # the _cpu chain
    bb, used = bone_boxes_cpu(B, arrays[0][0], arrays[0][2], arrays[0][3])
    boxes = skin_bounds_cpu(bb, used, skin)
    ref_state, ref_level, lists = cull_lod_cpu(boxes, planes, LR.CAMERA, ranges, state, flags=_lib.LOD_EXCLUSIVE)
    assert all(len(l) >= 5 for l in lists) and sum(len(l) for l in lists) < n
    want = []
    for (pos, _, idx, w), lst, V in zip(arrays, lists, Vs):
        padded = np.concatenate([lst, np.full(n - len(lst), -1, np.int32)])
        want.append(skin_vertices_listed_cpu(B, pos, idx, w, skin, padded, len(lst), max_list=n, compact=compact,
                                             out_positions=np.full((n, V, 3), F(-12345.678), F))[0])
    # the device chain
    d_skin = torch.from_numpy(skin).to(dev)
    d_b = torch.zeros(n * 6, dtype=torch.float32, device=dev)
    out = LodBuffers(torch, dev, n, 3, state)
    outs = [torch.full((n * V * 3 + PAD,), -12345.678, dtype=torch.float32, device=dev) for V in Vs]
    meshes = [Mesh(B, pos, idx, w) for pos, _, idx, w in arrays]
    try:
        lod = MeshLod(meshes, ranges)
        torch.cuda.synchronize()
        st = torch.cuda.Stream(device=dev)
        meshes[0].bounds(d_skin.data_ptr(), d_b.data_ptr(), n, stream=st.cuda_stream)
        p = out.ptrs()
        lod.select(d_b.data_ptr(), n, planes, LR.CAMERA, p["state_ptr"], p["indices_ptr"], p["list_counts_ptr"], level_ptr=p["level_ptr"],
                   stream=st.cuda_stream)
        lod.skin(d_skin.data_ptr(), [o.data_ptr() for o in outs], n, p["indices_ptr"], p["list_counts_ptr"], compact=compact,
                 stream=st.cuda_stream)
        st.synchronize()
    finally:
        for m in meshes:
            m.close()
    got_state, got_level, ind, cnt = out.read()
    assert np.array_equal(got_state, ref_state) and np.array_equal(got_level, ref_level) and cnt.tolist() == [len(l) for l in lists]
    for r, (V, o) in enumerate(zip(Vs, outs)):
        assert np.array_equal(ind[r, :cnt[r]], lists[r]) and (ind[r, cnt[r]:] == INT_SENTINEL).all()
        h = o.cpu().numpy()
        assert (h[n * V * 3:] == F(-12345.678)).all()
        assert S.same_bits(h[:n * V * 3].reshape(n, V, 3), want[r]), r


def test_nan_box_and_no_planes(mbik, torch_dev, small_mesh):
    torch, dev = torch_dev
    n = 200
    boxes = LR.crowd(61, n)
    boxes[5, 0], boxes[70, 4], boxes[199, 2] = np.nan, np.nan, np.inf
    no_planes = np.zeros((0, 4), F)
    for planes in (no_planes, LR.planes(62)):
        for flags in (0, 1):
            args = (boxes, planes, LR.CAMERA, LR.RANGES[3], np.zeros(n, np.uint8), None, 0.0, flags)
            ref = run_cpu(*args)
            assert ref[0][5] == 7 and ref[0][70] == 7 and ref[1][5] == 0         # NaN: in every range, and seen
            assert same_outputs(run_gpu(torch, dev, small_mesh, *args), ref)
    vis_all = run_cpu(boxes, no_planes, LR.CAMERA, np.zeros((1, 4), F), np.zeros(n, np.uint8))
    assert vis_all[3][0] == n                                             # no planes, one unlimited range: everyone


def test_cull_boxes_around_the_call_on_one_mesh(mbik, torch_dev, small_mesh):
    """The two calls share the mesh's block counts; the stream orders them, and mbik_cull_boxes gives its own bits."""
    torch, dev = torch_dev
    n = 5000
    boxes, planes, state = LR.crowd(81, n), LR.planes(82), LR.states(83, n)
    ref_vis, ref_ind = cull_boxes_cpu(boxes, planes)
    ref = run_cpu(boxes, planes, LR.CAMERA, LR.RANGES[8], state, None, 0.0, 0)
    d_boxes = torch.from_numpy(boxes).to(dev)
    culls = []
    for _ in range(2):
        culls.append((torch.full((n,), BYTE_SENTINEL, dtype=torch.uint8, device=dev), torch.full((n,), INT_SENTINEL, dtype=torch.int32, device=dev),
                      torch.full((1,), 123456789, dtype=torch.int32, device=dev)))
    out = LodBuffers(torch, dev, n, 8, state)
    torch.cuda.synchronize()
    st = torch.cuda.Stream(device=dev)
    cull = lambda v, i, c: small_mesh.cull(d_boxes.data_ptr(), n, planes, visible_ptr=v.data_ptr(), indices_ptr=i.data_ptr(),
                                           visible_count_ptr=c.data_ptr(), stream=st.cuda_stream)
    cull(*culls[0])
    small_mesh.cull_lod(d_boxes.data_ptr(), n, planes, LR.CAMERA, LR.RANGES[8], stream=st.cuda_stream, **out.ptrs())
    cull(*culls[1])
    st.synchronize()
    assert same_outputs(out.read(), ref)
    for v, i, c in culls:
        assert np.array_equal(v.cpu().numpy(), ref_vis) and c.cpu().tolist() == [len(ref_ind)]
        h = i.cpu().numpy()
        assert np.array_equal(h[:len(ref_ind)], ref_ind) and (h[len(ref_ind):] == INT_SENTINEL).all()


def test_refusals_and_count_zero_with_a_mesh(mbik, torch_dev, small_mesh):
    torch, dev = torch_dev
    L = _lib.load()
    n, R = 8, 3
    d_boxes = torch.from_numpy(LR.crowd(91, n)).to(dev)
    out = torch.zeros(512, dtype=torch.uint8, device=dev)
    p_state, p_level, p_ind, p_cnt = out.data_ptr(), out[16:].data_ptr(), out[32:].data_ptr(), out[256:].data_ptr()
    planes, cam, rg = LR.planes(92), np.zeros(3, F), lod_ranges(LR.RANGES[3])
    vp = lambda x: C.c_void_p(x or None)

    def call(mesh=small_mesh.h, count=n, b=d_boxes.data_ptr(), pc=6, rc=R, flags=0, camera=cam, ranges=rg, s=p_state, lv=p_level, i=p_ind, c=p_cnt):
        return L.mbik_cull_lod(mesh, count, vp(b), None, 0.0, pc, S.ptr(planes), S.ptr(camera), rc, S.ptr(ranges), flags, vp(s), vp(lv), vp(i),
                               vp(c), None)

    E = _lib.MBIK_EINVAL
    assert call(mesh=None) == E and call(count=-1) == E and call(b=0) == E and call(pc=17) == E
    assert call(rc=0) == E and call(rc=9) == E and call(flags=2) == E and call(camera=np.array([0, np.nan, 0], F)) == E
    assert call(s=0) == E and call(i=0) == E and call(c=0) == E
    assert call(lv=p_state + n - 1) == E and call(i=p_level + 4) == E and call(c=p_ind + 4 * (R * n - 1)) == E
    assert call(s=d_boxes.data_ptr() + n * 24 - 1) == E
    torch.cuda.synchronize()
    assert not bool(out.any())                                            # nothing was launched
    out[256:256 + 4 * R + 4] = 0x55
    assert call(count=0) == _lib.MBIK_OK                                  # count == 0: the counts are zeroed, nothing else
    torch.cuda.synchronize()
    h = out.cpu().numpy()
    assert not h[:256 + 4 * R].any() and (h[256 + 4 * R:256 + 4 * R + 4] == 0x55).all()
    assert call(lv=0) == _lib.MBIK_OK                                     # level is optional
    torch.cuda.synchronize()
    ref = run_cpu(d_boxes.cpu().numpy(), planes, cam, LR.RANGES[3], np.zeros(n, np.uint8))
    h = out.cpu().numpy()
    assert np.array_equal(h[:n], ref[0]) and not h[16:32].any()
    assert np.array_equal(h[256:256 + 4 * R].view(np.int32), ref[3])
    ind = h[32:32 + 4 * R * n].view(np.int32).reshape(R, n)
    assert all(np.array_equal(ind[r, :ref[3][r]], ref[2][r, :ref[3][r]]) for r in range(R))
