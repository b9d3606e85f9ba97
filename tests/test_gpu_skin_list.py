"""mbik_skin_vertices_listed on the GPU against the EXISTING host entries
mbik_skin_vertices_cpu / mbik_skin_vertices_shaped_cpu, bitwise (two NaNs count as equal): every output
is compared whole with tests/skin_list_cases.expected, so a listed row must carry the existing call's
bits and every other row its sentinel, and has a row and more of sentinels in front and behind.  skin
and shape_weights sit between a skeleton's worth of NaN on either side: a wrong range guard shows as a
failed compare.  Tile boundaries, empty tiles, the twelve instantiations, the identity list against the
plain and the shaped call on the device (all twelve again, bitwise), index patterns, out-of-range
entries, vertex lanes and chunks, shaped meshes, float-aligned buffers, the LDS limits, offsets past
2^31, the whole frame on one stream, error codes."""
import ctypes as C

import numpy as np
import pytest

from many_bone_ik_amd import _lib
from many_bone_ik_amd.skinning import Mesh, bone_boxes_cpu, cull_boxes_cpu, skin_bounds_cpu, skin_vertices_cpu
from many_bone_ik_amd.solver import Plan, pose_globals_cpu

from . import skin_cases as S
from . import skin_list_cases as LC
from .test_gpu_parity import torch_dev  # noqa: F401 (fixture)

pytestmark = pytest.mark.gpu

F = np.float32
SENTINEL = LC.SENTINEL
INT_SENTINEL = -777
PAD = LC.PAD
MAX_BONES = 3413   # MBIK_SKIN_MAX_BONES
# Skeletons (here: list entries) a block takes: min(20 KiB / (48 B a bone), 16, max_list) (host_skin.cpp)
TILE = {1: 16, 32: 13, 200: 2}


class DeviceCase:
    """A Case's inputs on the device: skin and shape_weights with one skeleton's worth of NaN in front and behind,
    shifted by off_skin / off_w floats."""

    def __init__(self, torch, dev, case, off_skin=0, off_w=0):
        self.case = case
        pad = max(case.B * 12, 4)
        self.skin = torch.full((off_skin + pad + case.skin.size + pad,), float("nan"), dtype=torch.float32, device=dev)
        self.skin[off_skin + pad:off_skin + pad + case.skin.size] = torch.from_numpy(case.skin.reshape(-1)).to(dev)
        self.skin_ptr = self.skin[off_skin + pad:].data_ptr()
        self.w_ptr = 0
        if case.P:
            wpad = max(case.P, 4)
            self.cw = torch.full((off_w + wpad + case.cw.size + wpad,), float("nan"), dtype=torch.float32, device=dev)
            self.cw[off_w + wpad:off_w + wpad + case.cw.size] = torch.from_numpy(case.cw.reshape(-1)).to(dev)
            self.w_ptr = self.cw[off_w + wpad:].data_ptr()


class Outputs:
    """One output buffer: `off` floats of shift, then a guard of one row + PAD, the rows, the same guard."""

    def __init__(self, torch, dev, rows, V, off=0):
        self.off, self.guard, self.rows, self.V = off, V * 3 + PAD, rows, V
        self.t = torch.full((off + 2 * self.guard + rows * V * 3,), SENTINEL, dtype=torch.float32, device=dev)
        self.ptr = self.t[off + self.guard:].data_ptr()

    def read(self):
        h = self.t.cpu().numpy()
        a, b = self.off + self.guard, self.off + self.guard + self.rows * self.V * 3
        assert (h[:a] == F(SENTINEL)).all() and (h[b:] == F(SENTINEL)).all()
        return h[a:b].reshape(self.rows, self.V, 3)


def list_buffers(torch, dev, indices, list_count, max_list):
    """(indices tensor with 8 guard entries either side, its data pointer, count tensor)."""
    t = torch.full((16 + max_list,), INT_SENTINEL, dtype=torch.int32, device=dev)
    if max_list:
        t[8:8 + max_list] = torch.from_numpy(np.ascontiguousarray(indices[:max_list], np.int32)).to(dev)
    c = torch.tensor([INT_SENTINEL, int(list_count), INT_SENTINEL], dtype=torch.int32, device=dev)
    return t, t[8:].data_ptr(), c


def check_listed(torch, dev, mesh, d, indices, list_count, max_list, compact, shaped, normals, off_p=0, off_n=0, stream=0):
    """One launch, compared whole with the existing calls' rows; -> the positions."""
    case = d.case
    rows = max_list if compact else case.count
    out_p = Outputs(torch, dev, rows, case.V, off_p)
    out_n = Outputs(torch, dev, rows, case.V, off_n) if normals else None
    t_ind, p_ind, t_cnt = list_buffers(torch, dev, indices, list_count, max_list)
    before = t_ind.clone()
    torch.cuda.synchronize()
    mesh.skin_listed(d.skin_ptr, out_p.ptr, case.count, p_ind, t_cnt[1:].data_ptr(), max_list=max_list, compact=compact,
                     out_normals_ptr=out_n.ptr if normals else 0, shape_weights_ptr=d.w_ptr if shaped else 0, stream=stream)
    torch.cuda.synchronize()
    assert torch.equal(t_ind, before) and t_cnt.cpu().tolist() == [INT_SENTINEL, int(list_count), INT_SENTINEL]
    full_p, full_n = case.full(shaped)
    got_p = out_p.read()
    tag = (len(indices), list_count, max_list, compact, shaped, normals)
    assert S.same_bits(got_p, LC.expected(full_p, indices, list_count, max_list, compact)), tag
    if normals:
        assert S.same_bits(out_n.read(), LC.expected(full_n, indices, list_count, max_list, compact)), tag
    return got_p


def cyclic_list(seed, count, length):
    """`length` entries: a seeded permutation of the skeletons, repeated when the list is longer than the batch."""
    perm = np.random.default_rng(seed).permutation(count)
    return np.resize(perm, max(length, 1)).astype(np.int32)[:length]


# ---------------- tile boundaries, empty tiles, instantiations ----------------
@pytest.mark.parametrize("normals", [False, True], ids=["positions", "normals"])
@pytest.mark.parametrize("K", [4, 8])
@pytest.mark.parametrize("B", [1, 32, 200])
def test_tile_boundaries(mbik, torch_dev, B, K, normals):
    """List lengths 0, 1, S-1, S, S+1, 5S+1 and max_list, each with max_list == n and with max_list well above n
    (whole tiles exit empty), in place and compact."""
    torch, dev = torch_dev
    Sx = TILE[B]
    count, V = 5 * Sx + 2, 70
    case = LC.Case(1000 + 10 * B + K, B, V, K, count)
    d = DeviceCase(torch, dev, case)
    big = 7 * Sx + 3                                   # above count: such a list names skeletons twice
    with Mesh(B, case.pos, case.idx, case.w, **case.mesh_kw()) as mesh:
        assert mesh.launch_shape(big)[0] == Sx and mesh.launch_shape(Sx + 1)[0] == Sx
        for n in (0, 1, Sx - 1, Sx, Sx + 1, 5 * Sx + 1, big):
            indices = cyclic_list(n + B, count, big)
            for max_list in (n, big):
                for compact in (False, True):
                    check_listed(torch, dev, mesh, d, indices, n, max_list, compact, False, normals)
        # counts the kernel clamps: negative, and above max_list
        check_listed(torch, dev, mesh, d, cyclic_list(5, count, big), -4, big, True, False, normals)
        check_listed(torch, dev, mesh, d, cyclic_list(6, count, Sx + 1), 2 ** 31 - 1, Sx + 1, False, False, normals)


# ---------------- the identity list against the plain and the shaped call, device with device ----------------
@pytest.mark.parametrize("mode", [None, "relative", "normalized"], ids=["plain", "relative", "normalized"])
@pytest.mark.parametrize("normals", [False, True], ids=["positions", "normals"])
@pytest.mark.parametrize("K", [4, 8])
def test_identity_list_is_the_direct_call(mbik, torch_dev, K, normals, mode):
    """The list 0 .. count-1, in place and compact, writes bitwise the rows mbik_skin_vertices /
    mbik_skin_vertices_shaped write from the same buffers: the two kernel families run one vertex loop.  Two full
    tiles and a last tile of one skeleton, more than one vertex chunk with the last one partial."""
    torch, dev = torch_dev
    B, V, P = 32, 700, 3 if mode else 0
    case = LC.Case(8000 + 10 * K + P + (mode == "normalized"), B, V, K, 2 * TILE[B] + 1, P=P, mode=mode or "relative",
                   special_weights=bool(P))
    count = case.count
    d = DeviceCase(torch, dev, case)
    t_ind, p_ind, t_cnt = list_buffers(torch, dev, np.arange(count), count, count)

    def outputs():
        return Outputs(torch, dev, count, V), (Outputs(torch, dev, count, V) if normals else None)

    with Mesh(B, case.pos, case.idx, case.w, **case.mesh_kw()) as mesh:
        Sx, chunks = mesh.launch_shape(count)
        assert Sx == TILE[B] and count == 2 * Sx + 1 and chunks > 1 and V % 256 != 0   # (a chunk is a multiple of 256 vertices)
        direct_p, direct_n = outputs()
        mesh.skin(d.skin_ptr, direct_p.ptr, count, out_normals_ptr=direct_n.ptr if normals else 0, shape_weights_ptr=d.w_ptr)
        listed = []
        for compact in (False, True):
            out_p, out_n = outputs()
            mesh.skin_listed(d.skin_ptr, out_p.ptr, count, p_ind, t_cnt[1:].data_ptr(), compact=compact,
                             out_normals_ptr=out_n.ptr if normals else 0, shape_weights_ptr=d.w_ptr)
            listed.append((out_p, out_n))
        torch.cuda.synchronize()
    full_p, full_n = case.full(bool(P))
    assert S.same_bits(direct_p.read(), full_p) and (not normals or S.same_bits(direct_n.read(), full_n))
    for out_p, out_n in listed:
        assert torch.equal(out_p.t.view(torch.int32), direct_p.t.view(torch.int32))
        assert not normals or torch.equal(out_n.t.view(torch.int32), direct_n.t.view(torch.int32))


# ---------------- index patterns ----------------
@pytest.fixture(scope="module")
def pattern_case(mbik):
    return LC.Case(2000, 32, 129, 4, 40)


@pytest.mark.parametrize("compact", [False, True], ids=["in_place", "compact"])
@pytest.mark.parametrize("pattern", ["every", "every_other", "only_first", "only_last", "descending", "duplicates"])
def test_index_patterns(mbik, torch_dev, pattern_case, pattern, compact):
    torch, dev = torch_dev
    case = pattern_case
    count = case.count
    indices = {"every": np.arange(count), "every_other": np.arange(0, count, 2), "only_first": np.array([0]),
               "only_last": np.array([count - 1]), "descending": np.arange(count - 1, -1, -1),
               "duplicates": np.array([5, 5, 5, 17, 5, 17, 39, 39, 0, 0, 5, 17, 17, 17, 3])}[pattern].astype(np.int32)
    d = DeviceCase(torch, dev, case)
    with Mesh(case.B, case.pos, case.idx, case.w, **case.mesh_kw()) as mesh:
        got = check_listed(torch, dev, mesh, d, indices, len(indices), len(indices), compact, False, True)
    written = int((got[:, 0, 0] != F(SENTINEL)).sum())
    assert written == (len(indices) if compact else len(set(indices.tolist())))


@pytest.mark.parametrize("compact", [False, True], ids=["in_place", "compact"])
def test_a_real_cull_list(mbik, torch_dev, pattern_case, compact):
    """mbik_skin_bounds -> mbik_cull_boxes -> listed skin on the default stream: the list and its count never
    leave the device; the stale part of the list buffer holds a valid skeleton number."""
    torch, dev = torch_dev
    case = pattern_case
    count, V = case.count, case.V
    bb, used = bone_boxes_cpu(case.B, case.pos, case.idx, case.w)
    boxes = skin_bounds_cpu(bb, used, case.skin)
    planes = LC.chain_planes(boxes)[0]
    ref = cull_boxes_cpu(boxes, planes)[1]
    assert 0 < len(ref) < count
    d = DeviceCase(torch, dev, case)
    d_boxes = torch.empty(count * 6, dtype=torch.float32, device=dev)
    d_ind = torch.zeros(count, dtype=torch.int32, device=dev)
    d_cnt = torch.full((1,), 123456789, dtype=torch.int32, device=dev)
    out_p, out_n = Outputs(torch, dev, count, V), Outputs(torch, dev, count, V)
    with Mesh(case.B, case.pos, case.idx, case.w, **case.mesh_kw()) as mesh:
        torch.cuda.synchronize()
        mesh.bounds(d.skin_ptr, d_boxes.data_ptr(), count)
        mesh.cull(d_boxes.data_ptr(), count, planes, indices_ptr=d_ind.data_ptr(), visible_count_ptr=d_cnt.data_ptr())
        mesh.skin_listed(d.skin_ptr, out_p.ptr, count, d_ind.data_ptr(), d_cnt.data_ptr(), compact=compact, out_normals_ptr=out_n.ptr)
        torch.cuda.synchronize()
    indices = np.zeros(count, np.int32)
    indices[:len(ref)] = ref
    assert d_cnt.cpu().tolist() == [len(ref)] and np.array_equal(d_ind.cpu().numpy(), indices)
    assert S.same_bits(out_p.read(), LC.expected(case.plain_p, indices, len(ref), count, compact))
    assert S.same_bits(out_n.read(), LC.expected(case.plain_n, indices, len(ref), count, compact))


# ---------------- out-of-range entries ----------------
@pytest.mark.parametrize("compact", [False, True], ids=["in_place", "compact"])
@pytest.mark.parametrize("shaped", [False, True], ids=["plain", "shaped"])
def test_out_of_range_entries(mbik, torch_dev, shaped, compact):
    """-1 and count among valid neighbours of one tile, at a tile's first and last slot and filling a tile: the
    skipped rows stay untouched and the valid ones are right; the NaN pads around skin and shape_weights and the
    sentinel rows around the outputs show an entry that was used."""
    torch, dev = torch_dev
    B, count = 32, 30
    case = LC.Case(3000, B, 65, 8, count, P=3, mode="normalized", special_weights=True)
    Sx = TILE[B]
    indices = np.array([4, -1, 9, count, 0, count - 1, -1, 2, 11, 29, count, 7, -1,          # tile 0: mixed, -1 at its last slot
                        count, 3, 8, 1, -1, 6, 10, 12, 14, 16, 18, 20, count,                # tile 1: count at its first and last slot
                        -1, count, -1, count, -1, count, -1, count, -1, count, -1, count, -1,  # tile 2: nothing valid
                        5, count, -1], np.int32)                                             # tile 3: a part tile
    assert len(indices) == 3 * Sx + 3 and set(indices.tolist()) - set(range(count)) == {-1, count}
    d = DeviceCase(torch, dev, case)
    with Mesh(B, case.pos, case.idx, case.w, **case.mesh_kw()) as mesh:
        assert mesh.launch_shape(len(indices))[0] == Sx
        got = check_listed(torch, dev, mesh, d, indices, len(indices), len(indices), compact, shaped, True)
    valid = (indices >= 0) & (indices < count)
    if compact:
        assert (got[~valid] == F(SENTINEL)).all() and not (got[valid][:, 0, 0] == F(SENTINEL)).any()
    else:
        assert int((got[:, 0, 0] != F(SENTINEL)).sum()) == len(set(indices[valid].tolist()))


# ---------------- vertex lanes and chunks ----------------
@pytest.mark.parametrize("V", [1, 63, 65, 129, 257])
def test_vertex_lanes(mbik, torch_dev, V):
    """64, 128 and 256 vertex lanes: 4, 2 and 1 skeleton groups share a tile's entries."""
    torch, dev = torch_dev
    case = LC.Case(4000 + V, 32, V, 8, 31)
    d = DeviceCase(torch, dev, case)
    indices = cyclic_list(V, case.count, 29)
    indices[[3, 17]] = [-1, case.count]
    with Mesh(case.B, case.pos, case.idx, case.w, **case.mesh_kw()) as mesh:
        for compact in (False, True):
            check_listed(torch, dev, mesh, d, indices, 29, 29, compact, False, True)
            check_listed(torch, dev, mesh, d, indices, 14, 29, compact, False, False)


def test_more_than_one_vertex_chunk(mbik, torch_dev):
    torch, dev = torch_dev
    case = LC.Case(4700, 32, 700, 4, 9, P=3)
    d = DeviceCase(torch, dev, case)
    indices = np.array([7, 2, 8], np.int32)
    with Mesh(case.B, case.pos, case.idx, case.w, **case.mesh_kw()) as mesh:
        assert mesh.launch_shape(3)[1] > 1
        for compact in (False, True):
            check_listed(torch, dev, mesh, d, indices, 3, 3, compact, False, True)
            check_listed(torch, dev, mesh, d, indices, 3, 3, compact, True, True)


# ---------------- shaped ----------------
@pytest.mark.parametrize("mode", ["relative", "normalized"])
@pytest.mark.parametrize("P", [1, 3, 16])
def test_shaped(mbik, torch_dev, P, mode):
    """Weights under the threshold and NaN weights sit on listed skeletons and on unlisted ones; the weights' base is
    16-byte aligned and shifted by 1 to 3 floats (P = 16: quads from the first boundary; otherwise dwords)."""
    torch, dev = torch_dev
    K = 4 if P != 3 else 8
    case = LC.Case(5000 + P, 32, 129, K, 30, P=P, mode=mode, special_weights=True)
    indices = np.array([0, 1, 3, 6, 29, 11, 5, 3, 16, 2, 21, 10, 27, 9, 12, 15], np.int32)
    listed, unlisted = set(indices.tolist()), set(range(30)) - set(indices.tolist())
    small, nans = set(range(0, 30, 3)), set(range(1, 30, 5))
    assert small & listed and small & unlisted and nans & listed and nans & unlisted
    assert np.isnan(case.cw).any() and not np.isnan(case.shaped_p[sorted(listed)]).any()
    with Mesh(case.B, case.pos, case.idx, case.w, **case.mesh_kw()) as mesh:
        for off_w in (0, 1, 2, 3):
            d = DeviceCase(torch, dev, case, off_w=off_w)
            for compact in (False, True):
                check_listed(torch, dev, mesh, d, indices, len(indices), len(indices), compact, True, True)
        d = DeviceCase(torch, dev, case)
        check_listed(torch, dev, mesh, d, indices, len(indices), len(indices), False, True, False)   # positions only
        check_listed(torch, dev, mesh, d, indices, len(indices), len(indices), True, False, True)    # the base arrays


# ---------------- float-aligned buffers ----------------
@pytest.mark.parametrize("shift", [1, 2, 3])
@pytest.mark.parametrize("which", ["skin", "out_positions", "out_normals", "shape_weights"])
def test_float_aligned_buffers(mbik, torch_dev, which, shift):
    torch, dev = torch_dev
    case = LC.Case(6000, 32, 65, 4, 20, P=4, special_weights=True)
    indices = np.array([19, 0, 7, 7, -1, 3, 12, 20, 5, 1, 18, 2, 9, 4, 11], np.int32)
    d = DeviceCase(torch, dev, case, off_skin=shift if which == "skin" else 0, off_w=shift if which == "shape_weights" else 0)
    kw = dict(off_p=shift if which == "out_positions" else 0, off_n=shift if which == "out_normals" else 0)
    with Mesh(case.B, case.pos, case.idx, case.w, **case.mesh_kw()) as mesh:
        for compact in (False, True):
            check_listed(torch, dev, mesh, d, indices, len(indices), len(indices), compact, True, True, **kw)
            check_listed(torch, dev, mesh, d, indices, len(indices), len(indices), compact, False, True, **kw)


# ---------------- LDS limits ----------------
@pytest.mark.parametrize("P", [0, 4], ids=["plain", "shaped_to_the_byte"])
def test_lds_limits(mbik, torch_dev, P):
    """The largest rig, one listed skeleton of three: the matrices (and, shaped, B * 48 + P * 4 == 163840 bytes) fill
    the LDS, so the list costs none."""
    torch, dev = torch_dev
    B, V = MAX_BONES, 130
    assert B * 48 + P * 4 <= 163840 and (P == 0 or B * 48 + P * 4 == 163840)
    case = LC.Case(7000 + P, B, V, 4, 3, P=P, special_weights=bool(P))
    case.idx[0, 0], case.idx[1, 1], case.idx[129, 3] = 0, B - 1, B - 1
    # (the first and the last bone are named: the reference is recomputed for the edited mesh)
    full = skin_vertices_cpu(B, case.pos, case.idx, case.w, case.skin, normals=case.nrm,
                             **(dict(shape_positions=case.sp, shape_normals=case.sn, shape_mode=case.mode, shape_weights=case.cw) if P else {}))
    if P:
        case.shaped_p, case.shaped_n = full
    else:
        case.plain_p, case.plain_n = full
    d = DeviceCase(torch, dev, case)
    with Mesh(B, case.pos, case.idx, case.w, **case.mesh_kw()) as mesh:
        assert mesh.launch_shape(1)[0] == 1
        check_listed(torch, dev, mesh, d, np.array([1], np.int32), 1, 1, False, bool(P), True)


# ---------------- offsets past 2^31 ----------------
def test_offsets_past_2_31(mbik, torch_dev):
    """count x V x 3 > 2^31 floats (8.6 GB of output), in place, the list [count-3, count-2, count-1]: the last
    three rows against a three-skeleton plain launch of the same matrices, compared on the device."""
    torch, dev = torch_dev
    B, V, K, count = 2, 65537, 4, 10923
    assert count * V * 3 > 2 ** 31
    free, _ = torch.cuda.mem_get_info(dev)
    if free < 12 * 10 ** 9:
        pytest.skip(f"needs 12 GB of free device memory, {free / 1e9:.1f} GB free")
    pos, nrm, idx, w = S.random_mesh(18, B, V, K)
    d_skin = torch.from_numpy(S.random_skin(19, count, B)).to(dev)
    big = torch.empty((count, V, 3), dtype=torch.float32, device=dev)
    big[-4:] = SENTINEL
    small = torch.full((3, V, 3), SENTINEL, dtype=torch.float32, device=dev)
    d_ind = torch.tensor([count - 3, count - 2, count - 1], dtype=torch.int32, device=dev)
    d_cnt = torch.tensor([3], dtype=torch.int32, device=dev)
    with Mesh(B, pos, idx, w) as mesh:
        mesh.skin_listed(d_skin.data_ptr(), big.data_ptr(), count, d_ind.data_ptr(), d_cnt.data_ptr(), max_list=3)
        mesh.skin(d_skin[-3:].data_ptr(), small.data_ptr(), 3)
        torch.cuda.synchronize()
    assert torch.equal(big[-3:], small)
    assert not bool((small == SENTINEL).any()) and bool((big[-4] == SENTINEL).all())
    ref = skin_vertices_cpu(B, pos, idx, w, d_skin[-1:].cpu().numpy())[0]
    assert S.same_bits(small[-1:].cpu().numpy(), ref)
    del big


# ---------------- the whole frame on one stream ----------------
@pytest.mark.parametrize("compact", [False, True], ids=["in_place", "compact"])
def test_frame_on_one_stream(mbik, torch_dev, compact):
    """solve -> pose_globals(inv_bind) -> bounds -> cull -> listed skin on one side stream with nothing in between,
    on the C2 rig with 64 skeletons, against the _cpu chain; then once more on the same buffers with other targets
    and a tighter frustum.  The second list is shorter, and its run leaves the rows that were visible first and are
    culled now with the FIRST run's bits although their matrices changed: the stale tail indices[n..] is not consumed."""
    torch, dev = torch_dev
    c = LC.cull_chain(n=64, V=300)
    wl, parents, pins, B, V = c["wl"], c["parents"], c["pins"], c["B"], 300
    n = wl.n
    plan = Plan.from_workload(wl)
    assert plan.info()["abi_version"] == 15
    targets2 = wl.targets.copy()
    targets2[..., 9:12] += F(0.15)
    pi, d_ib = torch.from_numpy(wl.pose).to(dev), torch.from_numpy(c["inv_bind"]).to(dev)
    tgs = [torch.from_numpy(wl.targets).to(dev), torch.from_numpy(targets2).to(dev)]
    po = torch.empty_like(pi)
    # a solve on its own first: the two frusta are cut through the reference boxes of its poses
    plan.solve(pi.data_ptr(), tgs[0].data_ptr(), po.data_ptr())
    torch.cuda.synchronize()
    _, planes1, planes2, _, _ = LC.chain_reference(c, po.cpu().numpy())
    d_g = torch.empty((n, B, 12), dtype=torch.float32, device=dev)
    d_b = torch.empty(n * 6, dtype=torch.float32, device=dev)
    d_ind = torch.full((n,), INT_SENTINEL, dtype=torch.int32, device=dev)
    d_cnt = torch.full((1,), 123456789, dtype=torch.int32, device=dev)
    out_p, out_n = Outputs(torch, dev, n, V), Outputs(torch, dev, n, V)
    bb, used = bone_boxes_cpu(B, c["pos"], c["idx"], c["w"])
    runs = []
    with Mesh(B, c["pos"], c["idx"], c["w"], normals=c["nrm"]) as mesh:
        torch.cuda.synchronize()
        st = torch.cuda.Stream(device=dev)
        for tg, planes in zip(tgs, (planes1, planes2)):
            plan.solve(pi.data_ptr(), tg.data_ptr(), po.data_ptr(), stream=st.cuda_stream)
            plan.pose_globals(po.data_ptr(), d_g.data_ptr(), n, inv_bind_ptr=d_ib.data_ptr(), stream=st.cuda_stream)
            mesh.bounds(d_g.data_ptr(), d_b.data_ptr(), n, stream=st.cuda_stream)
            mesh.cull(d_b.data_ptr(), n, planes, indices_ptr=d_ind.data_ptr(), visible_count_ptr=d_cnt.data_ptr(), stream=st.cuda_stream)
            mesh.skin_listed(d_g.data_ptr(), out_p.ptr, n, d_ind.data_ptr(), d_cnt.data_ptr(), compact=compact,
                             out_normals_ptr=out_n.ptr, stream=st.cuda_stream)
            st.synchronize()
            # the _cpu chain from this run's solved poses
            skin, _ = pose_globals_cpu(parents, pins, po.cpu().numpy(), inv_bind=c["inv_bind"])
            lst = cull_boxes_cpu(skin_bounds_cpu(bb, used, skin), planes)[1]
            full_p, full_n = skin_vertices_cpu(B, c["pos"], c["idx"], c["w"], skin, normals=c["nrm"])
            assert np.isfinite(full_p).all() and d_cnt.cpu().tolist() == [len(lst)]
            assert np.array_equal(d_ind.cpu().numpy()[:len(lst)], lst)
            runs.append(dict(lst=lst, full_p=full_p, full_n=full_n, got_p=out_p.read().copy(), got_n=out_n.read().copy()))
    plan.close()
    r1, r2 = runs
    assert 0 < len(r2["lst"]) < len(r1["lst"]) < n                        # asserted on the reference lists
    gone = sorted(set(r1["lst"].tolist()) - set(r2["lst"].tolist()))
    assert gone
    for key, full in (("got_p", "full_p"), ("got_n", "full_n")):
        want1 = LC.expected(r1[full], r1["lst"], len(r1["lst"]), n, compact)
        assert S.same_bits(r1[key], want1)
        want2 = want1.copy()                                               # the second run writes over the first
        for r, s in enumerate(r2["lst"]):
            want2[r if compact else s] = r2[full][s]
        assert S.same_bits(r2[key], want2)
    # the proof is not vacuous: what the second run would have written to those rows differs from what is there
    stale_rows = list(range(len(r2["lst"]), len(r1["lst"]))) if compact else gone
    stale_skeletons = r1["lst"][len(r2["lst"]):].tolist() if compact else gone
    assert S.same_bits(r2["got_p"][stale_rows], r1["got_p"][stale_rows])
    assert not S.same_bits(r2["full_p"][stale_skeletons], r1["full_p"][stale_skeletons])


# ---------------- error codes ----------------
def test_error_codes(mbik, torch_dev):
    torch, dev = torch_dev
    L = _lib.load()
    B, V, K, n, P, M = 5, 9, 4, 3, 2, 4
    pos, nrm, idx, w = S.random_mesh(1, B, V, K)
    skin = S.random_skin(2, n, B)
    sp = np.zeros((P, V, 3), F)
    nskin, ncw, nout = n * B * 12, n * P, M * V * 3
    buf = torch.zeros(nskin + ncw + 2 * nout + 8, dtype=torch.float32, device=dev)
    buf[:nskin] = torch.from_numpy(skin.reshape(-1)).to(dev)
    a, b = nskin + ncw, nskin + ncw + nout
    at = lambda i: buf[i:].data_ptr()
    ibuf = torch.tensor([0, 2, 1, 0, 3], dtype=torch.int32, device=dev)
    p_ind, p_cnt = ibuf.data_ptr(), ibuf[M:].data_ptr()
    big = torch.zeros(nout + M + 1, dtype=torch.float32, device=dev)      # an output with the list right behind it
    big_i = big.view(torch.int32)
    big_i[nout:] = ibuf
    big_i[n * V * 3:n * V * 3 + M] = ibuf[:M]                             # and once more behind the first n rows
    vp = lambda x: C.c_void_p(x or None)
    plain, with_n = Mesh(B, pos, idx, w), Mesh(B, pos, idx, w, normals=nrm)
    shaped = Mesh(B, pos, idx, w, normals=nrm, shape_positions=sp, shape_normals=sp)

    def call(mesh=with_n, count=n, i=p_ind, c=p_cnt, max_list=M, s=at(0), sw=0, flags=1, p=at(a), q=at(b)):
        return L.mbik_skin_vertices_listed(mesh.h if mesh else None, count, vp(i), vp(c), max_list, vp(s), vp(sw), flags, vp(p), vp(q), None)

    E, OK = _lib.MBIK_EINVAL, _lib.MBIK_OK
    # what the plain and the shaped call refuse
    assert call(mesh=None) == E and call(count=-1) == E and call(s=0) == E and call(p=0) == E
    assert call(mesh=plain) == E                                          # out_normals for a mesh without normals
    assert call(p=at(nskin - 1), q=0) == E and call(q=at(nskin - 1)) == E  # an output overlaps skin
    assert call(q=at(b - 1)) == E                                         # the outputs overlap
    assert call(mesh=shaped, sw=at(nskin), p=at(a - 1)) == E              # out_positions overlaps shape_weights
    assert call(mesh=shaped, sw=at(nskin), p=at(b), q=at(a - 1)) == E     # out_normals overlaps shape_weights
    # the list's own
    assert call(i=0) == E and call(c=0) == E and call(max_list=-1) == E
    assert call(flags=2) == E and call(flags=3) == E and call(flags=0x80000000) == E
    assert call(sw=at(nskin)) == E                                        # shape_weights on a mesh without shapes
    assert call(i=big_i[nout:].data_ptr(), p=big[1:].data_ptr(), q=0) == E               # out_positions overlaps indices
    assert call(c=big_i[nout + M:].data_ptr(), p=big[M + 1:].data_ptr(), q=0) == E       # out_positions overlaps list_count
    assert call(i=big_i[nout:].data_ptr(), q=big[1:].data_ptr()) == E                    # out_normals overlaps indices
    # output sizes follow the flag: n = 3 rows in place, M = 4 rows compact
    assert call(flags=1, i=big_i[n * V * 3:].data_ptr(), p=big.data_ptr(), q=0) == E
    # nothing to do: OK, no launch
    assert call(count=0, i=0, c=0, s=0, p=0, q=0) == OK and call(max_list=0, i=0, c=0, s=0, p=0, q=0) == OK
    with Mesh(B, pos[:0], idx[:0], w[:0]) as empty:
        assert call(mesh=empty, i=0, c=0, s=0, p=0, q=0) == OK
    assert call(count=0, flags=2) == E and call(max_list=0, sw=at(nskin)) == E
    torch.cuda.synchronize()
    assert not bool(buf[a:].any()) and not bool(big[:n * V * 3].any())    # nothing was launched
    # adjacent, not overlapping: in place behind the list's buffer, then compact with the shaped mesh
    assert call(flags=0, i=big_i[n * V * 3:].data_ptr(), c=p_cnt, p=big.data_ptr(), q=0) == OK
    assert call(mesh=shaped, sw=at(nskin), flags=1) == OK
    torch.cuda.synchronize()
    ref_p, ref_n = skin_vertices_cpu(B, pos, idx, w, skin, normals=nrm)
    lst = np.array([0, 2, 1], np.int32)
    assert S.same_bits(big[:n * V * 3].cpu().numpy().reshape(n, V, 3), ref_p)            # every skeleton is listed
    got = buf[a:b].cpu().numpy().reshape(M, V, 3)
    # (zero shapes with zero weights: the shaped call's positions are the base's + 0)
    sref_p, _ = skin_vertices_cpu(B, pos, idx, w, skin, normals=nrm, shape_positions=sp, shape_normals=sp, shape_weights=np.zeros((n, P), F))
    assert S.same_bits(got[:3], sref_p[lst]) and not got[3].any()
    for m in (plain, with_n, shaped):
        m.close()
