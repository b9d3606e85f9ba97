"""mbik_skin_vertices on the GPU (linear blend skinning) against mbik_skin_vertices_cpu,
bitwise (two NaNs count as equal), with sentinel floats around every output: rig sizes x influences
x normals over vertex counts and skeleton counts that end inside a wave, a block and a skeleton
tile; broadcast and conflict meshes; the LDS limit; float-aligned buffers; both grid paths;
offsets past 2^31; special values; stream order after a solve; error codes."""
import numpy as np
import pytest

from many_bone_ik_amd import _lib
from many_bone_ik_amd import workloads as W
from many_bone_ik_amd.skinning import Mesh, skin_vertices_cpu, synthetic_mesh
from many_bone_ik_amd.solver import Plan, pose_globals_cpu

from . import skin_cases as S
from .test_gpu_parity import torch_dev  # noqa: F401 (fixture)

pytestmark = pytest.mark.gpu

SENTINEL = -12345.678
PAD = 16
MAX_BONES = 3413   # MBIK_SKIN_MAX_BONES


def run_device(torch, dev, mesh, skin, want_normals, off_skin=0, off_p=0, off_n=0, stream=0, count=None):
    """Launches on device copies.  Every output has `off` sentinel floats in front (the buffer is
    shifted by that many floats) and PAD behind; they must come back untouched.  -> (positions, normals)."""
    n = skin.shape[0] if count is None else count
    V = mesh.vertex_count
    d_skin = torch.zeros(skin.size + off_skin, dtype=torch.float32, device=dev)
    d_skin[off_skin:] = torch.from_numpy(skin.reshape(-1)).to(dev)
    d_p = torch.full((off_p + n * V * 3 + PAD,), SENTINEL, dtype=torch.float32, device=dev)
    d_n = torch.full((off_n + n * V * 3 + PAD,), SENTINEL, dtype=torch.float32, device=dev) if want_normals else None
    torch.cuda.synchronize()
    mesh.skin(d_skin[off_skin:].data_ptr(), d_p[off_p:].data_ptr(), n,
              out_normals_ptr=d_n[off_n:].data_ptr() if want_normals else 0, stream=stream)
    torch.cuda.synchronize()
    out = []
    for d, off in ((d_p, off_p), (d_n, off_n)):
        if d is None:
            out.append(None)
            continue
        h = d.cpu().numpy()
        assert (h[:off] == np.float32(SENTINEL)).all() and (h[off + n * V * 3:] == np.float32(SENTINEL)).all()
        out.append(h[off:off + n * V * 3].reshape(n, V, 3))
    return out


def check_against_cpu(torch, dev, B, pos, nrm, idx, w, skin, want_normals, **kw):
    ref_p, ref_n = skin_vertices_cpu(B, pos, idx, w, skin, normals=nrm if want_normals else None)
    with Mesh(B, pos, idx, w, normals=nrm if want_normals else None) as mesh:
        p, n = run_device(torch, dev, mesh, skin, want_normals, **kw)
    assert S.same_bits(p, ref_p)
    assert (n is None and ref_n is None) or S.same_bits(n, ref_n)


@pytest.mark.parametrize("normals", [False, True], ids=["positions", "normals"])
@pytest.mark.parametrize("K", [4, 8])
@pytest.mark.parametrize("B", [1, 32, 200])
def test_device_matches_cpu(mbik, torch_dev, B, K, normals):
    """V ends inside a wave, just past one, just past a block; count ends inside a skeleton tile."""
    torch, dev = torch_dev
    skin = S.random_skin(40 + B, 67, B)
    for V in (1, 63, 65, 257, 1000):
        pos, nrm, idx, w = S.random_mesh(100 * B + V, B, V, K)
        use_n = nrm if normals else None
        ref_p, ref_n = skin_vertices_cpu(B, pos, idx, w, skin, normals=use_n)
        with Mesh(B, pos, idx, w, normals=use_n) as mesh:
            for count in (1, 2, 3, 5, 67):
                p, n = run_device(torch, dev, mesh, skin[:count], normals)
                assert S.same_bits(p, ref_p[:count]), (V, count)
                if normals:
                    assert S.same_bits(n, ref_n[:count]), (V, count)


@pytest.mark.parametrize("pattern", ["bone0", "last_bone", "distinct"])
def test_broadcast_and_conflict_meshes(mbik, torch_dev, pattern):
    """Every lane on one bone (LDS broadcast), and the 64 lanes of a wave on 64 distinct bones."""
    torch, dev = torch_dev
    B, V, K = 200, 1000, 4
    pos, nrm, idx, w = S.random_mesh(77, B, V, K)
    if pattern == "bone0":
        idx[:] = 0
    elif pattern == "last_bone":
        idx[:] = B - 1
    else:
        idx[:] = (3 * np.arange(V)[:, None] + 7 * np.arange(K)[None, :]) % B
        for v0 in range(0, V - 63, 64):   # (3 * 64 < B: no bone twice among 64 consecutive vertices)
            assert all(len(set(idx[v0:v0 + 64, k].tolist())) == 64 for k in range(K))
    check_against_cpu(torch, dev, B, pos, nrm, idx, w, S.random_skin(9, 5, B), True)


def test_lds_limit(mbik, torch_dev):
    """The largest rig: one skeleton's matrices fill the LDS, one skeleton a block.  One bone more is refused."""
    torch, dev = torch_dev
    B, V, K = MAX_BONES, 130, 4
    pos, nrm, idx, w = S.random_mesh(5, B, V, K)
    idx[0, 0], idx[1, 1], idx[129, 3] = 0, B - 1, B - 1
    skin = S.random_skin(6, 2, B)
    with Mesh(B, pos, idx, w, normals=nrm) as mesh:
        assert mesh.launch_shape(2)[0] == 1
        p, n = run_device(torch, dev, mesh, skin, True)
    ref_p, ref_n = skin_vertices_cpu(B, pos, idx, w, skin, normals=nrm)
    assert S.same_bits(p, ref_p) and S.same_bits(n, ref_n)
    with pytest.raises(_lib.MbikError) as e:
        Mesh(B + 1, pos, idx, w)
    assert e.value.code == _lib.MBIK_EUNSUPPORTED


@pytest.mark.parametrize("shift", [1, 2, 3])
@pytest.mark.parametrize("which", ["skin", "out_positions", "out_normals"])
def test_float_aligned_buffers(mbik, torch_dev, which, shift):
    torch, dev = torch_dev
    B, V, K = 32, 257, 4
    pos, nrm, idx, w = S.random_mesh(12, B, V, K)
    kw = {"skin": dict(off_skin=shift), "out_positions": dict(off_p=shift), "out_normals": dict(off_n=shift)}[which]
    check_against_cpu(torch, dev, B, pos, nrm, idx, w, S.random_skin(13, 5, B), True, **kw)


def test_vertex_chunk_grid_path(mbik, torch_dev):
    """Few skeletons, a large mesh: the vertex range is split over blocks."""
    torch, dev = torch_dev
    B, V, K = 32, 70001, 4
    pos, nrm, idx, w = S.random_mesh(14, B, V, K)
    skin = S.random_skin(15, 2, B)
    with Mesh(B, pos, idx, w) as mesh:
        assert mesh.launch_shape(2)[1] > 1
        p, _ = run_device(torch, dev, mesh, skin, False)
    assert S.same_bits(p, skin_vertices_cpu(B, pos, idx, w, skin)[0])


def test_skeleton_tile_grid_path(mbik, torch_dev):
    """Many skeletons, a small mesh: several skeletons share a block's LDS."""
    torch, dev = torch_dev
    B, V, K = 32, 64, 4
    pos, nrm, idx, w = S.random_mesh(16, B, V, K)
    skin = S.random_skin(17, 4096, B)
    with Mesh(B, pos, idx, w, normals=nrm) as mesh:
        assert mesh.launch_shape(4096)[0] > 1
        p, n = run_device(torch, dev, mesh, skin, True)
    ref_p, ref_n = skin_vertices_cpu(B, pos, idx, w, skin, normals=nrm)
    assert S.same_bits(p, ref_p) and S.same_bits(n, ref_n)


def test_offsets_past_2_31(mbik, torch_dev):
    """count x V x 3 > 2^31 floats (8.6 GB of output): the last three skeletons against a
    three-skeleton launch of the same matrices, compared on the device."""
    torch, dev = torch_dev
    B, V, K, count = 2, 65537, 4, 10923
    assert count * V * 3 > 2 ** 31
    free, _ = torch.cuda.mem_get_info(dev)
    if free < 12 * 10 ** 9:
        pytest.skip(f"needs 12 GB of free device memory, {free / 1e9:.1f} GB free")
    pos, nrm, idx, w = S.random_mesh(18, B, V, K)
    d_skin = torch.from_numpy(S.random_skin(19, count, B)).to(dev)
    big = torch.empty((count, V, 3), dtype=torch.float32, device=dev)
    big[-3:] = SENTINEL
    small = torch.full((3, V, 3), SENTINEL, dtype=torch.float32, device=dev)
    with Mesh(B, pos, idx, w) as mesh:
        mesh.skin(d_skin.data_ptr(), big.data_ptr(), count)
        mesh.skin(d_skin[-3:].data_ptr(), small.data_ptr(), 3)
        torch.cuda.synchronize()
    assert torch.equal(big[-3:], small)
    assert not bool((small == SENTINEL).any())
    ref = skin_vertices_cpu(B, pos, idx, w, d_skin[-1:].cpu().numpy())[0]
    assert S.same_bits(small[-1:].cpu().numpy(), ref)
    del big


def test_special_values(mbik, torch_dev):
    torch, dev = torch_dev
    B, V, K = 32, 300, 8
    rng = np.random.default_rng(20)
    # signed zeros everywhere they can meet: matrices, positions, normals and weights
    pos, nrm, idx, w = S.random_mesh(21, B, V, K, "signed")
    zeros = np.array([0.0, -0.0, 1.0, -1.0], np.float32)
    skin = zeros[rng.integers(0, 4, (3, B, 12))]
    pos[::3], nrm[::5], w[::2] = zeros[rng.integers(0, 4, pos[::3].shape)], -0.0, zeros[rng.integers(0, 2, w[::2].shape)]
    check_against_cpu(torch, dev, B, pos, nrm, idx, w, skin, True)
    # weights negative and not summing to 1
    pos, nrm, idx, w = S.random_mesh(22, B, V, K, "signed")
    check_against_cpu(torch, dev, B, pos, nrm, idx, w, S.random_skin(23, 3, B), True)
    # a NaN bone in one skeleton reaches exactly the vertices that list it, weight 0 included
    idx[idx == 4] = 5
    idx[10, 7], idx[20, 0] = 4, 4
    idx[30, 1], w[30, 1] = 4, 0.0
    skin = S.random_skin(24, 3, B)
    skin[1, 4] = np.nan
    with Mesh(B, pos, idx, w, normals=nrm) as mesh:
        p, n = run_device(torch, dev, mesh, skin, True)
    ref_p, ref_n = skin_vertices_cpu(B, pos, idx, w, skin, normals=nrm)
    assert S.same_bits(p, ref_p) and S.same_bits(n, ref_n)
    lists = (idx == 4).any(axis=1)
    assert np.array_equal(np.isnan(p[1]).all(axis=1), lists) and not np.isnan(p[0]).any() and not np.isnan(p[2]).any()


def test_stream_order_after_solve(mbik, torch_dev):
    """solve -> pose_globals(inv_bind) -> skin on one side stream, nothing in between; then once more."""
    torch, dev = torch_dev
    wl = W.generate(2, 64)
    parents, pins = wl.topo.parents.tolist(), wl.topo.pins.tolist()
    n, B, K, V = wl.n, len(parents), 4, 1500
    rest, _ = pose_globals_cpu(parents, [], wl.pose[:1])
    inv_bind = np.random.default_rng(25).uniform(-1.0, 1.0, (B, 12)).astype(np.float32)
    pos, nrm, idx, w = synthetic_mesh(parents, rest[0], V, K, seed=3)
    plan = Plan.from_workload(wl)
    pi, tg = torch.from_numpy(wl.pose).to(dev), torch.from_numpy(wl.targets).to(dev)
    po, d_ib = torch.empty_like(pi), torch.from_numpy(inv_bind).to(dev)
    d_g = torch.empty((n, B, 12), dtype=torch.float32, device=dev)
    d_p = torch.full((n * V * 3 + PAD,), SENTINEL, dtype=torch.float32, device=dev)
    d_n = torch.full((n * V * 3 + PAD,), SENTINEL, dtype=torch.float32, device=dev)
    with Mesh(B, pos, idx, w, normals=nrm) as mesh:
        torch.cuda.synchronize()
        st = torch.cuda.Stream(device=dev)
        plan.solve(pi.data_ptr(), tg.data_ptr(), po.data_ptr(), stream=st.cuda_stream)
        plan.pose_globals(po.data_ptr(), d_g.data_ptr(), n, inv_bind_ptr=d_ib.data_ptr(), stream=st.cuda_stream)
        mesh.skin(d_g.data_ptr(), d_p.data_ptr(), n, out_normals_ptr=d_n.data_ptr(), stream=st.cuda_stream)
        st.synchronize()
        first_p, first_n = d_p.cpu().numpy(), d_n.cpu().numpy()
        mesh.skin(d_g.data_ptr(), d_p.data_ptr(), n, out_normals_ptr=d_n.data_ptr(), stream=st.cuda_stream)
        st.synchronize()
    plan.close()
    skinned, _ = pose_globals_cpu(parents, pins, po.cpu().numpy(), inv_bind=inv_bind)
    ref_p, ref_n = skin_vertices_cpu(B, pos, idx, w, skinned, normals=nrm)
    assert np.isfinite(ref_p).all()
    for got, ref in ((first_p, ref_p), (first_n, ref_n), (d_p.cpu().numpy(), ref_p), (d_n.cpu().numpy(), ref_n)):
        assert (got[n * V * 3:] == np.float32(SENTINEL)).all()
        assert S.same_bits(got[:n * V * 3].reshape(n, V, 3), ref)


def test_error_codes(mbik, torch_dev):
    torch, dev = torch_dev
    B, V, K, n = 5, 9, 4, 2
    pos, nrm, idx, w = S.random_mesh(1, B, V, K)
    skin = S.random_skin(2, n, B)
    buf = torch.zeros(n * B * 12 + 2 * n * V * 3, dtype=torch.float32, device=dev)
    buf[: n * B * 12] = torch.from_numpy(skin.reshape(-1)).to(dev)
    p_skin, a, b = buf.data_ptr(), n * B * 12, n * B * 12 + n * V * 3
    plain, with_n = Mesh(B, pos, idx, w), Mesh(B, pos, idx, w, normals=nrm)

    def code(mesh, *args, **kw):
        with pytest.raises(_lib.MbikError) as e:
            mesh.skin(*args, **kw)
        return e.value.code

    E = _lib.MBIK_EINVAL
    assert code(plain, 0, buf[a:].data_ptr(), n) == E                                              # null skin
    assert code(plain, p_skin, 0, n) == E                                                          # null output
    assert code(plain, p_skin, buf[a:].data_ptr(), -1) == E                                        # negative count
    assert code(plain, p_skin, buf[a:].data_ptr(), n, out_normals_ptr=buf[b:].data_ptr()) == E     # no mesh normals
    assert code(plain, p_skin, buf[a - 4:].data_ptr(), n) == E                                     # output overlaps skin
    assert code(with_n, p_skin, buf[a:].data_ptr(), n, out_normals_ptr=buf[a - 4:].data_ptr()) == E  # normals overlap skin
    assert code(with_n, p_skin, buf[a:].data_ptr(), n, out_normals_ptr=buf[b - 4:].data_ptr()) == E  # outputs overlap
    plain.skin(0, 0, 0)                                                                            # count == 0: OK, no launch
    with Mesh(B, pos[:0], idx[:0], w[:0]) as empty:                                                # no vertices: OK, no launch
        empty.skin(p_skin, buf[a:].data_ptr(), n)
        assert empty.launch_shape(n)[0] >= 1
    for bad in (B, -1):                                                                            # refused before any device work
        i2 = idx.copy()
        i2[3, 2] = bad
        with pytest.raises(_lib.MbikError) as e:
            Mesh(B, pos, i2, w)
        assert e.value.code == E
    with pytest.raises(_lib.MbikError) as e:
        Mesh(B, pos, idx[:, :3], w[:, :3])
    assert e.value.code == E
    torch.cuda.synchronize()
    assert not bool(buf[a:].any())                                                                 # nothing was launched
    with_n.skin(p_skin, buf[a:].data_ptr(), n, out_normals_ptr=buf[b:].data_ptr())                 # adjacent, not overlapping
    torch.cuda.synchronize()
    ref_p, ref_n = skin_vertices_cpu(B, pos, idx, w, skin, normals=nrm)
    assert S.same_bits(buf[a:b].cpu().numpy().reshape(n, V, 3), ref_p) and S.same_bits(buf[b:].cpu().numpy().reshape(n, V, 3), ref_n)
    plain.close(), with_n.close()
