"""mbik_skin_vertices_shaped on the GPU (blend shapes in front of the skinning) against
mbik_skin_vertices_shaped_cpu, bitwise (two NaNs count as equal), with sentinel floats around every
output: rig sizes x influences x normals x modes over shape, vertex and skeleton counts that end
inside a wave, a block and a skeleton tile; the weight patterns of one tile; float-aligned buffers;
the LDS limit; the vertex-chunk grid; the plain call on a shaped mesh; stream order after a solve;
error codes."""
import ctypes as C

import numpy as np
import pytest

from many_bone_ik_amd import _lib
from many_bone_ik_amd import workloads as W
from many_bone_ik_amd.skinning import Mesh, skin_vertices_cpu, synthetic_mesh, synthetic_shapes
from many_bone_ik_amd.solver import Plan, pose_globals_cpu

from . import morph_recipe as R
from . import skin_cases as S
from .test_gpu_parity import torch_dev  # noqa: F401 (fixture)

pytestmark = pytest.mark.gpu

SENTINEL = -12345.678
PAD = 16
MAX_BONES = 3413   # MBIK_SKIN_MAX_BONES
MODES = {"relative": 0, "normalized": 1}


def run_device(torch, dev, mesh, skin, c, want_normals, off_skin=0, off_c=0, off_p=0, off_n=0, stream=0):
    """Launches the shaped call on device copies.  Every output has `off` sentinel floats in front (the
    buffer is shifted by that many floats) and PAD behind; they must come back untouched.  -> (positions, normals)."""
    n, V = skin.shape[0], mesh.vertex_count
    d_skin = torch.zeros(skin.size + off_skin, dtype=torch.float32, device=dev)
    d_skin[off_skin:] = torch.from_numpy(skin.reshape(-1)).to(dev)
    d_c = torch.zeros(c.size + off_c, dtype=torch.float32, device=dev)
    d_c[off_c:] = torch.from_numpy(c.reshape(-1)).to(dev)
    d_p = torch.full((off_p + n * V * 3 + PAD,), SENTINEL, dtype=torch.float32, device=dev)
    d_n = torch.full((off_n + n * V * 3 + PAD,), SENTINEL, dtype=torch.float32, device=dev) if want_normals else None
    torch.cuda.synchronize()
    mesh.skin(d_skin[off_skin:].data_ptr(), d_p[off_p:].data_ptr(), n, out_normals_ptr=d_n[off_n:].data_ptr() if want_normals else 0,
              stream=stream, shape_weights_ptr=d_c[off_c:].data_ptr())
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


def check_against_cpu(torch, dev, B, pos, nrm, idx, w, sp, sn, mode, c, skin, want_normals=True, launch=None, **kw):
    use_n, use_sn = (nrm, sn) if want_normals else (None, None)
    ref_p, ref_n = skin_vertices_cpu(B, pos, idx, w, skin, normals=use_n, shape_positions=sp, shape_normals=use_sn, shape_mode=mode,
                                     shape_weights=c)
    with Mesh(B, pos, idx, w, normals=use_n, shape_positions=sp, shape_normals=use_sn, shape_mode=mode) as mesh:
        if launch is not None:
            launch(mesh)
        p, n = run_device(torch, dev, mesh, skin, c, want_normals, **kw)
    assert S.same_bits(p, ref_p)
    assert (n is None and ref_n is None) or S.same_bits(n, ref_n)
    return ref_p


@pytest.mark.parametrize("mode", ["relative", "normalized"])
@pytest.mark.parametrize("normals", [False, True], ids=["positions", "normals"])
@pytest.mark.parametrize("K", [4, 8])
@pytest.mark.parametrize("B", [1, 32])
def test_device_matches_cpu(mbik, torch_dev, B, K, normals, mode):
    """P in {1, 3, 17}; V ends inside a wave, just past one, just past a block; count ends inside a
    skeleton tile.  Both a one-skeleton block and a several-skeleton block occur."""
    torch, dev = torch_dev
    skin = S.random_skin(40 + B, 67, B)
    seen = set()
    for P in (1, 3, 17):
        c = R.random_shape_weights(50 + P, 67, P, MODES[mode])
        for V in (1, 63, 65, 257):
            pos, nrm, idx, w = S.random_mesh(100 * B + V, B, V, K)
            sp, sn = R.random_shapes(200 + P + V, P, V, normal_magnitude=1.0)
            if not normals:
                nrm = sn = None
            ref_p, ref_n = skin_vertices_cpu(B, pos, idx, w, skin, normals=nrm, shape_positions=sp, shape_normals=sn,
                                             shape_mode=mode, shape_weights=c)
            with Mesh(B, pos, idx, w, normals=nrm, shape_positions=sp, shape_normals=sn, shape_mode=mode) as mesh:
                for count in (1, 3, 5, 67):
                    seen.add(mesh.launch_shape(count)[0])
                    p, n = run_device(torch, dev, mesh, skin[:count], c[:count], normals)
                    assert S.same_bits(p, ref_p[:count]), (P, V, count)
                    if normals:
                        assert S.same_bits(n, ref_n[:count]), (P, V, count)
    assert 1 in seen and max(seen) > 1, seen


@pytest.mark.parametrize("mode", ["relative", "normalized"])
@pytest.mark.parametrize("P", [3, 17])
def test_weight_patterns_inside_one_tile(mbik, torch_dev, P, mode):
    """Neighbouring skeletons of one block: every shape skipped; one active shape, the first; one, the
    last; all active; weights at and just above the threshold; a NaN weight."""
    torch, dev = torch_dev
    B, V, K = 32, 65, 4
    pos, nrm, idx, w = S.random_mesh(31, B, V, K)
    sp, sn = R.random_shapes(32 + P, P, V)
    t = np.float32(0.0001)
    above = np.nextafter(t, np.float32(1))
    c = np.zeros((6, P), np.float32)
    c[1, 0] = 0.75
    c[2, P - 1] = -0.5
    c[3] = np.random.default_rng(33).uniform(0.01, 0.2, P)
    c[4, 0::2], c[4, 1::2] = t, above
    c[5] = c[3]
    c[5, 1] = np.nan
    skin = S.random_skin(34, 6, B)

    def one_tile(mesh):
        assert mesh.launch_shape(6) == (6, 1)

    ref_p = check_against_cpu(torch, dev, B, pos, nrm, idx, w, sp, sn, mode, c, skin, launch=one_tile)
    assert np.isfinite(ref_p).all()
    # the patterns do what they are there for (on the reference, which the device equals)
    plain = skin_vertices_cpu(B, pos + np.float32(0.0), idx, w, skin)[0]
    assert S.same_bits(ref_p[0], plain[0]) and not S.same_bits(ref_p[4], plain[4])
    only_above = c[4].copy()
    only_above[0::2] = 0.0
    c2 = c.copy()
    c2[4], c2[5, 1] = only_above, 0.0
    ref2 = skin_vertices_cpu(B, pos, idx, w, skin, shape_positions=sp, shape_mode=mode, shape_weights=c2)[0]
    assert S.same_bits(ref2[4], ref_p[4]) and S.same_bits(ref2[5], ref_p[5])


@pytest.mark.parametrize("shift", [1, 2, 3])
@pytest.mark.parametrize("which", ["shape_weights", "skin", "out_positions", "out_normals"])
def test_float_aligned_buffers(mbik, torch_dev, which, shift):
    torch, dev = torch_dev
    B, V, K, P = 32, 257, 4, 3
    pos, nrm, idx, w = S.random_mesh(12, B, V, K)
    sp, sn = R.random_shapes(13, P, V)
    kw = {"shape_weights": dict(off_c=shift), "skin": dict(off_skin=shift), "out_positions": dict(off_p=shift),
          "out_normals": dict(off_n=shift)}[which]
    check_against_cpu(torch, dev, B, pos, nrm, idx, w, sp, sn, "relative", R.random_shape_weights(14, 5, P, 0),
                      S.random_skin(15, 5, B), **kw)


def test_lds_limit(mbik, torch_dev):
    """The largest rig with four shapes: one skeleton's matrices and weights fill the LDS exactly, one
    skeleton a block.  A fifth shape is refused at creation."""
    torch, dev = torch_dev
    B, V, K = MAX_BONES, 130, 4
    pos, nrm, idx, w = S.random_mesh(5, B, V, K)
    idx[0, 0], idx[1, 1], idx[129, 3] = 0, B - 1, B - 1
    sp, sn = R.random_shapes(6, 5, V)
    c = np.array([[0.5, -0.25, 0.125, 1.0], [0.0, 0.0, 0.0, -0.75]], np.float32)   # (the last weight is the LDS's last float)

    def one_skeleton(mesh):
        assert mesh.launch_shape(2)[0] == 1

    check_against_cpu(torch, dev, B, pos, nrm, idx, w, sp[:4], sn[:4], "normalized", c, S.random_skin(7, 2, B), launch=one_skeleton)
    with pytest.raises(_lib.MbikError) as e:
        Mesh(B, pos, idx, w, normals=nrm, shape_positions=sp, shape_normals=sn)
    assert e.value.code == _lib.MBIK_EUNSUPPORTED


def test_vertex_chunk_grid_path(mbik, torch_dev):
    """Few skeletons, a large mesh: the vertex range is split over blocks."""
    torch, dev = torch_dev
    B, V, K, P = 32, 70001, 4, 2
    pos, nrm, idx, w = S.random_mesh(14, B, V, K)
    sp, sn = R.random_shapes(15, P, V)

    def chunks(mesh):
        assert mesh.launch_shape(2)[1] > 1

    check_against_cpu(torch, dev, B, pos, nrm, idx, w, sp, sn, "relative", np.array([[0.5, -1.0], [0.0, 0.25]], np.float32),
                      S.random_skin(16, 2, B), launch=chunks)


@pytest.mark.parametrize("K", [4, 8])
def test_plain_call_on_a_shaped_mesh(mbik, torch_dev, K):
    """Mesh.skin without weights on a shaped mesh: the bits of the same mesh created without shapes."""
    from .test_gpu_skin import run_device as run_plain
    torch, dev = torch_dev
    B, V, P = 32, 1000, 3
    pos, nrm, idx, w = S.random_mesh(21, B, V, K)
    sp, sn = R.random_shapes(22, P, V)
    skin = S.random_skin(23, 67, B)
    with Mesh(B, pos, idx, w, normals=nrm) as plain, Mesh(B, pos, idx, w, normals=nrm, shape_positions=sp, shape_normals=sn) as shaped:
        p0, n0 = run_plain(torch, dev, plain, skin, True)
        p1, n1 = run_plain(torch, dev, shaped, skin, True)
    ref_p, ref_n = skin_vertices_cpu(B, pos, idx, w, skin, normals=nrm)
    assert S.same_bits(p1, p0) and S.same_bits(n1, n0) and S.same_bits(p1, ref_p) and S.same_bits(n1, ref_n)


def test_stream_order_after_solve(mbik, torch_dev):
    """solve -> pose_globals(inv_bind) -> skin(shape_weights) on one side stream, nothing in between; then once more."""
    torch, dev = torch_dev
    wl = W.generate(2, 64)
    parents, pins = wl.topo.parents.tolist(), wl.topo.pins.tolist()
    n, B, K, V, P = wl.n, len(parents), 4, 1500, 4
    rest, _ = pose_globals_cpu(parents, [], wl.pose[:1])
    inv_bind = np.random.default_rng(25).uniform(-1.0, 1.0, (B, 12)).astype(np.float32)
    pos, nrm, idx, w = synthetic_mesh(parents, rest[0], V, K, seed=3)
    sp, sn = synthetic_shapes(pos, nrm, P, seed=4)
    c = R.random_shape_weights(26, n, P, 1)
    plan = Plan.from_workload(wl)
    pi, tg = torch.from_numpy(wl.pose).to(dev), torch.from_numpy(wl.targets).to(dev)
    po, d_ib, d_c = torch.empty_like(pi), torch.from_numpy(inv_bind).to(dev), torch.from_numpy(c).to(dev)
    d_g = torch.empty((n, B, 12), dtype=torch.float32, device=dev)
    d_p = torch.full((n * V * 3 + PAD,), SENTINEL, dtype=torch.float32, device=dev)
    d_n = torch.full((n * V * 3 + PAD,), SENTINEL, dtype=torch.float32, device=dev)
    with Mesh(B, pos, idx, w, normals=nrm, shape_positions=sp, shape_normals=sn, shape_mode="normalized") as mesh:
        torch.cuda.synchronize()
        st = torch.cuda.Stream(device=dev)
        plan.solve(pi.data_ptr(), tg.data_ptr(), po.data_ptr(), stream=st.cuda_stream)
        plan.pose_globals(po.data_ptr(), d_g.data_ptr(), n, inv_bind_ptr=d_ib.data_ptr(), stream=st.cuda_stream)
        mesh.skin(d_g.data_ptr(), d_p.data_ptr(), n, out_normals_ptr=d_n.data_ptr(), stream=st.cuda_stream, shape_weights_ptr=d_c.data_ptr())
        st.synchronize()
        first_p, first_n = d_p.cpu().numpy(), d_n.cpu().numpy()
        mesh.skin(d_g.data_ptr(), d_p.data_ptr(), n, out_normals_ptr=d_n.data_ptr(), stream=st.cuda_stream, shape_weights_ptr=d_c.data_ptr())
        st.synchronize()
    plan.close()
    skinned, _ = pose_globals_cpu(parents, pins, po.cpu().numpy(), inv_bind=inv_bind)
    ref_p, ref_n = skin_vertices_cpu(B, pos, idx, w, skinned, normals=nrm, shape_positions=sp, shape_normals=sn, shape_mode="normalized",
                                     shape_weights=c)
    assert np.isfinite(ref_p).all()
    for got, ref in ((first_p, ref_p), (first_n, ref_n), (d_p.cpu().numpy(), ref_p), (d_n.cpu().numpy(), ref_n)):
        assert (got[n * V * 3:] == np.float32(SENTINEL)).all()
        assert S.same_bits(got[:n * V * 3].reshape(n, V, 3), ref)


def test_error_codes(mbik, torch_dev):
    torch, dev = torch_dev
    L = _lib.load()
    B, V, K, P, n = 5, 9, 4, 3, 2
    pos, nrm, idx, w = S.random_mesh(1, B, V, K)
    sp, sn = R.random_shapes(2, P, V)
    skin, c = S.random_skin(3, n, B), R.random_shape_weights(4, n, P, 0)
    n_skin, n_c, n_out = n * B * 12, n * P, n * V * 3
    buf = torch.zeros(n_skin + n_c + 2 * n_out, dtype=torch.float32, device=dev)
    buf[:n_skin] = torch.from_numpy(skin.reshape(-1)).to(dev)
    buf[n_skin:n_skin + n_c] = torch.from_numpy(c.reshape(-1)).to(dev)
    a = n_skin + n_c
    b = a + n_out
    at = lambda i: buf[i:].data_ptr()
    unshaped = Mesh(B, pos, idx, w, normals=nrm)
    no_normals = Mesh(B, pos, idx, w, shape_positions=sp)
    shaped = Mesh(B, pos, idx, w, normals=nrm, shape_positions=sp, shape_normals=sn)

    def call(mesh, count, p_skin, p_c, p_out, p_n=0):
        vp = lambda x: C.c_void_p(x or None)
        return L.mbik_skin_vertices_shaped(mesh.h if mesh is not None else None, count, vp(p_skin), vp(p_c), vp(p_out), vp(p_n), None)

    E = _lib.MBIK_EINVAL
    assert call(None, n, at(0), at(n_skin), at(a)) == E                            # null mesh
    assert call(unshaped, n, at(0), at(n_skin), at(a)) == E                        # a mesh without shapes
    assert "no shapes" in _lib.last_error()
    assert call(shaped, n, at(0), 0, at(a)) == E                                   # null weights
    assert call(shaped, n, at(0), at(n_skin), at(a - 1)) == E                      # weights overlap out_positions
    assert call(shaped, n, at(0), at(n_skin), at(b), at(a - 1)) == E               # weights overlap out_normals
    assert call(shaped, n, 0, at(n_skin), at(a)) == E                              # null skin
    assert call(shaped, n, at(0), at(n_skin), 0) == E                              # null output
    assert call(shaped, -1, at(0), at(n_skin), at(a)) == E                         # negative count
    assert call(no_normals, n, at(0), at(n_skin), at(a), at(b)) == E               # out_normals for a mesh without normals
    assert call(shaped, n, at(n_c + n_out), at(n_skin), at(a)) == E                # out_positions overlaps skin (read from there)
    assert call(shaped, n, at(0), at(n_skin), at(a), at(b - 4)) == E               # the outputs overlap
    assert call(shaped, 0, 0, 0, 0) == _lib.MBIK_OK                                # count == 0: OK, no launch
    with Mesh(B, pos[:0], idx[:0], w[:0], shape_positions=sp[:, :0]) as empty:     # no vertices: OK, no launch
        assert call(empty, n, at(0), 0, at(a)) == _lib.MBIK_OK
        assert empty.launch_shape(n)[0] >= 1
    for kw in (dict(shape_positions=sp, shape_normals=sn), dict(normals=nrm, shape_positions=sp),
               dict(normals=nrm, shape_positions=sp, shape_normals=sn, shape_mode="cubic")):
        with pytest.raises((_lib.MbikError, ValueError)):                          # refused before any device work
            Mesh(B, pos, idx, w, **kw)
    torch.cuda.synchronize()
    assert not bool(buf[a:].any())                                                 # nothing was launched
    assert call(shaped, n, at(0), at(n_skin), at(a), at(b)) == _lib.MBIK_OK        # adjacent, not overlapping
    torch.cuda.synchronize()
    ref_p, ref_n = skin_vertices_cpu(B, pos, idx, w, skin, normals=nrm, shape_positions=sp, shape_normals=sn, shape_weights=c)
    assert S.same_bits(buf[a:b].cpu().numpy().reshape(n, V, 3), ref_p) and S.same_bits(buf[b:].cpu().numpy().reshape(n, V, 3), ref_n)
    unshaped.close(), no_normals.close(), shaped.close()
