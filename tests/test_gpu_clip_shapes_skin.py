"""The chain blend-shape tracks exist for, on one side stream with one synchronisation at the end:
ClipSet.sample_layers -> Plan.pose_globals(inv_bind) -> ClipSet.sample_shapes_layers ->
Mesh.skin(shape_weights_ptr = the buffer just written), bitwise against the same chain computed
with the _cpu functions, in both shape modes.  The sampled weights reach the vertices (the result
differs from skinning with the init weights), and weights at or below morph.h's 0.0001 threshold
and a NaN weight are among them."""
import numpy as np
import pytest

from many_bone_ik_amd import animation as A
from many_bone_ik_amd import workloads as W
from many_bone_ik_amd.skinning import Mesh, skin_vertices_cpu, synthetic_mesh, synthetic_shapes
from many_bone_ik_amd.solver import Plan, pose_globals_cpu

from . import clip_shapes_recipe as R
from .test_gpu_clip_sample import _rig_clips
from .test_gpu_parity import torch_dev  # noqa: F401 (fixture)

pytestmark = pytest.mark.gpu

SENTINEL = float(np.uint32(0x4B1D4B1D).view(np.float32))
B, V, P, N, K = 5, 40, 5, 33, 2


@pytest.fixture(scope="module")
def scene(mbik):
    """The rig, its clips with shape tracks, the layer records, the mesh arrays and the host chain's
    poses, skin transforms and weights -- computed once, left unchanged."""
    parents = [b - 1 for b in range(B)]
    wl = W.generate(9, 2, topo=W.custom_topology(parents, [1]))
    rest = np.ascontiguousarray(wl.pose[0])
    clips = A.synthetic_shape_tracks(61, P, _rig_clips(rest, 6))
    init = np.array([0.0, 0.5, 0.00005, 1.0, 0.25], np.float32)
    rng = np.random.default_rng(62)
    w = rng.uniform(0.0, 1.0, N).astype(np.float32)
    layers = R.pack(rng.uniform(0.0, 10.0, (N, K)), np.tile([0, 1], (N, 1)), np.stack([w, np.float32(1) - w], axis=1))
    layers["clip"][4] = (0, R.OFF)
    # a NaN key value (taken as given) makes shape 1 NaN wherever clip 0 is accumulated; the poses stay finite
    L0 = clips[0]["length"]
    clips[0]["shape_tracks"] = [t for t in clips[0]["shape_tracks"] if t["shape"] != 1] + [
        dict(shape=1, interpolation=A.LINEAR, loop_wrap=1, times=np.array([0.0, 0.5]) * L0, values=np.array([np.nan, 0.3], np.float32))]
    inv_bind = rng.uniform(-1.0, 1.0, (B, 12)).astype(np.float32)
    rest_globals, _ = pose_globals_cpu(parents, [], rest[None])
    pos, nrm, idx, wgt = synthetic_mesh(parents, rest_globals[0], V, 4, seed=63)
    sp, sn = synthetic_shapes(pos, nrm, P, seed=64)
    poses = A.clip_sample_layers_cpu(B, rest, clips, layers, R.NORMALIZE)
    skinned, _ = pose_globals_cpu(parents, [], poses, inv_bind=inv_bind)
    weights = A.clip_sample_shapes_layers_cpu(P, clips, layers, R.NORMALIZE, shape_init=init)
    for a in (poses, skinned, weights):
        a.setflags(write=False)
    return dict(wl=wl, rest=rest, clips=clips, init=init, layers=layers, inv_bind=inv_bind, mesh=(pos, nrm, idx, wgt), shapes=(sp, sn),
                poses=poses, skinned=skinned, weights=weights)


def test_the_sampled_weights_meet_the_skip_threshold_and_nan(scene):
    w = scene["weights"]
    assert np.isnan(w).any() and (np.abs(w[~np.isnan(w)]) <= 0.0001).any() and (np.abs(w[~np.isnan(w)]) > 0.0001).any()
    assert (R.bits(w) != R.bits(np.broadcast_to(scene["init"], w.shape))).any(axis=1).all()


@pytest.mark.parametrize("mode", ("relative", "normalized"))
def test_chain_on_one_stream_matches_the_host_chain(scene, torch_dev, mode):
    torch, dev = torch_dev
    s = scene
    pos, nrm, idx, wgt = s["mesh"]
    sp, sn = s["shapes"]
    assert np.isfinite(s["poses"]).all() and np.isfinite(s["skinned"]).all()
    want_p, want_n = skin_vertices_cpu(B, pos, idx, wgt, s["skinned"], normals=nrm, shape_positions=sp, shape_normals=sn, shape_mode=mode,
                                       shape_weights=s["weights"])
    init_p, init_n = skin_vertices_cpu(B, pos, idx, wgt, s["skinned"], normals=nrm, shape_positions=sp, shape_normals=sn, shape_mode=mode,
                                       shape_weights=np.ascontiguousarray(np.broadcast_to(s["init"], (N, P))))
    assert np.isfinite(want_p).all() and np.isfinite(want_n).all()
    # the sampled weights reach the vertices: every skeleton differs from the init-weight result
    assert (R.bits(want_p) != R.bits(init_p)).any(axis=(1, 2)).all() and (R.bits(want_n) != R.bits(init_n)).any(axis=(1, 2)).all()

    plan = Plan.from_workload(s["wl"])
    with A.ClipSet(B, s["rest"], s["clips"], shape_count=P, shape_init=s["init"]) as cs, \
            Mesh(B, pos, idx, wgt, normals=nrm, shape_positions=sp, shape_normals=sn, shape_mode=mode) as mesh:
        d_l = torch.from_numpy(s["layers"].reshape(-1).view(np.uint8)).to(dev)
        d_ib = torch.from_numpy(s["inv_bind"]).to(dev)
        d_pose = torch.full((N, B, 10), SENTINEL, dtype=torch.float32, device=dev)
        d_g = torch.full((N, B, 12), SENTINEL, dtype=torch.float32, device=dev)
        d_w = torch.full((N, P), SENTINEL, dtype=torch.float32, device=dev)
        d_p = torch.full((N, V, 3), SENTINEL, dtype=torch.float32, device=dev)
        d_n = torch.full((N, V, 3), SENTINEL, dtype=torch.float32, device=dev)
        st = torch.cuda.Stream(device=dev)
        torch.cuda.synchronize()
        q = st.cuda_stream
        cs.sample_layers(d_l.data_ptr(), d_pose.data_ptr(), N, K, flags=R.NORMALIZE, stream=q)
        plan.pose_globals(d_pose.data_ptr(), d_g.data_ptr(), N, inv_bind_ptr=d_ib.data_ptr(), stream=q)
        cs.sample_shapes_layers(d_l.data_ptr(), d_w.data_ptr(), N, K, flags=R.NORMALIZE, stream=q)
        mesh.skin(d_g.data_ptr(), d_p.data_ptr(), N, out_normals_ptr=d_n.data_ptr(), stream=q, shape_weights_ptr=d_w.data_ptr())
        st.synchronize()
        got = [t.cpu().numpy() for t in (d_pose, d_g, d_w, d_p, d_n)]
    plan.close()
    assert R.same_bits(got[0], s["poses"]), "sampled poses"
    assert R.same_bits(got[1], s["skinned"]), "skin transforms"
    assert R.same_bits(got[2], s["weights"]), "sampled weights"
    assert R.same_bits(got[3], want_p), "positions"
    assert R.same_bits(got[4], want_n), "normals"
