"""Destroying a handle gives its device memory back: plans with every kind of buffer they own, a
plan whose creation fails after it took memory, and meshes.  Each case creates its torch tensors
first, reads the device's free memory, runs 8 create / use / destroy cycles that take at least
32 MiB each, and asserts that no more than 64 MiB went missing: a leak of a quarter of a cycle's
memory would exceed that.  (Clip sets, groups and multi handles own a few small buffers this
method cannot see.)  Needs an MI355X: -m gpu."""
import numpy as np
import pytest

from many_bone_ik_amd import _lib
from many_bone_ik_amd import workloads as W
from many_bone_ik_amd.skinning import Mesh, synthetic_mesh, synthetic_shapes
from many_bone_ik_amd.solver import Plan

pytestmark = pytest.mark.gpu

CYCLES = 8
MARGIN = 64 << 20


@pytest.fixture(scope="module")
def wl():
    return W.generate(5, 512)  # C5: ~32 MB of setup tables


def free_bytes(torch):
    torch.cuda.synchronize()
    return torch.cuda.mem_get_info(0)[0]


@pytest.mark.parametrize("constraint_mode", [False, True])
def test_plan_cycles_give_every_buffer_back(mbik, wl, constraint_mode):
    """Uploads, locals, state, checkpoint globals and tiled tables (placement 2), the state's grow
    path (one lane per skeleton stages no headings; the automatic lane count does), constraint_mode's
    node caches, the fk schedule, the host-solve scratch and the topology blob."""
    import torch
    dev = torch.device("cuda", 0)
    pi, tg = torch.from_numpy(wl.pose).to(dev), torch.from_numpy(wl.targets).to(dev)
    po = torch.empty_like(pi)
    gl = torch.empty((wl.n, wl.pose.shape[1], 12), dtype=torch.float32, device=dev)

    def cycle():
        plan = Plan.from_workload(wl, lanes=1, constraint_mode=constraint_mode)
        if not constraint_mode:
            plan.set_locals_placement(2)
        plan.solve(pi.data_ptr(), tg.data_ptr(), po.data_ptr())
        torch.cuda.synchronize()
        first, bytes1 = po.cpu().numpy(), plan.info()["device_bytes"]
        plan.set_layout(0, 0, 0)
        plan.solve(pi.data_ptr(), tg.data_ptr(), po.data_ptr())
        torch.cuda.synchronize()
        if not constraint_mode:
            assert plan.info()["lanes_per_skeleton"] > 1 and plan.info()["device_bytes"] > bytes1  # the state grew
            assert np.array_equal(first.view(np.uint32), po.cpu().numpy().view(np.uint32))
        plan.pose_globals(po.data_ptr(), gl.data_ptr())
        out = plan.solve_host(wl.pose[:8], wl.targets[:8])
        assert np.isfinite(out).all()
        plan.close()

    cycle()  # the runtime keeps what a kernel's first launch makes it load
    free0 = free_bytes(torch)
    for _ in range(CYCLES):
        cycle()
    assert free_bytes(torch) >= free0 - MARGIN


def test_plan_load_that_fails_after_its_uploads_leaks_nothing(mbik, wl):
    """A saved plan that pins 64-bit table addressing and state placement 2: mbik_plan_load uploads
    its D / CF / CD tables, then the launch layout refuses the combination."""
    import torch
    plan = Plan.from_workload(wl)
    plan.set_table_addressing(1)
    plan.set_locals_placement(2)
    data = plan.save()
    plan.close()
    free0 = free_bytes(torch)
    for _ in range(CYCLES):
        with pytest.raises(_lib.MbikError) as e:
            Plan.load(data)
        assert e.value.code == _lib.MBIK_EUNSUPPORTED and "need every setup table < 4 GiB" in str(e.value)
    assert free_bytes(torch) >= free0 - MARGIN


def test_mesh_cycles_give_the_mesh_back(mbik):
    """A shaped mesh of ~36 MB (131,072 vertices, 8 influences, normals, 8 shapes) on a 64-bone chain."""
    import torch
    dev = torch.device("cuda", 0)
    B, V, K, P = 64, 131072, 8, 8
    parents = [b - 1 for b in range(B)]
    rest = np.zeros((B, 12), np.float32)
    rest[:, [0, 4, 8]] = 1.0
    rest[:, 10] = 0.1 * np.arange(B)
    pos, nrm, idx, w = synthetic_mesh(parents, rest, V, K, seed=1)
    sp, sn = synthetic_shapes(pos, nrm, P, seed=2)
    skin = torch.from_numpy(rest[None]).to(dev)
    weights = torch.full((1, P), 0.25, dtype=torch.float32, device=dev)
    out_p = torch.empty((V, 3), dtype=torch.float32, device=dev)
    out_n = torch.empty_like(out_p)

    def cycle():
        mesh = Mesh(B, pos, idx, w, normals=nrm, shape_positions=sp, shape_normals=sn)
        mesh.skin(skin.data_ptr(), out_p.data_ptr(), 1, out_normals_ptr=out_n.data_ptr(), shape_weights_ptr=weights.data_ptr())
        torch.cuda.synchronize()
        mesh.close()

    cycle()  # the runtime keeps what a kernel's first launch makes it load
    free0 = free_bytes(torch)
    for _ in range(CYCLES):
        cycle()
    assert free_bytes(torch) >= free0 - MARGIN
    assert np.isfinite(out_p.cpu().numpy()).all()
