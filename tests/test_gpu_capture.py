"""mbik_capture_targets (IKEffector3D::update_target_global_transform, ik_effector_3d.cpp:77-84)
on the GPU vs the oracle's Transform3D affine_inverse and product (pinned by the reference's
test_ik_node_3d.h cases, tests/test_oracle_kats.py), bitwise; hidden target nodes keep the
previous target."""
import numpy as np
import pytest

from many_bone_ik_amd import workloads as W
from many_bone_ik_amd.solver import Plan

from .test_gpu_parity import assert_parity, torch_dev  # noqa: F401 (fixture)

pytestmark = pytest.mark.gpu


def random_xforms(rng, shape, scale=True):
    q = rng.normal(size=shape + (4,))
    q /= np.linalg.norm(q, axis=-1, keepdims=True)
    x, y, z, w = q[..., 0], q[..., 1], q[..., 2], q[..., 3]
    R = np.stack([1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w),
                  2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w),
                  2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)], -1).reshape(shape + (3, 3))
    if scale:
        R = R * rng.uniform(0.5, 2.0, shape + (1, 3))
    o = rng.uniform(-10, 10, shape + (3,))
    return np.concatenate([R.reshape(shape + (9,)), o], -1).astype(np.float32)


def test_capture_matches_oracle(oracle, mbik, torch_dev):
    torch, dev = torch_dev
    rng = np.random.default_rng(7)
    wl = W.generate(2, 64)
    plan = Plan.from_workload(wl)
    n, P = wl.n, wl.targets.shape[1]
    skel = random_xforms(rng, (n,))
    node = random_xforms(rng, (n, P))
    visible = (rng.random((n, P)) < 0.8).astype(np.uint8)
    prev = random_xforms(rng, (n, P), scale=False)
    d_skel, d_node = torch.from_numpy(skel).to(dev), torch.from_numpy(node).to(dev)
    d_vis, d_tg = torch.from_numpy(visible).to(dev), torch.from_numpy(prev.copy()).to(dev)
    plan.capture_targets(d_skel.data_ptr(), d_node.data_ptr(), d_tg.data_ptr(), d_vis.data_ptr())
    torch.cuda.synchronize()
    got = d_tg.cpu().numpy()
    for s in range(n):
        inv = oracle.xform_affine_inverse(skel[s])
        for e in range(P):
            want = oracle.xform_mul(inv, node[s, e]) if visible[s, e] else prev[s, e]
            assert np.array_equal(got[s, e].view(np.uint32), want.view(np.uint32)), (s, e)


def test_capture_subrange_keeps_everything_else(oracle, mbik, torch_dev):
    """Range [15, 33) of 83 skeletons, every buffer indexed from skeleton 15 and carrying 64 guard
    rows on each side: hidden pins sit inside the range and at both of its ends; rows outside the
    range and hidden entries keep their previous bits; skeleton_global and target_global are NaN
    outside the range, so a read from a wrong row cannot give the oracle's bits."""
    torch, dev = torch_dev
    rng = np.random.default_rng(9)
    n, a, c, G = 83, 15, 18, 64
    wl = W.generate(2, n)
    plan = Plan.from_workload(wl)
    P = wl.targets.shape[1]
    rows, lo, hi = G + n + G, G + a, G + a + c
    skel = np.full((rows, 12), np.nan, np.float32)
    node = np.full((rows, P, 12), np.nan, np.float32)
    skel[lo:hi] = random_xforms(rng, (c,))
    node[lo:hi] = random_xforms(rng, (c, P))
    visible = np.ones((rows, P), np.uint8)          # (a wrongly captured row outside the range would turn NaN)
    hidden = [(a, 0), (a, P - 1), (a + 7, 1), (a + c - 1, 0), (a + c - 1, P - 1)]
    for s, e in hidden:
        visible[G + s, e] = 0
    prev = random_xforms(rng, (rows, P), scale=False)
    d_skel, d_node = torch.from_numpy(skel).to(dev), torch.from_numpy(node).to(dev)
    d_vis, d_tg = torch.from_numpy(visible).to(dev), torch.from_numpy(prev.copy()).to(dev)
    plan.capture_targets(d_skel[lo].data_ptr(), d_node[lo].data_ptr(), d_tg[lo].data_ptr(), d_vis[lo].data_ptr(), first=a, count=c)
    torch.cuda.synchronize()
    got = d_tg.cpu().numpy()
    want = prev.copy()
    for s in range(lo, hi):
        inv = oracle.xform_affine_inverse(skel[s])
        for e in range(P):
            if visible[s, e]:
                want[s, e] = oracle.xform_mul(inv, node[s, e])
    assert not np.isnan(want).any()
    diff = np.argwhere(got.view(np.uint32) != want.view(np.uint32))
    assert diff.size == 0, f"{len(diff)} values differ; first (row - {G}, pin, float) {(diff[:5] - [G, 0, 0]).tolist()}"
    for t, h in ((d_skel, skel), (d_node, node)):
        assert np.array_equal(t.cpu().numpy().view(np.uint32), h.view(np.uint32))
    assert np.array_equal(d_vis.cpu().numpy(), visible)


def test_capture_then_solve(oracle, mbik, torch_dev):
    """Scene-space targets -> capture -> solve == the oracle solving the captured targets."""
    torch, dev = torch_dev
    rng = np.random.default_rng(8)
    wl = W.generate(2, 32)
    plan = Plan.from_workload(wl)
    skel = random_xforms(rng, (wl.n,), scale=False)
    # scene-space target nodes placed where the synthetic skeleton-space targets are
    node = np.stack([np.stack([oracle.xform_mul(skel[s], wl.targets[s, e]) for e in range(wl.targets.shape[1])])
                     for s in range(wl.n)])
    d_skel, d_node = torch.from_numpy(skel).to(dev), torch.from_numpy(node).to(dev)
    d_tg = torch.zeros(wl.targets.shape, dtype=torch.float32, device=dev)
    plan.capture_targets(d_skel.data_ptr(), d_node.data_ptr(), d_tg.data_ptr())
    pi = torch.from_numpy(wl.pose).to(dev)
    po = torch.empty_like(pi)
    plan.solve(pi.data_ptr(), d_tg.data_ptr(), po.data_ptr())
    torch.cuda.synchronize()
    captured = d_tg.cpu().numpy()
    ref = oracle.Oracle(wl).solve(wl.pose, captured)
    assert_parity(po.cpu().numpy(), ref, "capture + solve")
