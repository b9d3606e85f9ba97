"""mbik_pose_globals at the edges of its launch shape (k_fk.hip, host_fk.cpp), bitwise against
mbik_pose_globals_cpu and within the float64 bound of tests/pose_models_f64.py, sentinels in front
of and behind every output:

    a  745-bone chain x 3       the first rig whose block needs more than 64 KiB of dynamic LDS
    b  1861-bone chain x 3      MBIK_FK_MAX_BONES, the largest block (the whole 160 KiB but 68 bytes)
    c  root + 1860 children x 3 one level wider than the 256-thread block with one skeleton a block
    d  1862 bones               the device entry refuses (MBIK_EUNSUPPORTED), the host entry computes
    e  3 bones x 64, 65, 130    64 skeletons a block, the cap; tails of 1 and 2 skeletons
    f  4 bones x 115            57 skeletons a block by the LDS target; a tail of 1
    g  C2 x 67                  pose 1, 2, 3 floats past a 16-byte boundary with globals aligned, and the reverse

Every plan has one pin, on a child of the root, so that the solve's own limits stay out of the way:
mbik_pose_globals reads only the rig.  Poses are rotations with unit scales, so a depth of 1861 stays
finite.  Needs an MI355X: -m gpu."""
import numpy as np
import pytest

from many_bone_ik_amd import _lib
from many_bone_ik_amd import workloads as W
from many_bone_ik_amd.solver import Plan

from . import pose_globals_recipe as R
from . import pose_models_f64 as M
from .test_gpu_parity import torch_dev  # noqa: F401 (fixture)

pytestmark = pytest.mark.gpu

SENTINEL = -12345.678
PAD = 16
FK_MAX_BONES = 1861          # MBIK_FK_MAX_BONES (include/mbik.h)
LDS_TARGET, S_CAP = 20 * 1024, 64   # host_fk.cpp: the LDS a block aims for, the most skeletons it takes


def chain(B):
    return [b - 1 for b in range(B)]


def star(B):
    return [-1] + [0] * (B - 1)


def skeletons_per_block(B, count):
    """host_fk.cpp's S, restated: 22 B + 1 floats of LDS a skeleton."""
    return max(1, min(LDS_TARGET // ((B * 22 + 1) * 4), S_CAP, count))


def rig_inputs(seed, n, B):
    """Rotations (non-unit quaternions), positions within 1, unit scales; arbitrary inverse binds and
    one target a skeleton."""
    rng = np.random.default_rng(seed)
    pose = np.empty((n, B, 10), np.float32)
    pose[..., 0:4] = rng.normal(0.0, 1.0, (n, B, 4)) * rng.uniform(0.5, 1.5, (n, B, 1))
    pose[..., 4:7] = rng.uniform(-1.0, 1.0, (n, B, 3))
    pose[..., 7:10] = 1.0
    return pose, rng.uniform(-1.0, 1.0, (B, 12)).astype(np.float32), rng.uniform(-2.0, 2.0, (n, 1, 12)).astype(np.float32)


@pytest.fixture(scope="module")
def plans(mbik):
    """One two-skeleton plan per rig, pinned on bone 1."""
    made = {}

    def get(name, parents):
        if name not in made:
            made[name] = Plan.from_workload(W.generate(9, 2, topo=W.custom_topology(parents, [1])))
        return made[name]

    yield get
    for p in made.values():
        p.close()


def launch(torch, dev, plan, pose, inv_bind, targets, pose_off=0, globals_off=0):
    """mbik_pose_globals on device copies, pose and globals that many floats past a 16-byte boundary;
    PAD sentinels behind the globals and the distances and PAD + the offset in front of them.
    Returns (globals, distances)."""
    n, B, _ = pose.shape
    P = targets.shape[1]
    d_pose = torch.zeros(pose.size + pose_off, dtype=torch.float32, device=dev)
    d_pose[pose_off:] = torch.from_numpy(pose.reshape(-1)).to(dev)
    d_ib = None if inv_bind is None else torch.from_numpy(inv_bind).to(dev)
    d_tg = torch.from_numpy(targets).to(dev)
    g0 = PAD + globals_off
    d_g = torch.full((g0 + n * B * 12 + PAD,), SENTINEL, dtype=torch.float32, device=dev)
    d_d = torch.full((PAD + n * P + PAD,), SENTINEL, dtype=torch.float32, device=dev)
    assert d_pose.data_ptr() % 16 == 0 and d_g.data_ptr() % 16 == 0
    torch.cuda.synchronize()
    plan.pose_globals(d_pose[pose_off:].data_ptr(), d_g[g0:].data_ptr(), n, inv_bind_ptr=0 if d_ib is None else d_ib.data_ptr(),
                      targets_ptr=d_tg.data_ptr(), pin_distance_ptr=d_d[PAD:].data_ptr())
    torch.cuda.synchronize()
    hg, hd = d_g.cpu().numpy(), d_d.cpu().numpy()
    s = np.float32(SENTINEL)
    assert (hg[:g0] == s).all() and (hg[g0 + n * B * 12:] == s).all(), "written outside the globals"
    assert (hd[:PAD] == s).all() and (hd[PAD + n * P:] == s).all(), "written outside the distances"
    assert R.same_bits(d_pose[pose_off:].cpu().numpy(), pose.reshape(-1)), "pose written"
    return hg[g0:g0 + n * B * 12].reshape(n, B, 12), hd[PAD:PAD + n * P].reshape(n, P)


def check(torch, dev, plan, parents, pose, inv_bind, targets, model_skeletons=None, **offsets):
    """The device's globals (plain and skinned) and distances equal the host entry's bits; the first
    model_skeletons skeletons (all by default) also lie within the float64 bound."""
    n = pose.shape[0] if model_skeletons is None else model_skeletons
    model = M.globals_f64(parents, [1], pose[:n], inv_bind, targets[:n]) if n else None
    worst = []
    for ib, key in ((None, "globals"), (inv_bind, "skin")):
        rc, G, D = R.pose_globals_cpu_raw(parents, [1], pose, ib, targets)
        assert rc == _lib.MBIK_OK and np.isfinite(G).all()
        g, d = launch(torch, dev, plan, pose, ib, targets, **offsets)
        assert R.same_bits(g, G) and R.same_bits(d, D), key
        if n:
            rg = np.abs(g[:n].astype(np.float64) - model[key]) / np.maximum(model[key + "_bound"], 1e-300)
            rd = np.abs(d[:n].astype(np.float64) - model["dist"]) / model["dist_bound"]
            assert rg.max() <= 1.0 and rd.max() <= 1.0, key
            worst.append(max(rg.max(), rd.max()))
    return worst


@pytest.mark.parametrize("name,parents,lds", [("a_chain745", chain(745), 65564), ("b_chain1861", chain(FK_MAX_BONES), 163772),
                                              ("c_star1861", star(FK_MAX_BONES), 163772)], ids=["a_chain745", "b_chain1861", "c_star1861"])
def test_blocks_beyond_64_kib(plans, torch_dev, name, parents, lds):
    torch, dev = torch_dev
    B = len(parents)
    assert (B * 22 + 1) * 4 == lds and 65536 < lds <= 160 * 1024
    assert ((B - 1) * 22 + 1) * 4 <= 65536 if B == 745 else ((B + 1) * 22 + 1) * 4 > 160 * 1024
    assert skeletons_per_block(B, 3) == 1
    pose, inv_bind, targets = rig_inputs(B, 3, B)
    worst = check(torch, dev, plans(name, parents), parents, pose, inv_bind, targets)
    print(f"{name}: {lds} bytes of LDS a block; worst error over the float64 bound {max(worst):.3f}")


def test_one_bone_too_many_is_refused_on_the_device_only(plans, torch_dev):
    torch, dev = torch_dev
    B = FK_MAX_BONES + 1
    parents = chain(B)
    pose, inv_bind, targets = rig_inputs(B, 1, B)
    rc, G, D = R.pose_globals_cpu_raw(parents, [1], pose, None, targets)
    assert rc == _lib.MBIK_OK and np.isfinite(G).all() and np.isfinite(D).all()
    with pytest.raises(_lib.MbikError) as e:
        launch(torch, dev, plans("d_chain1862", parents), pose, None, targets)
    assert e.value.code == _lib.MBIK_EUNSUPPORTED and "MBIK_FK_MAX_BONES" in _lib.last_error()


@pytest.mark.parametrize("B,count,S,tail", [(3, 64, 64, 0), (3, 65, 64, 1), (3, 130, 64, 2), (4, 115, 57, 1)],
                         ids=["e_3x64", "e_3x65", "e_3x130", "f_4x115"])
def test_skeletons_per_block_cap_and_tails(plans, torch_dev, B, count, S, tail):
    torch, dev = torch_dev
    assert skeletons_per_block(B, count) == S and count % S == tail
    parents = chain(B)
    pose, inv_bind, targets = rig_inputs(10 * B + count, count, B)
    worst = check(torch, dev, plans(f"chain{B}", parents), parents, pose, inv_bind, targets)
    print(f"{B} bones x {count}: {S} skeletons a block, tail {tail}; worst error over the float64 bound {max(worst):.3f}")


@pytest.mark.parametrize("pose_off,globals_off", [(1, 0), (2, 0), (3, 0), (0, 1), (0, 2), (0, 3)], ids=str)
def test_pose_and_globals_shifted_independently(mbik, torch_dev, pose_off, globals_off):
    """C2 x 67 (7 skeletons a block): a block's poses are one run whose head and tail are dwords,
    its globals one run a skeleton, each with the head of the first."""
    torch, dev = torch_dev
    t = W.topology(2)
    parents = t.parents.tolist()
    assert skeletons_per_block(len(parents), 67) == 7 and parents[1] == 0
    pose, inv_bind, targets = rig_inputs(67, 67, len(parents))
    plan = Plan.from_workload(W.generate(9, 2, topo=W.custom_topology(parents, [1])))
    try:
        worst = check(torch, dev, plan, parents, pose, inv_bind, targets, model_skeletons=8, pose_off=pose_off, globals_off=globals_off)
    finally:
        plan.close()
    print(f"pose + {pose_off}, globals + {globals_off}: worst error over the float64 bound {max(worst):.3f}")
