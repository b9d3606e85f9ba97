"""The device code against independent float64 geometry: the generators, figures and limits of
tests/test_geometry_cpu.py (models in tests/geometry_f64.py) applied to what the kernels' own
device functions return through mbik_selftest_qcp, mbik_selftest_point_in_limits (on setup
tables built by the host and rebuilt on the device) and mbik_selftest_xform.  Every result must
also equal the oracle's bit for bit: a case that fails only that is a parity bug, a case that
fails both points at the shared restatement of the reference.  Needs an MI355X: -m gpu."""
import ctypes as C
import math

import numpy as np
import pytest

from many_bone_ik_amd import _lib
from many_bone_ik_amd.solver import Plan

from . import geometry_f64 as G
from . import test_geometry_cpu as T
from .test_geometry_cpu import lattice  # noqa: F401 (fixture)
from .test_gpu_kats import FP, _f, dev_qcp, dev_xform
from .test_gpu_parity import torch_dev  # noqa: F401 (fixture)

pytestmark = pytest.mark.gpu

CHAINS = 4   # per cone count, and as many again for the rebuild with other chains
POINTS = 40  # per chain


def same_bits(a, b):
    return np.array_equal(np.asarray(a, np.float32).view(np.uint32), np.asarray(b, np.float32).view(np.uint32))


@pytest.mark.parametrize("translate", [False, True], ids=["fixed", "translate"])
@pytest.mark.parametrize("n,zero_third", T.QCP_CLASSES, ids=lambda v: f"n{v}" if not isinstance(v, bool) else ("zeros" if v else "dense"))
def test_device_qcp_exact_fit_is_the_kabsch_rotation(oracle, mbik, n, zero_third, translate):
    figs, parity = [], []
    for i, case in enumerate(T.qcp_cases(n, zero_third, translate, 40)):
        rot, trans = dev_qcp(case["moved"], case["target"], case["w"], translate, T.QCP_PRECISION)
        figs.append(T.qcp_figures(case, rot, trans))
        o_rot, o_trans = oracle.qcp(case["moved"], case["target"], case["w"], translate, T.QCP_PRECISION)
        if not (same_bits(rot, o_rot) and same_bits(trans, o_trans)):
            parity.append(i)
    w = T.worst(figs)
    print(f"device qcp n={n} zeros={zero_third} translate={translate}: " + " ".join(f"{k}={v:.3g}" for k, v in w.items()))
    assert not T.qcp_failures(w), w
    assert not parity, f"cases {parity} differ from the oracle's bits"


def swing_plan(chain_list):
    """A two-bone rig whose child carries one constraint (slot 0), one skeleton per cone chain."""
    cones = np.stack(chain_list).astype(np.float32)[:, None]          # [n][1][k][4]
    n, k = cones.shape[0], cones.shape[2]
    pose = np.zeros((n, 2, 10), np.float32)
    pose[:, :, 3] = 1.0
    pose[:, :, 7:10] = 1.0
    pose[:, 1, 5] = 1.0
    pins = [dict(bone=1, weight=1.0, direction_priorities=(0.2, 0.0, 0.2), motion_propagation_factor=1.0)]
    twist = np.tile(np.array([0.0, 2 * math.pi], np.float32), (n, 1, 1))
    return Plan([-1, 0], pins, [dict(bone=1, cone_count=k)], pose, cones, twist, max_cones=k), pose, cones, twist


def dev_limits(plan, skeleton, point):
    L = _lib.load()
    out = np.zeros(6, np.float32)
    ib = np.zeros(2, np.float64)
    _lib.check(L.mbik_selftest_point_in_limits(plan.h, 0, skeleton, _f(point).ctypes.data_as(FP), out.ctypes.data_as(FP),
                                               ib.ctypes.data_as(C.POINTER(C.c_double))))
    assert same_bits(out[:3], out[3:]) and ib[0] == ib[1], "plain and select-form builds differ"
    return out[:3].copy(), ib[0]


def check_swing(plan, chain_list, oracle, lattice, what):
    """Assertions (a)-(e) of the plan's skeletons against their chains' float64 regions, and bit
    equality with the oracle.  Returns every (result, in_bounds), in order."""
    figs, parity, got = [], [], []
    for s, cones in enumerate(chain_list):
        seen = []

        def query(p):
            seen.append(dev_limits(plan, s, p))
            return seen[-1]

        points = T.query_points(cones, POINTS)
        figs.append(T.swing_figures(cones, points, query, lattice))
        for i, (p, (out, ib)) in enumerate(zip(points, seen)):
            o_out, o_ib = oracle.local_point_in_limits(cones, p)
            if not (same_bits(out, o_out) and ib == o_ib):
                parity.append((s, i))
        got += seen
    t = T.swing_total(figs)
    print(f"device swing, {what}: left out {t['left_out']}/{t['points']} " +
          " ".join(f"{k}={v:.3g}" for k, v in t.items() if k not in ("points", "left_out")))
    assert not T.swing_failures(t), (what, t)
    assert not parity, f"{what}: (skeleton, point) {parity} differ from the oracle's bits"
    return got


@pytest.mark.parametrize("k", T.CONE_COUNTS)
def test_device_swing_limit_is_the_nearest_point_of_the_region(oracle, mbik, lattice, k):
    """The device reads the plan's setup tables, so this also checks the tangent circles that the
    host builder put there."""
    chain_list = T.chains(k, 2 * CHAINS)[:CHAINS]
    plan = swing_plan(chain_list)[0]
    check_swing(plan, chain_list, oracle, lattice, f"{k} cones, host-built setup")
    plan.close()


@pytest.mark.parametrize("k", T.CONE_COUNTS)
def test_device_built_setup_gives_the_same_region_and_follows_new_cones(oracle, mbik, torch_dev, lattice, k):
    """mbik_plan_rebuild_setup with the same inputs: the same bits for the same points.  With
    other cone chains: (a)-(e) against the new chains, which a stale table would miss."""
    torch, dev = torch_dev
    both = T.chains(k, 2 * CHAINS)
    first, second = both[:CHAINS], both[CHAINS:]
    plan, pose, cones, twist = swing_plan(first)
    before = check_swing(plan, first, oracle, lattice, f"{k} cones, before the rebuild")
    stream = torch.cuda.current_stream().cuda_stream
    d_pose, d_twist = torch.from_numpy(pose).to(dev), torch.from_numpy(twist).to(dev)
    d_cones = torch.from_numpy(cones).to(dev)
    plan.rebuild_setup(d_pose.data_ptr(), d_cones.data_ptr(), d_twist.data_ptr(), stream=stream)
    torch.cuda.synchronize()
    after = [dev_limits(plan, s, p) for s, c in enumerate(first) for p in T.query_points(c, POINTS)]
    assert len(after) == len(before)
    assert all(same_bits(a[0], b[0]) and a[1] == b[1] for a, b in zip(after, before)), "device-built setup changes results"
    d_cones2 = torch.from_numpy(np.stack(second).astype(np.float32)[:, None].copy()).to(dev)
    plan.rebuild_setup(d_pose.data_ptr(), d_cones2.data_ptr(), d_twist.data_ptr(), stream=stream)
    torch.cuda.synchronize()
    check_swing(plan, second, oracle, lattice, f"{k} cones, rebuilt from other chains")
    plan.close()


def test_device_transform_ops_within_rounding_bounds_of_float64(oracle, mbik):
    rm = ri = 0.0
    for a, b in T.xform_cases():
        mul, inv = dev_xform(0, a, b), dev_xform(1, a)
        m, i = T.xform_ratios(a, b, mul, inv)
        rm, ri = max(rm, m), max(ri, i)
        assert same_bits(mul, oracle.xform_mul(a, b)) and same_bits(inv, oracle.xform_affine_inverse(a))
    print(f"device transform: worst error / bound: product {rm:.3f}, affine inverse {ri:.3f}")
    assert rm <= 1.0 and ri <= 1.0
