"""mbik_pose_globals_cpu (Skeleton3D::get_bone_global_pose for every bone, skin transforms, pin
distances; host only) against the oracle-primitive recipe of tests/pose_globals_recipe.py, bitwise:
C2, rigs with unsorted parents / several roots / a pinned root, and a 300-bone chain."""
import os
import subprocess

import numpy as np
import pytest

from many_bone_ik_amd import _lib
from many_bone_ik_amd import workloads as W
from many_bone_ik_amd.ik import ManyBoneIK3D
from many_bone_ik_amd.solver import pose_globals_cpu

from . import pose_globals_recipe as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _rigs():
    t = W.topology(2)
    yield "c2", t.parents.tolist(), t.pins.tolist(), 8, 0.4
    for name, (parents, pins) in R.EDGE_RIGS.items():
        yield name, parents, pins, 3, 0.4
    yield "chain300", R.CHAIN300, [299], 2, 0.1   # (300 levels: scales near 1 keep the products finite)


RIGS = {r[0]: r[1:] for r in _rigs()}


@pytest.fixture(scope="module")
def cases(oracle):
    """name -> (parents, pins, pose, inv_bind, targets, expected globals, skinned, distances), computed once."""
    out = {}
    for i, (name, (parents, pins, n, spread)) in enumerate(RIGS.items()):
        pose, inv_bind, targets = R.random_inputs(100 + i, n, len(parents), len(pins), spread)
        out[name] = (parents, pins, pose, inv_bind, targets) + R.expected(oracle, parents, pins, pose, inv_bind, targets)
    return out


@pytest.mark.parametrize("skin", [False, True], ids=["plain", "inv_bind"])
@pytest.mark.parametrize("outputs", ["globals", "distances", "both"])
@pytest.mark.parametrize("name", list(RIGS))
def test_cpu_matches_recipe(mbik, cases, name, outputs, skin):
    parents, pins, pose, inv_bind, targets, G, S, D = cases[name]
    assert np.isfinite(G).all() and np.isfinite(S).all() and (pose[..., 7:10] < 0).any()
    rc, g, d = R.pose_globals_cpu_raw(parents, pins, pose, inv_bind if skin else None, targets,
                                      want_globals=outputs != "distances", want_dist=outputs != "globals")
    assert rc == _lib.MBIK_OK, _lib.last_error()
    if g is not None:
        assert R.same_bits(g, S if skin else G)
    if d is not None:
        assert R.same_bits(d, D)   # always the unskinned global's origin


def test_python_wrappers(mbik, cases):
    parents, pins, pose, inv_bind, targets, G, S, D = cases["unsorted_parents"]
    g, d = pose_globals_cpu(parents, pins, pose, targets=targets)
    assert R.same_bits(g, G) and R.same_bits(d, D)
    g, d = pose_globals_cpu(parents, pins, pose, inv_bind=inv_bind)
    assert R.same_bits(g, S) and d is None
    ik = ManyBoneIK3D(parents)
    assert R.same_bits(ik.bone_global_poses(pose), G)
    assert R.same_bits(ik.bone_global_poses(pose, inv_bind), S)


def test_argument_errors(mbik, cases):
    parents, pins, pose, inv_bind, targets, G, S, D = cases["pinned_root"]
    L = _lib.load()
    d = R.desc_of(parents, pins)
    n, B = pose.shape[:2]
    g = np.zeros((n, B, 12), np.float32)
    dist = np.zeros((n, len(pins)), np.float32)
    import ctypes as C
    call = lambda desc, count, p, gl, tg, di: L.mbik_pose_globals_cpu(desc, count, R.ptr(p), None, R.ptr(gl), R.ptr(tg), R.ptr(di))
    assert call(C.byref(d.desc), n, pose, None, targets, None) == _lib.MBIK_EINVAL      # no output
    assert call(C.byref(d.desc), n, pose, g, None, dist) == _lib.MBIK_EINVAL            # distances without targets
    assert call(C.byref(d.desc), n, None, g, targets, dist) == _lib.MBIK_EINVAL         # no pose
    assert call(C.byref(d.desc), -1, pose, g, targets, dist) == _lib.MBIK_EINVAL        # negative count
    assert call(None, n, pose, g, targets, dist) == _lib.MBIK_EINVAL                    # no rig
    # pose overlapping globals: one buffer holding both, the globals starting inside the poses
    buf = np.zeros(n * B * 22, np.float32)
    buf[: n * B * 10] = pose.reshape(-1)
    assert L.mbik_pose_globals_cpu(C.byref(d.desc), n, R.ptr(buf), None, R.ptr(buf[n * B * 10 - 4:]), None, None) == _lib.MBIK_EINVAL
    assert L.mbik_pose_globals_cpu(C.byref(d.desc), n, R.ptr(buf), None, R.ptr(buf[n * B * 10:]), None, None) == _lib.MBIK_OK
    assert R.same_bits(buf[n * B * 10:].reshape(n, B, 12), G)
    # invalid rigs
    for bad_parents, bad_pins in (([0, 0], []), ([-1, 7], []), ([-1, 0], [5])):
        rc, _, _ = R.pose_globals_cpu_raw(bad_parents, bad_pins, np.zeros((1, 2, 10), np.float32), None,
                                          np.zeros((1, len(bad_pins), 12), np.float32))
        assert rc == _lib.MBIK_EINVAL
    # count == 0 and a pinless rig asked for distances
    assert call(C.byref(d.desc), 0, None, None, None, None) == _lib.MBIK_OK
    rc, g0, _ = R.pose_globals_cpu_raw(parents, [], pose, None, None, want_globals=True, want_dist=True)
    assert rc == _lib.MBIK_OK and R.same_bits(g0, G)


def test_fk_san_runs_clean():
    """tools/san/fk_san: fk.h's schedule builder and host core under ASan + UBSan (a stand-alone program)."""
    exe = os.path.join(ROOT, "build", "san", "fk_san")
    subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "tools", "san"), exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "chain300: ok B=300 levels=300" in r.stdout and "cycle: refused (-2)" in r.stdout
    assert "ERROR" not in r.stderr and "runtime error" not in r.stderr
