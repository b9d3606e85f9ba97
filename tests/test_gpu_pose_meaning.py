"""The device entries of the four pose stages around the solve -- mbik_clip_sample, mbik_pose_blend,
mbik_pose_globals, mbik_capture_targets -- judged directly against the float64 models of
tests/pose_models_f64.py, with the bounds, the measured tolerances and the conditions of
tests/test_pose_meaning_cpu.py (its docstring states them): not through the _cpu entries, which the
other GPU tests compare bitwise.  One launch per stage and case, a few thousand bones each, the last
block partly filled.  Needs an MI355X: -m gpu."""
import math

import numpy as np
import pytest

from many_bone_ik_amd import animation as A
from many_bone_ik_amd import workloads as W
from many_bone_ik_amd.solver import Plan

from . import blend_recipe as BR
from . import pose_globals_recipe as GR
from . import pose_models_f64 as M
from . import test_pose_meaning_cpu as C
from .test_gpu_clip_sample import device_sample
from .test_gpu_parity import torch_dev  # noqa: F401 (fixture)
from .test_gpu_pose_blend import device_blend, plans as blend_plans  # noqa: F401 (fixture)
from .test_gpu_pose_globals import run_device

pytestmark = pytest.mark.gpu

SHAPES = [(33, 20), (7, 150)]   # (bones, skeletons): 660 and 1,050 bones, ending inside a 256-bone block


@pytest.mark.parametrize("libm_variant", [0, 1], ids=["fma", "sse2"])
@pytest.mark.parametrize("B,n", SHAPES, ids=[f"{b}x{n}" for b, n in SHAPES])
def test_blend_on_the_device(blend_plans, torch_dev, B, n, libm_variant):   # noqa: F811
    """Every kind of BR.mixed_inputs in every skeleton's bones, one weight per skeleton: the weights
    of the CPU test, 0.5, 1 and uniform ones."""
    torch, dev = torch_dev
    a, m, kind = BR.mixed_inputs(40 + B, n * B)
    rng = np.random.default_rng(B)
    w = np.array(C.BLEND_WEIGHTS + (0.5, 1.0), np.float32)[rng.integers(0, len(C.BLEND_WEIGHTS) + 2, n)]
    pick = rng.uniform(0.0, 1.0, n) < 0.4
    w[pick] = rng.uniform(0.0, 1.0, pick.sum()).astype(np.float32)
    got = device_blend(torch, dev, blend_plans(B, libm_variant), a.reshape(n, B, 10), m.reshape(n, B, 10), w).reshape(-1, 10)
    assert np.isfinite(got).all()
    model = M.blend_f64(a, m, np.repeat(w, B))
    early, judged = model["early"], M.blend_judged(model)
    assert BR.same_bits(got[early], m[early])
    err = M.blend_transform_error(got, model)
    live = ~early
    origin = np.abs(got[live, 4:7].astype(np.float64) - model["origin"][live]) / model["origin_bound"][live]
    print(f"blend {B}x{n}: worst transform error {err[judged].max():.3e} over {judged.sum()} bones (bound {C.BLEND_BOUND:.3e}); "
          f"worst origin error over its bound {origin.max():.3f}; left out {(live & ~judged).sum()} of {live.sum()}")
    assert (err[judged] <= C.BLEND_BOUND).all() and origin.max() <= 1.0
    assert judged.sum() >= 0.8 * live.sum() and early.sum() >= n * B // 5 and live.sum() >= n * B // 2


@pytest.mark.parametrize("libm_variant", [0, 1], ids=["fma", "sse2"])
@pytest.mark.parametrize("B,n", SHAPES, ids=[f"{b}x{n}" for b, n in SHAPES])
def test_clip_sample_on_the_device(mbik, torch_dev, B, n, libm_variant):
    """C.meaning_clips for this bone count; every skeleton at its own time in its own clip, drawn from
    C.meaning_times (on keys, outside the clip, lengths away)."""
    torch, dev = torch_dev
    rest, clips = C.meaning_clips(80 + B, B)
    t, ci = C.meaning_times(81 + B, clips)
    rng = np.random.default_rng(B)
    order = [rng.permutation(np.nonzero(ci == k)[0]) for k in range(len(clips))]
    pick = np.array([order[j % len(clips)][j // len(clips)] for j in range(n)])   # the clips in turn, distinct times of each
    t, ci = t[pick], ci[pick]
    with A.ClipSet(B, rest, clips, libm_variant=libm_variant) as cs:
        got = device_sample(torch, dev, cs, B, t, ci)
    assert np.isfinite(got).all()
    model = M.clip_sample_f64(B, rest, clips, t, ci)
    mismatches, ratio, angles, left_out = C.clip_figures(got, model)
    print(f"clip {B}x{n}: {model['interp'].sum()} interpolated channels; worst lerp error over its bound {ratio:.3f}; "
          f"worst rotation angle {angles.max():.3e} rad over {angles.size} (bound {C.CLIP_ANGLE_BOUND:.3e}); left out {left_out:.2%}")
    assert mismatches == 0 and ratio <= 1.0
    assert (angles <= C.CLIP_ANGLE_BOUND).all()
    assert left_out <= C.LEFT_OUT_TOTAL and angles.size >= 100 and (model["on_key"] & ~model["interp"]).sum() >= 20


GLOBALS_RIGS = {"c2x67": (W.topology(2).parents.tolist(), W.topology(2).pins.tolist(), 67),
                "star400x3": (C.STAR400, [1], 3)}


@pytest.fixture(scope="module")
def globals_plans(mbik):
    made = {}

    def get(name):
        if name not in made:
            parents, pins, _ = GLOBALS_RIGS[name]
            topo = W.topology(2) if name == "c2x67" else W.custom_topology(parents, pins)
            made[name] = Plan.from_workload(W.generate(9, 2, topo=topo))
        return made[name]

    yield get
    for p in made.values():
        p.close()


@pytest.mark.parametrize("skin", [False, True], ids=["plain", "inv_bind"])
@pytest.mark.parametrize("name", list(GLOBALS_RIGS))
def test_globals_on_the_device(globals_plans, torch_dev, name, skin):
    torch, dev = torch_dev
    parents, pins, n = GLOBALS_RIGS[name]
    pose, inv_bind, targets = GR.random_inputs(900 + len(parents), n, len(parents), len(pins))
    g, d = run_device(torch, dev, globals_plans(name), pose, inv_bind if skin else None, targets, True, True)
    assert np.isfinite(g).all() and np.isfinite(d).all()
    model = M.globals_f64(parents, pins, pose, inv_bind if skin else None, targets)
    key = "skin" if skin else "globals"
    rg = np.abs(g.astype(np.float64) - model[key]) / np.maximum(model[key + "_bound"], 1e-300)
    rd = np.abs(d.astype(np.float64) - model["dist"]) / model["dist_bound"]
    print(f"globals {name} {key}: worst error over its bound {rg.max():.3f}, distances {rd.max():.3f}")
    assert rg.max() <= 1.0 and rd.max() <= 1.0


def test_capture_on_the_device(mbik, torch_dev):
    """83 skeletons of C2's four pins, a fifth of the entries hidden: those keep the previous target's bits."""
    torch, dev = torch_dev
    wl = W.generate(2, 83)
    P = wl.targets.shape[1]
    skel, node = C.capture_inputs(17, 83, P)
    rng = np.random.default_rng(18)
    visible = (rng.random((83, P)) < 0.8).astype(np.uint8)
    prev = rng.uniform(-3.0, 3.0, (83, P, 12)).astype(np.float32)
    plan = Plan.from_workload(wl)
    d_skel, d_node = torch.from_numpy(skel).to(dev), torch.from_numpy(node).to(dev)
    d_vis, d_tg = torch.from_numpy(visible).to(dev), torch.from_numpy(prev.copy()).to(dev)
    plan.capture_targets(d_skel.data_ptr(), d_node.data_ptr(), d_tg.data_ptr(), d_vis.data_ptr())
    torch.cuda.synchronize()
    got = d_tg.cpu().numpy()
    plan.close()
    hidden = visible == 0
    assert 30 <= hidden.sum() <= 110 and BR.same_bits(got[hidden], prev[hidden])
    ratios = C.capture_ratios(got, skel, node)
    print(f"capture: worst error over its bound {ratios[~hidden].max():.3f} over {(~hidden).sum()} targets")
    assert (ratios[~hidden] <= 1.0).all()
    assert math.isfinite(ratios[~hidden].max())
