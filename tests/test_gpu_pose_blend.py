"""mbik_pose_blend on the GPU (the modifier influence of Skeleton3D::_process_modifiers) against
mbik_pose_blend_cpu, bitwise: bone counts and batch sizes around the 256-bone block, blocks that
span dozens of skeletons with their own weights, float-aligned (odd) buffers, 64 guard skeletons
around every buffer, in place on either input, waves with partial early-outs, both libm variants,
2^20 bones, non-finite poses, and stream order between a solve and mbik_pose_globals."""
import numpy as np
import pytest

from many_bone_ik_amd import _lib
from many_bone_ik_amd import workloads as W
from many_bone_ik_amd.ik import ManyBoneIK3D
from many_bone_ik_amd.solver import Plan, pose_blend_cpu, pose_globals_cpu

from . import blend_recipe as R
from .test_gpu_parity import torch_dev  # noqa: F401 (fixture)

pytestmark = pytest.mark.gpu

SENTINEL = np.uint32(0x4B1D4B1D).view(np.float32)   # a finite float no blend produces
GUARD = 64                                           # guard skeletons (and weights) on each side
GUARD_WEIGHT = np.float32(0.77)                      # a weight that would blend, were it read
BLOCK = 256                                          # bones a block (k_blend.hip)


@pytest.fixture(scope="module")
def plans(mbik):
    """One two-skeleton pinless chain plan per (bone count, libm_variant): mbik_pose_blend reads
    only the device, the bone count and the variant from it."""
    made = {}

    def get(B, libm_variant=0):
        if (B, libm_variant) not in made:
            topo = W.custom_topology([-1] + list(range(B - 1)), [], [])
            made[B, libm_variant] = Plan.from_workload(W.generate(9, 2, topo=topo), libm_variant=libm_variant)
        return made[B, libm_variant]

    yield get
    for p in made.values():
        p.close()


def inputs(seed, n, B):
    """Poses of every kind (R.KINDS cycles per bone, so every wave mixes early-outs with blends) and
    one weight per skeleton: the weights of interest and uniform ones, all distinct skeletons apart."""
    a, m, _ = R.mixed_inputs(seed, n * B)
    rng = np.random.default_rng(seed + 1)
    w = R.WEIGHTS[rng.integers(0, len(R.WEIGHTS), n)].copy()
    pick = rng.uniform(0.0, 1.0, n) < 0.5
    w[pick] = rng.uniform(0.0, 1.0, pick.sum()).astype(np.float32)
    return a.reshape(n, B, 10), m.reshape(n, B, 10), w


def device_blend(torch, dev, plan, a, m, w, offs=(0, 0, 0, 0), in_place=None, stream=0):
    """Launches on device copies and returns pose_out [n][B][10].  Every buffer starts `offs` floats
    (pose_in, pose_mod, pose_out, weights) past an allocation and has GUARD skeletons on each side:
    NaN around the inputs, SENTINEL around (and in) the output, GUARD_WEIGHT around the weights;
    all of them must come back untouched.  w: [n] per-skeleton weights, or a scalar.
    in_place: None, "in" or "mod" (pose_out is that input)."""
    n, B, _ = a.shape
    g, body = GUARD * B * 10, n * B * 10

    def padded(data, off, fill):
        h = np.full(off + g + body + g, fill, np.float32)
        if data is not None:
            h[off + g:off + g + body] = data.reshape(-1)
        return h

    h_a, h_m, h_o = padded(a, offs[0], np.nan), padded(m, offs[1], np.nan), padded(None, offs[2], SENTINEL)
    d_a, d_m, d_o = (torch.from_numpy(h).to(dev) for h in (h_a, h_m, h_o))
    p_a, p_m, p_o = (d[off + g:].data_ptr() for d, off in ((d_a, offs[0]), (d_m, offs[1]), (d_o, offs[2])))
    if in_place:
        p_o = p_a if in_place == "in" else p_m
    per = np.ndim(w) != 0
    d_w = None
    if per:
        h_w = np.full(offs[3] + GUARD + n + GUARD, GUARD_WEIGHT, np.float32)
        h_w[offs[3] + GUARD:offs[3] + GUARD + n] = w
        d_w = torch.from_numpy(h_w).to(dev)
    torch.cuda.synchronize()
    plan.pose_blend(p_a, p_m, p_o, n, influence=0.5 if per else float(w),
                    influence_ptr=d_w[offs[3] + GUARD:].data_ptr() if per else None, stream=stream)
    torch.cuda.synchronize()
    got = {"in": d_a, "mod": d_m, None: d_o}[in_place].cpu().numpy()
    off = {"in": offs[0], "mod": offs[1], None: offs[2]}[in_place]
    want_guard = {"in": h_a, "mod": h_m, None: h_o}[in_place]
    lo, hi = off + g, off + g + body
    assert R.same_bits(got[:lo], want_guard[:lo]) and R.same_bits(got[hi:], want_guard[hi:]), "guard band written"
    if in_place != "in":
        assert R.same_bits(d_a.cpu().numpy(), h_a), "pose_in written"
    if in_place != "mod":
        assert R.same_bits(d_m.cpu().numpy(), h_m), "pose_mod written"
    if in_place:
        assert R.same_bits(d_o.cpu().numpy(), h_o)
    if per:
        assert R.same_bits(d_w.cpu().numpy(), h_w)
    return got[lo:hi].reshape(n, B, 10)


def assert_same(got, want, what=""):
    bad = np.nonzero((R.bits(got) != R.bits(want)).any(axis=2))
    assert bad[0].size == 0, f"{what}: {bad[0].size} bones differ; first: skeleton {bad[0][0]} bone {bad[1][0]}"


# (bones, count): 1 bone in all; one block exactly (two ways); one block + 1; several blocks with a
# ragged tail, at every bone count; bones = 7: a block spans 36 skeletons, each with its own weight
SHAPES = [(1, 1), (1, BLOCK), (32, BLOCK // 32), (1, BLOCK + 1), (3, 300), (7, 150), (32, 21), (33, 20), (200, 7)]


@pytest.mark.parametrize("B,n", SHAPES, ids=[f"{b}x{n}" for b, n in SHAPES])
def test_device_matches_cpu_entry(plans, torch_dev, B, n):
    torch, dev = torch_dev
    a, m, w = inputs(100 + B, n, B)
    want = pose_blend_cpu(a, m, w)
    assert np.isfinite(want).all()
    assert_same(device_blend(torch, dev, plans(B), a, m, w), want, "per-skeleton weights")
    if B == 7:
        assert len(set(R.bits(w[:BLOCK // 7]).tolist())) > 12   # the first block's 36 skeletons: many distinct weights
    for scalar in (0.3, 1.0, float("nan")):
        assert_same(device_blend(torch, dev, plans(B), a, m, scalar), pose_blend_cpu(a, m, scalar), f"influence {scalar}")


@pytest.mark.parametrize("offs", [(1, 2, 3, 1), (3, 0, 1, 2), (2, 2, 2, 3), (0, 1, 0, 0), (3, 3, 3, 3)], ids=str)
def test_float_aligned_buffers(plans, torch_dev, offs):
    """Every pointer 0..3 floats past a 16-byte boundary: unaligned heads and tails, nothing outside the range."""
    torch, dev = torch_dev
    a, m, w = inputs(7, 150, 7)
    assert_same(device_blend(torch, dev, plans(7), a, m, w, offs=offs), pose_blend_cpu(a, m, w), str(offs))


@pytest.mark.parametrize("which", ["in", "mod"])
@pytest.mark.parametrize("B,n", [(7, 150), (33, 20)])
def test_in_place(plans, torch_dev, B, n, which):
    torch, dev = torch_dev
    a, m, w = inputs(21, n, B)
    off = (1, 0, 0, 0) if which == "in" else (0, 3, 0, 0)
    assert_same(device_blend(torch, dev, plans(B), a, m, w, offs=off, in_place=which), pose_blend_cpu(a, m, w), which)


def test_partial_early_outs_in_a_wave(plans, torch_dev):
    """3 blocks of one-bone skeletons: a wave where only two lanes blend, a wave where only two lanes
    do not (one by its weight, one by equal transforms), a wave that skips whole, and plain ones."""
    torch, dev = torch_dev
    n = 3 * BLOCK
    a, m, _ = R.mixed_inputs(5, n * len(R.KINDS))
    general = np.arange(n) * len(R.KINDS)            # the "general" bones: they always blend below weight 1
    a, m = a[general].reshape(n, 1, 10), m[general].reshape(n, 1, 10)
    w = np.full(n, 0.4, np.float32)
    w[0:64] = 1.0
    w[[5, 40]] = 0.25                                # wave 0: lanes 5 and 40 blend
    w[64 + 9] = np.nan                               # wave 1: all blend but lane 9 (weight) and lane 33 (equal transforms)
    m[64 + 33] = a[64 + 33]
    m[64 + 33, 0, 0:4] = -a[64 + 33, 0, 0:4]
    w[128:192] = 1.5                                 # wave 2: nothing to do
    m[BLOCK:BLOCK + 64] = a[BLOCK:BLOCK + 64]        # block 1, wave 0: equal poses, weight 0.4
    want = pose_blend_cpu(a, m, w)
    changed = (R.bits(want) != R.bits(m)).any(axis=(1, 2))
    assert changed[0:64].sum() == 2 and changed[64:128].sum() == 62 and not changed[128:192].any()
    assert not changed[BLOCK:BLOCK + 64].any() and changed[BLOCK + 64:].all()
    assert_same(device_blend(torch, dev, plans(1), a, m, w), want)


def test_both_libm_variants(plans, torch_dev):
    torch, dev = torch_dev
    a, m, w = inputs(33, 40, 32)
    for lv in (0, 1):
        assert_same(device_blend(torch, dev, plans(32, lv), a, m, w), pose_blend_cpu(a, m, w, libm_variant=lv), f"variant {lv}")


def test_million_bones(plans, torch_dev):
    """2^20 bones (32,768 x 32): every kind of pose pair -- both slerp branches, the sign flip, all
    four get_quaternion branches, determinants of both signs -- at the weights of interest and at
    uniform ones, against the host entry."""
    torch, dev = torch_dev
    a, m, w = inputs(77, 32768, 32)
    w[::5] = np.float32(1e-7) * np.arange(w[::5].size, dtype=np.float32)   # tiny weights too
    assert_same(device_blend(torch, dev, plans(32), a, m, w), pose_blend_cpu(a, m, w))


def test_non_finite_poses(plans, torch_dev):
    """NaN and +-Inf scattered through both inputs: the same bits as the host (a NaN result is the
    canonical quiet NaN on both sides)."""
    torch, dev = torch_dev
    a, m, w = inputs(55, 150, 7)
    rng = np.random.default_rng(56)
    for arr in (a, m):
        flat = arr.reshape(-1)
        idx = rng.choice(flat.size, flat.size // 25, replace=False)
        flat[idx] = rng.choice(np.array([np.nan, np.inf, -np.inf, 0.0, -0.0, 3e38, 1e-45], np.float32), idx.size)
    want = pose_blend_cpu(a, m, w)
    assert np.isnan(want).any() and np.isinf(want).any()
    assert_same(device_blend(torch, dev, plans(7), a, m, w), want)


def test_stream_order_solve_blend_globals(oracle, mbik, torch_dev):
    """solve -> pose_blend -> pose_globals queued on one side stream, one synchronisation at the end,
    against the host pipeline: the oracle's solve, pose_blend_cpu, pose_globals_cpu."""
    torch, dev = torch_dev
    wl = W.generate(2, 64)
    parents, pins = wl.topo.parents.tolist(), wl.topo.pins.tolist()
    plan = Plan.from_workload(wl)
    n, B = wl.n, len(parents)
    w = np.linspace(0.0, 1.2, n).astype(np.float32)
    pi, tg, d_w = (torch.from_numpy(x).to(dev) for x in (wl.pose, wl.targets, w))
    po, pb = torch.empty_like(pi), torch.empty_like(pi)
    d_g = torch.zeros(n * B * 12, dtype=torch.float32, device=dev)
    torch.cuda.synchronize()
    st = torch.cuda.Stream(device=dev)
    plan.solve(pi.data_ptr(), tg.data_ptr(), po.data_ptr(), stream=st.cuda_stream)
    plan.pose_blend(pi.data_ptr(), po.data_ptr(), pb.data_ptr(), n, influence_ptr=d_w.data_ptr(), stream=st.cuda_stream)
    plan.pose_globals(pb.data_ptr(), d_g.data_ptr(), n, stream=st.cuda_stream)
    st.synchronize()
    solved = oracle.Oracle(wl).solve(wl.pose, wl.targets, threads=8)
    blended = pose_blend_cpu(wl.pose, solved, w)
    assert R.same_bits(po.cpu().numpy(), solved)
    assert_same(pb.cpu().numpy(), blended)
    assert (R.bits(blended) != R.bits(solved)).any() and (R.bits(blended) != R.bits(wl.pose)).any()
    assert R.same_bits(d_g.cpu().numpy().reshape(n, B, 12), pose_globals_cpu(parents, pins, blended)[0])
    plan.close()


def test_argument_errors(plans, torch_dev):
    torch, dev = torch_dev
    B, n = 7, 10
    a, m, w = inputs(3, n, B)
    plan = plans(B)
    body = n * B * 10
    buf = torch.zeros(3 * body + 10, dtype=torch.float32, device=dev)
    buf[0:body] = torch.from_numpy(a.reshape(-1)).to(dev)
    buf[body:2 * body] = torch.from_numpy(m.reshape(-1)).to(dev)
    p_a, p_m, p_o = buf.data_ptr(), buf[body:].data_ptr(), buf[2 * body:].data_ptr()

    def code(*args, **k):
        with pytest.raises(_lib.MbikError) as e:
            plan.pose_blend(*args, **k)
        return e.value.code

    assert code(0, p_m, p_o, n, influence=0.5) == _lib.MBIK_EINVAL
    assert code(p_a, 0, p_o, n, influence=0.5) == _lib.MBIK_EINVAL
    assert code(p_a, p_m, 0, n, influence=0.5) == _lib.MBIK_EINVAL
    assert code(p_a, p_m, p_o, -1, influence=0.5) == _lib.MBIK_EINVAL
    assert code(p_a, p_m, buf[10:].data_ptr(), n, influence=0.5) == _lib.MBIK_EINVAL          # one bone into pose_in
    assert code(p_a, p_m, buf[2 * body - 1:].data_ptr(), n, influence=0.5) == _lib.MBIK_EINVAL  # one float into pose_mod
    assert code(p_a, p_m, buf[body - 10:].data_ptr(), n, influence=0.5) == _lib.MBIK_EINVAL   # across both
    plan.pose_blend(0, 0, 0, 0, influence=0.5)                                                 # count == 0: OK, no launch
    plan.pose_blend(p_a, p_m, p_o, n, influence=0.5)                                           # adjacent, not overlapping
    torch.cuda.synchronize()
    h = buf.cpu().numpy()
    assert R.same_bits(h[2 * body:3 * body].reshape(n, B, 10), pose_blend_cpu(a, m, 0.5))
    assert R.same_bits(h[0:body].reshape(n, B, 10), a) and R.same_bits(h[body:2 * body].reshape(n, B, 10), m)
    assert (h[3 * body:] == 0).all()


def test_mirror_influence_on_the_device_solve(oracle, mbik):
    """ManyBoneIK3D with influence 0.3: pose_blend_cpu of the solve's output; the defaults: the solve's output."""
    wl = W.generate(2, 8)
    ik = ManyBoneIK3D(wl.topo.parents)
    ik.set_iterations_per_frame(16)
    ik.set_total_effector_count(len(wl.topo.pins))
    for i, b in enumerate(wl.topo.pins):
        ik.set_effector_bone_name(i, f"bone_{b}")
        ik.set_pin_weight(i, 1.0)
    solved = ik.process_modification(wl.pose, wl.targets)
    assert (R.bits(solved) != R.bits(wl.pose)).any()
    ik.set_influence(0.3)
    assert R.same_bits(ik.process_modification(wl.pose, wl.targets), pose_blend_cpu(wl.pose, solved, 0.3))
    ik.set_active(False)
    assert R.same_bits(ik.process_modification(wl.pose, wl.targets), wl.pose)
    ik.set_active(True)
    ik.set_influence(1.0)
    assert R.same_bits(ik.process_modification(wl.pose, wl.targets), solved)
