"""mbik_clip_root_motion, mbik_clip_root_motion_layers and mbik_root_motion_apply on the GPU against
their _cpu forms, bitwise: skeleton counts around the 64-skeleton block, 1 and 5 bones with the root
first and last, 1, 2, 3 and 8 layers, both modes, both libm variants, seam crossings and off,
zero-weight, invalid and non-finite records scattered through every batch, guard bands around every
output, inputs verified unwritten, float-aligned outputs at odd offsets, the pose fix-up behind
sample_layers on one stream, and a small crowd's whole frame with the device's skeleton_global."""
import numpy as np
import pytest

from many_bone_ik_amd import _lib
from many_bone_ik_amd import animation as A
from many_bone_ik_amd import workloads as W
from many_bone_ik_amd.skinning import Mesh, cull_boxes_cpu, synthetic_mesh
from many_bone_ik_amd.solver import Plan, pose_globals_cpu

from . import bounds_recipe as BR
from . import root_motion_recipe as R
from .test_gpu_clip_sample import _rig_clips
from .test_gpu_parity import torch_dev  # noqa: F401 (fixture)

pytestmark = pytest.mark.gpu

SENTINEL = np.uint32(0x4B1D4B1D).view(np.float32)   # a finite float no call produces
GUARD = 16                                           # guard skeletons on each side of every output
COUNTS = (1, 63, 64, 65, 255, 257, 600)              # 64 skeletons a block (k_root_motion.hip)
RIGS = ((1, 0), (5, 0), (5, 4))                      # (bones, root bone)
LAYER_COUNTS = (1, 2, 3, 8)
IDENTITY = np.array([1, 0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0], np.float32)


@pytest.fixture(scope="module")
def sets(mbik):
    """One seeded walking clip set per (bones, root, libm_variant): (rest, clips, ClipSet)."""
    made = {}

    def get(B, root, libm_variant=0):
        key = (B, root, libm_variant)
        if key not in made:
            rest, clips = A.synthetic_walk_clips(500 + 10 * B + root, B, root)
            made[key] = (rest, clips, A.ClipSet(B, rest, clips, libm_variant=libm_variant))
        return made[key]

    yield get
    for _, _, s in made.values():
        s.close()


def guarded(torch, dev, body, off):
    """A device buffer of SENTINEL with `body` (float32, flat) `off` floats plus a guard band in, and
    a guard band behind: (tensor, pointer to the body, host copy)."""
    g = GUARD * 10
    h = np.full(off + g + body.size + g, SENTINEL, np.float32)
    h[off + g:off + g + body.size] = body.reshape(-1)
    d = torch.from_numpy(h).to(dev)
    return d, d[off + g:].data_ptr(), h


def check_guards(d, h, off, size):
    got = d.cpu().numpy()
    lo, hi = off + GUARD * 10, off + GUARD * 10 + size
    assert R.same_bits(got[:lo], h[:lo]) and R.same_bits(got[hi:], h[hi:]), "guard band written"
    return got[lo:hi]


def device_motion(torch, dev, cs, B, root, layers, t0, flags, pose=None, out_off=0, pose_off=0, plain=False, stream=0):
    """Launches on device copies: (motion [n][10], pose [n][B][10] or None).  motion_out and pose lie
    out_off / pose_off floats past an allocation between guard bands of SENTINEL, which must come back
    untouched, as must every input."""
    n, K = layers.shape
    d_o, p_o, h_o = guarded(torch, dev, np.full(n * 10, SENTINEL, np.float32), out_off)
    d_p = p_p = h_p = None
    if pose is not None:
        d_p, p_p, h_p = guarded(torch, dev, pose, pose_off)
    h_t0 = np.ascontiguousarray(t0, np.float64)
    d_t0 = torch.from_numpy(h_t0).to(dev)
    if plain:
        assert K == 1
        h_t1, h_ci = np.ascontiguousarray(layers["time"][:, 0]), np.ascontiguousarray(layers["clip"][:, 0])
        d_t1, d_ci = torch.from_numpy(h_t1).to(dev), torch.from_numpy(h_ci).to(dev)
        torch.cuda.synchronize()
        cs.root_motion(d_t0.data_ptr(), d_t1.data_ptr(), p_o, n, root, clip_index_ptr=d_ci.data_ptr(), pose_ptr=p_p or 0, stream=stream)
        torch.cuda.synchronize()
        assert np.array_equal(d_t1.cpu().numpy().view(np.uint64), h_t1.view(np.uint64)) and np.array_equal(d_ci.cpu().numpy(), h_ci)
    else:
        h_l = layers.reshape(-1).view(np.uint8)
        d_l = torch.from_numpy(h_l.copy()).to(dev)
        torch.cuda.synchronize()
        cs.root_motion_layers(d_l.data_ptr(), d_t0.data_ptr(), p_o, n, K, root, flags=flags, pose_ptr=p_p or 0, stream=stream)
        torch.cuda.synchronize()
        assert np.array_equal(d_l.cpu().numpy(), h_l), "layers written"
    assert np.array_equal(d_t0.cpu().numpy().view(np.uint64), h_t0.view(np.uint64)), "time_prev written"
    motion = check_guards(d_o, h_o, out_off, n * 10).reshape(n, 10)
    assert not (R.bits(motion) == R.bits(np.array([SENTINEL]))[0]).any(), "motion_out left unwritten"
    got_pose = None if pose is None else check_guards(d_p, h_p, pose_off, pose.size).reshape(n, B, 10)
    return motion, got_pose


def assert_same(got, want, what=""):
    bad = np.nonzero((R.bits(got) != R.bits(want)).any(axis=-1))[0]
    assert bad.size == 0, f"{what}: {bad.size} records differ; first {bad[0]}: got {got[bad[0]]}, want {want[bad[0]]}"


def random_pose(seed, n, B):
    return np.random.default_rng(seed).uniform(-1.0, 1.0, (n, B, 10)).astype(np.float32)


@pytest.mark.parametrize("n", COUNTS)
def test_device_matches_cpu_entry(sets, torch_dev, n):
    torch, dev = torch_dev
    for B, root in RIGS:
        rest, clips, cs = sets(B, root)
        for K in LAYER_COUNTS:
            layers, t0 = R.random_frames(800 + n + K, n, K, clips, specials=n >= 3)
            pose = random_pose(n + K, n, B)
            for flags in (0, R.NORMALIZE):
                want_pose = pose.copy()
                want = A.clip_root_motion_layers_cpu(B, rest, clips, layers, t0, root, flags, pose=want_pose)
                got, got_pose = device_motion(torch, dev, cs, B, root, layers, t0, flags, pose=pose, out_off=K % 4, pose_off=(K + flags) % 4)
                assert_same(got, want, f"B={B} root={root} K={K} flags={flags}")
                assert R.same_bits(got_pose, want_pose), f"pose: B={B} root={root} K={K} flags={flags}"


def test_specials_are_in_the_batches(sets):
    """The recipe's statistics of one of the batches above: every branch is there."""
    rest, clips, _ = sets(5, 4)
    layers, t0 = R.random_frames(800 + 257 + 3, 257, 3, clips)
    for flags in (0, R.NORMALIZE):
        _, stats = R.expected(5, rest, clips, layers, t0, 4, flags)
        for k in ("invalid_skeletons", "looped", "nonfinite", "start_channels", "on_key"):
            assert stats[k] >= 3, (k, stats)
    assert (layers["clip"] == -1).any() and (layers["weight"] == 0).any() and np.isnan(layers["weight"]).any()


@pytest.mark.parametrize("n", (1, 65, 600))
def test_plain_call(sets, torch_dev, n):
    """The plain call against its _cpu form, and the same bits as the one-layer call, without a pose."""
    torch, dev = torch_dev
    for B, root in RIGS:
        rest, clips, cs = sets(B, root)
        layers, t0 = R.random_frames(60 + n, n, 1, clips, specials=n >= 3)
        ci, t1 = layers["clip"][:, 0], layers["time"][:, 0]
        pose = random_pose(n, n, B)
        want_pose = pose.copy()
        want = A.clip_root_motion_cpu(B, rest, clips, t0[:, 0], t1, root, clip_index=ci, pose=want_pose)
        got, got_pose = device_motion(torch, dev, cs, B, root, layers, t0, 0, pose=pose, out_off=1, pose_off=3, plain=True)
        assert_same(got, want, f"plain B={B} root={root}")
        assert R.same_bits(got_pose, want_pose)
        one = layers.copy()
        one["weight"] = 1.0
        same, _ = device_motion(torch, dev, cs, B, root, one, t0, 0)
        assert R.same_bits(got, same), "plain call != one-layer call"
    # the one `clip` for every skeleton
    d_t0, d_t1 = torch.from_numpy(np.ascontiguousarray(t0[:, 0])).to(dev), torch.from_numpy(np.ascontiguousarray(t1)).to(dev)
    d_o = torch.full((n * 10,), float(SENTINEL), dtype=torch.float32, device=dev)
    cs.root_motion(d_t0.data_ptr(), d_t1.data_ptr(), d_o.data_ptr(), n, root, clip=1)
    torch.cuda.synchronize()
    assert_same(d_o.cpu().numpy().reshape(n, 10), A.clip_root_motion_cpu(B, rest, clips, t0[:, 0], t1, root, clip=1))


def test_both_libm_variants(sets, torch_dev):
    torch, dev = torch_dev
    for lv in (0, 1):
        rest, clips, cs = sets(5, 0, lv)
        layers, t0 = R.random_frames(33, 257, 3, clips)
        for flags in (0, R.NORMALIZE):
            got, _ = device_motion(torch, dev, cs, 5, 0, layers, t0, flags)
            assert_same(got, A.clip_root_motion_layers_cpu(5, rest, clips, layers, t0, 0, flags, libm_variant=lv), f"variant {lv} flags={flags}")
        one = layers[:, :1].copy()
        got, _ = device_motion(torch, dev, cs, 5, 0, one, t0[:, :1], 0, plain=True)
        assert_same(got, A.clip_root_motion_cpu(5, rest, clips, t0[:, 0], one["time"][:, 0], 0, clip_index=one["clip"][:, 0], libm_variant=lv))


def test_pose_fix_up_behind_sample_layers_on_one_stream(sets, torch_dev):
    torch, dev = torch_dev
    B, root, n, K = 5, 4, 257, 2
    rest, clips, cs = sets(B, root)
    layers, t0 = R.random_frames(91, n, K, clips)
    want_pose = A.clip_sample_layers_cpu(B, rest, clips, layers, R.NORMALIZE)
    sampled = want_pose.copy()
    want = A.clip_root_motion_layers_cpu(B, rest, clips, layers, t0, root, R.NORMALIZE, pose=want_pose)
    assert (R.bits(want_pose) != R.bits(sampled)).any()
    d_l = torch.from_numpy(layers.reshape(-1).view(np.uint8).copy()).to(dev)
    d_t0 = torch.from_numpy(t0).to(dev)
    d_p = torch.full((n, B, 10), float(SENTINEL), dtype=torch.float32, device=dev)
    d_o = torch.full((n, 10), float(SENTINEL), dtype=torch.float32, device=dev)
    st = torch.cuda.Stream(device=dev)
    torch.cuda.synchronize()
    cs.sample_layers(d_l.data_ptr(), d_p.data_ptr(), n, K, flags=R.NORMALIZE, stream=st.cuda_stream)
    cs.root_motion_layers(d_l.data_ptr(), d_t0.data_ptr(), d_o.data_ptr(), n, K, root, flags=R.NORMALIZE, pose_ptr=d_p.data_ptr(),
                          stream=st.cuda_stream)
    st.synchronize()
    assert_same(d_o.cpu().numpy(), want)
    assert R.same_bits(d_p.cpu().numpy(), want_pose)


def apply_inputs(seed, n, rest, clips):
    rng = np.random.default_rng(seed)
    layers, t0 = R.random_frames(seed, n, 2, clips, specials=n >= 3)
    motion = A.clip_root_motion_layers_cpu(rest.shape[0], rest, clips, layers, t0, 0, R.NORMALIZE)
    q = rng.normal(0.0, 1.0, (n, 4))
    q /= np.linalg.norm(q, axis=1, keepdims=True)
    G = np.empty((n, 12), np.float32)
    for s in range(n):
        G[s, 0:9] = (R.quat_to_matrix64(q[s]) * rng.uniform(0.8, 1.2)).reshape(9)
    G[:, 9:12] = rng.uniform(-50.0, 50.0, (n, 3))
    if n >= 16:
        motion[3], motion[5, 4] = np.nan, np.inf
        motion[7, 0:4] = 0.0
        G[11, 2] = np.nan
        G[13, 0:9] = 0.0
    return motion, G


@pytest.mark.parametrize("n", COUNTS)
def test_apply(sets, torch_dev, n):
    torch, dev = torch_dev
    rest, clips, cs = sets(5, 0)
    motion, G = apply_inputs(n, n, rest, clips)
    for flags in (0, R.ORTHONORMALIZE):
        for off in (0, 1, 3):
            g = GUARD * 12
            h = np.full(off + g + n * 12 + g, SENTINEL, np.float32)
            h[off + g:off + g + n * 12] = G.reshape(-1)
            d_g = torch.from_numpy(h).to(dev)
            d_m = torch.from_numpy(np.concatenate([np.full(off + 1, SENTINEL, np.float32), motion.reshape(-1)])).to(dev)
            torch.cuda.synchronize()
            cs.apply_root_motion(d_m[off + 1:].data_ptr(), d_g[off + g:].data_ptr(), n, flags=flags)
            torch.cuda.synchronize()
            got = d_g.cpu().numpy()
            assert R.same_bits(got[:off + g], h[:off + g]) and R.same_bits(got[off + g + n * 12:], h[off + g + n * 12:]), "guard band written"
            assert R.same_bits(d_m.cpu().numpy()[off + 1:].reshape(n, 10), motion), "motion written"
            assert_same(got[off + g:off + g + n * 12].reshape(n, 12), A.root_motion_apply_cpu(motion, G, flags), f"flags={flags} off={off}")


def test_nothing_to_do_and_argument_errors(sets, torch_dev):
    torch, dev = torch_dev
    B, root, n, K = 5, 0, 10, 2
    rest, clips, cs = sets(B, root)
    layers, t0 = R.random_frames(3, n, K, clips, specials=False)
    d_l = torch.from_numpy(layers.reshape(-1).view(np.uint8).copy()).to(dev)
    d_t0 = torch.from_numpy(t0).to(dev)
    d_t1 = torch.from_numpy(np.ascontiguousarray(layers["time"][:, 0])).to(dev)
    d_o = torch.full((n * 12 + 12,), float(SENTINEL), dtype=torch.float32, device=dev)
    d_g = torch.full((n * 12,), float(SENTINEL), dtype=torch.float32, device=dev)
    torch.cuda.synchronize()
    L, T0, T1, O, G = d_l.data_ptr(), d_t0.data_ptr(), d_t1.data_ptr(), d_o.data_ptr(), d_g.data_ptr()
    cs.root_motion_layers(L, T0, O, 0, K, root)                       # count == 0: OK, no launch
    cs.root_motion_layers(0, 0, 0, 0, K, root)
    cs.root_motion(T0, T1, O, 0, root)
    cs.apply_root_motion(O, G, 0)
    torch.cuda.synchronize()
    assert (R.bits(d_o.cpu().numpy()) == R.bits(np.array([SENTINEL]))[0]).all()
    assert (R.bits(d_g.cpu().numpy()) == R.bits(np.array([SENTINEL]))[0]).all()

    def code(fn, *args, **k):
        with pytest.raises(_lib.MbikError) as e:
            fn(*args, **k)
        assert str(e.value)
        return e.value.code

    E = _lib.MBIK_EINVAL
    lay, plain, app = cs.root_motion_layers, cs.root_motion, cs.apply_root_motion
    assert code(lay, 0, T0, O, n, K, root) == E and code(lay, L, 0, O, n, K, root) == E and code(lay, L, T0, 0, n, K, root) == E
    assert code(lay, L, T0, O, -1, K, root) == E
    for bad_k in (0, -1, 9):
        assert code(lay, L, T0, O, n, bad_k, root) == E
    for bad_root in (-1, B):
        assert code(lay, L, T0, O, n, K, bad_root) == E and code(plain, T0, T1, O, n, bad_root) == E
    assert code(lay, L, T0, O, n, K, root, flags=2) == E
    assert code(lay, L + 4, T0, O, n - 1, K, root) == E and code(lay, L, T0 + 4, O, n - 1, K, root) == E
    assert code(lay, L, T0, L + 8, 1, 1, root) == E and code(lay, L, T0, T0, 1, 1, root) == E          # motion_out overlaps an input
    assert code(lay, L, T0, O, n, K, root, pose_ptr=O + 4) == E                                       # ... or pose
    assert code(plain, 0, T1, O, n, root) == E and code(plain, T0, 0, O, n, root) == E and code(plain, T0, T1, 0, n, root) == E
    assert code(plain, T0, T1, O, n, root, clip=len(clips)) == E and code(plain, T0, T1, O, n, root, clip=-1) == E
    assert code(plain, T0, T1, T1, 1, root) == E
    assert code(app, 0, G, n) == E and code(app, O, 0, n) == E and code(app, O, G, -1) == E and code(app, O, G, n, flags=2) == E
    assert code(app, O, O + 8, n) == E
    with A.ClipSet(0, np.zeros((0, 10), np.float32), [dict(length=1.0, loop_mode=0, tracks=[])]) as empty:
        assert code(empty.root_motion_layers, L, T0, O, n, K, 0) == E                                  # a set without bones
    lay(L, T0, O, n, K, root)
    torch.cuda.synchronize()
    h = d_o.cpu().numpy()
    assert_same(h[:n * 10].reshape(n, 10), A.clip_root_motion_layers_cpu(B, rest, clips, layers, t0, root, 0))
    assert (R.bits(h[n * 10:]) == R.bits(np.array([SENTINEL]))[0]).all()


def test_a_small_crowd_walks_through_the_whole_frame(mbik, torch_dev):
    """A C2 plan, 130 skeletons, 4 frames on one side stream: sample_layers -> root motion (+pose) ->
    apply -> capture targets -> solve -> globals -> bounds -> cull with the device's skeleton_global.
    The transforms, the motion records and the fixed-up poses must equal the CPU twins' bit for bit,
    and the visible list must be the one cull_boxes_cpu gives with the CPU twins' transforms."""
    torch, dev = torch_dev
    wl = W.generate(2, 130)
    parents = wl.topo.parents.tolist()
    n, B, P = wl.n, len(parents), wl.targets.shape[1]
    root = parents.index(-1)
    rest = np.ascontiguousarray(wl.pose[0])
    clips = _rig_clips(rest, 4)
    rng = np.random.default_rng(17)
    for c, clip in enumerate(clips):       # a walk and a turn on the root, at another pace in each clip
        L = clip["length"]
        clip["tracks"] = [t for t in clip["tracks"] if t["bone"] != root]
        yaw = np.radians(40.0 + 30.0 * c) * np.array([0.0, 0.5, 1.0])
        clip["tracks"] += [
            dict(bone=root, channel=A.POSITION, interpolation=A.LINEAR, loop_wrap=1, times=np.array([0.0, 0.4 * L, L]),
                 values=np.array([[0, 0, 0], [0.1, 0, 0.5 + c], [0, 0, 1.5 + 2 * c]], np.float32)),
            dict(bone=root, channel=A.ROTATION, interpolation=A.LINEAR, loop_wrap=1, times=np.array([0.0, 0.5 * L, L]),
                 values=np.stack([0 * yaw, np.sin(yaw / 2), 0 * yaw, np.cos(yaw / 2)], axis=1).astype(np.float32))]
    rest_globals, _ = pose_globals_cpu(parents, [], wl.pose[:1])
    pos, _, idx, w = synthetic_mesh(parents, rest_globals[0], 300, 4, seed=3)
    planes = BR.frustum_planes(4)
    w0 = rng.uniform(0.0, 1.0, n).astype(np.float32)
    weights = np.stack([w0, np.float32(1) - w0], axis=1)
    clip_of = np.tile([0, 1], (n, 1))
    t = rng.uniform(0.0, 2.0, (n, 2))
    dt = 0.35                               # a clip is 1 to 2 s long: most layers cross the seam within 4 frames
    sg = np.tile(IDENTITY, (n, 1))
    sg[:, 9:12] = rng.uniform(-10.0, 10.0, (n, 3)).astype(np.float32)
    origin0 = sg[:, 9:12].copy()
    node = np.ascontiguousarray(np.broadcast_to(IDENTITY, (n, P, 12))).copy()
    node[:, :, 9:12] = wl.targets[:, :, 9:12] + sg[:, None, 9:12]

    plan = Plan.from_workload(wl)
    flags = R.NORMALIZE
    with A.ClipSet(B, rest, clips) as cs, Mesh(B, pos, idx, w) as mesh:
        d_sg, d_node = torch.from_numpy(sg.copy()).to(dev), torch.from_numpy(node).to(dev)
        d_pose = torch.empty((n, B, 10), dtype=torch.float32, device=dev)
        d_out, d_tg = torch.empty_like(d_pose), torch.empty((n, P, 12), dtype=torch.float32, device=dev)
        d_m = torch.empty((n, 10), dtype=torch.float32, device=dev)
        d_g = torch.empty((n, B, 12), dtype=torch.float32, device=dev)
        d_b = torch.empty((n, 6), dtype=torch.float32, device=dev)
        d_vis = torch.zeros(n, dtype=torch.uint8, device=dev)
        d_ind = torch.full((n,), -1, dtype=torch.int32, device=dev)
        d_cnt = torch.zeros(1, dtype=torch.int32, device=dev)
        st = torch.cuda.Stream(device=dev)
        looped = 0
        for frame in range(4):
            layers = A.pack_layers(t + dt, clip_of, weights)
            d_l = torch.from_numpy(layers.reshape(-1).view(np.uint8).copy()).to(dev)
            d_t0 = torch.from_numpy(t.copy()).to(dev)
            torch.cuda.synchronize()
            s = st.cuda_stream
            cs.sample_layers(d_l.data_ptr(), d_pose.data_ptr(), n, 2, flags=flags, stream=s)
            cs.root_motion_layers(d_l.data_ptr(), d_t0.data_ptr(), d_m.data_ptr(), n, 2, root, flags=flags, pose_ptr=d_pose.data_ptr(), stream=s)
            cs.apply_root_motion(d_m.data_ptr(), d_sg.data_ptr(), n, flags=R.ORTHONORMALIZE, stream=s)
            plan.capture_targets(d_sg.data_ptr(), d_node.data_ptr(), d_tg.data_ptr(), stream=s)
            plan.solve(d_pose.data_ptr(), d_tg.data_ptr(), d_out.data_ptr(), stream=s)
            plan.pose_globals(d_out.data_ptr(), d_g.data_ptr(), n, stream=s)
            mesh.bounds(d_g.data_ptr(), d_b.data_ptr(), n, stream=s)
            mesh.cull(d_b.data_ptr(), n, planes, skeleton_global_ptr=d_sg.data_ptr(), visible_ptr=d_vis.data_ptr(),
                      indices_ptr=d_ind.data_ptr(), visible_count_ptr=d_cnt.data_ptr(), stream=s)
            st.synchronize()
            # the CPU twins' frame
            pose = A.clip_sample_layers_cpu(B, rest, clips, layers, flags)
            motion = A.clip_root_motion_layers_cpu(B, rest, clips, layers, t, root, flags, pose=pose)
            sg = A.root_motion_apply_cpu(motion, sg, R.ORTHONORMALIZE)
            looped += R.expected(B, rest, clips, layers, t, root, flags)[1]["looped"]
            assert R.same_bits(d_m.cpu().numpy(), motion), f"frame {frame}: motion"
            assert R.same_bits(d_pose.cpu().numpy(), pose), f"frame {frame}: poses"
            assert R.same_bits(d_sg.cpu().numpy(), sg), f"frame {frame}: skeleton_global"
            vis, ind = cull_boxes_cpu(d_b.cpu().numpy(), planes, skeleton_global=sg)[:2]
            cnt = int(d_cnt.cpu().numpy()[0])
            assert np.array_equal(d_vis.cpu().numpy(), vis), f"frame {frame}: visible"
            assert cnt == int(vis.sum()) and np.array_equal(d_ind.cpu().numpy()[:cnt], np.flatnonzero(vis)), f"frame {frame}: the visible list"
            assert 0 < cnt < n, "the frustum cuts the crowd"
            t = t + dt
        assert np.isfinite(sg).all() and looped >= 10
        assert np.abs(sg[:, 9:12] - origin0).max() > 0.5, "the crowd walked"
    plan.close()
