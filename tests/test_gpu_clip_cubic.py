"""Cubic interpolation on the GPU: the six clip calls on sets made by mbik_clipset_create_desc
against mbik_clip_call_cpu, bitwise, between guard bands: bone, weight and skeleton counts around
the kernels' block edges, both libm variants, nearest / linear / cubic tracks mixed across the lanes
of one wave, 1, 2 and 8 layers with off layers and zero weights; a set without a cubic track made by
the new entry against one made by mbik_clipset_create; and a 130-skeleton frame loop on a cubic set
-- Playback.advance, sample_layers, sample_shapes_layers, root_motion_layers, apply_root_motion --
whose poses, shape weights and skeleton_global equal the CPU twins' every frame."""
import numpy as np
import pytest

from many_bone_ik_amd import animation as A

from . import clip_cubic_cases as K
from . import clip_cubic_recipe as Q
from . import clip_layers_recipe as LR
from . import root_motion_recipe as RM
from .test_gpu_parity import torch_dev  # noqa: F401 (fixture)

pytestmark = pytest.mark.gpu

SENTINEL = np.uint32(0x4B1D4B1D).view(np.float32)   # a finite float no sample produces
GUARD = 640                                          # guard floats on each side of an output
P = 3
LAYER_CASES = ((1, 0), (2, 1), (8, 0), (8, 1))       # (layer_count, flags)


@pytest.fixture(scope="module")
def sets(mbik):
    """One seeded cubic set per (bone count, libm_variant): (rest, clips, ClipSet), each with P shapes."""
    made = {}

    def get(B, libm_variant=0):
        if (B, libm_variant) not in made:
            rest, clips = K.cubic_set(500 + B, B, P)
            made[B, libm_variant] = (rest, clips, A.ClipSet(B, rest, clips, libm_variant=libm_variant, shape_count=P, cubic=True))
        return made[B, libm_variant]

    yield get
    for _, _, s in made.values():
        s.close()


class Out:
    """A device output of `floats` floats between two guard bands of SENTINEL."""

    def __init__(self, torch, dev, floats):
        self.host = np.full(GUARD + floats + GUARD, SENTINEL, np.float32)
        self.dev = torch.from_numpy(self.host).to(dev)
        self.floats = floats
        self.ptr = self.dev[GUARD:].data_ptr()

    def body(self, shape):
        got = self.dev.cpu().numpy()
        lo, hi = GUARD, GUARD + self.floats
        assert Q.same_bits(got[:lo], self.host[:lo]) and Q.same_bits(got[hi:], self.host[hi:]), "guard band written"
        return got[lo:hi].reshape(shape)


def up(torch, dev, a):
    """A host array on the device, as bytes (records included)."""
    return torch.from_numpy(np.ascontiguousarray(a).reshape(-1).view(np.uint8).copy()).to(dev)


def assert_same(got, want, what, written=True):
    bad = np.argwhere(Q.bits(got) != Q.bits(want))
    assert bad.shape[0] == 0, f"{what}: {bad.shape[0]} floats differ; first at {tuple(bad[0])}: got {got[tuple(bad[0])]!r}, want {want[tuple(bad[0])]!r}"
    if written:
        assert not (Q.bits(got) == Q.bits(np.array([SENTINEL]))[0]).any(), f"{what}: output left unwritten"


def spread_times(seed, clips, n, key="tracks"):
    """(time [n], clip_index [n]): the times of interest of every clip, cycled to n skeletons, so that
    neighbouring lanes sit on keys, between them, outside the clip and on NaN."""
    t, ci = K.plain_batch(seed, clips, key, limit=12)
    idx = np.random.default_rng(seed).permutation(max(n, t.shape[0]))[:n] % t.shape[0]
    return np.ascontiguousarray(t[idx]), np.ascontiguousarray(ci[idx])


# (bones, skeletons): 1 bone in all; 255, 256 and 257 bones in all; 5 bones at 255 bones in all and at
# three blocks with a partial last one
POSE_SHAPES = [(1, 1), (1, 255), (1, 256), (1, 257), (5, 51), (5, 130)]


@pytest.mark.parametrize("B,n", POSE_SHAPES, ids=[f"{b}x{n}" for b, n in POSE_SHAPES])
def test_sample_matches_cpu_twin(sets, torch_dev, B, n):
    torch, dev = torch_dev
    for lv in ((0, 1) if (B, n) == (5, 130) else (0,)):
        rest, clips, cs = sets(B, lv)
        t, ci = spread_times(11 + n, clips, n)
        out = Out(torch, dev, n * B * 10)
        d_t, d_ci = up(torch, dev, t), up(torch, dev, ci)
        torch.cuda.synchronize()
        cs.sample(d_t.data_ptr(), out.ptr, n, clip_index_ptr=d_ci.data_ptr())
        torch.cuda.synchronize()
        assert_same(out.body((n, B, 10)), A.clip_sample_cpu(B, rest, clips, t, ci, libm_variant=lv, cubic=True), f"sample libm {lv}")


@pytest.mark.parametrize("B,n", POSE_SHAPES, ids=[f"{b}x{n}" for b, n in POSE_SHAPES])
def test_sample_layers_matches_cpu_twin(sets, torch_dev, B, n):
    torch, dev = torch_dev
    for lv in ((0, 1) if (B, n) == (5, 130) else (0,)):
        rest, clips, cs = sets(B, lv)
        for layer_count, flags in LAYER_CASES:
            layers = LR.random_layers(800 + n + layer_count, n, layer_count, clips, specials=n >= 3)
            out = Out(torch, dev, n * B * 10)
            d_l = up(torch, dev, layers)
            torch.cuda.synchronize()
            cs.sample_layers(d_l.data_ptr(), out.ptr, n, layer_count, flags=flags)
            torch.cuda.synchronize()
            want = A.clip_sample_layers_cpu(B, rest, clips, layers, flags, libm_variant=lv, cubic=True)
            assert_same(out.body((n, B, 10)), want, f"layers K={layer_count} flags={flags} libm {lv}")


# skeletons of P = 3 shapes: 1 weight short of a block, across the edge, three blocks; and one skeleton
@pytest.mark.parametrize("n", (1, 85, 86, 130))
def test_shapes_match_cpu_twin(sets, torch_dev, n):
    torch, dev = torch_dev
    rest, clips, cs = sets(5)
    t, ci = spread_times(31 + n, clips, n, "shape_tracks")
    out = Out(torch, dev, n * P)
    d_t, d_ci = up(torch, dev, t), up(torch, dev, ci)
    torch.cuda.synchronize()
    cs.sample_shapes(d_t.data_ptr(), out.ptr, n, clip_index_ptr=d_ci.data_ptr())
    torch.cuda.synchronize()
    assert_same(out.body((n, P)), A.clip_sample_shapes_cpu(P, clips, t, ci, cubic=True), "shapes")
    for layer_count, flags in LAYER_CASES:
        layers = K.shape_layers(900 + n + layer_count, n, layer_count, clips)
        out = Out(torch, dev, n * P)
        d_l = up(torch, dev, layers)
        torch.cuda.synchronize()
        cs.sample_shapes_layers(d_l.data_ptr(), out.ptr, n, layer_count, flags=flags)
        torch.cuda.synchronize()
        assert_same(out.body((n, P)), A.clip_sample_shapes_layers_cpu(P, clips, layers, flags, cubic=True), f"shape layers K={layer_count} flags={flags}")


@pytest.mark.parametrize("n", (1, 63, 64, 65, 257))
def test_root_motion_matches_cpu_twin(sets, torch_dev, n):
    torch, dev = torch_dev
    B = 5
    for lv in ((0, 1) if n == 65 else (0,)):
        rest, clips, cs = sets(B, lv)
        t0, t1, ci = K.root_times(41 + n, clips, n)
        out = Out(torch, dev, n * 10)
        pose = Out(torch, dev, n * B * 10)
        d_t0, d_t1, d_ci = up(torch, dev, t0), up(torch, dev, t1), up(torch, dev, ci)
        torch.cuda.synchronize()
        cs.root_motion(d_t0.data_ptr(), d_t1.data_ptr(), out.ptr, n, K.ROOT, clip_index_ptr=d_ci.data_ptr(), pose_ptr=pose.ptr)
        torch.cuda.synchronize()
        want_pose = np.full((n, B, 10), SENTINEL, np.float32)
        want = A.clip_root_motion_cpu(B, rest, clips, t0, t1, K.ROOT, ci, pose=want_pose, libm_variant=lv, cubic=True)
        assert_same(out.body((n, 10)), want, f"root motion libm {lv}")
        assert_same(pose.body((n, B, 10)), want_pose, "root motion pose", written=False)
        for layer_count, flags in LAYER_CASES:
            layers, prev = RM.random_frames(600 + n + layer_count, n, layer_count, clips, specials=n >= 3)
            out = Out(torch, dev, n * 10)
            d_l, d_p = up(torch, dev, layers), up(torch, dev, prev)
            torch.cuda.synchronize()
            cs.root_motion_layers(d_l.data_ptr(), d_p.data_ptr(), out.ptr, n, layer_count, K.ROOT, flags=flags)
            torch.cuda.synchronize()
            want = A.clip_root_motion_layers_cpu(B, rest, clips, layers, prev, K.ROOT, flags, libm_variant=lv, cubic=True)
            assert_same(out.body((n, 10)), want, f"root layers K={layer_count} flags={flags} libm {lv}")


def test_lanes_of_one_wave_mix_the_kinds(sets):
    """The 5-bone set's neighbouring bones and neighbouring skeletons differ in interpolation kind:
    within the first 64 lanes of the 130-skeleton batch all three kinds are evaluated, the spherical
    cubic beside the slerp."""
    rest, clips, _ = sets(5)
    kinds = {(c, tr["bone"], tr["channel"]): tr["interpolation"] for c, clip in enumerate(clips) for tr in clip["tracks"] if len(tr["times"]) > 1}
    t, ci = spread_times(11 + 130, clips, 130)
    lanes = [(s, b) for s in range(13) for b in range(5)][:64]
    seen = {kinds.get((int(ci[s]), b, ch)) for s, b in lanes for ch in (A.POSITION, A.ROTATION, A.SCALE)}
    assert {A.NEAREST, A.LINEAR, A.CUBIC} <= seen
    assert {A.LINEAR, A.CUBIC} <= {kinds.get((int(ci[s]), b, A.ROTATION)) for s, b in lanes}


def test_set_without_cubic_from_the_new_entry_matches_the_old(mbik, torch_dev):
    """mbik_clipset_create_desc on nearest / linear tracks: the bits of mbik_clipset_create[_shaped]'s
    set, for all six calls."""
    torch, dev = torch_dev
    B, n = 5, 130
    rest, clips = K.cubic_set(77, B, P, kinds=(A.NEAREST, A.LINEAR))
    t, ci = spread_times(5, clips, n)
    layers, prev = RM.random_frames(6, n, 2, clips)
    t0, t1, cr = K.root_times(7, clips, n)
    d = {k: up(torch, dev, v) for k, v in dict(t=t, ci=ci, layers=layers, prev=prev, t0=t0, t1=t1, cr=cr).items()}
    got = []
    for cubic in (False, True):
        with A.ClipSet(B, rest, clips, shape_count=P, cubic=cubic) as cs:
            outs = [Out(torch, dev, f) for f in (n * B * 10, n * B * 10, n * P, n * P, n * 10, n * 10)]
            torch.cuda.synchronize()
            cs.sample(d["t"].data_ptr(), outs[0].ptr, n, clip_index_ptr=d["ci"].data_ptr())
            cs.sample_layers(d["layers"].data_ptr(), outs[1].ptr, n, 2, flags=1)
            cs.sample_shapes(d["t"].data_ptr(), outs[2].ptr, n, clip_index_ptr=d["ci"].data_ptr())
            cs.sample_shapes_layers(d["layers"].data_ptr(), outs[3].ptr, n, 2, flags=1)
            cs.root_motion(d["t0"].data_ptr(), d["t1"].data_ptr(), outs[4].ptr, n, K.ROOT, clip_index_ptr=d["cr"].data_ptr())
            cs.root_motion_layers(d["layers"].data_ptr(), d["prev"].data_ptr(), outs[5].ptr, n, 2, K.ROOT, flags=1)
            torch.cuda.synchronize()
            got.append([o.body((-1,)) for o in outs])
    for name, a, b in zip(("sample", "sample_layers", "shapes", "shapes_layers", "root_motion", "root_motion_layers"), *got):
        assert_same(b, a, name)
    assert_same(got[0][0].reshape(n, B, 10), A.clip_sample_cpu(B, rest, clips, t, ci), "the old entry's set against its CPU twin")


def test_a_crowd_plays_a_cubic_set_through_the_frame_loop(mbik, torch_dev):
    """130 skeletons, 8 frames on one side stream, two slots, on a set with cubic pose and shape
    tracks: advance -> sample_layers -> sample_shapes_layers -> root_motion_layers (+pose) ->
    apply_root_motion, the layer records never leaving the device; a third of the crowd switches
    clips with a blend in frame 2.  Poses, shape weights and skeleton_global equal the chain of CPU
    twins bit for bit, every frame."""
    torch, dev = torch_dev
    n, B, slots, root = 130, 7, 2, K.ROOT
    rest, clips = K.cubic_set(91, B, P)
    assert any(tr["interpolation"] == A.CUBIC and tr["bone"] == root and len(tr["times"]) > 1 for c in clips for tr in c["tracks"])
    rng = np.random.default_rng(29)
    st, fl = A.empty_state(n, slots)
    st["pos"][:, 0], st["clip"][:, 0], st["speed"][:, 0] = rng.uniform(0.0, clips[0]["length"], n), 0, rng.choice([1.0, 0.5, 2.0], n)
    switch = A.pack_commands(np.arange(0, n, 3), 1, blend_time=0.3)
    delta, flags = 0.15, A.LAYERS_NORMALIZE
    sg = np.tile(np.array([1, 0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0], np.float32), (n, 1))
    sg[:, 9:12] = rng.uniform(-10.0, 10.0, (n, 3)).astype(np.float32)
    with A.ClipSet(B, rest, clips, shape_count=P, cubic=True) as cs, A.Playback(cs, n, slots) as pb:
        pb.write(st, fl)
        d_sg = torch.from_numpy(sg.copy()).to(dev)
        d_cmd = up(torch, dev, switch)
        d_l = torch.empty(n * slots * 16, dtype=torch.uint8, device=dev)
        d_t0 = torch.empty((n, slots), dtype=torch.float64, device=dev)
        d_pose = torch.empty((n, B, 10), dtype=torch.float32, device=dev)
        d_w = torch.empty((n, P), dtype=torch.float32, device=dev)
        d_m = torch.empty((n, 10), dtype=torch.float32, device=dev)
        stream = torch.cuda.Stream(device=dev)
        torch.cuda.synchronize()
        fading = 0
        for frame in range(8):
            s = stream.cuda_stream
            pb.advance(delta, d_l.data_ptr(), d_t0.data_ptr(), n, cmds_ptr=d_cmd.data_ptr() if frame == 2 else 0,
                       cmd_count=len(switch) if frame == 2 else 0, stream=s)
            cs.sample_layers(d_l.data_ptr(), d_pose.data_ptr(), n, slots, flags=flags, stream=s)
            cs.sample_shapes_layers(d_l.data_ptr(), d_w.data_ptr(), n, slots, flags=flags, stream=s)
            cs.root_motion_layers(d_l.data_ptr(), d_t0.data_ptr(), d_m.data_ptr(), n, slots, root, flags=flags, pose_ptr=d_pose.data_ptr(), stream=s)
            cs.apply_root_motion(d_m.data_ptr(), d_sg.data_ptr(), n, flags=A.ROOT_MOTION_ORTHONORMALIZE, stream=s)
            stream.synchronize()
            st, fl, layers, t0, ev = A.playback_advance_cpu(clips, st, fl, delta, cmds=switch if frame == 2 else None)
            pose = A.clip_sample_layers_cpu(B, rest, clips, layers, flags, cubic=True)
            weights = A.clip_sample_shapes_layers_cpu(P, clips, layers, flags, cubic=True)
            motion = A.clip_root_motion_layers_cpu(B, rest, clips, layers, t0, root, flags, pose=pose, cubic=True)
            sg = A.root_motion_apply_cpu(motion, sg, A.ROOT_MOTION_ORTHONORMALIZE)
            fading += int((layers["clip"][:, 1] != -1).sum())
            assert np.array_equal(d_l.cpu().numpy().view(A.LAYER_DTYPE).reshape(n, slots).view(np.uint8), layers.view(np.uint8)), f"frame {frame}: layers"
            assert_same(d_pose.cpu().numpy(), pose, f"frame {frame}: poses", written=False)
            assert_same(d_w.cpu().numpy(), weights, f"frame {frame}: shape weights", written=False)
            assert_same(d_sg.cpu().numpy(), sg, f"frame {frame}: skeleton_global", written=False)
        assert fading >= len(switch) and np.isfinite(sg).all()
