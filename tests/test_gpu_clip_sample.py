"""mbik_clip_sample on the GPU (Godot's Animation track interpolation for a batch of skeletons,
each at its own time in its own clip) against mbik_clip_sample_cpu, bitwise: bone counts and batch
sizes around the 256-bone block, blocks that span dozens of skeletons, a clip-index buffer and a
scalar clip, float-aligned (odd) output offsets, guard bands around every buffer, invalid clip
indices and non-finite times in the batch, both libm variants, 2^20 bones, and stream order in
front of a solve and mbik_pose_globals."""
import numpy as np
import pytest

from many_bone_ik_amd import _lib
from many_bone_ik_amd import animation as A
from many_bone_ik_amd import workloads as W
from many_bone_ik_amd.solver import Plan, pose_globals_cpu

from . import clip_recipe as R
from .test_gpu_parity import torch_dev  # noqa: F401 (fixture)

pytestmark = pytest.mark.gpu

SENTINEL = np.uint32(0x4B1D4B1D).view(np.float32)   # a finite float no sample produces
GUARD = 64                                           # guard skeletons (and times, clip indices) on each side
GUARD_TIME = 0.4242                                  # a time and a clip that would sample something else, were they read
GUARD_CLIP = 1
BLOCK = 256                                          # bones a block (k_clip.hip)
INT32_MIN = -2 ** 31


@pytest.fixture(scope="module")
def sets(mbik):
    """One seeded clip set per (bone count, libm_variant): (rest, clips, ClipSet)."""
    made = {}

    def get(B, libm_variant=0):
        if (B, libm_variant) not in made:
            rest, clips = A.synthetic_clips(300 + B, B)
            made[B, libm_variant] = (rest, clips, A.ClipSet(B, rest, clips, libm_variant=libm_variant))
        return made[B, libm_variant]

    yield get
    for _, _, s in made.values():
        s.close()


def inputs(seed, n, clips, specials=True):
    """One time and one clip index per skeleton, all distinct: uniform times from one loop before to
    two loops after the clip, a tenth exactly on a key, and (specials) NaN, the infinities and
    invalid clip indices scattered through the batch."""
    rng = np.random.default_rng(seed)
    ci = rng.integers(0, len(clips), n).astype(np.int32)
    L = np.array([c["length"] for c in clips])[ci]
    t = rng.uniform(-1.0, 3.0, n) * L
    for s in np.nonzero(rng.uniform(0.0, 1.0, n) < 0.1)[0]:
        tracks = clips[ci[s]]["tracks"]
        if tracks:
            T = tracks[rng.integers(0, len(tracks))]["times"]
            t[s] = T[rng.integers(0, len(T))]
    if specials and n >= 20:
        k = rng.choice(n, 10, replace=False)
        t[k[0:2]], t[k[2]], t[k[3]], t[k[4]] = np.nan, np.inf, -np.inf, 1e9
        ci[k[5]], ci[k[6]], ci[k[7]], ci[k[8]] = -1, len(clips), INT32_MIN, 2 ** 31 - 1
    return t, ci


def device_sample(torch, dev, cs, B, t, ci=None, clip=0, offs=(0, 0, 0), stream=0):
    """Launches on device copies and returns pose_out [n][B][10].  pose_out starts offs[0] floats, time
    offs[1] doubles and clip_index offs[2] ints past an allocation; each has GUARD skeletons' worth
    of guard entries on both sides -- SENTINEL around (and in) the output, GUARD_TIME and GUARD_CLIP
    around the inputs -- which must come back untouched."""
    n = t.shape[0]
    g, body = GUARD * B * 10, n * B * 10
    h_o = np.full(offs[0] + g + body + g, SENTINEL, np.float32)
    h_t = np.full(offs[1] + GUARD + n + GUARD, GUARD_TIME, np.float64)
    h_t[offs[1] + GUARD:offs[1] + GUARD + n] = t
    d_o, d_t = torch.from_numpy(h_o).to(dev), torch.from_numpy(h_t).to(dev)
    d_c = None
    if ci is not None:
        h_c = np.full(offs[2] + GUARD + n + GUARD, GUARD_CLIP, np.int32)
        h_c[offs[2] + GUARD:offs[2] + GUARD + n] = ci
        d_c = torch.from_numpy(h_c).to(dev)
    torch.cuda.synchronize()
    cs.sample(d_t[offs[1] + GUARD:].data_ptr(), d_o[offs[0] + g:].data_ptr(), n,
              clip_index_ptr=0 if d_c is None else d_c[offs[2] + GUARD:].data_ptr(), clip=clip, stream=stream)
    torch.cuda.synchronize()
    got = d_o.cpu().numpy()
    lo, hi = offs[0] + g, offs[0] + g + body
    assert R.same_bits(got[:lo], h_o[:lo]) and R.same_bits(got[hi:], h_o[hi:]), "guard band written"
    assert np.array_equal(d_t.cpu().numpy().view(np.uint64), h_t.view(np.uint64)), "time written"
    if d_c is not None:
        assert np.array_equal(d_c.cpu().numpy(), h_c), "clip_index written"
    return got[lo:hi].reshape(n, B, 10)


def assert_same(got, want, what=""):
    bad = np.nonzero((R.bits(got) != R.bits(want)).any(axis=2))
    assert bad[0].size == 0, (f"{what}: {bad[0].size} bones differ; first: skeleton {bad[0][0]} bone {bad[1][0]}: "
                              f"got {got[bad[0][0], bad[1][0]]}, want {want[bad[0][0], bad[1][0]]}")
    assert not (R.bits(got) == R.bits(np.array([SENTINEL]))[0]).any(), f"{what}: output left unwritten"


# (bones, count): 1 bone in all; one block exactly (two ways); one block + 1; several blocks with a
# ragged tail, at every bone count; bones = 7: a block spans 36 skeletons, each with its own time and clip
SHAPES = [(1, 1), (1, 5), (1, BLOCK), (32, BLOCK // 32), (1, BLOCK + 1), (3, 300), (7, 150), (33, 20), (200, 7)]


@pytest.mark.parametrize("B,n", SHAPES, ids=[f"{b}x{n}" for b, n in SHAPES])
def test_device_matches_cpu_entry(sets, torch_dev, B, n):
    torch, dev = torch_dev
    rest, clips, cs = sets(B)
    t, ci = inputs(500 + B, n, clips)
    want = A.clip_sample_cpu(B, rest, clips, t, ci)
    assert_same(device_sample(torch, dev, cs, B, t, ci), want, "clip_index buffer")
    if B == 7:   # the first block's 36 skeletons: distinct times, every clip
        assert len(set(t[:BLOCK // 7].tolist())) == BLOCK // 7 and len(set(ci[:BLOCK // 7].tolist())) >= len(clips)
    for clip in range(len(clips)):
        assert_same(device_sample(torch, dev, cs, B, t, None, clip=clip), A.clip_sample_cpu(B, rest, clips, t, clip=clip),
                    f"scalar clip {clip}")


@pytest.mark.parametrize("B", (1, 3))
def test_a_set_without_any_track(mbik, torch_dev, B):
    """The tables' edge layout: no clip has a track, so the key sections hold the spare record only and every header is
    empty; every pose is the rest pose, on the device as on the host."""
    torch, dev = torch_dev
    rest = A.synthetic_clips(300 + B, B)[0]
    clips = [dict(length=1.5, loop_mode=A.LOOP_LINEAR, tracks=[]), dict(length=0.5, loop_mode=A.LOOP_NONE, tracks=[])]
    t, ci = np.array([0.0, 0.25, 0.75, 1.5, -2.0]), np.array([0, 1, 0, 1, 0], np.int32)
    want = A.clip_sample_cpu(B, rest, clips, t, ci)
    assert R.same_bits(want, np.tile(rest, (5, 1, 1)))
    with A.ClipSet(B, rest, clips) as cs:
        assert_same(device_sample(torch, dev, cs, B, t, ci), want, "no tracks")
        layers = A.pack_layers(np.stack([t, t[::-1]], axis=1), np.stack([ci, 1 - ci], axis=1), np.full((5, 2), 0.5))
        d_l, d_o = torch.from_numpy(layers.view(np.uint8).reshape(-1).copy()).to(dev), torch.zeros((5, B, 10), dtype=torch.float32, device=dev)
        cs.sample_layers(d_l.data_ptr(), d_o.data_ptr(), 5, 2)
        torch.cuda.synchronize()
        assert R.same_bits(d_o.cpu().numpy(), A.clip_sample_layers_cpu(B, rest, clips, layers))


def test_guard_entries_would_change_the_result(sets):
    """Were a guard time or guard clip index read in place of a skeleton's own, its pose would differ."""
    rest, clips, _ = sets(7)
    t, ci = inputs(507, 150, clips, specials=False)
    want = A.clip_sample_cpu(7, rest, clips, t, ci)
    swapped_t = A.clip_sample_cpu(7, rest, clips, np.full_like(t, GUARD_TIME), ci)
    assert (R.bits(swapped_t) != R.bits(want)).any(axis=(1, 2)).all()
    other = ci != GUARD_CLIP
    swapped_c = A.clip_sample_cpu(7, rest, clips, t, np.full_like(ci, GUARD_CLIP))
    assert (R.bits(swapped_c) != R.bits(want)).any(axis=(1, 2))[other].all() and other.sum() > 50


@pytest.mark.parametrize("offs", [(1, 1, 1), (3, 0, 2), (2, 3, 3), (0, 1, 0), (3, 2, 1)], ids=str)
def test_float_aligned_buffers(sets, torch_dev, offs):
    """pose_out 0..3 floats past a 16-byte boundary, time and clip_index at odd elements:
    unaligned heads and tails, nothing outside the range."""
    torch, dev = torch_dev
    rest, clips, cs = sets(7)
    t, ci = inputs(9, 150, clips)
    assert_same(device_sample(torch, dev, cs, 7, t, ci, offs=offs), A.clip_sample_cpu(7, rest, clips, t, ci), str(offs))


def test_invalid_clips_and_non_finite_times_in_the_batch(sets, torch_dev):
    """A third of the batch is invalid or non-finite, in every wave next to plain skeletons."""
    torch, dev = torch_dev
    rest, clips, cs = sets(3)
    n = 300
    t, ci = inputs(77, n, clips, specials=False)
    t[0::9], t[4::9] = np.nan, np.array([np.inf, -np.inf])[np.arange(len(t[4::9])) % 2]
    ci[2::9] = np.array([-1, len(clips), INT32_MIN, 12345], np.int32)[np.arange(len(ci[2::9])) % 4]
    want = A.clip_sample_cpu(3, rest, clips, t, ci)
    bad = (ci < 0) | (ci >= len(clips))
    assert (R.bits(want[bad]) == R.NAN_BITS).all() and np.isfinite(want[~bad & np.isfinite(t)]).all()
    assert_same(device_sample(torch, dev, cs, 3, t, ci), want)


def test_both_libm_variants(sets, torch_dev):
    torch, dev = torch_dev
    for lv in (0, 1):
        rest, clips, cs = sets(32, lv)
        t, ci = inputs(33, 40, clips)
        assert_same(device_sample(torch, dev, cs, 32, t, ci), A.clip_sample_cpu(32, rest, clips, t, ci, libm_variant=lv), f"variant {lv}")


def test_million_bones(sets, torch_dev):
    """2^20 bones (32,768 x 32) in one call, every skeleton at its own time."""
    torch, dev = torch_dev
    rest, clips, cs = sets(32)
    t, ci = inputs(78, 32768, clips)
    assert_same(device_sample(torch, dev, cs, 32, t, ci), A.clip_sample_cpu(32, rest, clips, t, ci))


def _rig_clips(rest, seed, clip_count=2):
    """Clips for a real rig: every bone's rotation moves around its rest rotation (4 linear keys within
    25 degrees of it); positions and scales stay untracked, so the skeleton keeps its proportions."""
    rng = np.random.default_rng(seed)
    clips = []
    for c in range(clip_count):
        L = float(rng.uniform(1.0, 2.0))
        tracks = []
        for bone in range(rest.shape[0]):
            ax = rng.normal(0.0, 1.0, (4, 3))
            ax /= np.linalg.norm(ax, axis=1, keepdims=True)
            ang = np.radians(rng.uniform(5.0, 25.0, 4))
            dq = np.concatenate([ax * np.sin(ang / 2)[:, None], np.cos(ang / 2)[:, None]], axis=1)
            q = A._quat_mul(np.tile(rest[bone, 0:4].astype(np.float64), (4, 1)), dq)
            tracks.append(dict(bone=bone, channel=A.ROTATION, interpolation=A.LINEAR, loop_wrap=1,
                               times=np.array([0.0, 0.3, 0.6, 0.9]) * L, values=q.astype(np.float32)))
        clips.append(dict(length=L, loop_mode=A.LOOP_LINEAR, tracks=tracks))
    return clips


def test_stream_order_sample_solve_globals(oracle, mbik, torch_dev):
    """ClipSet.sample -> Plan.solve -> Plan.pose_globals queued on one side stream with one
    synchronisation at the end, against the host pipeline: clip_sample_cpu, the oracle's solve,
    pose_globals_cpu, on the first and last skeletons."""
    torch, dev = torch_dev
    wl = W.generate(2, 64)
    parents, pins = wl.topo.parents.tolist(), wl.topo.pins.tolist()
    n, B = wl.n, len(parents)
    rest = np.ascontiguousarray(wl.pose[0])
    clips = _rig_clips(rest, 4)
    rng = np.random.default_rng(5)
    t = rng.uniform(0.0, 10.0, n)
    ci = (np.arange(n) % len(clips)).astype(np.int32)
    plan = Plan.from_workload(wl)
    with A.ClipSet(B, rest, clips) as cs:
        d_t, d_c, tg = (torch.from_numpy(x).to(dev) for x in (t, ci, wl.targets))
        pi = torch.full((n, B, 10), float(SENTINEL), dtype=torch.float32, device=dev)
        po = torch.empty_like(pi)
        d_g = torch.zeros(n * B * 12, dtype=torch.float32, device=dev)
        torch.cuda.synchronize()
        st = torch.cuda.Stream(device=dev)
        cs.sample(d_t.data_ptr(), pi.data_ptr(), n, clip_index_ptr=d_c.data_ptr(), stream=st.cuda_stream)
        plan.solve(pi.data_ptr(), tg.data_ptr(), po.data_ptr(), stream=st.cuda_stream)
        plan.pose_globals(po.data_ptr(), d_g.data_ptr(), n, stream=st.cuda_stream)
        st.synchronize()
    sampled = A.clip_sample_cpu(B, rest, clips, t, ci)
    assert np.isfinite(sampled).all() and (R.bits(sampled[0]) != R.bits(sampled[-1])).any()
    assert_same(pi.cpu().numpy(), sampled, "sampled poses")
    solved = oracle.Oracle(wl).solve(sampled, wl.targets, threads=8)
    got = po.cpu().numpy()
    assert (R.bits(solved) != R.bits(sampled)).any()
    want_g = pose_globals_cpu(parents, pins, solved)[0]
    got_g = d_g.cpu().numpy().reshape(n, B, 12)
    for s in (0, n - 1):
        assert R.same_bits(got[s], solved[s]), f"solve of skeleton {s}"
        assert R.same_bits(got_g[s], want_g[s]), f"globals of skeleton {s}"
    plan.close()


def test_argument_errors(sets, torch_dev):
    torch, dev = torch_dev
    B, n = 7, 10
    rest, clips, cs = sets(B)
    t, ci = inputs(3, n, clips, specials=False)
    d_t, d_c = torch.from_numpy(t).to(dev), torch.from_numpy(ci).to(dev)
    d_o = torch.zeros(n * B * 10 + 10, dtype=torch.float32, device=dev)

    def code(*args, **k):
        with pytest.raises(_lib.MbikError) as e:
            cs.sample(*args, **k)
        assert str(e.value)
        return e.value.code

    E = _lib.MBIK_EINVAL
    assert code(0, d_o.data_ptr(), n, clip_index_ptr=d_c.data_ptr()) == E
    assert code(d_t.data_ptr(), 0, n, clip_index_ptr=d_c.data_ptr()) == E
    assert code(d_t.data_ptr(), d_o.data_ptr(), -1, clip_index_ptr=d_c.data_ptr()) == E
    for clip in (-1, len(clips), INT32_MIN):
        assert code(d_t.data_ptr(), d_o.data_ptr(), n, clip=clip) == E
    cs.sample(0, 0, 0)                                                        # count == 0: OK, no launch
    cs.sample(d_t.data_ptr(), d_o.data_ptr(), n, clip_index_ptr=d_c.data_ptr(), clip=99)   # `clip` is unused with an index array
    torch.cuda.synchronize()
    h = d_o.cpu().numpy()
    assert R.same_bits(h[:n * B * 10].reshape(n, B, 10), A.clip_sample_cpu(B, rest, clips, t, ci)) and (h[n * B * 10:] == 0).all()
    with pytest.raises(_lib.MbikError) as e:
        A.ClipSet(B, rest, clips, device=4096)
    assert e.value.code == E
    with A.ClipSet(0, np.zeros((0, 10), np.float32), [dict(length=1.0, loop_mode=0, tracks=[])]) as empty:
        empty.sample(d_t.data_ptr(), 0, n)                                    # a rig without bones: OK, no launch
