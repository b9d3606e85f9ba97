"""mbik_clip_sample_layers on the GPU (AnimationMixer's blend of up to 8 clip layers a skeleton)
against mbik_clip_sample_layers_cpu, bitwise: bone counts and batch sizes around the 256-bone block,
1, 2, 3 and 8 layers, both modes, off / zero-weight / invalid / non-finite layers scattered through
every batch, float-aligned outputs, 16- and 8-byte aligned layer arrays, guard bands around every
buffer, both libm variants, 2^16 bones, and stream order in front of a solve and mbik_pose_globals."""
import numpy as np
import pytest

from many_bone_ik_amd import _lib
from many_bone_ik_amd import animation as A
from many_bone_ik_amd import workloads as W
from many_bone_ik_amd.solver import Plan

from . import clip_layers_recipe as R
from .test_gpu_clip_sample import _rig_clips
from .test_gpu_parity import torch_dev  # noqa: F401 (fixture)

pytestmark = pytest.mark.gpu

SENTINEL = np.uint32(0x4B1D4B1D).view(np.float32)   # a finite float no sample produces
GUARD = 16                                           # guard skeletons on each side of the output and of the layer array
GUARD_LAYER = (0.4242, 1, 1.0)                       # a record that would sample something else, were it read
BLOCK = 256                                          # bones a block (k_clip.hip)
LAYER_COUNTS = (1, 2, 3, 8)


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


def device_layers(torch, dev, cs, B, layers, flags, out_off=0, layer_pad=0, stream=0):
    """Launches on device copies and returns pose_out [n][B][10].  pose_out starts out_off floats and
    the layer array layer_pad bytes past an allocation; each has GUARD skeletons' worth of guard
    entries on both sides -- SENTINEL around (and in) the output, GUARD_LAYER records around the
    layers -- which must come back untouched."""
    n, K = layers.shape
    g, body = GUARD * B * 10, n * B * 10
    h_o = np.full(out_off + g + body + g, SENTINEL, np.float32)
    recs = np.empty((GUARD + n + GUARD, K), R.LAYER_DTYPE)
    recs[:] = np.array(GUARD_LAYER, R.LAYER_DTYPE)
    recs[GUARD:GUARD + n] = layers
    h_l = np.zeros(layer_pad + recs.nbytes, np.uint8)
    h_l[layer_pad:] = recs.reshape(-1).view(np.uint8)
    d_o, d_l = torch.from_numpy(h_o).to(dev), torch.from_numpy(h_l).to(dev)
    assert d_l.data_ptr() % 16 == 0
    torch.cuda.synchronize()
    cs.sample_layers(d_l.data_ptr() + layer_pad + GUARD * K * 16, d_o[out_off + g:].data_ptr(), n, K, flags=flags, stream=stream)
    torch.cuda.synchronize()
    got = d_o.cpu().numpy()
    lo, hi = out_off + g, out_off + g + body
    assert R.same_bits(got[:lo], h_o[:lo]) and R.same_bits(got[hi:], h_o[hi:]), "guard band written"
    assert np.array_equal(d_l.cpu().numpy(), h_l), "layers written"
    return got[lo:hi].reshape(n, B, 10)


def assert_same(got, want, what=""):
    bad = np.nonzero((R.bits(got) != R.bits(want)).any(axis=2))
    assert bad[0].size == 0, (f"{what}: {bad[0].size} bones differ; first: skeleton {bad[0][0]} bone {bad[1][0]}: "
                              f"got {got[bad[0][0], bad[1][0]]}, want {want[bad[0][0], bad[1][0]]}")
    assert not (R.bits(got) == R.bits(np.array([SENTINEL]))[0]).any(), f"{what}: output left unwritten"


# (bones, count): 1 bone in all; 255, 256 and 257 bones in all, as one skeleton and as many; three
# blocks with a partial last one, at small and large bone counts
SHAPES = [(1, 1), (1, BLOCK - 1), (1, BLOCK + 1), (5, 51), (5, 130), (255, 1), (256, 1), (257, 1), (255, 3), (300, 2)]


@pytest.mark.parametrize("B,n", SHAPES, ids=[f"{b}x{n}" for b, n in SHAPES])
def test_device_matches_cpu_entry(sets, torch_dev, B, n):
    torch, dev = torch_dev
    rest, clips, cs = sets(B)
    for K in LAYER_COUNTS:
        layers = R.random_layers(700 + 10 * B + K, n, K, clips, specials=n >= 3)
        for flags in (0, R.NORMALIZE):
            want = A.clip_sample_layers_cpu(B, rest, clips, layers, flags)
            assert_same(device_layers(torch, dev, cs, B, layers, flags), want, f"K={K} flags={flags}")


def test_specials_are_in_the_batches_and_guards_would_change_the_result(sets):
    """The recipe's statistics of one of the batches above: every branch is there; and were a guard
    record read in place of a skeleton's own, its pose would differ."""
    rest, clips, _ = sets(5)
    layers = R.random_layers(700 + 50 + 3, 130, 3, clips)
    for flags in (0, R.NORMALIZE):
        _, stats = R.expected(5, rest, clips, layers, flags)
        for k in ("layers_off", "skipped_by_weight", "untracked", "accumulated", "invalid_skeletons", "slerp_trig"):
            assert stats[k] >= 3, (k, stats)
    assert np.isnan(layers["time"]).any() and np.isnan(layers["weight"]).any()
    want = A.clip_sample_layers_cpu(5, rest, clips, layers, 0)
    guard = np.empty_like(layers)
    guard[:] = np.array(GUARD_LAYER, R.LAYER_DTYPE)
    swapped = A.clip_sample_layers_cpu(5, rest, clips, guard, 0)
    assert (R.bits(swapped) != R.bits(want)).any(axis=(1, 2)).all()


@pytest.mark.parametrize("out_off,layer_pad", [(1, 0), (0, 16), (0, 8), (1, 8), (3, 16), (2, 24)], ids=str)
def test_alignment(sets, torch_dev, out_off, layer_pad):
    """pose_out one to three floats past a 16-byte boundary; layers one record into an allocation
    (still 16-byte aligned) and 8 bytes into one (the 8-byte aligned path)."""
    torch, dev = torch_dev
    rest, clips, cs = sets(5)
    for K in (2, 3):
        layers = R.random_layers(40 + K, 130, K, clips)
        for flags in (0, R.NORMALIZE):
            assert_same(device_layers(torch, dev, cs, 5, layers, flags, out_off=out_off, layer_pad=layer_pad),
                        A.clip_sample_layers_cpu(5, rest, clips, layers, flags), f"K={K} flags={flags}")


def test_both_libm_variants(sets, torch_dev):
    torch, dev = torch_dev
    for lv in (0, 1):
        rest, clips, cs = sets(32, lv)
        layers = R.random_layers(33, 24, 3, clips)
        _, stats = R.expected(32, rest, clips, layers, R.NORMALIZE)
        assert stats["slerp_trig"] >= 200, stats
        for flags in (0, R.NORMALIZE):
            assert_same(device_layers(torch, dev, cs, 32, layers, flags),
                        A.clip_sample_layers_cpu(32, rest, clips, layers, flags, libm_variant=lv), f"variant {lv} flags={flags}")


def test_many_blocks(sets, torch_dev):
    """2^16 bones (2,048 x 32) in one call at K = 2: 256 blocks."""
    torch, dev = torch_dev
    rest, clips, cs = sets(32)
    layers = R.random_layers(78, 2048, 2, clips)
    for flags in (0, R.NORMALIZE):
        assert_same(device_layers(torch, dev, cs, 32, layers, flags), A.clip_sample_layers_cpu(32, rest, clips, layers, flags))


def test_stream_order_sample_layers_solve_globals(mbik, torch_dev):
    """ClipSet.sample_layers -> Plan.solve -> Plan.pose_globals queued on one side stream with one
    synchronisation at the end, against the same solve and globals run from the CPU-sampled poses."""
    torch, dev = torch_dev
    wl = W.generate(2, 64)
    n, B = wl.n, len(wl.topo.parents.tolist())
    rest = np.ascontiguousarray(wl.pose[0])
    clips = _rig_clips(rest, 4)
    rng = np.random.default_rng(5)
    w = rng.uniform(0.0, 1.0, n).astype(np.float32)
    layers = R.pack(rng.uniform(0.0, 10.0, (n, 2)), np.tile([0, 1], (n, 1)), np.stack([w, np.float32(1) - w], axis=1))
    sampled = A.clip_sample_layers_cpu(B, rest, clips, layers, R.NORMALIZE)
    assert np.isfinite(sampled).all() and (R.bits(sampled[0]) != R.bits(sampled[-1])).any()
    plan = Plan.from_workload(wl)
    with A.ClipSet(B, rest, clips) as cs:
        d_l = torch.from_numpy(layers.reshape(-1).view(np.uint8)).to(dev)
        tg = torch.from_numpy(wl.targets).to(dev)
        st = torch.cuda.Stream(device=dev)

        def chain(pi, sample):
            po = torch.empty_like(pi)
            d_g = torch.zeros(n * B * 12, dtype=torch.float32, device=dev)
            torch.cuda.synchronize()
            if sample:
                cs.sample_layers(d_l.data_ptr(), pi.data_ptr(), n, 2, flags=R.NORMALIZE, stream=st.cuda_stream)
            plan.solve(pi.data_ptr(), tg.data_ptr(), po.data_ptr(), stream=st.cuda_stream)
            plan.pose_globals(po.data_ptr(), d_g.data_ptr(), n, stream=st.cuda_stream)
            st.synchronize()
            return pi.cpu().numpy(), po.cpu().numpy(), d_g.cpu().numpy()

        got = chain(torch.full((n, B, 10), float(SENTINEL), dtype=torch.float32, device=dev), True)
        want = chain(torch.from_numpy(sampled).to(dev), False)
    assert_same(got[0], sampled, "sampled poses")
    assert (R.bits(want[1]) != R.bits(sampled)).any()
    assert R.same_bits(got[1], want[1]), "solved poses"
    assert R.same_bits(got[2], want[2]), "globals"
    plan.close()


def test_nothing_to_do_and_argument_errors(sets, torch_dev):
    torch, dev = torch_dev
    B, n, K = 5, 10, 2
    rest, clips, cs = sets(B)
    layers = R.random_layers(3, n, K, clips, specials=False)
    d_l = torch.from_numpy(layers.reshape(-1).view(np.uint8)).to(dev)
    d_o = torch.full((n * B * 10 + 10,), float(SENTINEL), dtype=torch.float32, device=dev)
    torch.cuda.synchronize()
    cs.sample_layers(d_l.data_ptr(), d_o.data_ptr(), 0, K)                 # count == 0: OK, no launch
    cs.sample_layers(0, 0, 0, K)
    with A.ClipSet(0, np.zeros((0, 10), np.float32), [dict(length=1.0, loop_mode=0, tracks=[])]) as empty:
        empty.sample_layers(d_l.data_ptr(), d_o.data_ptr(), n, K)          # a rig without bones: OK, no launch
    torch.cuda.synchronize()
    assert (R.bits(d_o.cpu().numpy()) == R.bits(np.array([SENTINEL]))[0]).all()
    assert np.array_equal(d_l.cpu().numpy(), layers.reshape(-1).view(np.uint8))

    def code(*args, **k):
        with pytest.raises(_lib.MbikError) as e:
            cs.sample_layers(*args, **k)
        assert str(e.value)
        return e.value.code

    E = _lib.MBIK_EINVAL
    assert code(0, d_o.data_ptr(), n, K) == E and code(d_l.data_ptr(), 0, n, K) == E
    assert code(d_l.data_ptr(), d_o.data_ptr(), -1, K) == E
    for bad_k in (0, -1, 9):
        assert code(d_l.data_ptr(), d_o.data_ptr(), n, bad_k) == E
    assert code(d_l.data_ptr(), d_o.data_ptr(), n, K, flags=2) == E
    assert code(d_l.data_ptr() + 4, d_o.data_ptr(), n - 1, K) == E
    assert code(d_l.data_ptr(), d_l.data_ptr() + 8, 1, 1) == E              # pose_out overlaps layers
    cs.sample_layers(d_l.data_ptr(), d_o.data_ptr(), n, K)
    torch.cuda.synchronize()
    h = d_o.cpu().numpy()
    assert R.same_bits(h[:n * B * 10].reshape(n, B, 10), A.clip_sample_layers_cpu(B, rest, clips, layers, 0))
    assert (R.bits(h[n * B * 10:]) == R.bits(np.array([SENTINEL]))[0]).all()
