"""mbik_clip_sample_shapes and mbik_clip_sample_shapes_layers on the GPU (the blend-shape tracks of a
clip set, sampled and layered into the weights the shaped skinning reads) against their _cpu
entries, bitwise: shape counts and batch sizes around the 256-lane block, the plain call with a
clip index array and with one clip, 1, 2, 3 and 8 layers in both modes with off / zero-weight /
invalid / non-finite records scattered through every batch, float-aligned outputs, 8-byte aligned
layer arrays, guard bands around every buffer, 2^16 lanes, a face-only set, the no-launch cases,
every argument error, and the invalid-skeleton verdict shared with mbik_clip_sample_layers."""
import numpy as np
import pytest

from many_bone_ik_amd import _lib
from many_bone_ik_amd import animation as A

from . import clip_shapes_recipe as R
from .test_gpu_parity import torch_dev  # noqa: F401 (fixture)

pytestmark = pytest.mark.gpu

SENTINEL = np.uint32(0x4B1D4B1D).view(np.float32)   # a finite float no sample produces
GUARD = 16                                           # guard skeletons on each side of every buffer
GUARD_LAYER = (0.4242, 1, 1.0)                       # a record that would sample something else, were it read
GUARD_TIME, GUARD_CLIP = 0.4242, 1
BLOCK = 256                                          # lanes a block (k_clip_shapes.hip)
LAYER_COUNTS = (1, 2, 3, 8)
BONES = 2                                            # the sets are ordinary sets too


def make(P, bones=BONES):
    rest, clips = A.synthetic_clips(300 + P, bones)
    clips = A.synthetic_shape_tracks(400 + P, P, clips)
    init = np.random.default_rng(P).uniform(-0.25, 1.25, P).astype(np.float32)
    return rest, clips, init


@pytest.fixture(scope="module")
def sets(mbik):
    """One seeded shaped clip set per shape count: (rest, clips, init, ClipSet)."""
    made = {}

    def get(P):
        if P not in made:
            rest, clips, init = make(P)
            made[P] = (rest, clips, init, A.ClipSet(BONES, rest, clips, shape_count=P, shape_init=init))
        return made[P]

    yield get
    for s in made.values():
        s[3].close()


def _banded(n_body, out_off, P):
    g, body = GUARD * P, n_body * P
    h_o = np.full(out_off + g + body + g, SENTINEL, np.float32)
    return h_o, out_off + g, out_off + g + body


def _check_out(got, h_o, lo, hi, n, P):
    assert R.same_bits(got[:lo], h_o[:lo]) and R.same_bits(got[hi:], h_o[hi:]), "guard band written"
    return got[lo:hi].reshape(n, P)


def device_plain(torch, dev, cs, P, t, ci=None, clip=0, out_off=0, stream=0):
    """Launches the plain call on device copies and returns weights [n][P].  The output starts out_off
    floats past an allocation between bands of SENTINEL; time and clip_index lie between GUARD entries
    that would sample something else; every input must come back unwritten."""
    n = t.shape[0]
    h_o, lo, hi = _banded(n, out_off, P)
    h_t = np.concatenate([np.full(GUARD, GUARD_TIME), t, np.full(GUARD, GUARD_TIME)])
    d_o, d_t = torch.from_numpy(h_o).to(dev), torch.from_numpy(h_t).to(dev)
    d_c = h_c = None
    if ci is not None:
        h_c = np.concatenate([np.full(GUARD, GUARD_CLIP, np.int32), ci.astype(np.int32), np.full(GUARD, GUARD_CLIP, np.int32)])
        d_c = torch.from_numpy(h_c).to(dev)
    torch.cuda.synchronize()
    cs.sample_shapes(d_t[GUARD:].data_ptr(), d_o[lo:].data_ptr(), n, clip_index_ptr=0 if d_c is None else d_c[GUARD:].data_ptr(),
                     clip=clip, stream=stream)
    torch.cuda.synchronize()
    assert np.array_equal(d_t.cpu().numpy().view(np.uint64), h_t.view(np.uint64)), "time written"
    assert d_c is None or np.array_equal(d_c.cpu().numpy(), h_c), "clip_index written"
    return _check_out(d_o.cpu().numpy(), h_o, lo, hi, n, P)


def device_layers(torch, dev, cs, P, layers, flags, out_off=0, layer_pad=0, stream=0):
    """The same for the layered call: GUARD_LAYER records around the layers, which start layer_pad
    bytes past an allocation."""
    n, K = layers.shape
    h_o, lo, hi = _banded(n, out_off, P)
    recs = np.empty((GUARD + n + GUARD, K), R.LAYER_DTYPE)
    recs[:] = np.array(GUARD_LAYER, R.LAYER_DTYPE)
    recs[GUARD:GUARD + n] = layers
    h_l = np.zeros(layer_pad + recs.nbytes, np.uint8)
    h_l[layer_pad:] = recs.reshape(-1).view(np.uint8)
    d_o, d_l = torch.from_numpy(h_o).to(dev), torch.from_numpy(h_l).to(dev)
    assert d_l.data_ptr() % 16 == 0 and d_o.data_ptr() % 16 == 0
    torch.cuda.synchronize()
    cs.sample_shapes_layers(d_l.data_ptr() + layer_pad + GUARD * K * 16, d_o[lo:].data_ptr(), n, K, flags=flags, stream=stream)
    torch.cuda.synchronize()
    assert np.array_equal(d_l.cpu().numpy(), h_l), "layers written"
    return _check_out(d_o.cpu().numpy(), h_o, lo, hi, n, P)


def assert_same(got, want, what=""):
    bad = np.nonzero(R.bits(got) != R.bits(want))
    assert got.shape == want.shape and bad[0].size == 0, (
        f"{what}: {bad[0].size} weights differ; first: skeleton {bad[0][0]} shape {bad[1][0]}: "
        f"got {got[bad[0][0], bad[1][0]]!r}, want {want[bad[0][0], bad[1][0]]!r}")
    assert not (R.bits(got) == R.bits(np.array([SENTINEL]))[0]).any(), f"{what}: output left unwritten"


# (shapes, count): 1 lane in all; 255, 256 and 257 lanes in all, as one skeleton and as many; several
# blocks with a partial last one, at small and large shape counts; a block boundary inside a skeleton
SHAPES = [(1, 1), (1, BLOCK - 1), (1, BLOCK + 1), (5, 51), (5, 130), (52, 5), (255, 1), (256, 1), (257, 1), (255, 3), (300, 2)]


@pytest.mark.parametrize("P,n", SHAPES, ids=[f"{p}x{n}" for p, n in SHAPES])
def test_plain_matches_cpu_entry(sets, torch_dev, P, n):
    torch, dev = torch_dev
    _, clips, init, cs = sets(P)
    t, ci = R.random_times(600 + 10 * P + n, n, clips, specials=n >= 3)
    want = A.clip_sample_shapes_cpu(P, clips, t, clip_index=ci, shape_init=init)
    assert_same(device_plain(torch, dev, cs, P, t, ci), want, "clip_index")
    for clip in range(len(clips)):
        assert_same(device_plain(torch, dev, cs, P, t, clip=clip), A.clip_sample_shapes_cpu(P, clips, t, clip=clip, shape_init=init),
                    f"clip={clip}")


@pytest.mark.parametrize("P,n", SHAPES, ids=[f"{p}x{n}" for p, n in SHAPES])
def test_layered_matches_cpu_entry(sets, torch_dev, P, n):
    torch, dev = torch_dev
    _, clips, init, cs = sets(P)
    for K in LAYER_COUNTS:
        layers = R.random_layers(700 + 10 * P + K, n, K, clips, specials=n >= 3)
        for flags in (0, R.NORMALIZE):
            want = A.clip_sample_shapes_layers_cpu(P, clips, layers, flags, shape_init=init)
            assert_same(device_layers(torch, dev, cs, P, layers, flags), want, f"K={K} flags={flags}")


def test_a_shaped_set_without_shape_tracks(mbik, torch_dev):
    """The shape tables' edge layout: P = 1 and no shape track in any clip, so the key section holds the spare record only;
    every weight is the shape's init, plain and layered, on the device as on the host."""
    torch, dev = torch_dev
    rest, clips = A.synthetic_clips(301, BONES)
    init = np.array([0.625], np.float32)
    t, ci = np.array([0.0, 0.3, 0.9, 2.5, -1.0]), np.array([0, 1, 2, 1, 0], np.int32)
    want = A.clip_sample_shapes_cpu(1, clips, t, clip_index=ci, shape_init=init)
    assert R.same_bits(want, np.full((5, 1), 0.625, np.float32))
    with A.ClipSet(BONES, rest, clips, shape_count=1, shape_init=init) as cs:
        assert_same(device_plain(torch, dev, cs, 1, t, ci), want, "no shape tracks")
        layers = R.random_layers(5, 5, 2, clips, specials=False)
        assert_same(device_layers(torch, dev, cs, 1, layers, 0), A.clip_sample_shapes_layers_cpu(1, clips, layers, 0, shape_init=init), "layered")


def test_specials_are_in_the_batches_and_guards_would_change_the_result(sets):
    """The recipe's statistics of the 5 x 130 batches above: every branch is there; and were a guard
    entry read in place of a skeleton's own, its weights would differ."""
    _, clips, init, _ = sets(5)
    for flags in (0, R.NORMALIZE):
        total = {}
        for K in LAYER_COUNTS:
            layers = R.random_layers(700 + 50 + K, 130, K, clips)
            assert np.isnan(layers["time"]).any() and np.isnan(layers["weight"]).any()
            for k, v in R.expected_layers(5, clips, layers, flags, init=init)[1].items():
                total[k] = total.get(k, 0) + v
        for k in ("layers_off", "skipped_by_weight", "untracked_layers", "accumulated", "invalid_skeletons", "nonfinite"):
            assert total[k] >= 3, (k, total)
    layers = R.random_layers(700 + 50 + 3, 130, 3, clips)
    t, ci = R.random_times(600 + 50 + 130, 130, clips)
    _, stats = R.expected(5, clips, t, ci, init=init)
    for k in R.PLAIN_BRANCHES:
        assert stats[k] >= 3, (k, stats)
    want = A.clip_sample_shapes_layers_cpu(5, clips, layers, 0, shape_init=init)
    guard = np.empty_like(layers)
    guard[:] = np.array(GUARD_LAYER, R.LAYER_DTYPE)
    swapped = A.clip_sample_shapes_layers_cpu(5, clips, guard, 0, shape_init=init)
    assert (R.bits(swapped) != R.bits(want)).any(axis=1).all()
    swapped = A.clip_sample_shapes_cpu(5, clips, np.full(130, GUARD_TIME), clip=GUARD_CLIP, shape_init=init)
    assert (R.bits(swapped) != R.bits(A.clip_sample_shapes_cpu(5, clips, t, clip_index=ci, shape_init=init))).any(axis=1).all()


@pytest.mark.parametrize("out_off,layer_pad", [(1, 0), (2, 8), (3, 16), (0, 8), (1, 24)], ids=str)
def test_alignment(sets, torch_dev, out_off, layer_pad):
    """weights_out one to three floats past a 16-byte boundary; layers one record into an allocation
    and 8 bytes into one (the 8-byte aligned path)."""
    torch, dev = torch_dev
    _, clips, init, cs = sets(5)
    t, ci = R.random_times(41, 130, clips)
    assert_same(device_plain(torch, dev, cs, 5, t, ci, out_off=out_off), A.clip_sample_shapes_cpu(5, clips, t, clip_index=ci, shape_init=init))
    for K in (2, 3):
        layers = R.random_layers(40 + K, 130, K, clips)
        for flags in (0, R.NORMALIZE):
            assert_same(device_layers(torch, dev, cs, 5, layers, flags, out_off=out_off, layer_pad=layer_pad),
                        A.clip_sample_shapes_layers_cpu(5, clips, layers, flags, shape_init=init), f"K={K} flags={flags}")


def test_many_blocks(sets, torch_dev):
    """2^16 lanes (1,261 x 52 = 65,572) in one call: 257 blocks."""
    torch, dev = torch_dev
    _, clips, init, cs = sets(52)
    t, ci = R.random_times(79, 1261, clips)
    assert_same(device_plain(torch, dev, cs, 52, t, ci), A.clip_sample_shapes_cpu(52, clips, t, clip_index=ci, shape_init=init))
    layers = R.random_layers(78, 1261, 2, clips)
    for flags in (0, R.NORMALIZE):
        assert_same(device_layers(torch, dev, cs, 52, layers, flags),
                    A.clip_sample_shapes_layers_cpu(52, clips, layers, flags, shape_init=init), f"flags={flags}")


def test_face_only_set_and_null_init(mbik, torch_dev):
    """bone_count == 0 with shapes is a valid set; a NULL init is all +0."""
    torch, dev = torch_dev
    _, clips, _ = make(5, bones=0)
    with A.ClipSet(0, np.zeros((0, 10), np.float32), clips, shape_count=5) as cs:
        t, ci = R.random_times(8, 40, clips)
        assert_same(device_plain(torch, dev, cs, 5, t, ci), A.clip_sample_shapes_cpu(5, clips, t, clip_index=ci))
        layers = R.random_layers(9, 40, 3, clips)
        assert_same(device_layers(torch, dev, cs, 5, layers, R.NORMALIZE), A.clip_sample_shapes_layers_cpu(5, clips, layers, R.NORMALIZE))
        d = torch.zeros(64, dtype=torch.float64, device=dev)
        cs.sample(d.data_ptr(), d.data_ptr(), 4)                      # the pose calls on it: no bones, no launch
        cs.sample_layers(d.data_ptr(), d.data_ptr() + 256, 4, 1)


def test_a_shaped_set_samples_poses_as_before_and_shares_the_invalid_verdict(sets, torch_dev):
    """mbik_clip_sample_layers on a shaped set gives the bits of the pose entry, and the same record
    array marks the same skeletons invalid in the pose call and in the shape call."""
    torch, dev = torch_dev
    rest, clips, init, cs = sets(5)
    layers = R.random_layers(123, 200, 3, clips, specials=False)      # finite times and weights: a NaN means invalid
    rng = np.random.default_rng(124)
    for s in rng.choice(200, 24, replace=False):
        layers["clip"][s, rng.integers(0, 3)] = (len(clips), -2, -2 ** 31, 2 ** 31 - 1)[rng.integers(0, 4)]
    d_l = torch.from_numpy(layers.reshape(-1).view(np.uint8)).to(dev)
    d_p = torch.full((200, BONES, 10), float(SENTINEL), dtype=torch.float32, device=dev)
    d_w = torch.full((200, 5), float(SENTINEL), dtype=torch.float32, device=dev)
    torch.cuda.synchronize()
    cs.sample_layers(d_l.data_ptr(), d_p.data_ptr(), 200, 3, flags=R.NORMALIZE)
    cs.sample_shapes_layers(d_l.data_ptr(), d_w.data_ptr(), 200, 3, flags=R.NORMALIZE)
    torch.cuda.synchronize()
    pose, w = d_p.cpu().numpy(), d_w.cpu().numpy()
    assert R.same_bits(pose, A.clip_sample_layers_cpu(BONES, rest, clips, layers, R.NORMALIZE))
    clip = layers["clip"].astype(np.int64)
    invalid = ((clip != R.OFF) & ((clip < 0) | (clip >= len(clips)))).any(axis=1)
    assert invalid.sum() == 24
    assert np.array_equal((R.bits(pose) == 0x7FC00000).all(axis=(1, 2)), invalid) and np.isfinite(pose[~invalid]).all()
    assert np.array_equal((R.bits(w) == 0x7FC00000).all(axis=1), invalid) and np.isfinite(w[~invalid]).all()
    assert R.same_bits(w, A.clip_sample_shapes_layers_cpu(5, clips, layers, R.NORMALIZE, shape_init=init))


def test_nothing_to_do_and_argument_errors(sets, torch_dev):
    torch, dev = torch_dev
    P, n, K = 5, 10, 2
    rest, clips, init, cs = sets(P)
    layers = R.random_layers(3, n, K, clips, specials=False)
    t, ci = R.random_times(4, n, clips, specials=False)
    d_l = torch.from_numpy(layers.reshape(-1).view(np.uint8)).to(dev)
    d_t, d_c = torch.from_numpy(t).to(dev), torch.from_numpy(ci).to(dev)
    d_o = torch.full((n * P + 10,), float(SENTINEL), dtype=torch.float32, device=dev)
    torch.cuda.synchronize()
    o, l, tp, cp = d_o.data_ptr(), d_l.data_ptr(), d_t.data_ptr(), d_c.data_ptr()
    cs.sample_shapes(tp, o, 0, clip_index_ptr=cp)                      # count == 0: OK, no launch
    cs.sample_shapes(0, 0, 0)
    cs.sample_shapes_layers(l, o, 0, K)
    cs.sample_shapes_layers(0, 0, 0, K)
    torch.cuda.synchronize()
    assert (R.bits(d_o.cpu().numpy()) == R.bits(np.array([SENTINEL]))[0]).all()

    def code(fn, *args, **k):
        with pytest.raises(_lib.MbikError) as e:
            fn(*args, **k)
        assert str(e.value)
        return e.value.code

    E = _lib.MBIK_EINVAL
    plain, lay = cs.sample_shapes, cs.sample_shapes_layers
    assert code(plain, 0, o, n) == E and code(plain, tp, 0, n) == E and code(plain, tp, o, -1) == E
    assert code(plain, tp, o, n, clip=len(clips)) == E and code(plain, tp, o, n, clip=-1) == E
    assert code(plain, tp, tp + 8, 2) == E                                  # weights_out overlaps time
    assert code(plain, tp, cp + 4, 2, clip_index_ptr=cp) == E               # weights_out overlaps clip_index
    assert code(lay, 0, o, n, K) == E and code(lay, l, 0, n, K) == E and code(lay, l, o, -1, K) == E
    for bad_k in (0, -1, 9):
        assert code(lay, l, o, n, bad_k) == E
    assert code(lay, l, o, n, K, flags=2) == E
    assert code(lay, l + 4, o, n - 1, K) == E
    assert code(lay, l, l + 8, 1, 1) == E                                   # weights_out overlaps layers
    with A.ClipSet(BONES, rest, clips) as unshaped:                         # a set without shapes
        assert code(unshaped.sample_shapes, tp, o, n) == E and code(unshaped.sample_shapes_layers, l, o, n, K) == E
        assert code(unshaped.sample_shapes, tp, o, 0) == E
    # mbik_clipset_create_shaped's own checks, on the device path
    for bad in (dict(shape=P), dict(interpolation=2), dict(times=[0.5, 0.5], values=[0.0, 1.0]), dict(times=[0.0, 1e9], values=[0.0, 1.0])):
        broken = [dict(c) for c in clips]
        broken[0]["shape_tracks"] = [dict(dict(shape=0, interpolation=1, loop_wrap=1, times=[0.0], values=[0.5]), **bad)]
        assert code(A.ClipSet, BONES, rest, broken, shape_count=P) == E
    dup = [dict(c) for c in clips]
    dup[0]["shape_tracks"] = [dict(shape=1, interpolation=1, loop_wrap=1, times=[0.0], values=[0.5])] * 2
    assert code(A.ClipSet, BONES, rest, dup, shape_count=P) == E
    assert code(A.ClipSet, BONES, rest, clips, shape_count=-1) == E
    # after all that the set still works, and writes its own range only
    plain(tp, o, n, clip_index_ptr=cp)
    torch.cuda.synchronize()
    h = d_o.cpu().numpy()
    assert R.same_bits(h[:n * P].reshape(n, P), A.clip_sample_shapes_cpu(P, clips, t, clip_index=ci, shape_init=init))
    assert (R.bits(h[n * P:]) == R.bits(np.array([SENTINEL]))[0]).all()
    lay(l, o, n, K)
    torch.cuda.synchronize()
    h = d_o.cpu().numpy()
    assert R.same_bits(h[:n * P].reshape(n, P), A.clip_sample_shapes_layers_cpu(P, clips, layers, 0, shape_init=init))
    assert (R.bits(h[n * P:]) == R.bits(np.array([SENTINEL]))[0]).all()
