"""What mbik_clip_sample_layers_cpu means, against an independent float64 model of the blend factor
and the accumulation (tests/clip_layers_recipe.py model64), fed the float32 layer samples.

Positions and scales: |entry - model| <= 4 K 2^-24 S per component, S = |I| + sum_l |blend_l|
(|x_l| + |I|) in float64 with the float32 blend_l.  Derivation: each accumulated layer rounds three
times -- x - I, the product with blend_l, the sum onto acc -- and each rounding is at most 2^-24 of
its result, whose magnitude is bounded by S (|x - I| <= |x| + |I|, the product by |blend| times that,
every partial sum by S itself); K layers give 3 K 2^-24 S, and the factor 4 instead of 3 covers the
second-order terms (an earlier rounding error carried through the later operations).

Rotations: the angle between the entry's quaternion and the model's.  Measured on the CPU, float32
recipe against the float64 model over the seeded cases below (72 batches, 1 to 8 layers, both modes): the
observed maximum is 6.86e-7 rad; the test allows 4 times that, 2.75e-6 rad, the margin covering
seeds not tried.  The recipe is not the code under test, and the entry equals it bitwise
(tests/test_clip_layers_cpu.py).

Weights in [0, 1] that sum to 1: the position is the weighted mean of the samples, within the same
bound -- what a user expects of a cross-fade."""
import numpy as np
import pytest

from many_bone_ik_amd import animation as A

from . import clip_layers_recipe as R

ANGLE_OBSERVED = 6.86e-7
ANGLE_BOUND = 4 * ANGLE_OBSERVED
SKELETONS = {1: 160, 5: 60, 32: 24}
CASES = [(B, K) for B in (1, 5, 32) for K in (1, 2, 3, 8)]


@pytest.mark.parametrize("B,K", CASES, ids=[f"{b}x{k}" for b, k in CASES])
def test_entry_stays_within_the_float64_meaning(mbik, B, K):
    rest, clips = A.synthetic_clips(70 + B, B)
    accumulated = 0
    for seed in range(3):
        layers = R.random_layers(5000 + 100 * B + 10 * K + seed, SKELETONS[B], K, clips, specials=False)
        for flags in (0, R.NORMALIZE):
            got = A.clip_sample_layers_cpu(B, rest, clips, layers, flags)
            model, S, blend, acc, x = R.model64(B, rest, clips, layers, flags)
            assert np.isfinite(got).all() and np.isfinite(model).all()
            accumulated += int(acc.sum())
            err = np.abs(got.astype(np.float64) - model)[:, :, 4:]
            bound = 4 * K * 2.0 ** -24 * S[:, :, 4:]
            print(f"B={B} K={K} seed={seed} flags={flags}: worst position / scale error over its bound "
                  f"{(err / bound).max():.3f}")
            assert (err <= bound).all()
            angle = R.angle_between(got[:, :, 0:4], model[:, :, 0:4])
            print(f"    worst rotation angle {angle.max():.3e} rad (bound {ANGLE_BOUND:.3e})")
            assert (angle <= ANGLE_BOUND).all()
            # a channel nothing is accumulated on keeps the rest pose: model and entry agree exactly
            idle = ~acc.any(axis=1)
            for ch in (0, 1, 2):
                sl = R.C.SLICE[ch]
                assert np.array_equal(got[:, :, sl][idle[:, :, ch]], model[:, :, sl][idle[:, :, ch]].astype(np.float32))
    assert accumulated > 100


@pytest.mark.parametrize("K", (2, 3, 8))
def test_weights_that_sum_to_one_give_the_weighted_mean(mbik, K):
    """Every position channel tracked by every clip; weights k / 256 with sum 256, so their sum is 1
    exactly and I's coefficient 1 - sum w vanishes: the blend is the samples' weighted mean."""
    B, n = 5, 60
    rest, clips = A.synthetic_clips(90, B, key_counts=(1, 2, 3, 17))
    rng = np.random.default_rng(K)
    ci = rng.integers(0, len(clips), (n, K)).astype(np.int32)
    t = rng.uniform(0.0, 3.0, (n, K))
    cuts = np.sort(rng.integers(0, 257, (n, K - 1)), axis=1)
    k = np.diff(np.concatenate([np.zeros((n, 1), int), cuts, np.full((n, 1), 256)], axis=1), axis=1)
    w = (k / 256.0).astype(np.float32)
    assert (w.astype(np.float64).sum(axis=1) == 1.0).all() and (w >= 0).all() and (w <= 1).all()
    layers = R.pack(t, ci, w)
    got = A.clip_sample_layers_cpu(B, rest, clips, layers, 0)
    x = np.stack([A.clip_sample_cpu(B, rest, clips, t[:, l], ci[:, l]) for l in range(K)], axis=1).astype(np.float64)
    w64 = w.astype(np.float64)[:, :, None, None]
    mean = (w64 * x[:, :, :, 4:7]).sum(axis=1)
    I = np.abs(rest[None, :, 4:7].astype(np.float64))
    S = I + (np.abs(w64) * (np.abs(x[:, :, :, 4:7]) + I[:, None])).sum(axis=1)
    err = np.abs(got[:, :, 4:7].astype(np.float64) - mean)
    print(f"K={K}: worst error over its bound {(err / (4 * K * 2.0 ** -24 * S)).max():.3f}")
    assert (err <= 4 * K * 2.0 ** -24 * S).all()
    assert (np.abs(mean - rest[None, :, 4:7]) > 1e-3).any()
