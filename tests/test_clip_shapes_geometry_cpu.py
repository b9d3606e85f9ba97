"""What the blend-shape sampler's floats mean, against an independent float64 model (host only):

    1. a plain linear sample lies within 4 * 2^-24 * (|V[a]| + |V[b]|) of V[a] + (V[b] - V[a]) * c in
       float64, c the float32 weight: three roundings (the difference, the product, the sum), each
       at most 2^-24 of a magnitude bounded by |V[a]| + |V[b]| (c is in [0, 1]), and 4 in place of 3
       for the second-order terms;
    2. a layered result lies within DESIGN.md §20's 4 K 2^-24 S of I + sum (x_l - I) blend_l in
       float64, S = |I| + sum |blend_l| (|x_l| + |I|), fed the float32 samples and blend factors;
    3. with weights in [0, 1] that sum to 1, in normalize mode, on shapes every layer's clip tracks,
       the result is the samples' weighted mean sum w_l x_l / sum w_l within the same bound.

The worst used fraction of each bound is printed (DESIGN.md §23 records them)."""
import numpy as np
import pytest

from many_bone_ik_amd import animation as A

from . import clip_layers_recipe as LR
from . import clip_recipe as C
from . import clip_shapes_recipe as R

D = np.float64
U = 2.0 ** -24
P = 12


@pytest.fixture(scope="module")
def tracks(mbik):
    _, clips = A.synthetic_clips(31, 1)
    clips = A.synthetic_shape_tracks(32, P, clips)
    init = np.random.default_rng(33).uniform(-0.25, 1.25, P).astype(np.float32)
    return clips, init


def test_plain_linear_sample_is_the_lerp_of_its_two_keys(tracks):
    clips, init = tracks
    t, ci = R.random_times(34, 1500, clips, specials=False)
    got = A.clip_sample_shapes_cpu(P, clips, t, clip_index=ci, shape_init=init)
    index = R.index_tracks(clips)
    worst, checked = 0.0, 0
    for s in range(t.shape[0]):
        clip = clips[ci[s]]
        length = D(clip["length"])
        tp = C.sample_time(t[s], length, clip["loop_mode"])
        for j, (T, V, linear, wrap) in index[ci[s]].items():
            i = int(np.searchsorted(T, tp, side="right")) - 1
            a, b, c, _ = C.pick(T, T.shape[0], i, wrap, linear, tp, length)
            if b is None:
                assert got[s, j] == V[a]
                continue
            assert 0.0 <= c <= 1.0
            model = D(V[a]) + (D(V[b]) - D(V[a])) * D(c)
            bound = 4 * U * (abs(D(V[a])) + abs(D(V[b])))
            err = abs(D(got[s, j]) - model)
            assert err <= bound, (s, j, got[s, j], model, err, bound)
            if bound > 0:
                worst = max(worst, err / bound)
            checked += 1
    print(f"plain linear samples: {checked} checked, worst used fraction of 4 * 2^-24 * (|Va| + |Vb|): {worst:.3f}")
    assert checked >= 2000


def _model(clips, init, layers, flags):
    """(model64 [n][P], S [n][P], accumulated [n][K][P], x [n][K][P]) of finite, valid layers."""
    n, K = layers.shape
    tracked = np.array([[j in d for j in range(P)] for d in R.index_tracks(clips)])
    on = layers["clip"] != R.OFF
    w = LR.clamp_weight(layers["weight"])
    x = np.stack([A.clip_sample_shapes_cpu(P, clips, layers["time"][:, l], clip_index=np.where(on[:, l], layers["clip"][:, l], 0),
                                           shape_init=init) for l in range(K)], axis=1)
    contrib = on[:, :, None] & tracked[np.where(on, layers["clip"], 0)]
    wb = np.broadcast_to(w[:, :, None], contrib.shape)
    if flags & R.NORMALIZE:
        total = np.zeros((n, P), np.float32)
        for l in range(K):
            total = np.where(contrib[:, l], total + wb[:, l], total)
        with np.errstate(all="ignore"):
            blend = (wb / total[:, None]).astype(np.float32)
        acc = contrib & ~(np.abs(total) < R.EPS)[:, None]
    else:
        blend, acc = wb.astype(np.float32), contrib.copy()
    with np.errstate(invalid="ignore"):
        acc &= ~(np.abs(blend) < R.EPS)
    I = init.astype(D)[None, None, :]
    b64 = np.where(acc, blend.astype(D), 0.0)
    model = I[:, 0] + ((x.astype(D) - I) * b64).sum(axis=1)
    S = np.abs(I[:, 0]) + (np.abs(b64) * (np.abs(x.astype(D)) + np.abs(I))).sum(axis=1)
    return model, S, acc, x


@pytest.mark.parametrize("K", (1, 2, 3, 8))
def test_layered_result_is_the_weighted_sum_of_offsets(tracks, K):
    clips, init = tracks
    layers = R.random_layers(35 + K, 300, K, clips, specials=False)
    for flags in (0, R.NORMALIZE):
        got = A.clip_sample_shapes_layers_cpu(P, clips, layers, flags, shape_init=init)
        model, S, acc, _ = _model(clips, init, layers, flags)
        any_acc = acc.any(axis=1)
        assert np.isfinite(got).all() and any_acc.sum() >= 500
        assert R.same_bits(got[~any_acc], np.broadcast_to(init, got.shape)[~any_acc])
        frac = np.abs(got.astype(D) - model)[any_acc] / (4 * K * U * S[any_acc])
        print(f"layered K={K} flags={flags}: {any_acc.sum()} checked, worst used fraction of 4 K 2^-24 S: {frac.max():.3f}")
        assert frac.max() <= 1.0


@pytest.mark.parametrize("K", (2, 3, 8))
def test_normalized_weights_summing_to_one_give_the_weighted_mean(tracks, K):
    clips, init = tracks
    rng = np.random.default_rng(36 + K)
    n = 300
    ci = rng.integers(0, len(clips), (n, K)).astype(np.int32)
    t = rng.uniform(-1.0, 3.0, (n, K)) * np.array([c["length"] for c in clips])[ci]
    w = rng.dirichlet(np.ones(K), n).astype(np.float32)
    layers = R.pack(t, ci, w)
    got = A.clip_sample_shapes_layers_cpu(P, clips, layers, R.NORMALIZE, shape_init=init)
    _, S, acc, x = _model(clips, init, layers, R.NORMALIZE)
    every = acc.all(axis=1)   # every layer's clip tracks the shape, none skipped by weight
    assert every.sum() >= 300
    w64 = w.astype(D)[:, :, None]
    mean = (w64 * x.astype(D)).sum(axis=1) / w64.sum(axis=1)
    frac = np.abs(got.astype(D) - mean)[every] / (4 * K * U * S[every])
    print(f"weighted mean K={K}: {every.sum()} checked, worst used fraction of 4 K 2^-24 S: {frac.max():.3f}")
    assert frac.max() <= 1.0
