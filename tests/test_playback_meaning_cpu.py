"""What the playback numbers mean, against exact and float64 arithmetic (the bitwise tests pin the
operations, these pin their sense): a looping clip ends where the exact sum of its steps ends; a
cross-fade's weight runs down linearly over the blend time and the weights add up to 1; the records
drive root motion through loop seams without losing or doubling one; and a clip that ends shows its
exact end before its successor shows its exact start.  u = 2^-24 and v = 2^-53 are the relative
errors of one float32 and one float64 rounding."""
from fractions import Fraction

import numpy as np
import pytest

from many_bone_ik_amd import animation as A

from . import playback_recipe as R
from . import root_motion_recipe as RM

U, V = 2.0 ** -24, 2.0 ** -53
REST1 = np.array([[0, 0, 0, 1, 0, 0, 0, 1, 1, 1]], np.float32)   # one bone, the root


def play(clips, n, delta, speed_scale=1.0, K=2, cmds=None, state=None, **desc):
    """n frames from an empty crowd of one (or `state`), `cmds` in the first: a list of the frames' outputs."""
    st, fl = state if state is not None else A.empty_state(1, K)
    out = []
    for frame in range(n):
        st, fl, layers, prev, ev = A.playback_advance_cpu(clips, st, fl, delta, speed_scale, cmds=cmds if frame == 0 else None, **desc)
        out.append((st, fl, layers, prev, ev))
    return out


@pytest.mark.parametrize("seed", range(8))
def test_a_looping_clip_ends_at_the_exact_sum_of_its_steps(mbik, seed):
    """N frames of a LOOP_LINEAR clip from `start`: pos = fmod(start + N * g * speed, L), compared on
    the circle of length L against exact rationals.  A frame rounds three times: the step g * speed
    (|step| * v), the sum pos + step (at most (L + |step|) * v) and, for a negative remainder,
    v + L (at most L * v); fmod is exact.  Bound: N * 3 * (L + |step|) * v, plus g's own rounding
    N * |step| * v -- 4 * N * (L + |step|) * v in all."""
    rng = np.random.default_rng(seed)
    L, start = float(rng.uniform(0.5, 3.0)), float(rng.uniform(0.0, 0.5))
    speed, scale = float(np.float32(rng.choice([1.0, 0.5, -0.5, 2.0, 1.37]))), float(np.float32(rng.choice([1.0, -1.0, 0.73])))
    delta, N = float(rng.choice([1.0 / 60.0, 0.25, 1.0 / 24.0])), int(rng.integers(40, 200))
    clips = [dict(length=L, loop_mode=A.LOOP_LINEAR, tracks=[])]
    run = play(clips, N + 1, delta, scale, cmds=A.pack_commands([0], [0], start=start, speed=speed))   # the first frame shows the start
    assert run[0][2][0, 0]["time"] == start and run[0][4][0] == R.STARTED
    got = Fraction(float(run[-1][0][0, 0]["pos"]))
    step = Fraction(scale) * Fraction(delta) * Fraction(speed)
    want = (Fraction(start) + N * step) % Fraction(L)
    d = abs(got - want)
    err = float(min(d, Fraction(L) - d))
    bound = 4.0 * N * (L + abs(float(step))) * V
    print(f"looping seed {seed}: N {N} err {err:.3e} bound {bound:.3e} ratio {err / bound:.4f}")
    assert err <= bound
    loops = sum(bool(f[4][0] & R.LOOPED) for f in run)
    assert loops == abs((Fraction(start) + N * step) // Fraction(L)), "one LOOPED event a seam"


def test_a_fade_runs_down_linearly_and_the_weights_add_up(mbik):
    """A blended play with bt = 0.26 at 60 frames a second: in the k-th advance since the command
    (the command's own is k = 1) the fade's weight is 1 - k * |g| / bt, the two weights add up to 1,
    and the fade is gone at the first k with k * |g| >= bt -- k = 16, k * |g| / bt being no closer
    to 1 than 0.025 at any frame.  A frame rounds q = (float)(|g| / bt) (q * (u + v)) and the float
    difference (at most u, the weight being at most 1): k * (q * (u + v) + u) after k frames.  w_0 =
    1 - w_1 rounds once more: the sum is within u of 1."""
    clips = [dict(length=1.0, loop_mode=A.LOOP_LINEAR, tracks=[]), dict(length=2.0, loop_mode=A.LOOP_LINEAR, tracks=[])]
    bt, delta = float(np.float32(0.26)), 1.0 / 60.0
    st, fl = A.empty_state(1, 2)
    st[0, 0] = (0.25, 0, 1.0, 0, 0)
    run = play(clips, 20, delta, cmds=A.pack_commands([0], [1], blend_time=bt), state=(st, fl))
    q = delta / bt
    worst = 0.0
    for k, (st, fl, layers, prev, ev) in enumerate(run, 1):
        assert layers[0, 0]["clip"] == 1
        if k * delta >= bt:
            assert k >= 16 and layers[0, 1]["clip"] == -1 and layers[0, 0]["weight"] == 1.0 and st[0, 1]["clip"] == -1
            continue
        assert k <= 15 and abs(k * q - 1.0) > 0.02
        w0, w1 = float(layers[0, 0]["weight"]), float(layers[0, 1]["weight"])
        bound = k * (q * (U + V) + U)
        err = abs(w1 - (1.0 - k * q))
        worst = max(worst, err / bound)
        assert layers[0, 1]["clip"] == 0 and err <= bound, (k, err, bound)
        assert abs(w0 + w1 - 1.0) <= U
        assert st[0, 1]["blend_left"] == layers[0, 1]["weight"]
    print(f"fade worst ratio {worst:.4f}")


@pytest.mark.parametrize("seed", range(6))
def test_the_records_carry_root_motion_across_the_seams(mbik, seed):
    """2.5 loops of synthetic_walk_clips' first clip (its root position track made linear), played by
    the advance at `per_loop` frames a loop and extracted frame by frame from the advance's own
    layers_out and time_prev_out (NORMALIZE, one layer on): the summed displacement equals loops * D
    + x64(pos) with the loops counted by the LOOPED events and pos the final position.  The bound is
    test_root_motion_geometry_cpu's, 4 * S * u * M, S the segments accumulated -- one a frame and one
    more for each frame that crossed the seam; the positions are the extraction's own inputs, so
    their float64 roundings cost nothing.  A dropped or doubled seam misses by |D|."""
    rest, clips = A.synthetic_walk_clips(40 + seed, 1, 0)
    clip = clips[0]
    assert clip["loop_mode"] == A.LOOP_LINEAR
    track = next(t for t in clip["tracks"] if t["channel"] == A.POSITION)
    track["interpolation"] = A.LINEAR
    length, T, Vk = float(clip["length"]), track["times"], track["values"]
    per_loop = int(np.random.default_rng(seed).integers(7, 41))
    frames = int(round(2.5 * per_loop))
    delta = 2.5 * length / frames
    st, fl = A.empty_state(1, 2)
    walked, loops, S = np.zeros(3), 0, 0
    for frame in range(frames + 1):      # the first frame shows the start: a segment of no length
        st, fl, layers, prev, ev = A.playback_advance_cpu(clips, st, fl, delta, cmds=A.pack_commands([0], [0]) if frame == 0 else None)
        motion = A.clip_root_motion_layers_cpu(1, rest, clips, layers, prev, 0, A.LAYERS_NORMALIZE)
        walked += motion[0, 4:7].astype(np.float64)
        looped = bool(ev[0] & R.LOOPED)
        assert looped == (layers[0, 0]["time"] < prev[0, 0])
        loops += looped
        S += 1 + looped
    want = loops * Vk[-1].astype(np.float64) + RM.value64(T, Vk, float(st[0, 0]["pos"]))
    M = max(float(np.abs(Vk).max()), float(np.abs(want).max()))
    err, bound = float(np.abs(walked - want).max()), 4.0 * S * U * M
    print(f"root motion seed {seed}: frames {frames} err {err:.3e} bound {bound:.3e} ratio {err / bound:.4f}")
    assert loops == 2 and abs(float(st[0, 0]["pos"]) - 0.5 * length) < 1e-9
    assert err <= bound
    assert float(np.abs(Vk[-1]).max()) > 100.0 * bound, "a missed seam would show"


@pytest.mark.parametrize("speed", (1.0, -1.0))
def test_a_clip_ends_on_its_end_and_its_successor_starts_on_its_start(mbik, speed):
    clips = [dict(length=0.7, loop_mode=A.LOOP_NONE, tracks=[]), dict(length=1.3, loop_mode=A.LOOP_NONE, tracks=[])]
    end0, start1 = (0.7, 0.0) if speed > 0 else (0.0, 1.3)
    run = play(clips, 12, 1.0 / 60.0 * 7, cmds=A.pack_commands([0], [0], speed=speed), next=[1, -1], default_blend_time=0.2)
    k = next(i for i, f in enumerate(run) if f[4][0] & R.ENDED)
    last, first = run[k], run[k + 1]
    assert last[2][0, 0]["clip"] == 0 and last[2][0, 0]["time"] == end0 and last[4][0] == R.ENDED | R.TRANSITIONED
    assert 0.0 < abs(last[3][0, 0] - end0) < 0.12, "the last frame still moves"
    assert first[2][0, 0]["clip"] == 1 and first[2][0, 0]["time"] == start1 and first[3][0, 0] == start1 and first[4][0] == R.STARTED
    assert first[2][0, 1]["clip"] == 0 and first[2][0, 1]["time"] == end0 and first[3][0, 1] == end0      # the clip that ended fades out from its end
    assert run[k + 2][2][0, 0]["time"] != start1 and run[k + 2][3][0, 0] == start1
