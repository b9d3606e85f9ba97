"""What cubic interpolation means, against float64 (mbik_clip_call_cpu through the Python calls;
nothing here calls tests/clip_cubic_recipe.py).

The float64 side is a restatement of include/mbik.h's step 5c on (value, error) pairs -- class E: the
float64 value and a first-order bound of the absolute error its float32 counterpart has collected,
e' = propagated + u |value| for each float32 rounding, u = 2^-24 -- so every bound below is counted
from the roundings of the float32 sequence, per sample, before the code under test runs.  SLACK =
1 + 2^-4 covers the second-order terms the first-order propagation drops.  The worst observed ratio
of an error to its bound is printed by each test and recorded in DESIGN.md §26.

Rotations.  eps_q = 50 u bounds a component of Basis(q).get_rotation_quaternion(): Basis::
set_quaternion rounds at most 8 times an entry (|entry| <= 1), Gram-Schmidt's three stages at most 12
times each, get_quaternion halves the difference of two entries over s >= 1 and rounds 4 more times.
A product of two such quaternions is within eps_p = 4 eps_q + 8 u.  A logarithm of a quaternion
with kappa = 1 / sqrt(1 - w^2) and angle theta <= 2 pi is within eps_p kappa (theta (1 + kappa) + 2)
(the axis divides by sqrt(1 - w^2), the angle is 2 acos(w)).  The cubic of the logarithms goes
through class E with those input errors; exp halves the error of its argument (+ 8 u), the product
with the base adds eps_q + 4 u, the slerp of the two halves 8 u, and the angle between two unit
quaternions is at most 4 times their largest component difference.
"""
import numpy as np
import pytest

from many_bone_ik_amd import animation as A

U = 2.0 ** -24
SLACK = 1.0 + 2.0 ** -4
EPS_Q = 50 * U
EPS_P = 4 * EPS_Q + 8 * U
CMP_EPSILON = 1e-5


class E:
    """A float64 value and the first-order absolute error bound of its float32 counterpart."""
    __slots__ = ("v", "e")

    def __init__(self, v, e=0.0):
        self.v, self.e = float(v), float(e)

    @staticmethod
    def rounded(v, e=0.0):
        return E(v, e + U * abs(v))

    def __add__(self, o):
        return E.rounded(self.v + o.v, self.e + o.e)

    def __sub__(self, o):
        return E.rounded(self.v - o.v, self.e + o.e)

    def __mul__(self, o):
        return E.rounded(self.v * o.v, abs(self.v) * o.e + abs(o.v) * self.e)

    def __truediv__(self, o):
        q = self.v / o.v
        return E.rounded(q, (self.e + abs(q) * o.e) / abs(o.v))

    def __neg__(self):
        return E(-self.v, self.e)


def lerp(a, b, w):
    return a + (b - a) * w


def pick(T, tp, wrap, length):
    """include/mbik.h step 5 / 5c: None for a copy of V[k] -> ("copy", k), else (a, b, pre, post) and
    the exact float64 times pre_t, to_t, post_t, delta, from."""
    n = T.shape[0]
    i = int(np.searchsorted(T, tp, side="right")) - 1
    if n == 1:
        return "copy", 0
    if not wrap and i < 0:
        return "copy", 0
    if not wrap and i == n - 1:
        return "copy", n - 1
    if not wrap:
        a, b, pre, post = i, i + 1, max(i - 1, 0), min(i + 2, n - 1)
    else:
        a = i if i >= 0 else n - 1
        b, pre, post = (a + 1) % n, (a - 1) % n, (a + 2) % n
    pre_t = (-length + T[pre]) - T[a] if pre > a else T[pre] - T[a]
    to_t = (length + T[b]) - T[a] if b < a else T[b] - T[a]
    post_t = (length + T[post]) - T[a] if (b < a or post <= a) else T[post] - T[a]
    if 0 <= i < n - 1:
        delta, frm = T[b] - T[a], tp - T[a]
    else:
        delta = (length - T[a]) + T[b]
        frm = (length - T[a]) + tp if i < 0 else tp - T[a]
    return (a, b, pre, post), (pre_t, to_t, post_t, delta, frm)


def cubic_weights(times):
    """The lerp weights of the Barry-Goldman scheme as E pairs, from the exact float64 times: each of
    pre_t, to_t, post_t, delta and from is rounded once to float32."""
    pre_t, to_t, post_t, delta, frm = (E.rounded(x) for x in times)
    zero = E(0.0)
    c = zero if abs(delta.v) < CMP_EPSILON else frm / delta
    t = lerp(zero, to_t, c)
    a1 = zero if pre_t.v == 0 else (t - pre_t) / -pre_t
    a2 = E(0.5) if to_t.v == 0 else t / to_t
    a3 = E(1.0) if (post_t - to_t).v == 0 else (t - to_t) / (post_t - to_t)
    b1 = zero if (to_t - pre_t).v == 0 else (t - pre_t) / (to_t - pre_t)
    b2 = E(1.0) if post_t.v == 0 else t / post_t
    return c, (a1, a2, a3, b1, b2)


def cubic(frm, to, pre, post, w):
    a1, a2, a3 = lerp(pre, frm, w[0]), lerp(frm, to, w[1]), lerp(to, post, w[2])
    b1, b2 = lerp(a1, a2, w[3]), lerp(a2, a3, w[4])
    return lerp(b1, b2, w[1])


def scalar_model(T, V, tp, wrap, length):
    """(value64, bound) of one float32 component track V at the mapped time tp."""
    how, x = pick(T, tp, wrap, length)
    if how == "copy":
        return float(V[x]), 0.0
    a, b, pre, post = how
    c, w = cubic_weights(x)
    if c.v == 0:   # on a key: V[a], copied
        return float(V[a]), 0.0
    r = cubic(E(V[a]), E(V[b]), E(V[pre]), E(V[post]), w)
    return r.v, r.e * SLACK


REST1 = np.array([[0, 0, 0, 1, 0, 0, 0, 1, 1, 1]], np.float32)


def sample_channel(channel, T, V, times, wrap, length):
    clips = [dict(length=length, loop_mode=1 if wrap else 0, tracks=[dict(bone=0, channel=channel, interpolation=A.CUBIC, loop_wrap=int(wrap),
                                                                        times=T, values=V)])]
    return A.clip_sample_cpu(1, REST1, clips, times, clip=0, cubic=True)[:, 0, A.CHANNEL_SLICE[channel]]


def sample_shape(T, V, times, wrap, length):
    clips = [dict(length=length, loop_mode=1 if wrap else 0, tracks=[],
                  shape_tracks=[dict(shape=0, interpolation=A.CUBIC, loop_wrap=int(wrap), times=T, values=V)])]
    return A.clip_sample_shapes_cpu(1, clips, times, clip=0, cubic=True)[:, 0]


def uneven_times(rng, n, length, lo=0.05, hi=0.95):
    """n key times in (lo, hi) * length, neighbouring gaps within a factor of 4 of each other."""
    gaps = rng.uniform(1.0, 4.0, n + 1)
    return (lo + (hi - lo) * np.cumsum(gaps)[:n] / gaps.sum()) * length


def check(got, want, bound, what):
    """Asserts |got - want| <= bound element-wise; returns the worst ratio."""
    err = np.abs(np.asarray(got, np.float64) - want)
    ratio = np.where(bound > 0, err / np.where(bound > 0, bound, 1.0), np.where(err == 0, 0.0, np.inf))
    k = int(np.argmax(ratio))
    print(f"{what}: worst error / bound = {ratio.reshape(-1)[k]:.3g} (error {err.reshape(-1)[k]:.3e}, bound {np.asarray(bound).reshape(-1)[k]:.3e})")
    assert (err <= bound).all(), f"{what}: error {err.reshape(-1)[k]:.3e} above its bound {np.asarray(bound).reshape(-1)[k]:.3e}"
    return float(ratio.reshape(-1)[k])


# ---------------------------------------------------------------- interpolation: the curve passes through its keys
@pytest.mark.parametrize("wrap", (False, True))
def test_on_a_key_position_scale_and_shape_equal_the_key_bits(mbik, wrap):
    """At every key time the position, scale and shape value equal the key's bits, on general float32
    keys: step 5c copies V[a] at c == 0.  (The scheme evaluated there gives lerp(pre + (from - pre),
    from, w), which is `from` only when from - pre is representable: without the rule 4 of these 27
    position floats differed from their key, by at most 5.96e-08 -- 22 ulps of a small key.)"""
    rng = np.random.default_rng(5)
    L = 2.0
    T = np.sort(rng.uniform(0.1, 1.9, 9))
    V = rng.uniform(-1.0, 1.0, (9, 3)).astype(np.float32)
    for what, got, want in [("position", sample_channel(A.POSITION, T, V, T, wrap, L), V), ("scale", sample_channel(A.SCALE, T, V, T, wrap, L), V),
                            ("shape", sample_shape(T, V[:, 0].copy(), T, wrap, L), V[:, 0])]:
        differ = int((got.view(np.uint32) != want.view(np.uint32)).sum())
        ulps = int(np.abs(got.view(np.int32).astype(np.int64) - want.view(np.int32).astype(np.int64)).max())
        print(f"{what} on its keys, wrap={wrap}: {differ} of {want.size} floats differ, by at most {np.abs(got - want).max():.3e} ({ulps} ulps)")
        assert differ == 0, f"{what}: {differ} of {want.size} floats differ from their key, by at most {np.abs(got - want).max():.3e} ({ulps} ulps)"


def canonical64(q):
    q = np.asarray(q, np.float64)
    return q / np.linalg.norm(q, axis=-1, keepdims=True)


def angle_between(q, p):
    q, p = canonical64(q), canonical64(p)
    d = q - p * np.where(np.sum(q * p, axis=-1, keepdims=True) < 0, -1.0, 1.0)
    return 4.0 * np.arcsin(np.minimum(1.0, np.linalg.norm(d, axis=-1) / 2.0))


@pytest.mark.parametrize("wrap", (False, True))
def test_on_a_key_the_rotation_is_the_keys_canonical_rotation(mbik, wrap):
    """At c == 0 the first half is `from` exactly (its logarithm cubic is 0 + (0 - 0) ...) and the
    slerp weighs the second half by sin(0) = 0: the result is Basis(V[a]).get_rotation_quaternion()
    times a coefficient within 2 roundings of 1 -- eps_q + 2 u a component, up to sign, 4 times
    that as an angle.  Keys are unit, scaled by 0.5 .. 1.5, one with |w| > 1."""
    rng = np.random.default_rng(7)
    L = 2.0
    T = np.sort(rng.uniform(0.1, 1.9, 9))
    V = A._key_rotations(rng, 9) * rng.uniform(0.5, 1.5, (9, 1))
    V[3] *= 1.2 / abs(V[3, 3]) if abs(V[3, 3]) > 0.3 else 1.0
    V = V.astype(np.float32)
    got = sample_channel(A.ROTATION, T, V, T, wrap, L)
    check(angle_between(got, V), 0.0, np.full(9, 4 * (EPS_Q + 2 * U) * SLACK), f"rotation on a key, wrap={wrap}")
    computed = got if wrap else got[:-1]   # (without wrap the last key is a copy of the key as given)
    assert np.abs(np.linalg.norm(computed.astype(np.float64), axis=1) - 1).max() < 8 * EPS_Q
    if not wrap:
        assert np.array_equal(got[-1].view(np.uint32), V[-1].view(np.uint32))


# ---------------------------------------------------------------- quadratic reproduction
def quadratic(rng):
    c = rng.uniform(-1.0, 1.0, 3)
    return lambda t: c[0] + c[1] * t + c[2] * t * t


def between_keys(rng, T, per=7):
    return np.concatenate([rng.uniform(T[k], T[k + 1], per) for k in range(T.shape[0] - 1)])


def test_quadratics_are_reproduced_on_interior_segments_and_modelled_on_edge_segments(mbik):
    """Keys sampled from a quadratic in time at uneven key times (rounded to float32: an input error
    of u |key| that class E carries through).  On a segment with distinct pre and post the scheme
    blends two quadratic Lagrange interpolants, so the float64 model is the quadratic itself, and
    the float32 result is within the counted bound of it.  On the first and last segment (pre == a
    or post == b) the result is held to the float64 model of the same degenerate formula."""
    rng = np.random.default_rng(11)
    L, n = 2.0, 8
    worst = 0.0
    for trial in range(4):
        T = uneven_times(rng, n, L)
        q = [quadratic(rng) for _ in range(3)]
        exact = np.stack([f(T) for f in q], axis=1)
        V = exact.astype(np.float32)
        times = between_keys(rng, T)
        got = sample_channel(A.POSITION, T, V, times, False, L)
        got_shape = sample_shape(T, V[:, 0].copy(), times, False, L)
        for s, tp in enumerate(times):
            (a, b, pre, post), x = pick(T, tp, False, L)
            _, w = cubic_weights(x)
            interior = pre != a and post != b
            for k in range(3):
                keys = [E(V[j, k], abs(exact[j, k] - float(V[j, k])) if interior else 0.0) for j in (a, b, pre, post)]
                r = cubic(*keys, w)
                want = q[k](tp) if interior else r.v
                worst = max(worst, check(got[s, k], want, r.e * SLACK, f"trial {trial} t'={tp:.4f} component {k} {'interior' if interior else 'edge'}"))
                if k == 0:
                    check(got_shape[s], want, r.e * SLACK, "shape")
    print(f"quadratic reproduction: worst error / bound = {worst:.3g}")


def test_the_float64_scheme_reproduces_quadratics_exactly(mbik):
    """The property itself, on the float64 side alone: with exact keys the model is the quadratic to
    float64's rounding on every interior segment, and is not on an edge segment."""
    rng = np.random.default_rng(12)
    L, n = 2.0, 8
    T = uneven_times(rng, n, L)
    f = quadratic(rng)
    worst_interior, worst_edge = 0.0, 0.0
    for tp in between_keys(rng, T):
        (a, b, pre, post), x = pick(T, tp, False, L)
        pre_t, to_t, post_t, delta, frm = x
        c = frm / delta
        t = to_t * c
        w = [0.0 if pre_t == 0 else (t - pre_t) / -pre_t, t / to_t, 1.0 if post_t == to_t else (t - to_t) / (post_t - to_t),
             0.0 if to_t == pre_t else (t - pre_t) / (to_t - pre_t), 1.0 if post_t == 0 else t / post_t]
        v = [f(T[j]) for j in (a, b, pre, post)]
        a1, a2, a3 = v[2] + (v[0] - v[2]) * w[0], v[0] + (v[1] - v[0]) * w[1], v[1] + (v[3] - v[1]) * w[2]
        b1, b2 = a1 + (a2 - a1) * w[3], a2 + (a3 - a2) * w[4]
        err = abs(b1 + (b2 - b1) * w[1] - f(tp))
        if pre != a and post != b:
            worst_interior = max(worst_interior, err)
        else:
            worst_edge = max(worst_edge, err)
    assert worst_interior < 1e-13 and worst_edge > 1e-6


def test_quadratics_are_reproduced_across_the_seam(mbik):
    """A wrapping clip of 4 keys whose values are samples of one quadratic at the unwrapped times of
    the seam segment: V[2], V[3] at T[2], T[3] and V[0], V[1] at T[0] + length, T[1] + length.  Both
    wrap branches (after the last key, before the first) reproduce the quadratic in unwrapped time."""
    rng = np.random.default_rng(13)
    L = 2.0
    worst = 0.0
    for trial in range(4):
        T = uneven_times(rng, 4, L, 0.15, 0.85)
        f = quadratic(rng)
        exact = np.array([f(T[0] + L), f(T[1] + L), f(T[2]), f(T[3])])
        V = exact.astype(np.float32)
        times = np.concatenate([rng.uniform(T[3], L, 9), rng.uniform(0.0, T[0], 9), [L, 0.0]])
        got = sample_shape(T, V, times, True, L)
        for s, tp in enumerate(times):
            (a, b, pre, post), x = pick(T, tp, True, L)
            assert (a, b, pre, post) == (3, 0, 2, 1)
            _, w = cubic_weights(x)
            r = cubic(*[E(V[j], abs(exact[j] - float(V[j]))) for j in (a, b, pre, post)], w)
            unwrapped = tp if tp >= T[3] else tp + L
            worst = max(worst, check(got[s], f(unwrapped), r.e * SLACK, f"seam trial {trial} t'={tp:.4f}"))
    print(f"quadratic reproduction across the seam: worst error / bound = {worst:.3g}")


# ---------------------------------------------------------------- rotation
def qmul64(a, b):
    v = a[3] * b[:3] + b[3] * a[:3] + np.cross(a[:3], b[:3])
    return np.concatenate([v, [a[3] * b[3] - a[:3] @ b[:3]]])


def conj64(q):
    return q * np.array([-1.0, -1.0, -1.0, 1.0])


def log64(q):
    """(log vector, kappa, theta) of a unit quaternion, float64."""
    w = min(1.0, max(-1.0, q[3]))
    s = np.sqrt(max(1.0 - w * w, 0.0))
    theta = 2.0 * np.arccos(w)
    if abs(w) > 1 - CMP_EPSILON:
        return q[:3] * theta, 1.0, theta
    return q[:3] / s * theta, 1.0 / s, theta


def exp64(v):
    th = np.linalg.norm(v)
    if th < CMP_EPSILON:
        return np.array([0.0, 0.0, 0.0, 1.0])
    return np.concatenate([v / th * np.sin(th / 2), [np.cos(th / 2)]])


def slerp64(a, b, t):
    d = a @ b
    if d < 0:
        b, d = -b, -d
    om = np.arccos(min(1.0, d))
    if np.sin(om) < 1e-9:
        return (1 - t) * a + t * b
    return (np.sin((1 - t) * om) * a + np.sin(t * om) * b) / np.sin(om)


def rotation_model(T, V, tp, wrap, length):
    """(unit quaternion float64, angle bound) of a cubic rotation track: the docstring's count."""
    how, x = pick(T, tp, wrap, length)
    if how == "copy":
        return canonical64(V[x]), 0.0
    a, b, pre, post = how
    c, w = cubic_weights(x)
    frm, to, p, po = (canonical64(V[j]) for j in (a, b, pre, post))
    if np.signbit(frm @ p):
        p = -p
    flip2 = bool(np.signbit(frm @ to))
    if flip2:
        to = -to
    d = to @ po
    if (d <= 0) if flip2 else bool(np.signbit(d)):
        po = -po
    halves, err = [], 0.0
    for base, f_, t_ in ((frm, None, to), (to, frm, None)):
        logs = []
        for other in (f_, t_, p, po):
            if other is None:
                logs.append([E(0.0)] * 3)
                continue
            l, kappa, theta = log64(qmul64(conj64(base), other))
            e = EPS_P * kappa * (theta * (1.0 + kappa) + 2.0)
            logs.append([E(l[k], e) for k in range(3)])
        ln = [cubic(logs[0][k], logs[1][k], logs[2][k], logs[3][k], w) for k in range(3)]
        halves.append(qmul64(base, exp64(np.array([z.v for z in ln]))))
        err = max(err, 0.5 * max(z.e for z in ln) + 8 * U + EPS_Q + 4 * U)
    q = slerp64(halves[0], halves[1], c.v)
    # the slerp's weight carries c's error too: the two halves differ by at most their angle
    apart = float(angle_between(halves[0], halves[1]))
    return q / np.linalg.norm(q), (4 * (err + 8 * U) + c.e * apart) * SLACK


def test_a_rotation_about_one_axis_follows_its_quadratic_angle(mbik):
    """Keys about one fixed axis with an angle that is a quadratic of time, total arc below pi / 2: no
    flip occurs, the exponential map is exact on a one-parameter subgroup, and both halves -- so
    their slerp -- are the rotation by the quadratic's angle on every interior segment."""
    rng = np.random.default_rng(17)
    L, n = 2.0, 7
    worst = 0.0
    for trial in range(3):
        T = uneven_times(rng, n, L)
        axis = rng.normal(0.0, 1.0, 3)
        axis /= np.linalg.norm(axis)
        c2 = rng.uniform(0.1, 0.2)
        ang = lambda t: 0.2 + 0.15 * t + c2 * t * t   # 0.2 .. at most 1.3 rad over [0, 2]: an arc below pi / 2
        assert ang(L) - ang(0.0) < np.pi / 2
        V = np.stack([np.concatenate([axis * np.sin(ang(t) / 2), [np.cos(ang(t) / 2)]]) for t in T]).astype(np.float32)
        times = between_keys(rng, T[1:-1], 5)
        got = sample_channel(A.ROTATION, T, V, times, False, L)
        for s, tp in enumerate(times):
            model, bound = rotation_model(T, V, tp, False, L)
            want = np.concatenate([axis * np.sin(ang(tp) / 2), [np.cos(ang(tp) / 2)]])
            # the float64 model is the quadratic's rotation up to the keys' float32 rounding (4 u an angle, amplified by the cubic's weights <= 8)
            assert angle_between(model, want) < 64 * U
            worst = max(worst, check(angle_between(got[s], want), 0.0, np.array(bound + 64 * U), f"axis trial {trial} t'={tp:.4f}"))
    print(f"rotation about one axis: worst error / bound = {worst:.3g}")


@pytest.mark.parametrize("wrap", (False, True))
def test_rotations_match_an_independent_float64_spherical_cubic(mbik, wrap):
    """Random key sets (neighbours 10 .. 120 degrees apart), every segment, wrap on and off."""
    rng = np.random.default_rng(19 + wrap)
    L, n = 2.0, 6
    worst = 0.0
    for trial in range(4):
        T = uneven_times(rng, n, L)
        V = A._key_rotations(rng, n).astype(np.float32)
        times = np.concatenate([between_keys(rng, T, 4), rng.uniform(0.0, T[0], 3), rng.uniform(T[-1], L, 3)])
        got = sample_channel(A.ROTATION, T, V, times, wrap, L)
        for s, tp in enumerate(times):
            how, k = pick(T, tp, wrap, L)
            if how == "copy":   # before the first and after the last key of a track that does not wrap: the key as given
                assert np.array_equal(got[s].view(np.uint32), V[k].view(np.uint32))
                continue
            model, bound = rotation_model(T, V, tp, wrap, L)
            worst = max(worst, check(angle_between(got[s], model), 0.0, np.array(bound), f"random rotations trial {trial} t'={tp:.4f} wrap={wrap}"))
    print(f"random rotations, wrap={wrap}: worst error / bound = {worst:.3g}")


# ---------------------------------------------------------------- continuity
def test_the_curve_is_continuous_at_its_keys_and_across_the_seam(mbik):
    """One ulp of time before a key and on it: two samples of neighbouring segments, each within its
    counted bound of its model, and the models one ulp of time apart differ by less than the
    bounds' sum.  The same at t' = 0 against t' = the last double below length on a wrapping track
    whose first key (at 0) and last key (at length) hold one value."""
    rng = np.random.default_rng(23)
    L, n = 2.0, 7
    T = uneven_times(rng, n, L)
    V = rng.uniform(-1.0, 1.0, (n, 3)).astype(np.float32)
    before = np.nextafter(T[1:-1], -np.inf)
    got_on, got_before = sample_channel(A.POSITION, T, V, T[1:-1], False, L), sample_channel(A.POSITION, T, V, before, False, L)
    worst = 0.0
    for s in range(n - 2):
        for k in range(3):
            b0 = scalar_model(T, V[:, k], before[s], False, L)[1]
            b1 = scalar_model(T, V[:, k], T[1 + s], False, L)[1]
            worst = max(worst, check(got_before[s, k], float(got_on[s, k]), np.array(b0 + b1 + 1e-12), f"continuity at key {1 + s} component {k}"))
    # the seam
    T = np.concatenate([[0.0], uneven_times(rng, n - 2, L, 0.1, 0.9), [L]])
    V = rng.uniform(-1.0, 1.0, (n, 3)).astype(np.float32)
    V[-1] = V[0]
    ends = np.array([0.0, np.nextafter(L, 0.0)])
    got = sample_channel(A.POSITION, T, V, ends, True, L)
    for k in range(3):
        b0, b1 = scalar_model(T, V[:, k], ends[0], True, L)[1], scalar_model(T, V[:, k], ends[1], True, L)[1]
        worst = max(worst, check(got[1, k], float(got[0, k]), np.array(b0 + b1 + 1e-12), f"continuity across the seam component {k}"))
    print(f"continuity: worst error / bound = {worst:.3g}")
