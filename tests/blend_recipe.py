"""Expected values for the pose-blend tests (CPU and GPU): Godot 4.3's Skeleton3D::_process_modifiers
blend of one bone, old.interpolate_with(new, influence) written back with set_bone_pose, in float32
numpy operations in Godot's order:

    1. !(w < 1): out = m
    2. A = xform_mul([quat_to_basis(a.q), 0], [diag(a.scale), 0]) with origin a.position, M likewise;
       all 12 floats equal (float ==): out = m
    3. w < 0 (not -0): w = 0
    4. sa = get_scale(A), qa = basis_to_quat(A) (== get_rotation_quaternion); sm, qm from M
    5. q = normalized(slerp(qa, qm, w)); sc = sa + (sm - sa) * w; o = A.o + (M.o - A.o) * w
    6. T = xform_mul([quat_to_basis(q), 0], [diag(sc), 0])
    7. out = (basis_to_quat(T), o, get_scale(T))

quat_to_basis, basis_to_quat and xform_mul are the oracle's exported primitives; sinf, acosf, sqrtf
and the double sin are the platform glibc's through ctypes (the libm the oracle itself calls); slerp
and get_scale are restated from oracle/godot_math.h:166-187 and :308.  Every array operation below
is one IEEE float32 operation per element.  Nothing here calls the code under test.  Comparisons
are on uint32 views: every value, no tolerance.
"""
import ctypes as C
import ctypes.util

import numpy as np

F = np.float32
CMP_EPSILON = F(0.00001)

# the weights of the issue: 0, -0, 1e-7, 0.25, 0.5, 1 - 2^-24, 1, 1.5, -0.5, NaN
WEIGHTS = np.array([0.0, -0.0, 1e-7, 0.25, 0.5, 1.0 - 2.0 ** -24, 1.0, 1.5, -0.5, np.nan], np.float32)

_libm = None


def libm():
    global _libm
    if _libm is None:
        m = C.CDLL(ctypes.util.find_library("m") or "libm.so.6")
        for name in ("sinf", "acosf", "sqrtf"):
            f = getattr(m, name)
            f.restype, f.argtypes = C.c_float, [C.c_float]
        m.sin.restype, m.sin.argtypes = C.c_double, [C.c_double]
        _libm = m
    return _libm


def _map(fn, x):
    return np.array([fn(float(v)) for v in x], np.float32).reshape(x.shape)


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def same_bits(a, b):
    return a.shape == b.shape and np.array_equal(bits(a), bits(b))


_oracle = None


def _prims(po):
    """The oracle's primitives, called with plain addresses (one call per bone: numpy's checked
    array arguments would cost more than the calls)."""
    global _oracle
    if _oracle is None:
        po.lib()   # builds the oracle if it is missing
        L = C.CDLL(po.LIB_PATH)
        for name, nargs in (("oracle_quat_to_basis", 2), ("oracle_basis_to_quat", 2), ("oracle_xform_mul", 3)):
            f = getattr(L, name)
            f.restype, f.argtypes = None, [C.c_void_p] * nargs
        _oracle = L
    return _oracle


def basis_times_scale(po, q, scale):
    """[N][9]: Basis(q) * diag(scale) by the oracle's quat_to_basis and xform_mul."""
    L = _prims(po)
    n = q.shape[0]
    q = np.ascontiguousarray(q, np.float32)
    a, d, r = np.zeros((n, 12), np.float32), np.zeros((n, 12), np.float32), np.zeros((n, 12), np.float32)
    d[:, 0], d[:, 4], d[:, 8] = scale[:, 0], scale[:, 1], scale[:, 2]
    pq, pa, pd, pr = q.ctypes.data, a.ctypes.data, d.ctypes.data, r.ctypes.data
    for i in range(n):
        L.oracle_quat_to_basis(pq + 16 * i, pa + 48 * i)
        L.oracle_xform_mul(pa + 48 * i, pd + 48 * i, pr + 48 * i)
    return np.ascontiguousarray(r[:, 0:9])


def rotation_quaternion(po, b9):
    """[N][4]: Basis::get_rotation_quaternion by the oracle's basis_to_quat."""
    L = _prims(po)
    b9 = np.ascontiguousarray(b9, np.float32)
    out = np.zeros((b9.shape[0], 4), np.float32)
    pb, po_ = b9.ctypes.data, out.ctypes.data
    for i in range(b9.shape[0]):
        L.oracle_basis_to_quat(pb + 36 * i, po_ + 16 * i)
    return out


def get_scale(b9):
    """Basis::get_scale (godot_math.h:308): SIGN(det) * column lengths; rows r0 = b9[0:3], ..."""
    r = b9.reshape(-1, 3, 3)
    det = (r[:, 0, 0] * (r[:, 1, 1] * r[:, 2, 2] - r[:, 2, 1] * r[:, 1, 2]) -
           r[:, 1, 0] * (r[:, 0, 1] * r[:, 2, 2] - r[:, 2, 1] * r[:, 0, 2]) +
           r[:, 2, 0] * (r[:, 0, 1] * r[:, 1, 2] - r[:, 1, 1] * r[:, 0, 2]))
    sg = np.where(det > 0, F(1), np.where(det < 0, F(-1), F(0))).astype(np.float32)
    out = np.zeros((r.shape[0], 3), np.float32)
    for c in range(3):
        x, y, z = r[:, 0, c], r[:, 1, c], r[:, 2, c]
        out[:, c] = _map(libm().sqrtf, x * x + y * y + z * z) * sg
    assert det.dtype == np.float32 and out.dtype == np.float32
    return out


def slerp(qa, qm, w):
    """Quaternion::slerp (godot_math.h:166-187) at per-row weights w."""
    m = libm()
    cosom = qa[:, 0] * qm[:, 0] + qa[:, 1] * qm[:, 1] + qa[:, 2] * qm[:, 2] + qa[:, 3] * qm[:, 3]
    flip = cosom < 0
    cosom = np.where(flip, -cosom, cosom)
    to1 = np.where(flip[:, None], -qm, qm)
    scale0 = F(1) - w
    scale1 = w.copy()
    for i in np.nonzero((F(1) - cosom) > CMP_EPSILON)[0]:
        omega = F(m.acosf(float(cosom[i])))
        sinom = F(m.sinf(float(omega)))
        scale0[i] = F(m.sin((1.0 - float(w[i])) * float(omega)) / float(sinom))
        scale1[i] = F(m.sinf(float(w[i] * omega))) / sinom
    out = scale0[:, None] * qa + scale1[:, None] * to1
    assert cosom.dtype == np.float32 and out.dtype == np.float32
    return out


def normalized(q):
    d = q[:, 0] * q[:, 0] + q[:, 1] * q[:, 1] + q[:, 2] * q[:, 2] + q[:, 3] * q[:, 3]
    return q * (F(1) / _map(libm().sqrtf, d))[:, None]


def expected(po, pose_in, pose_mod, weights):
    """The blend of bones pose_in / pose_mod [N][10] at per-bone weights [N]: ([N][10], blended mask [N])."""
    a = np.ascontiguousarray(pose_in, np.float32).reshape(-1, 10)
    m = np.ascontiguousarray(pose_mod, np.float32).reshape(-1, 10)
    w = np.ascontiguousarray(weights, np.float32).reshape(-1)
    assert a.shape == m.shape and w.shape[0] == a.shape[0]
    out = m.copy()
    with np.errstate(all="ignore"):
        A = np.concatenate([basis_times_scale(po, a[:, 0:4], a[:, 7:10]), a[:, 4:7]], axis=1)
        M = np.concatenate([basis_times_scale(po, m[:, 0:4], m[:, 7:10]), m[:, 4:7]], axis=1)
        blend = (w < F(1)) & ~np.all(A == M, axis=1)
        A, M, w = A[blend], M[blend], w[blend]
        w = np.where(w < F(0), F(0), w)
        sa, sm = get_scale(A[:, 0:9]), get_scale(M[:, 0:9])
        qa, qm = rotation_quaternion(po, A[:, 0:9]), rotation_quaternion(po, M[:, 0:9])
        q = normalized(slerp(qa, qm, w))
        sc = sa + (sm - sa) * w[:, None]
        o = A[:, 9:12] + (M[:, 9:12] - A[:, 9:12]) * w[:, None]
        T = basis_times_scale(po, q, sc)
        res = np.concatenate([rotation_quaternion(po, T), o, get_scale(T)], axis=1)
    assert res.dtype == np.float32
    out[blend] = res
    return out.reshape(np.shape(pose_in)), blend


# ---------------------------------------------------------------- inputs
def _quat_mul(a, b):
    x = a[..., 3] * b[..., 0] + a[..., 0] * b[..., 3] + a[..., 1] * b[..., 2] - a[..., 2] * b[..., 1]
    y = a[..., 3] * b[..., 1] + a[..., 1] * b[..., 3] + a[..., 2] * b[..., 0] - a[..., 0] * b[..., 2]
    z = a[..., 3] * b[..., 2] + a[..., 2] * b[..., 3] + a[..., 0] * b[..., 1] - a[..., 1] * b[..., 0]
    w = a[..., 3] * b[..., 3] - a[..., 0] * b[..., 0] - a[..., 1] * b[..., 1] - a[..., 2] * b[..., 2]
    return np.stack([x, y, z, w], axis=-1)


def _axis_angle(rng, n, angle):
    ax = rng.normal(0.0, 1.0, (n, 3))
    ax /= np.linalg.norm(ax, axis=1, keepdims=True)
    return np.concatenate([ax * np.sin(angle / 2)[:, None], np.cos(angle / 2)[:, None]], axis=1)


KINDS = ("general", "q_vs_minus_q", "identical", "one_ulp", "near_rotation", "far_rotation", "near_pi_axis", "unit")


def mixed_inputs(seed, n_bones):
    """(pose_in, pose_mod, kind) for n_bones bones, kind[i] an index into KINDS, cycling:
    general         non-unit quaternions, non-uniform scales, a quarter of them negative (so
                    determinants of both signs), unrelated poses
    q_vs_minus_q    the modifier's quaternion is the input's negated: equal transforms, other triples
    identical       the same pose
    one_ulp         the same pose but for one float, one ulp away
    near_rotation   rotations within 1e-6 rad of each other (slerp's linear branch)
    far_rotation    rotations 185..355 degrees apart (quaternions more than 90 degrees apart: the sign flip)
    near_pi_axis    rotations by almost pi about x, y or z (get_quaternion's three trace <= 0 branches)
    unit            unit quaternions, unit scales, unrelated rotations
    """
    rng = np.random.default_rng(seed)
    n = n_bones
    kind = np.arange(n) % len(KINDS)
    a = np.empty((n, 10), np.float64)
    a[:, 0:4] = rng.normal(0.0, 1.0, (n, 4)) * rng.uniform(0.5, 1.5, (n, 1))
    a[:, 4:7] = rng.uniform(-1.0, 1.0, (n, 3))
    a[:, 7:10] = rng.uniform(0.6, 1.4, (n, 3)) * np.where(rng.uniform(0.0, 1.0, (n, 3)) < 0.25, -1.0, 1.0)
    m = np.empty((n, 10), np.float64)
    m[:, 0:4] = rng.normal(0.0, 1.0, (n, 4)) * rng.uniform(0.5, 1.5, (n, 1))
    m[:, 4:7] = rng.uniform(-1.0, 1.0, (n, 3))
    m[:, 7:10] = rng.uniform(0.6, 1.4, (n, 3)) * np.where(rng.uniform(0.0, 1.0, (n, 3)) < 0.25, -1.0, 1.0)

    unit_a = a[:, 0:4] / np.linalg.norm(a[:, 0:4], axis=1, keepdims=True)
    k = kind == KINDS.index("near_rotation")
    a[k, 0:4] = unit_a[k]
    m[k, 0:4] = _quat_mul(unit_a[k], _axis_angle(rng, k.sum(), rng.uniform(0.0, 1e-6, k.sum())))
    m[k, 7:10] = np.abs(m[k, 7:10])
    a[k, 7:10] = np.abs(a[k, 7:10])
    k = kind == KINDS.index("far_rotation")
    m[k, 0:4] = _quat_mul(unit_a[k], _axis_angle(rng, k.sum(), np.radians(rng.uniform(185.0, 355.0, k.sum()))))
    k = kind == KINDS.index("near_pi_axis")
    for arr in (a, m):
        q = rng.normal(0.0, 0.02, (k.sum(), 4))
        q[np.arange(k.sum()), rng.integers(0, 3, k.sum())] = 1.0
        arr[k, 0:4] = q
    k = kind == KINDS.index("unit")
    a[k, 0:4] = unit_a[k]
    m[k, 0:4] /= np.linalg.norm(m[k, 0:4], axis=1, keepdims=True)
    a[k, 7:10] = m[k, 7:10] = 1.0

    a = a.astype(np.float32)
    m = m.astype(np.float32)
    k = kind == KINDS.index("q_vs_minus_q")
    m[k] = a[k]
    m[k, 0:4] = -a[k, 0:4]
    k = kind == KINDS.index("identical")
    m[k] = a[k]
    k = np.nonzero(kind == KINDS.index("one_ulp"))[0]
    m[k] = a[k]
    col = rng.integers(0, 10, k.shape[0])
    m[k, col] = np.nextafter(a[k, col], np.float32(np.inf))
    return a, m, kind
