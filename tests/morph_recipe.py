"""Blend shapes in front of the skinning (include/mbik.h, ABI 13) written twice without
the code under test, for tests/test_morph_cpu.py and tests/test_gpu_morph.py.

`morph_vertex` follows the header's steps literally in numpy float32 scalars: one rounding per
operation, shapes in ascending order, `fabsf(c) > 0.0001f` as the test, normalized() as
(x*x + y*y) + z*z, np.sqrt, three float32 divisions, the zero vector staying zero.

`reference64` evaluates the same formula in float64, and `bounds` derives how far the float32
result may lie from it by counting roundings (u = 2^-24), as tests/skin_cases.py does for the
skinning alone:

  morphed position, per component: the shape term c_j * sp_j is rounded once as a product and once
  by each of the at most P - 1 later sums of bp and by the final pos + bp: at most P + 1 roundings.
  The base term passes the final sum, and in normalized mode the product pos * base_w, whose factor
  base_w = 1 - total carries the P - 1 sums of `total` and the subtraction (each bounded by u times
  the absolute sum 1 + sum |c_j|): at most P + 2.  So
      |dpos| <= (P + 3) u A_p,   A_p = |pos| (1 + sum |c_j|) + sum |c_j| |sp_j|
  (relative mode: A_p = |pos| + sum |c_j| |sp_j|), with one u of slack for the O(u^2) terms.
  The sum that enters normalized(), a = nrm * base_w + bn, is bounded the same way with A_n.

  normalized(): for exact input a the three squares, two sums, the square root and the division
  cost at most 3 u / 2 + u + u = 3.5 u relative on a component of magnitude <= 1: 4 u.  The input's
  own error moves the unit vector by at most 2 |da| / (|a| + |a + da|) <= |da| / (|a| - |da| / 2)
  (the Dunkl-Williams inequality in a Euclidean space), |.| the 2-norm.  So per component
      |dn| <= |da|_2 / (|a|_2 - |da|_2 / 2) + 4 u.

  skinning a perturbed vertex: the float32 chain on v + dv is within skin_cases.bound(K) * S(|v| + |dv|)
  of its exact value, which differs from the exact value on v by at most sum_j |M_ij| |dv_j| <=
  sum_k |w_k| sum_j |m_ij| |dv_j|.
"""
import numpy as np

from . import skin_cases as S

F = np.float32
U = 2.0 ** -24
THRESHOLD = F(0.0001)


def normalized(x, y, z):
    l = (x * x + y * y) + z * z
    if l == 0:
        return F(0), F(0), F(0)
    d = np.sqrt(l)
    return x / d, y / d, z / d


def morph_vertex(mode, pos, nrm, shape_pos, shape_nrm, c):
    """One vertex of one skeleton: pos, nrm [3]; shape_pos, shape_nrm [P][3]; c [P]; nrm and
    shape_nrm None for a mesh without normals.  mode 0 relative, 1 normalized.  -> (pos [3], nrm [3] or None)."""
    with np.errstate(all="ignore"):
        bp = [F(0), F(0), F(0)]
        bn = [F(0), F(0), F(0)]
        total = F(0)
        for j in range(len(c)):
            cj = F(c[j])
            if np.abs(cj) > THRESHOLD:
                for a in range(3):
                    bp[a] = bp[a] + F(shape_pos[j][a]) * cj
                if nrm is not None:
                    for a in range(3):
                        bn[a] = bn[a] + F(shape_nrm[j][a]) * cj
                total = total + cj
        p = [F(pos[a]) for a in range(3)]
        n = None if nrm is None else [F(nrm[a]) for a in range(3)]
        if mode == 1:
            base_w = F(1) - total
            p = [p[a] * base_w for a in range(3)]
            if n is not None:
                n = [n[a] * base_w for a in range(3)]
        p = [p[a] + bp[a] for a in range(3)]
        if n is not None:
            n = normalized(n[0] + bn[0], n[1] + bn[1], n[2] + bn[2])
        return np.array(p, F), None if n is None else np.array(n, F)


def morph_mesh(mode, pos, nrm, shape_pos, shape_nrm, c):
    """Every vertex of one skeleton with morph_vertex: -> (pos [V][3], nrm [V][3] or None)."""
    V = pos.shape[0]
    out_p = np.empty((V, 3), F)
    out_n = None if nrm is None else np.empty((V, 3), F)
    for v in range(V):
        p, n = morph_vertex(mode, pos[v], None if nrm is None else nrm[v], shape_pos[:, v],
                            None if nrm is None else shape_nrm[:, v], c)
        out_p[v] = p
        if n is not None:
            out_n[v] = n
    return out_p, out_n


def random_shapes(seed, P, V, normal_magnitude=0.1):
    """(shape positions [P][V][3] in [-0.5, 0.5], shape normals [P][V][3] of magnitude <= normal_magnitude)."""
    rng = np.random.default_rng(seed)
    sp = rng.uniform(-0.5, 0.5, (P, V, 3)).astype(F)
    d = rng.normal(0.0, 1.0, (P, V, 3))
    d /= np.linalg.norm(d, axis=2, keepdims=True)
    sn = (d * rng.uniform(0.0, normal_magnitude * 0.999, (P, V, 1))).astype(F)
    return sp, sn


def random_shape_weights(seed, count, P, mode):
    """[count][P] with sum |c_j| <= 2 per skeleton and, in normalized mode, |sum c_j| <= 0.5; about a
    third of the weights exactly 0 (skipped) unless P == 1."""
    rng = np.random.default_rng(seed)
    c = rng.uniform(-1.0, 1.0, (count, P))
    if P > 1:
        c[rng.uniform(0.0, 1.0, (count, P)) < 0.33] = 0.0
    c *= rng.uniform(0.5, 1.95, (count, 1)) / np.maximum(np.abs(c).sum(axis=1, keepdims=True), 1e-9)
    if mode == 1:
        t = c.sum(axis=1, keepdims=True)
        c *= np.minimum(1.0, 0.49 / np.maximum(np.abs(t), 1e-9))
    return c.astype(F)


def reference64(mode, pos, nrm, shape_pos, shape_nrm, c, idx, w, skin):
    """The formula in float64 and the bounds on the float32 result, all [count][V][3]:
    (positions, normals, bound on positions, bound on normals, min |nrm * base_w + bn|_2)."""
    K = idx.shape[1]
    P = shape_pos.shape[0]
    c64 = c.astype(np.float64)
    used = np.abs(c) > THRESHOLD                                   # the float32 test decides, as in the code
    cu = np.where(used, c64, 0.0)                                  # [count][P]
    total = cu.sum(axis=1)[:, None, None]
    abs_total = 1.0 + np.abs(cu).sum(axis=1)[:, None, None]
    base_w = 1.0 - total if mode == 1 else np.ones_like(total)
    base_a = abs_total if mode == 1 else np.ones_like(total)

    def morphed(base, shapes):
        b64, s64 = base.astype(np.float64), shapes.astype(np.float64)
        value = b64[None] * base_w + np.einsum("sp,pvi->svi", cu, s64)
        scale = np.abs(b64)[None] * base_a + np.einsum("sp,pvi->svi", np.abs(cu), np.abs(s64))
        return value, (P + 3) * U * scale

    p64, dp = morphed(pos, shape_pos)
    a64, da = morphed(nrm, shape_nrm)
    la = np.linalg.norm(a64, axis=2, keepdims=True)
    lda = np.linalg.norm(da, axis=2, keepdims=True)
    n64 = a64 / la
    dn = lda / (la - lda / 2.0) + 4.0 * U

    X = skin.astype(np.float64)[:, idx]                            # [count][V][K][12]
    w64 = w.astype(np.float64)[None, :, :, None]
    M = (X * w64).sum(axis=2)
    A = (np.abs(X) * np.abs(w64)).sum(axis=2)
    basis, origin = M[..., :9].reshape(M.shape[:2] + (3, 3)), M[..., 9:]
    abasis, aorigin = A[..., :9].reshape(A.shape[:2] + (3, 3)), A[..., 9:]
    rp = np.einsum("svij,svj->svi", basis, p64) + origin
    rn = np.einsum("svij,svj->svi", basis, n64)
    bp = S.bound(K) * (np.einsum("svij,svj->svi", abasis, np.abs(p64) + dp) + aorigin) + np.einsum("svij,svj->svi", abasis, dp)
    bn = S.bound(K) * np.einsum("svij,svj->svi", abasis, np.abs(n64) + dn) + np.einsum("svij,svj->svi", abasis, np.broadcast_to(dn, n64.shape))
    return rp, rn, bp, bn, float(la.min())
