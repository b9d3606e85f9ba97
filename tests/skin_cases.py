"""Inputs and references shared by the skinning tests (tests/test_skin_cpu.py, tests/test_gpu_skin.py).

The float64 reference evaluates DESIGN.md §14's formula in numpy and never calls the code under
test; the bound on the float32 result is derived from the chain's rounding count:

    a blended element is K products and K - 1 sums: at most 2K - 1 roundings,
    the transform adds 3 products, 2 sums and the origin's sum (normals: one fewer): at most 6,
    so |got - ref| <= (2K + 6) * 2^-24 * S, with a little slack over (2K + 5) u + O(u^2),
    S = sum_k |w_k| * (sum_j |m_ij| |v_j| + |o_i|)   (normals: without o).
"""
import ctypes as C

import numpy as np

from many_bone_ik_amd import _lib


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def same_bits(a, b):
    """Bitwise equal, two NaNs of any payload counting as equal."""
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    if a.shape != b.shape:
        return False
    na, nb = np.isnan(a), np.isnan(b)
    return bool(np.array_equal(na, nb) and np.array_equal(bits(a)[~na], bits(b)[~nb]))


def ptr(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def random_mesh(seed, B, V, K, weights="normalised"):
    """Arbitrary (not spatially sorted) mesh arrays: positions, normals, indices, weights."""
    rng = np.random.default_rng(seed)
    pos = rng.uniform(-2.0, 2.0, (V, 3)).astype(np.float32)
    nrm = rng.normal(0.0, 1.0, (V, 3)).astype(np.float32)
    idx = rng.integers(0, B, (V, K)).astype(np.int32)
    if weights == "normalised":
        w = rng.uniform(0.05, 1.0, (V, K))
        w /= w.sum(axis=1, keepdims=True)
    else:  # signed, sums anywhere
        w = rng.uniform(-1.5, 1.5, (V, K))
    return pos, nrm, idx, w.astype(np.float32)


def random_skin(seed, count, B):
    """Arbitrary affine transforms [count][B][12]."""
    return np.random.default_rng(seed).uniform(-1.5, 1.5, (count, B, 12)).astype(np.float32)


def reference64(pos, nrm, idx, w, skin):
    """(positions, normals, bound scale S for positions, S for normals), all float64 [count][V][3]."""
    X = skin.astype(np.float64)[:, idx]                          # [count][V][K][12]
    w64 = w.astype(np.float64)[None, :, :, None]
    M = (X * w64).sum(axis=2)                                    # [count][V][12]
    A = (np.abs(X) * np.abs(w64)).sum(axis=2)
    p, n = pos.astype(np.float64), nrm.astype(np.float64)
    basis, origin = M[..., :9].reshape(M.shape[:2] + (3, 3)), M[..., 9:]
    abasis, aorigin = A[..., :9].reshape(A.shape[:2] + (3, 3)), A[..., 9:]
    rp = np.einsum("svij,vj->svi", basis, p) + origin
    rn = np.einsum("svij,vj->svi", basis, n)
    sp = np.einsum("svij,vj->svi", abasis, np.abs(p)) + aorigin
    sn = np.einsum("svij,vj->svi", abasis, np.abs(n))
    return rp, rn, sp, sn


def bound(K):
    return (2 * K + 6) * 2.0 ** -24


def skin_cpu_raw(B, pos, nrm, idx, w, skin, K=None, count=None, want_normals=None, out_p=None, out_n=None):
    """mbik_skin_vertices_cpu through ctypes with any argument combination: (rc, out_p, out_n)."""
    L = _lib.load()
    V = 0 if pos is None else pos.shape[0]
    K = idx.shape[1] if K is None else K
    count = skin.shape[0] if count is None else count
    if want_normals is None:
        want_normals = nrm is not None
    if out_p is None:
        out_p = np.full((max(count, 0), V, 3), np.nan, np.float32)
    if out_n is None and want_normals:
        out_n = np.full((max(count, 0), V, 3), np.nan, np.float32)
    rc = L.mbik_skin_vertices_cpu(B, V, K, ptr(pos), ptr(nrm), ptr(idx), ptr(w), count, ptr(skin), ptr(out_p), ptr(out_n))
    return rc, out_p, out_n
