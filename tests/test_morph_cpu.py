"""mbik_skin_vertices_shaped_cpu (blend shapes in front of the skinning, host only): the
bitwise numpy recipe, the weight threshold, the zero normal, the derived bound against float64, the
plain entry on the same arrays, and every argument error of the shaped entries.  No GPU."""
import ctypes as C

import numpy as np
import pytest

from many_bone_ik_amd import _lib
from many_bone_ik_amd.skinning import skin_vertices_cpu, synthetic_shapes

from . import morph_recipe as R
from . import skin_cases as S

MODES = {"relative": 0, "normalized": 1}
MAX_BONES = 3413   # MBIK_SKIN_MAX_BONES


def unit(n):
    return (n / np.linalg.norm(n.astype(np.float64), axis=1, keepdims=True)).astype(np.float32)


def per_skeleton_reference(mode, B, pos, nrm, idx, w, sp, sn, c, skin):
    """The recipe's morphed arrays of each skeleton through the plain entry, one skeleton a call."""
    out_p, out_n = [], []
    for s in range(skin.shape[0]):
        mp, mn = R.morph_mesh(MODES[mode], pos, nrm, sp, sn, c[s])
        p, n = skin_vertices_cpu(B, mp, idx, w, skin[s:s + 1], normals=mn)
        out_p.append(p[0])
        out_n.append(None if n is None else n[0])
    return np.stack(out_p), None if nrm is None else np.stack(out_n)


@pytest.mark.parametrize("P", [1, 3, 17])
@pytest.mark.parametrize("normals", [False, True], ids=["positions", "normals"])
@pytest.mark.parametrize("K", [4, 8])
@pytest.mark.parametrize("mode", ["relative", "normalized"])
def test_entry_equals_recipe_bitwise(mbik, mode, K, normals, P):
    """4 skeletons x 50 vertices a case, 4,800 (skeleton, vertex) pairs in all."""
    B, V, count = 7, 50, 4
    pos, nrm, idx, w = S.random_mesh(300 + P + K, B, V, K)
    sp, sn = R.random_shapes(310 + P, P, V, normal_magnitude=1.0)
    if not normals:
        nrm = sn = None
    c = R.random_shape_weights(320 + P, count, P, MODES[mode])
    skin = S.random_skin(330, count, B)
    got_p, got_n = skin_vertices_cpu(B, pos, idx, w, skin, normals=nrm, shape_positions=sp, shape_normals=sn, shape_mode=mode,
                                     shape_weights=c)
    ref_p, ref_n = per_skeleton_reference(mode, B, pos, nrm, idx, w, sp, sn, c, skin)
    assert S.same_bits(got_p, ref_p)
    assert (got_n is None and ref_n is None) or S.same_bits(got_n, ref_n)
    plain_p, _ = skin_vertices_cpu(B, pos, idx, w, skin, normals=nrm)
    assert not S.same_bits(got_p, plain_p)          # the shapes moved something


@pytest.mark.parametrize("mode", ["relative", "normalized"])
def test_threshold(mbik, mode):
    """One shape, one skeleton per weight: 0.0001f, NaN and 0 are skipped, the next float above
    0.0001f and -0.0002 are used, +inf is used and propagates."""
    B, V, K = 5, 40, 4
    pos, nrm, idx, w = S.random_mesh(41, B, V, K)
    pos[::4, 0], pos[1::4, 2] = -0.0, -0.0
    sp, sn = R.random_shapes(42, 1, V)
    assert (sp != 0).all() and (sn != 0).all()
    t = np.float32(0.0001)
    c = np.array([[t], [np.nextafter(t, np.float32(1))], [-0.0002], [np.nan], [np.inf], [0.0]], np.float32)
    skipped, used, infinite = [0, 3, 5], [1, 2], 4
    skin = np.broadcast_to(S.random_skin(43, 1, B), (len(c), B, 12)).copy()
    got_p, got_n = skin_vertices_cpu(B, pos, idx, w, skin, normals=nrm, shape_positions=sp, shape_normals=sn, shape_mode=mode,
                                     shape_weights=c)
    ref_p, ref_n = per_skeleton_reference(mode, B, pos, nrm, idx, w, sp, sn, c, skin)
    assert S.same_bits(got_p, ref_p) and S.same_bits(got_n, ref_n)
    # all skipped: the base's bits except that -0 becomes +0, and the renormalised base normal
    plus_zero = pos + np.float32(0.0)
    assert not np.signbit(plus_zero[pos == 0]).any() and np.array_equal(plus_zero, pos)
    unit_n = np.array([R.normalized(*n) for n in nrm], np.float32)
    base_p, base_n = skin_vertices_cpu(B, plus_zero, idx, w, skin[:1], normals=unit_n)
    for s in skipped:
        assert S.same_bits(got_p[s], base_p[0]) and S.same_bits(got_n[s], base_n[0]), s
    for s in used:
        assert (S.bits(got_p[s]) != S.bits(base_p[0])).any() and (S.bits(got_n[s]) != S.bits(base_n[0])).any(), s
        assert np.isfinite(got_p[s]).all() and np.isfinite(got_n[s]).all()
    assert not np.isfinite(got_p[infinite]).any() and not np.isfinite(got_n[infinite]).any()


def test_zero_normal(mbik):
    """A shape normal that cancels the base normal exactly: the zero vector stays zero through
    normalized(), and the skinned normal is that of a zero input."""
    B, V, K = 5, 30, 8
    pos, nrm, idx, w = S.random_mesh(51, B, V, K)
    sp, _ = R.random_shapes(52, 2, V)
    sn = np.stack([-nrm, np.zeros_like(nrm)])
    c = np.array([[1.0, 0.0], [1.0, 0.5]], np.float32)
    skin = S.random_skin(53, 2, B)
    got_p, got_n = skin_vertices_cpu(B, pos, idx, w, skin, normals=nrm, shape_positions=sp, shape_normals=sn, shape_weights=c)
    _, zero_n = skin_vertices_cpu(B, pos, idx, w, skin, normals=np.zeros_like(nrm))
    assert S.same_bits(got_n, zero_n) and np.isfinite(got_n).all()
    ref_p, ref_n = per_skeleton_reference("relative", B, pos, nrm, idx, w, sp, sn, c, skin)
    assert S.same_bits(got_p, ref_p) and S.same_bits(got_n, ref_n)


@pytest.mark.parametrize("P", [3, 17])
@pytest.mark.parametrize("K", [4, 8])
@pytest.mark.parametrize("mode", ["relative", "normalized"])
def test_bound_against_float64(mbik, mode, K, P):
    """Inputs on which float64 itself is well conditioned: unit base normals, shape normals of
    magnitude <= 0.1, sum |c_j| <= 2 and, in normalized mode, |total| <= 0.5.  The bound is derived
    in tests/morph_recipe.py."""
    B, V, count = 37, 2000, 3
    pos, nrm, idx, w = S.random_mesh(60 + K, B, V, K)
    nrm = unit(nrm)
    sp, sn = R.random_shapes(61 + P, P, V)
    c = R.random_shape_weights(62 + P, count, P, MODES[mode])
    assert (np.abs(c.astype(np.float64)).sum(axis=1) <= 2.0).all() and (np.linalg.norm(sn.astype(np.float64), axis=2) <= 0.1).all()
    assert mode == "relative" or (np.abs(c.astype(np.float64).sum(axis=1)) <= 0.5).all()
    skin = S.random_skin(63, count, B)
    got_p, got_n = skin_vertices_cpu(B, pos, idx, w, skin, normals=nrm, shape_positions=sp, shape_normals=sn, shape_mode=mode,
                                     shape_weights=c)
    rp, rn, bp, bn, least = R.reference64(MODES[mode], pos, nrm, sp, sn, c, idx, w, skin)
    ratio_p, ratio_n = (np.abs(got_p - rp) / bp).max(), (np.abs(got_n - rn) / bn).max()
    print(f"{mode} K={K} P={P}: worst error / bound: positions {ratio_p:.3f}, normals {ratio_n:.3f}; least |nrm * base_w + bn| {least:.3f}")
    assert least >= 0.3
    assert (np.abs(got_p - rp) <= bp).all()
    assert (np.abs(got_n - rn) <= bn).all()


def test_plain_entry_on_the_same_arrays(mbik):
    """mbik_skin_vertices_cpu on the base arrays is what it was: the shaped entry with every weight
    skipped gives its position bits, and its normals stay unnormalised."""
    B, V, K = 37, 500, 8
    pos, nrm, idx, w = S.random_mesh(71, B, V, K)
    skin = S.random_skin(72, 2, B)
    sp, sn = synthetic_shapes(pos, nrm, 3, seed=4)
    plain_p, plain_n = skin_vertices_cpu(B, pos, idx, w, skin, normals=nrm)
    shaped_p, shaped_n = skin_vertices_cpu(B, pos, idx, w, skin, normals=nrm, shape_positions=sp, shape_normals=sn,
                                           shape_weights=np.zeros((2, 3), np.float32))
    assert S.same_bits(plain_p, shaped_p) and not S.same_bits(plain_n, shaped_n)
    rp, rn, s_p, s_n = S.reference64(pos, nrm, idx, w, skin)
    assert (np.abs(plain_p - rp) <= S.bound(K) * s_p).all() and (np.abs(plain_n - rn) <= S.bound(K) * s_n).all()


def test_synthetic_shapes_are_deterministic_and_small(mbik):
    pos, nrm, _, _ = S.random_mesh(81, 5, 300, 4)
    a, b, c = synthetic_shapes(pos, nrm, 5, seed=1), synthetic_shapes(pos, nrm, 5, seed=1), synthetic_shapes(pos, nrm, 5, seed=2)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and not np.array_equal(a[0], c[0])
    assert a[0].shape == (5, 300, 3) and a[1].shape == (5, 300, 3) and a[0].dtype == np.float32 and a[1].dtype == np.float32
    assert np.abs(a[0]).max() < 0.1 and (np.linalg.norm(a[1], axis=2) <= 0.1 + 1e-6).all()
    assert synthetic_shapes(pos, None, 5, seed=1)[1] is None


# ---------------------------------------------------------------- argument errors


def shapes_struct(P, mode, sp, sn, size=None):
    return _lib.MbikMeshShapes(C.sizeof(_lib.MbikMeshShapes) if size is None else size, P, mode, S.ptr(sp), S.ptr(sn))


class Case:
    """A small valid shaped call; `raw` runs mbik_skin_vertices_shaped_cpu with overrides."""

    def __init__(self, B=5, V=9, K=4, P=3, count=2):
        self.B, self.V, self.K, self.P, self.count = B, V, K, P, count
        self.pos, self.nrm, self.idx, self.w = S.random_mesh(1, B, V, K)
        self.sp, self.sn = R.random_shapes(2, P, V)
        self.skin = S.random_skin(3, count, B)
        self.c = R.random_shape_weights(4, count, P, 0)
        self.out_p, self.out_n = np.zeros((count, V, 3), np.float32), np.zeros((count, V, 3), np.float32)

    def defaults(self):
        return dict(B=self.B, V=self.V, K=self.K, pos=self.pos, nrm=self.nrm, idx=self.idx, w=self.w,
                    shapes=shapes_struct(self.P, 0, self.sp, self.sn), count=self.count, skin=self.skin, c=self.c,
                    out_p=self.out_p, out_n=self.out_n)

    def raw(self, **kw):
        a = self.defaults()
        a.update(kw)
        sh = a["shapes"]
        return _lib.load().mbik_skin_vertices_shaped_cpu(
            a["B"], a["V"], a["K"], S.ptr(a["pos"]), S.ptr(a["nrm"]), S.ptr(a["idx"]), S.ptr(a["w"]),
            None if sh is None else C.byref(sh), a["count"], S.ptr(a["skin"]), S.ptr(a["c"]), S.ptr(a["out_p"]), S.ptr(a["out_n"]))

    def create(self, **kw):
        """mbik_mesh_create_shaped on device 0: (rc, handle)."""
        a = self.defaults()
        a.update(kw)
        sh, h = a["shapes"], C.c_void_p()
        rc = _lib.load().mbik_mesh_create_shaped(a["B"], a["V"], a["K"], S.ptr(a["pos"]), S.ptr(a["nrm"]), S.ptr(a["idx"]),
                                                 S.ptr(a["w"]), None if sh is None else C.byref(sh), 0, C.byref(h))
        return rc, h


def bad_shapes(cs):
    """(name, overrides) of every shapes argument both entries must refuse with MBIK_EINVAL."""
    yield "null struct", dict(shapes=None)
    yield "struct_size too small", dict(shapes=shapes_struct(cs.P, 0, cs.sp, cs.sn, size=C.sizeof(_lib.MbikMeshShapes) - 1))
    yield "struct_size zero", dict(shapes=shapes_struct(cs.P, 0, cs.sp, cs.sn, size=0))
    yield "no shapes", dict(shapes=shapes_struct(0, 0, cs.sp, cs.sn))
    yield "negative shape count", dict(shapes=shapes_struct(-1, 0, cs.sp, cs.sn))
    yield "mode 2", dict(shapes=shapes_struct(cs.P, 2, cs.sp, cs.sn))
    yield "mode -1", dict(shapes=shapes_struct(cs.P, -1, cs.sp, cs.sn))
    yield "null shape positions", dict(shapes=shapes_struct(cs.P, 0, None, cs.sn))
    yield "shape normals without mesh normals", dict(nrm=None, out_n=None)
    yield "mesh normals without shape normals", dict(shapes=shapes_struct(cs.P, 0, cs.sp, None))


def test_shaped_cpu_argument_errors(mbik):
    cs = Case()
    E, OK = _lib.MBIK_EINVAL, _lib.MBIK_OK
    assert cs.raw() == OK and cs.out_p.any() and cs.out_n.any()
    ref_p, ref_n = cs.out_p.copy(), cs.out_n.copy()
    for name, kw in bad_shapes(cs):
        assert cs.raw(**kw) == E, name
    # a larger struct_size (a later ABI's struct) is accepted
    assert cs.raw(shapes=shapes_struct(cs.P, 0, cs.sp, cs.sn, size=C.sizeof(_lib.MbikMeshShapes) + 8)) == OK
    # the call's own arguments
    assert cs.raw(c=None) == E                                                     # null weights
    assert "shape_weights" in _lib.last_error()
    buf = np.zeros(cs.count * cs.P + cs.count * cs.V * 3, np.float32)
    buf[:cs.count * cs.P] = cs.c.reshape(-1)
    assert cs.raw(c=buf, out_p=buf[cs.count * cs.P - 1:], nrm=None, out_n=None, shapes=shapes_struct(cs.P, 0, cs.sp, None)) == E
    assert cs.raw(c=buf, out_n=buf[cs.count * cs.P - 1:]) == E                     # weights overlap either output
    assert cs.raw(c=buf, out_n=buf[cs.count * cs.P:]) == OK                        # adjacent is fine
    assert S.same_bits(buf[cs.count * cs.P:].reshape(cs.count, cs.V, 3), ref_n)
    # everything the plain entry refuses
    assert cs.raw(skin=None) == E and cs.raw(out_p=None) == E and cs.raw(count=-1) == E
    assert cs.raw(K=3) == E and cs.raw(B=-1) == E and cs.raw(V=-1) == E
    assert cs.raw(pos=None) == E and cs.raw(idx=None) == E and cs.raw(w=None) == E
    i2 = cs.idx.copy()
    i2[8, 3] = cs.B
    assert cs.raw(idx=i2) == E and "bone index" in _lib.last_error()
    assert cs.raw(nrm=None, shapes=shapes_struct(cs.P, 0, cs.sp, None)) == E       # out_normals for a mesh without normals
    two = np.zeros(2 * cs.count * cs.V * 3, np.float32)
    assert cs.raw(out_p=two, out_n=two[cs.count * cs.V * 3 - 4:]) == E             # outputs overlap
    # nothing to do: MBIK_OK without touching anything, null weights included
    out = np.full((cs.count, cs.V, 3), 7.0, np.float32)
    assert cs.raw(count=0, c=None, skin=None, out_p=out, out_n=None) == OK and (out == 7.0).all()
    assert cs.raw(V=0, pos=None, idx=None, w=None, nrm=None, c=None, shapes=shapes_struct(cs.P, 0, None, None), out_p=out, out_n=None) == OK
    assert (out == 7.0).all()
    assert S.same_bits(cs.out_p, ref_p) and S.same_bits(cs.out_n, ref_n)


def test_create_shaped_argument_errors_before_any_device_query(mbik):
    """mbik_mesh_create_shaped makes every check of its arguments before it asks for a device, so the
    codes are the same with and without a GPU."""
    cs = Case()
    for name, kw in bad_shapes(cs):
        rc, h = cs.create(**kw)
        assert rc == _lib.MBIK_EINVAL and not h.value, name
    assert cs.create(K=3)[0] == _lib.MBIK_EINVAL and cs.create(pos=None)[0] == _lib.MBIK_EINVAL
    i2 = cs.idx.copy()
    i2[0, 0] = -1
    assert cs.create(idx=i2)[0] == _lib.MBIK_EINVAL
    rc, h = cs.create()
    assert rc in (_lib.MBIK_OK, _lib.MBIK_ENODEV)
    if rc == _lib.MBIK_OK:
        _lib.load().mbik_mesh_destroy(h)


def test_lds_limit(mbik):
    """B = 3413: four shape weights fit beside the matrices (163,824 + 16 = 160 KiB), five do not.  The
    refusal comes before the device query; the accepted mesh gets as far as that query.  The host
    entry has no such limit."""
    cs = Case(B=MAX_BONES, V=6, P=5, count=1)
    sh4, sh5 = shapes_struct(4, 0, cs.sp[:4].copy(), cs.sn[:4].copy()), shapes_struct(5, 0, cs.sp, cs.sn)
    rc, h = cs.create(shapes=sh5)
    assert rc == _lib.MBIK_EUNSUPPORTED and not h.value and "160 KiB" in _lib.last_error()
    rc, h = cs.create(shapes=sh4)
    assert rc in (_lib.MBIK_OK, _lib.MBIK_ENODEV)
    if rc == _lib.MBIK_OK:
        _lib.load().mbik_mesh_destroy(h)
    assert cs.create(B=MAX_BONES + 1, shapes=sh4)[0] == _lib.MBIK_EUNSUPPORTED
    assert cs.raw(shapes=sh5) == _lib.MBIK_OK and cs.raw(B=MAX_BONES + 1, skin=S.random_skin(5, 1, MAX_BONES + 1), shapes=sh5) == _lib.MBIK_OK
