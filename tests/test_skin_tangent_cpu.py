"""mbik_skin_vertices_call_cpu and mbik_mesh_create_desc without a GPU (include/mbik.h): the tangent
stream against a float32 recipe that does not call the code (tests/tangent_recipe.py), against the EXISTING _cpu
entries fed the tangents as normals, against float64 references with the derived bounds of tests/skin_cases.py and
tests/morph_recipe.py, special values, and every refusal with its text.  Bitwise compares use skin_cases.same_bits (two
NaNs count as equal); the sign w is compared bit for bit, NaN payloads included."""
import ctypes as C
import os

import numpy as np
import pytest

from many_bone_ik_amd import _lib
from many_bone_ik_amd.skinning import (_skin_call, skin_vertices_cpu, skin_vertices_listed_cpu, synthetic_mesh, synthetic_shape_tangents,
                                       synthetic_shapes, synthetic_tangents)

from . import morph_recipe as MR
from . import skin_cases as S
from . import tangent_recipe as T

F = np.float32
U = 2.0 ** -24
# (V, B, P, count): every V, B and P of the recipe test; the largest mesh has the fewest skeletons
SHAPES = [(1, 32, 17, 5), (63, 32, 3, 4), (257, 1, 17, 2)]
FORMS = ["range", "in_place", "compact"]


def bits_equal(a, b):
    return np.array_equal(np.ascontiguousarray(a, F).view(np.uint32), np.ascontiguousarray(b, F).view(np.uint32))


def a_list(count):
    """Duplicates, -1 and `count` among valid entries; longer than the batch."""
    return np.array([count - 1, -1, 0, count, 0, count - 1, 0][:count + 3], np.int32)


def form_kw(form, count):
    if form == "range":
        return {}
    ind = a_list(count)
    return dict(indices=ind, list_count=len(ind) - 1, max_list=len(ind), compact=form == "compact")


# ---------------- 1. the recipe ----------------
@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("mode", [None, "relative", "normalized"], ids=["plain", "relative", "normalized"])
@pytest.mark.parametrize("K", [4, 8])
def test_matches_the_recipe(mbik, K, mode, form):
    for V, B, P, count in SHAPES:
        case = T.Case(100 + 10 * K + V, B, V, K, count, P=P if mode else 0, mode=mode or "relative", special_weights=bool(mode))
        desc, _keep = case.desc()
        kw = form_kw(form, count)
        rc, out_p, out_n, out_t = T.call_cpu(desc, count, case.skin, V, shape_weights=case.cw if mode else None, **kw)
        assert rc == 0, T.last_error()
        named = range(count) if form == "range" else [s for s in kw["indices"][:kw["list_count"]] if 0 <= s < count]
        rows = T.skin_rows(case, named, bool(mode))
        for i, (got, width) in enumerate(((out_p, 3), (out_n, 3), (out_t, 4))):
            want = T.place({s: r[i] for s, r in rows.items()}, width, count, V, kw.get("indices"), kw.get("list_count", 0),
                           kw.get("max_list", 0), kw.get("compact", False))
            assert S.same_bits(got, want), (V, B, P, i)
        want_w = T.place({s: r[2] for s, r in rows.items()}, 4, count, V, kw.get("indices"), kw.get("list_count", 0), kw.get("max_list", 0),
                         kw.get("compact", False))[..., 3]
        assert bits_equal(out_t[..., 3], want_w)


# ---------------- 2. the existing entries as oracle ----------------
def existing(case, form, shaped, normals, shape_normals):
    """The existing _cpu entry of the form on `normals` / `shape_normals`: (positions, normals), SENTINEL where unwritten."""
    kw = dict(normals=normals)
    if case.P:
        kw.update(shape_positions=case.sp, shape_normals=shape_normals, shape_mode=case.mode)
    if shaped:
        kw.update(shape_weights=case.cw)
    if form == "range":
        if not shaped:
            kw = dict(normals=normals)
        return skin_vertices_cpu(case.B, case.pos, case.idx, case.w, case.skin, **kw)
    f = form_kw(form, case.count)
    rows = f["max_list"] if f["compact"] else case.count
    out_p, out_n = np.full((rows, case.V, 3), T.SENTINEL, F), np.full((rows, case.V, 3), T.SENTINEL, F)
    return skin_vertices_listed_cpu(case.B, case.pos, case.idx, case.w, case.skin, f["indices"], f["list_count"], max_list=f["max_list"],
                                    compact=f["compact"], out_positions=out_p, out_normals=out_n, **kw)


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("mode", [None, "relative", "normalized"], ids=["plain", "relative", "normalized"])
@pytest.mark.parametrize("K", [4, 8])
def test_tangents_as_normals_through_the_existing_entries(mbik, K, mode, form):
    """out_tangents.xyz is what the existing entry writes as normals when it is given the tangents as normals and the shape
    tangents as shape normals; w is tangents[:, 3]; positions and normals of the same call are the existing entry's; and with
    out_tangents NULL the call is the existing entry."""
    V, B, P, count = 63, 32, 3, 4
    case = T.Case(200 + K, B, V, K, count, P=P if mode else 0, mode=mode or "relative", special_weights=bool(mode))
    desc, _keep = case.desc()
    kw = form_kw(form, count)
    cw = case.cw if mode else None
    rc, out_p, out_n, out_t = T.call_cpu(desc, count, case.skin, V, shape_weights=cw, **kw)
    assert rc == 0, T.last_error()
    ref_p, ref_n = existing(case, form, bool(mode), case.nrm, case.sn)
    as_p, as_n = existing(case, form, bool(mode), np.ascontiguousarray(case.tan[:, :3]), case.st)
    assert S.same_bits(out_p, ref_p) and S.same_bits(out_n, ref_n) and S.same_bits(as_p, ref_p)
    assert S.same_bits(out_t[..., :3], as_n)
    written = out_p[:, 0, 0] != F(T.SENTINEL)
    assert written.any() and bits_equal(out_t[written][..., 3], np.broadcast_to(case.tan[:, 3], (int(written.sum()), V)))
    assert (out_t[~written] == F(T.SENTINEL)).all()
    # out_tangents NULL, on the mesh with tangents and on the one without
    for tangents in (True, False):
        d2, _k2 = case.desc(tangents=tangents)
        rc, p2, n2, t2 = T.call_cpu(d2, count, case.skin, V, shape_weights=cw, tangents=False, **kw)
        assert rc == 0 and t2 is None and S.same_bits(p2, ref_p) and S.same_bits(n2, ref_n)
    # positions only
    rc, p3, n3, _ = T.call_cpu(desc, count, case.skin, V, shape_weights=cw, tangents=False, normals=False, **kw)
    assert rc == 0 and n3 is None and S.same_bits(p3, ref_p)


def test_shaped_mesh_without_shape_weights_uses_the_base_tangents(mbik):
    case = T.Case(230, 32, 63, 4, 3, P=3)
    desc, _keep = case.desc()
    for form in FORMS:
        rc, _, _, out_t = T.call_cpu(desc, 3, case.skin, 63, **form_kw(form, 3))
        assert rc == 0
        plain = T.Case(230, 32, 63, 4, 3)                         # the same base arrays, no shapes
        _, as_n = existing(plain, form, False, np.ascontiguousarray(case.tan[:, :3]), None)
        assert S.same_bits(out_t[..., :3], as_n)                   # not renormalised: the plain entry never does


def test_python_wrappers_return_the_third_array(mbik):
    case = T.Case(240, 5, 17, 4, 3, P=3)
    p, n, t = skin_vertices_cpu(case.B, case.pos, case.idx, case.w, case.skin, shape_weights=case.cw, **case.mesh_kw())
    desc, _keep = case.desc()
    rc, rp, rn, rt = T.call_cpu(desc, 3, case.skin, 17, shape_weights=case.cw)
    assert rc == 0 and S.same_bits(p, rp) and S.same_bits(n, rn) and S.same_bits(t, rt)
    ind = np.array([2, 0], np.int32)
    lp, ln, lt = skin_vertices_listed_cpu(case.B, case.pos, case.idx, case.w, case.skin, ind, 2, compact=True, shape_weights=case.cw,
                                          **case.mesh_kw())
    assert S.same_bits(lt, rt[[2, 0]]) and S.same_bits(lp, rp[[2, 0]]) and S.same_bits(ln, rn[[2, 0]])


# ---------------- 3. float64 ----------------
@pytest.mark.parametrize("K", [4, 8])
def test_unshaped_float64_bound(mbik, K):
    """skin_cases.reference64 on the tangent array: the tangent's chain is the normal's, so its bound is."""
    for weights in ("normalised", "signed"):
        case = T.Case(300 + K, 32, 257, K, 3, weights=weights)
        desc, _keep = case.desc()
        rc, _, _, out_t = T.call_cpu(desc, 3, case.skin, 257)
        assert rc == 0
        _, rt, _, st = S.reference64(case.pos, case.tan[:, :3], case.idx, case.w, case.skin)
        assert (np.abs(out_t[..., :3].astype(np.float64) - rt) <= S.bound(K) * st).all()


@pytest.mark.parametrize("mode", ["relative", "normalized"])
@pytest.mark.parametrize("K,P", [(4, 3), (8, 17)])
def test_shaped_float64_bound(mbik, K, P, mode):
    """morph_recipe.reference64 and its bounds on the tangent arrays, with that module's input conditions: unit base vectors,
    shape vectors of norm <= 0.1, sum |c| <= 2 and, normalized, |total| <= 0.5 (T.Case draws them so)."""
    case = T.Case(320 + K, 32, 257, K, 3, P=P, mode=mode)
    desc, _keep = case.desc()
    rc, _, _, out_t = T.call_cpu(desc, 3, case.skin, 257, shape_weights=case.cw)
    assert rc == 0
    _, rt, _, bt, least = MR.reference64(case.mode_id, case.pos, case.tan[:, :3], case.sp, case.st, case.cw, case.idx, case.w, case.skin)
    assert least > 0.25          # (1 - 0.5) - 2 * 0.1: the vector in front of normalized() is nowhere near zero
    assert (np.abs(out_t[..., :3].astype(np.float64) - rt) <= bt).all()


@pytest.mark.parametrize("K", [4, 8])
def test_a_rigid_transform_keeps_the_angle(mbik, K):
    """One rotation plus translation on every bone, normalised weights: out_n . out_t equals n . t.

    Bound: with rn, rt the exact images of n and t under the blended float32 matrices (skin_cases.reference64) and
    bn_i = bound(K) * Sn_i, bt_i likewise, |out_n . out_t - rn . rt| <= sum_i (|rn_i| bt_i + |rt_i| bn_i + bn_i bt_i), the derived
    per-component bound carried through the three products.  rn . rt itself is sigma^2 n^T R32^T R32 t with sigma = sum_k w_k:
    R32 is the float32 rounding of a rotation, |E_ij| <= u, so |n^T (R32^T R32 - I) t| <= (2 sqrt(3) u + 3 u^2) |n| |t|, and the
    float32 weights w_k = fl(raw_k / sum) give |sigma - 1| <= u, |sigma^2 - 1| <= 2 u + u^2: together under 6 u |n| |t|."""
    rng = np.random.default_rng(340 + K)
    B, V, count = 32, 257, 3
    case = T.Case(340 + K, B, V, K, count)
    for s in range(count):
        q = rng.normal(0.0, 1.0, 4)
        q /= np.linalg.norm(q)
        w, x, y, z = q
        R = np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                      [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                      [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])
        case.skin[s, :, :9] = R.reshape(9).astype(F)
        case.skin[s, :, 9:] = rng.uniform(-3.0, 3.0, 3).astype(F)
    desc, _keep = case.desc()
    rc, _, out_n, out_t = T.call_cpu(desc, count, case.skin, V)
    assert rc == 0
    _, rn, _, sn = S.reference64(case.pos, case.nrm, case.idx, case.w, case.skin)
    _, rt, _, st = S.reference64(case.pos, case.tan[:, :3], case.idx, case.w, case.skin)
    bn, bt = S.bound(K) * sn, S.bound(K) * st
    got = (out_n.astype(np.float64) * out_t[..., :3].astype(np.float64)).sum(axis=2)
    n64, t64 = case.nrm.astype(np.float64), case.tan[:, :3].astype(np.float64)
    want = (n64 * t64).sum(axis=1)[None]
    limit = (np.abs(rn) * bt + np.abs(rt) * bn + bn * bt).sum(axis=2) + 6 * U * (np.linalg.norm(n64, axis=1) * np.linalg.norm(t64, axis=1))[None]
    assert (np.abs(got - want) <= limit).all()
    assert limit.max() < 1e-5 and np.abs(want).max() > 0.5       # a real statement about angles that differ


def test_synthetic_generators(mbik):
    parents = [-1, 0, 1, 1, 3, 0, 5]
    rest = np.zeros((7, 12), F)
    rest[:, [0, 4, 8]] = 1
    rest[:, 9] = np.arange(7)
    pos, nrm, idx, w = synthetic_mesh(parents, rest, 300, 4, seed=5)
    tan = synthetic_tangents(pos, nrm, seed=6)
    assert tan.dtype == F and tan.shape == (300, 4) and set(np.unique(tan[:, 3]).tolist()) == {-1.0, 1.0}
    assert np.abs(np.linalg.norm(tan[:, :3].astype(np.float64), axis=1) - 1).max() < 1e-6
    assert np.abs((tan[:, :3].astype(np.float64) * nrm).sum(axis=1)).max() < 1e-6
    st = synthetic_shape_tangents(tan, 5, seed=7)
    assert st.dtype == F and st.shape == (5, 300, 3) and np.linalg.norm(st.astype(np.float64), axis=2).max() <= 0.1 + 1e-7
    assert np.array_equal(tan, synthetic_tangents(pos, nrm, seed=6)) and not np.array_equal(tan, synthetic_tangents(pos, nrm, seed=8))
    # the existing generators return what they returned: the tangent generators draw from streams of their own
    again = synthetic_mesh(parents, rest, 300, 4, seed=5)
    assert all(np.array_equal(a, b) for a, b in zip((pos, nrm, idx, w), again))
    sp, sn = synthetic_shapes(pos, nrm, 5, seed=9)
    assert sp.shape == (5, 300, 3) and sn.shape == (5, 300, 3)


# ---------------- 4. special values ----------------
def test_the_sign_travels_as_bits(mbik):
    """-0, a signalling and a quiet NaN with payloads, +-inf, denormals: out_tangents.w is the same 32 bits, in every form."""
    patterns = np.array([0x80000000, 0x7FA12345, 0xFFC00001, 0x7F800000, 0xFF800000, 0x00000001, 0x807FFFFF, 0x00000000, 0xBF800000],
                        np.uint32)
    for mode in (None, "relative", "normalized"):
        case = T.Case(400, 5, 40, 4, 3, P=3 if mode else 0, mode=mode or "relative")
        case.tan.view(np.uint32)[:, 3] = np.resize(patterns, 40)
        desc, _keep = case.desc()
        for form in FORMS:
            rc, out_p, _, out_t = T.call_cpu(desc, 3, case.skin, 40, shape_weights=case.cw if mode else None, **form_kw(form, 3))
            assert rc == 0
            written = out_p[:, 0, 0] != F(T.SENTINEL)
            assert written.any()
            assert np.array_equal(out_t[written].view(np.uint32)[..., 3], np.broadcast_to(np.resize(patterns, 40), (int(written.sum()), 40)))
            assert np.isfinite(out_t[written][..., :3]).all()     # and it reached no arithmetic


@pytest.mark.parametrize("mode", [None, "relative", "normalized"], ids=["plain", "relative", "normalized"])
def test_non_finite_tangents_go_where_the_normals_arithmetic_sends_them(mbik, mode):
    case = T.Case(410, 5, 40, 8, 3, P=3 if mode else 0, mode=mode or "relative")
    case.tan[3, 0], case.tan[7, 1], case.tan[11, 2], case.tan[12, :3] = np.inf, -np.inf, np.nan, 0.0
    if mode:
        case.st[1, 20, 0], case.st[2, 21, 2] = np.nan, np.inf
    desc, _keep = case.desc()
    rc, _, _, out_t = T.call_cpu(desc, 3, case.skin, 40, shape_weights=case.cw if mode else None)
    assert rc == 0
    _, as_n = existing(case, "range", bool(mode), np.ascontiguousarray(case.tan[:, :3]), case.st)
    assert S.same_bits(out_t[..., :3], as_n) and not np.isfinite(out_t[:, [3, 7, 11], :3]).all()
    assert np.isfinite(out_t[:, 0, :3]).all()


@pytest.mark.parametrize("mode", ["relative", "normalized"])
def test_all_weights_skipped_gives_the_renormalised_base_tangent(mbik, mode):
    """Every weight under the threshold, zero or NaN: bt stays (0,0,0), total 0, base_w 1, and the tangent that reaches the bone
    transform is normalized(t + 0), by morph_recipe.normalized, skinned by the EXISTING plain entry as a normal."""
    case = T.Case(420, 5, 40, 4, 3, P=3, mode=mode)
    case.cw[0], case.cw[1], case.cw[2] = 0.0, (0.00005, -0.0001, np.nan), (np.nan, 0.0, -0.0)
    case.tan[:, :3] *= F(1.7)                                       # not unit: the renormalisation shows
    case.tan[5, :3] = 0.0                                           # the zero vector stays zero
    desc, _keep = case.desc()
    rc, _, _, out_t = T.call_cpu(desc, 3, case.skin, 40, shape_weights=case.cw)
    assert rc == 0
    base = np.array([MR.normalized(*(t + F(0) for t in case.tan[v, :3])) for v in range(40)], F)
    _, want = skin_vertices_cpu(case.B, case.pos, case.idx, case.w, case.skin, normals=base)
    assert S.same_bits(out_t[..., :3], want) and not out_t[:, 5, :3].any()
    assert np.abs(np.linalg.norm(base[6].astype(np.float64)) - 1) < 1e-6


# ---------------- 5. refusals ----------------
def test_call_refusals_and_their_texts(mbik):
    """Every refusal of the call through mbik_skin_vertices_call_cpu; tests/test_gpu_skin_tangent.py sends the same table
    through the device entry and compares the texts with these."""
    L = _lib.load()
    B, V, P, n, M = 5, 9, 2, 3, 4
    lay = T.RefusalLayout(B, V, P, n, M)
    buf = np.zeros(lay.words, F)
    case = T.Case(500, B, V, 4, n, P=P)
    plain_case = T.Case(500, B, V, 4, n)
    descs = {"tan": plain_case.desc(), "shaped_tan": case.desc(), "normals": plain_case.desc(tangents=False)}
    d = plain_case.desc(tangents=False)
    d[0].normals = None
    descs["plain"] = d

    def run(mesh, skin, cw, ind, cnt, p, q, t, count, max_list, flags, struct_size):
        at = lambda o: None if o is None else buf.ctypes.data + 4 * o
        call = _skin_call(count, at(skin), at(p), at(q), at(t), at(cw), at(ind), at(cnt), max_list, flags)
        if struct_size is not None:
            call.struct_size = struct_size
        rc = L.mbik_skin_vertices_call_cpu(C.byref(descs[mesh][0]), C.byref(call))
        return rc, T.last_error()

    seen = T.call_refusals(lay, run)
    assert len(seen) >= 20
    # a null call, through both entries (the device entry refuses it before it looks at its mesh)
    good = descs["tan"][0]
    assert L.mbik_skin_vertices_call_cpu(C.byref(good), None) == _lib.MBIK_EINVAL and T.last_error() == "null call"
    assert L.mbik_skin_vertices_call(None, None, None) == _lib.MBIK_EINVAL and T.last_error() == "null call"
    small = _skin_call(n, buf.ctypes.data, buf.ctypes.data)
    small.struct_size = C.sizeof(_lib.MbikSkinCall) - 1
    assert L.mbik_skin_vertices_call(None, C.byref(small), None) == _lib.MBIK_EINVAL
    assert T.last_error() == "mbik_skin_call.struct_size is too small"
    small.struct_size += 1
    assert L.mbik_skin_vertices_call(None, C.byref(small), None) == _lib.MBIK_EINVAL and T.last_error() == "null mesh"


def test_desc_refusals_through_both_entries(mbik):
    """The descriptor's refusals through mbik_skin_vertices_call_cpu and through mbik_mesh_create_desc, which makes them
    before it asks for a device: equal codes and texts."""
    L = _lib.load()
    case = T.Case(510, 5, 9, 4, 2, P=2)
    out = np.zeros(2 * 9 * 3, F)
    call = _skin_call(2, S.ptr(case.skin), S.ptr(out))

    def cpu(d):
        return L.mbik_skin_vertices_call_cpu(None if d is None else C.byref(d), C.byref(call)), T.last_error()

    def create(d):
        h = C.c_void_p(1)
        rc = L.mbik_mesh_create_desc(None if d is None else C.byref(d), 0, C.byref(h))
        assert h.value is None                                      # *out_mesh is cleared
        return rc, T.last_error()

    assert T.desc_refusals(case, cpu) == T.desc_refusals(case, create)
    good, _keep = case.desc()
    assert L.mbik_mesh_create_desc(C.byref(good), 0, None) == _lib.MBIK_EINVAL and T.last_error() == "null out_mesh"


def test_nothing_to_do_returns_ok(mbik):
    L = _lib.load()
    case = T.Case(520, 5, 9, 4, 2)
    desc, _keep = case.desc()
    one = np.zeros(1, np.int32)
    for call in (_skin_call(0, None, None), _skin_call(2, None, None, indices=S.ptr(one), list_count=S.ptr(one), max_list=0, flags=1)):
        assert L.mbik_skin_vertices_call_cpu(C.byref(desc), C.byref(call)) == _lib.MBIK_OK
    empty = T.Case(521, 5, 0, 4, 2)
    d0, _k0 = empty.desc()
    call = _skin_call(2, None, None)
    assert L.mbik_skin_vertices_call_cpu(C.byref(d0), C.byref(call)) == _lib.MBIK_OK


def test_abi_version_stays_15():
    src = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "mbik.h")).read()
    assert "#define MBIK_ABI_VERSION 15" in src
    for name in ("mbik_mesh_create_desc", "mbik_skin_vertices_call", "mbik_skin_vertices_call_cpu"):
        assert name in _lib.EXPORTED_SYMBOLS
