"""The tangent stream of mbik_skin_vertices_call (include/mbik.h) written once more without the
code under test, for tests/test_skin_tangent_cpu.py and tests/test_gpu_skin_tangent.py, with the inputs and
the raw ctypes calls the two files share.

`tangent_vertex` restates the header's steps in numpy float32 scalars, one IEEE operation at a time: the
shape step is tests/morph_recipe.py's `morph_vertex` with the tangent's xyz in the normal's place (the
position part of its result is the position's own, by the same loop), the blend is M = X_0 * w_0, then
M = M + X_k * w_k in influence order, the transform ((r.x*v.x + r.y*v.y) + r.z*v.z) per row without the
origin, and w is copied as bits.  `skin_rows` applies it to whole skeletons and `place` puts rows where a
range or a listed call writes them.
"""
import ctypes as C

import numpy as np

from many_bone_ik_amd import _lib
from many_bone_ik_amd.skinning import _mesh_desc, _skin_call

from . import morph_recipe as MR
from . import skin_cases as S
from .morph_recipe import morph_vertex, normalized  # noqa: F401 (the recipe's two primitives, unchanged)

F = np.float32
SENTINEL = -12345.678


# ---------------- the recipe ----------------
def blend(skin_s, idx_v, w_v):
    """M [12] of one vertex of one skeleton: skin_s [B][12] float32."""
    m = [F(skin_s[idx_v[0]][e]) * F(w_v[0]) for e in range(12)]
    for k in range(1, len(idx_v)):
        wk = F(w_v[k])
        m = [m[e] + F(skin_s[idx_v[k]][e]) * wk for e in range(12)]
    return m


def xform_basis(m, v):
    return [(m[3 * r] * v[0] + m[3 * r + 1] * v[1]) + m[3 * r + 2] * v[2] for r in range(3)]


def xform(m, v):
    return [((m[3 * r] * v[0] + m[3 * r + 1] * v[1]) + m[3 * r + 2] * v[2]) + m[9 + r] for r in range(3)]


def tangent_vertex(skin_s, idx_v, w_v, pos, nrm, tan4, mode=None, shape_pos=None, shape_nrm=None, shape_tan=None, c=None):
    """One vertex of one skeleton -> (position [3], normal [3], tangent [4]) float32.  mode None: no shape step;
    0 relative, 1 normalized with shape_pos / shape_nrm / shape_tan [P][3] and c [P]."""
    with np.errstate(all="ignore"):
        p = [F(x) for x in pos]
        n = [F(x) for x in nrm]
        t = [F(x) for x in tan4[:3]]
        if mode is not None:
            p, n = morph_vertex(mode, pos, nrm, shape_pos, shape_nrm, c)
            _, t = morph_vertex(mode, pos, tan4[:3], shape_pos, shape_tan, c)   # (the normal's steps on the tangent's records)
        m = blend(skin_s, idx_v, w_v)
        out_t = np.empty(4, F)
        out_t[:3] = xform_basis(m, t)
        out_t.view(np.uint32)[3] = np.asarray(tan4, F).view(np.uint32)[3]      # the bits, never a float operation
        return np.array(xform(m, p), F), np.array(xform_basis(m, n), F), out_t


def skin_rows(case, skeletons, shaped):
    """{s: (positions [V][3], normals [V][3], tangents [V][4])} by tangent_vertex for the skeletons named."""
    rows = {}
    for s in sorted(set(int(x) for x in skeletons)):
        p, n, t = np.empty((case.V, 3), F), np.empty((case.V, 3), F), np.empty((case.V, 4), F)
        for v in range(case.V):
            kw = {}
            if shaped:
                kw = dict(mode=case.mode_id, shape_pos=case.sp[:, v], shape_nrm=case.sn[:, v], shape_tan=case.st[:, v], c=case.cw[s])
            p[v], n[v], t[v] = tangent_vertex(case.skin[s], case.idx[v], case.w[v], case.pos[v], case.nrm[v], case.tan[v], **kw)
        rows[s] = (p, n, t)
    return rows


def list_length(list_count, max_list):
    return min(max(int(list_count), 0), int(max_list))


def place(full, width, count, V, indices=None, list_count=0, max_list=0, compact=False):
    """full: [count][V][width] array or {s: [V][width]}.  -> what a call leaves in a buffer of SENTINEL: every row for
    the range call (indices None), the listed rows by include/mbik.h's rule otherwise."""
    if indices is None:
        return np.stack([full[s] for s in range(count)]).astype(F) if count else np.empty((0, V, width), F)
    out = np.full(((max_list if compact else count), V, width), SENTINEL, F)
    for r in range(list_length(list_count, max_list)):
        s = int(indices[r])
        if 0 <= s < count:
            out[r if compact else s] = full[s]
    return out


# ---------------- inputs ----------------
def random_tangents(seed, nrm):
    """[V][4]: unit xyz (any direction: the arithmetic does not care) and a sign of +1 or -1."""
    rng = np.random.default_rng(seed)
    t = rng.normal(0.0, 1.0, (nrm.shape[0], 3))
    t /= np.linalg.norm(t, axis=1, keepdims=True)
    sign = np.where(rng.uniform(0, 1, (nrm.shape[0], 1)) < 0.5, -1.0, 1.0)
    return np.concatenate([t, sign], axis=1).astype(F)


class Case:
    """A random mesh with unit normals and tangents, optionally shaped (shape normals and tangents of norm <= 0.1,
    weights by morph_recipe.random_shape_weights: morph_recipe.reference64's input conditions), and `count` skeletons."""

    def __init__(self, seed, B, V, K, count, P=0, mode="relative", special_weights=False, weights="normalised"):
        self.B, self.V, self.K, self.count, self.P, self.mode = B, V, K, count, P, mode
        self.mode_id = 0 if mode == "relative" else 1
        self.pos, nrm, self.idx, self.w = S.random_mesh(seed, B, V, K, weights=weights)
        self.nrm = (nrm / np.maximum(np.linalg.norm(nrm.astype(np.float64), axis=1, keepdims=True), 1e-12)).astype(F)
        self.tan = random_tangents(seed + 7, self.nrm)
        self.skin = S.random_skin(seed + 1, count, B)
        self.sp = self.sn = self.st = self.cw = None
        if P:
            self.sp, self.sn = MR.random_shapes(seed + 2, P, V)
            _, self.st = MR.random_shapes(seed + 5, P, V)
            self.cw = MR.random_shape_weights(seed + 3, count, P, self.mode_id).astype(F)
            if special_weights:   # below the shader's threshold, NaN, and whole skeletons with every weight skipped
                self.cw[::3, 0] = 0.00005
                self.cw[1::5, P - 1] = np.nan
                self.cw[2::7, :] = 0.0

    def mesh_kw(self, tangents=True):
        kw = dict(normals=self.nrm)
        if self.P:
            kw.update(shape_positions=self.sp, shape_normals=self.sn, shape_mode=self.mode)
        if tangents:
            kw.update(tangents=self.tan)
            if self.P:
                kw.update(shape_tangents=self.st)
        return kw

    def shapes(self, normals=None):
        """(mbik_mesh_shapes, keep-alive) with `normals` in the shape normals' place (default: the shape normals)."""
        if not self.P:
            return None, ()
        sn = self.sn if normals is None else normals
        return _lib.MbikMeshShapes(C.sizeof(_lib.MbikMeshShapes), self.P, self.mode_id, S.ptr(self.sp), S.ptr(sn)), (self.sp, sn)

    def desc(self, tangents=True):
        """(mbik_mesh_desc, keep-alive)."""
        sh, keep = self.shapes()
        d = _mesh_desc(self.B, self.pos, self.idx, self.w, self.nrm, self.tan if tangents else None, sh,
                       self.st if tangents and self.P else None)
        return d, (sh, keep)


def call_cpu(desc, count, skin, V, shape_weights=None, indices=None, list_count=None, max_list=0, compact=False, tangents=True,
             normals=True, rows=None):
    """mbik_skin_vertices_call_cpu into buffers of SENTINEL: (rc, out_p, out_n, out_t)."""
    L = _lib.load()
    if rows is None:
        rows = count if indices is None or not compact else max_list
    out_p = np.full((rows, V, 3), SENTINEL, F)
    out_n = np.full((rows, V, 3), SENTINEL, F) if normals else None
    out_t = np.full((rows, V, 4), SENTINEL, F) if tangents else None
    cnt = None if list_count is None else np.asarray([int(list_count)], np.int32)
    ind = None if indices is None else np.ascontiguousarray(indices, np.int32)
    call = _skin_call(count, S.ptr(skin), S.ptr(out_p), S.ptr(out_n), S.ptr(out_t), S.ptr(shape_weights), S.ptr(ind), S.ptr(cnt), max_list,
                      _lib.SKIN_LIST_COMPACT if compact else 0)
    rc = L.mbik_skin_vertices_call_cpu(C.byref(desc), C.byref(call))
    return rc, out_p, out_n, out_t


def last_error():
    return _lib.load().mbik_last_error().decode()


# ---------------- refusals (both entries, equal texts) ----------------
class RefusalLayout:
    """One buffer of 4-byte words that holds every argument of a call on a mesh of B bones, V vertices, P shapes for n
    skeletons and lists of M entries, each area followed by a gap of 8 words:
    skin | shape_weights | indices | list_count | out_positions | out_normals | out_tangents (M rows each) | x, a spare
    area that holds any one of them.  All zeros is a valid call: the list names skeleton 0 and its length is 0."""

    def __init__(self, B, V, P, n, M):
        self.B, self.V, self.P, self.n, self.M = B, V, P, n, M
        self.at, o = {}, 0
        for name, words in (("skin", n * B * 12), ("cw", n * P), ("ind", M), ("cnt", 1), ("p", M * V * 3), ("q", M * V * 3), ("t", M * V * 4),
                            ("x", max(n * B * 12, M * V * 4))):
            self.at[name] = o
            o += words + 8
        self.words = o


def call_refusals(lay, run):
    """Every refusal of mbik_skin_vertices_call's list (include/mbik.h) that needs a mesh.  run(mesh, **fields) -> (rc, text)
    makes the call on the mesh kind 'plain' (no normals), 'normals', 'tan' or 'shaped_tan' with the fields skin, cw, ind,
    cnt, p, q, t as word offsets into the layout's buffer (None: a null pointer), count, max_list, flags and struct_size
    (None: the right one).  -> [(what, rc, text)] for the caller to compare with the other entry's; asserts each here."""
    a, n, M, V = lay.at, lay.n, lay.M, lay.V
    ok = dict(skin=a["skin"], cw=None, ind=None, cnt=None, p=a["p"], q=a["q"], t=a["t"], count=n, max_list=0, flags=0, struct_size=None)
    listed = dict(ok, ind=a["ind"], cnt=a["cnt"], max_list=M, flags=1)
    nt = n * V * 4
    cases = [
        ("struct_size", "tan", dict(ok, struct_size=8), "mbik_skin_call.struct_size is too small"),
        ("out_tangents without mesh tangents", "normals", ok, "out_tangents given for a mesh without tangents"),
        ("out_tangents without out_normals", "tan", dict(ok, q=None), "out_tangents given without out_normals"),
        ("indices alone", "tan", dict(ok, ind=a["ind"]), "indices and list_count must be given together"),
        ("list_count alone", "tan", dict(ok, cnt=a["cnt"]), "indices and list_count must be given together"),
        # out_tangents ends one word inside, or begins one word before the end of, another argument
        ("overlaps skin", "tan", dict(ok, t=a["skin"] + n * lay.B * 12 - 1, p=a["q"], q=a["t"]), "out_tangents overlaps skin"),
        ("overlaps shape_weights", "shaped_tan", dict(ok, cw=a["cw"], t=a["cw"] - nt + 1, skin=a["x"]),
         "out_tangents overlaps shape_weights"),
        ("overlaps indices", "tan", dict(listed, t=a["ind"] + M - 1, flags=0, p=a["p"], q=a["q"]), "out_tangents overlaps indices"),
        ("overlaps list_count", "tan", dict(listed, t=a["cnt"], flags=0), "out_tangents overlaps list_count"),
        ("overlaps out_positions", "tan", dict(ok, t=a["p"] + n * V * 3 - 1, q=a["t"]), "out_tangents overlaps out_positions"),
        ("overlaps out_normals", "tan", dict(ok, t=a["q"] - nt + 1, p=a["x"]), "out_tangents overlaps out_normals"),
        # (compact: M rows, so the normals reach past their first n rows)
        ("rows follow the flag", "tan", dict(listed, t=a["q"] + n * V * 3), "out_tangents overlaps out_normals"),
        # what the matching existing entry refuses, with its text
        ("negative count", "tan", dict(ok, count=-1), "negative count"),
        ("null skin", "tan", dict(ok, skin=None), "null skin"),
        ("null out_positions", "tan", dict(ok, p=None), "null out_positions"),
        ("out_normals without mesh normals", "plain", dict(ok, t=None), "out_normals given for a mesh without normals"),
        ("outputs overlap", "tan", dict(ok, q=a["p"] + 1), "out_normals overlaps out_positions"),
        ("shape_weights without shapes", "tan", dict(ok, cw=a["cw"]), "the mesh has no shapes (mbik_mesh_create_shaped)"),
        ("listed: shape_weights without shapes", "tan", dict(listed, cw=a["cw"]), "shape_weights given for a mesh without shapes"),
        ("listed: flags", "tan", dict(listed, flags=2), "unknown flag bits"),
        ("listed: max_list", "tan", dict(listed, max_list=-1), "negative max_list"),
        ("listed: out_positions overlaps indices", "tan", dict(listed, p=a["ind"] - M * V * 3 + 1, skin=a["x"]), "out_positions overlaps indices"),
    ]
    seen = []
    for what, mesh, fields, text in cases:
        rc, got = run(mesh, **fields)
        assert rc == _lib.MBIK_EINVAL and got == text, (what, rc, got)
        seen.append((what, rc, got))
    # the overlap tests are tight: one word further the same calls pass
    for what, mesh, fields in (("next to out_normals", "tan", dict(ok, t=a["q"] - nt, p=a["x"])),
                               ("in place behind n rows of normals", "tan", dict(listed, t=a["q"] + n * V * 3, flags=0)),
                               ("next to list_count", "tan", dict(listed, t=a["cnt"] + 1, flags=0, p=a["x"]))):
        rc, got = run(mesh, **fields)
        assert rc == _lib.MBIK_OK, (what, rc, got)
    return seen


def desc_refusals(case, run):
    """The descriptor's refusals: run(desc or None) -> (rc, text) through an entry that takes one.  `case` is shaped."""
    L = _lib
    good, keep = case.desc()
    sh, _ = case.shapes()

    def variant(**kw):
        d, _k = case.desc()
        for k, v in kw.items():
            setattr(d, k, v)
        return d

    cases = [
        ("null desc", None, "null desc"),
        ("struct_size", variant(struct_size=16), "mbik_mesh_desc.struct_size is too small"),
        ("tangents without normals", variant(normals=None, shapes=None, shape_tangents=None), "tangents given for a mesh without normals"),
        ("shape_tangents missing", variant(shape_tangents=None), "shape_tangents must be given exactly when the mesh has both shapes and tangents"),
        ("shape_tangents without shapes", variant(shapes=None), "shape_tangents must be given exactly when the mesh has both shapes and tangents"),
        ("shape_tangents without tangents", variant(tangents=None), "shape_tangents must be given exactly when the mesh has both shapes and tangents"),
        ("influences", variant(influences=5), "influences must be 4 or 8"),
    ]
    seen = []
    for what, d, text in cases:
        rc, got = run(d)
        assert rc == L.MBIK_EINVAL and got == text, (what, rc, got)
        seen.append((what, rc, got))
    return seen
