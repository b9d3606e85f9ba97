"""mbik_skin_vertices_listed_cpu (include/mbik.h, ABI 15) without a GPU: the listed rows
carry the bits of mbik_skin_vertices_cpu / mbik_skin_vertices_shaped_cpu and every other row, and the
guard floats around every output, keep their sentinel (tests/skin_list_cases.py); list counts and
contents; the cull chain on the host; every error code."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from many_bone_ik_amd import _lib
from many_bone_ik_amd.skinning import skin_vertices_cpu, skin_vertices_listed_cpu

from . import skin_cases as S
from . import skin_list_cases as LC

F = np.float32


def run_listed(case, indices, list_count, max_list, compact, shaped):
    """The listed host call into guarded sentinel buffers -> (positions, normals), the whole outputs."""
    rows = max_list if compact else case.count
    flat_p, out_p = LC.guarded(rows, case.V)
    flat_n, out_n = LC.guarded(rows, case.V) if case.nrm is not None else (None, None)
    kw = case.mesh_kw()
    if shaped:
        kw["shape_weights"] = case.cw
    skin_vertices_listed_cpu(case.B, case.pos, case.idx, case.w, case.skin, indices, list_count, max_list=max_list, compact=compact,
                             out_positions=out_p, out_normals=out_n, **kw)
    assert LC.guards_intact(flat_p) and (flat_n is None or LC.guards_intact(flat_n))
    return out_p, out_n


def check_listed(case, indices, list_count, max_list, compact, shaped):
    got_p, got_n = run_listed(case, indices, list_count, max_list, compact, shaped)
    full_p, full_n = case.full(shaped)
    assert S.same_bits(got_p, LC.expected(full_p, indices, list_count, max_list, compact))
    if case.nrm is not None:
        assert S.same_bits(got_n, LC.expected(full_n, indices, list_count, max_list, compact))
    return got_p, got_n


@pytest.fixture(scope="module")
def cases(mbik):
    return {"plain": LC.Case(300, 7, 50, 4, 9), "plain8": LC.Case(310, 7, 33, 8, 9, normals=False),
            "relative": LC.Case(320, 7, 50, 4, 9, P=3, mode="relative", special_weights=True),
            "normalized": LC.Case(330, 7, 50, 8, 9, P=5, mode="normalized", special_weights=True)}


@pytest.mark.parametrize("compact", [False, True], ids=["in_place", "compact"])
@pytest.mark.parametrize("name,shaped", [("plain", False), ("plain8", False), ("relative", True), ("normalized", True), ("relative", False)],
                         ids=["plain", "plain8_positions", "relative", "normalized", "shaped_mesh_base_arrays"])
def test_same_bits_as_the_existing_calls(cases, name, shaped, compact):
    """A list of 4 in a buffer of 6: the stale tail (valid skeleton numbers) is not consumed."""
    case = cases[name]
    indices = np.array([3, 0, 7, 5, 8, 1], np.int32)
    got_p, _ = check_listed(case, indices, 4, 6, compact, shaped)
    assert np.isfinite(got_p[0 if compact else 3]).all()
    untouched = got_p[4:] if compact else got_p[[1, 2, 4, 6, 8]]
    assert (untouched == F(LC.SENTINEL)).all()
    if shaped:   # the shapes moved something: the shaped rows differ from the plain call's
        assert not S.same_bits(case.shaped_p[[3, 0, 7, 5]], case.plain_p[[3, 0, 7, 5]])


def test_compact_rows_are_the_in_place_rows(cases):
    case = cases["relative"]
    indices = np.array([8, 2, 2, 6, 0], np.int32)
    for shaped in (False, True):
        in_place, _ = run_listed(case, indices, 5, 5, False, shaped)
        compact, _ = run_listed(case, indices, 5, 5, True, shaped)
        for r, s in enumerate(indices):
            assert S.same_bits(compact[r], in_place[s])


@pytest.mark.parametrize("compact", [False, True], ids=["in_place", "compact"])
@pytest.mark.parametrize("list_count,n", [(0, 0), (-3, 0), (-2 ** 31, 0), (5, 5), (6, 5), (2 ** 31 - 1, 5)])
def test_list_counts(cases, list_count, n, compact):
    """0, negative, equal to max_list, above it (clamped)."""
    case = cases["plain"]
    indices = np.array([4, 1, 8, 0, 6], np.int32)
    assert LC.list_length(list_count, 5) == n
    got_p, _ = check_listed(case, indices, list_count, 5, compact, False)
    assert int((got_p[:, 0, 0] != F(LC.SENTINEL)).sum()) == n
    # max_list above count, the list shorter than the buffer
    long_list = np.array([8, 7, 6, 5, 4, 3, 2, 1, 0, 4, 4, 0], np.int32)
    check_listed(case, long_list, 11, 12, compact, False)


@pytest.mark.parametrize("shaped", [False, True], ids=["plain", "shaped"])
@pytest.mark.parametrize("compact", [False, True], ids=["in_place", "compact"])
def test_list_contents(cases, compact, shaped):
    """-1 and count are skipped (their compact rows stay untouched); duplicates and descending order are accepted."""
    case = cases["normalized"]
    count = case.count
    skipped = np.array([2, -1, 5, count, 0], np.int32)
    got_p, _ = check_listed(case, skipped, 5, 5, compact, shaped)
    if compact:
        assert (got_p[[1, 3]] == F(LC.SENTINEL)).all() and not (got_p[[0, 2, 4]] == F(LC.SENTINEL)).any()
    else:
        assert int((got_p[:, 0, 0] != F(LC.SENTINEL)).sum()) == 3
    check_listed(case, np.array([-1, count, -1], np.int32), 3, 3, compact, shaped)          # nothing but skipped entries
    check_listed(case, np.array([4, 4, 1, 4, 1], np.int32), 5, 5, compact, shaped)           # duplicates
    check_listed(case, np.arange(count - 1, -1, -1).astype(np.int32), count, count, compact, shaped)   # descending, everything


@pytest.mark.parametrize("compact", [False, True], ids=["in_place", "compact"])
def test_cull_chain_on_the_host(mbik, compact):
    """pose_globals_cpu -> skin_bounds_cpu -> cull_boxes_cpu -> listed skin, fed as mbik_cull_boxes leaves its outputs:
    the list in a buffer of `count` entries whose tail is stale, and the count beside it."""
    c = LC.cull_chain(n=24, V=120)
    skin, planes1, planes2, l1, l2 = LC.chain_reference(c, c["wl"].pose)
    count = skin.shape[0]
    assert 0 < len(l1) < count
    full_p, full_n = skin_vertices_cpu(c["B"], c["pos"], c["idx"], c["w"], skin, normals=c["nrm"])
    stale = np.full(count, 0, np.int32)           # (a stale tail of valid numbers: consuming it would show)
    for lst in (l1, l2):
        indices = stale.copy()
        indices[:len(lst)] = lst
        flat_p, out_p = LC.guarded(count, 120)
        flat_n, out_n = LC.guarded(count, 120)
        skin_vertices_listed_cpu(c["B"], c["pos"], c["idx"], c["w"], skin, indices, len(lst), compact=compact, normals=c["nrm"],
                                 out_positions=out_p, out_normals=out_n)
        assert LC.guards_intact(flat_p) and LC.guards_intact(flat_n)
        assert S.same_bits(out_p, LC.expected(full_p, indices, len(lst), count, compact))
        assert S.same_bits(out_n, LC.expected(full_n, indices, len(lst), count, compact))


def test_error_codes(mbik):
    L = _lib.load()
    B, V, K, n, P, M = 5, 9, 4, 3, 2, 4
    pos, nrm, idx, w = S.random_mesh(1, B, V, K)
    sp = np.zeros((P, V, 3), F)
    shapes = _lib.MbikMeshShapes(C.sizeof(_lib.MbikMeshShapes), P, 0, S.ptr(sp), S.ptr(sp))
    nskin, nout, ncw = n * B * 12, M * V * 3, n * P
    buf = np.zeros(nskin + ncw + 2 * nout + 8, F)
    skin, cw = buf[:nskin], buf[nskin:nskin + ncw]
    a, b = nskin + ncw, nskin + ncw + nout
    out_p, out_n = buf[a:b], buf[b:b + nout]
    ibuf = np.zeros(M + 1, np.int32)
    ind, cnt = ibuf[:M], ibuf[M:]
    ind[:], cnt[0] = [0, 2, 1, 0], 3

    def call(count=n, i=ind, c=cnt, max_list=M, s=skin, sw=None, flags=1, p=out_p, q=out_n, normals=nrm, sh=None, B=B, K=K):
        return L.mbik_skin_vertices_listed_cpu(B, V, K, S.ptr(pos), S.ptr(normals), S.ptr(idx), S.ptr(w), None if sh is None else C.byref(sh),
                                               count, S.ptr(i), S.ptr(c), max_list, S.ptr(s), S.ptr(sw), flags, S.ptr(p), S.ptr(q))

    E, OK = _lib.MBIK_EINVAL, _lib.MBIK_OK
    assert call() == OK and call(flags=0, p=out_p[:n * V * 3], q=out_n[:n * V * 3]) == OK        # adjacent buffers, both modes
    assert call(sw=cw, sh=shapes) == OK
    # what the plain and the shaped call refuse
    assert call(count=-1) == E and call(s=None) == E and call(p=None) == E
    assert call(normals=None) == E                                      # out_normals for a mesh without normals
    assert call(K=3) == E and call(B=1) == E                            # the mesh's own checks
    assert call(p=buf[nskin - 1:nskin - 1 + nout], q=None) == E         # out_positions overlaps skin
    assert call(q=buf[nskin - 1:nskin - 1 + nout]) == E                 # out_normals overlaps skin
    assert call(q=buf[b - 1:b - 1 + nout]) == E                         # outputs overlap
    assert call(sw=cw, sh=shapes, p=buf[a - 1:a - 1 + nout]) == E       # out_positions overlaps shape_weights
    assert call(sw=cw, sh=shapes, q=buf[a - 1:a - 1 + nout], p=buf[b:b + nout]) == E   # out_normals overlaps shape_weights
    # the list's own
    assert call(i=None) == E and call(c=None) == E                      # null indices / list_count with work to do
    assert call(max_list=-1) == E
    assert call(flags=2) == E and call(flags=3) == E and call(flags=0x80000000) == E
    assert call(sw=cw) == E                                             # shape_weights on a mesh without shapes
    iout = ibuf.view(F)
    assert call(p=iout[M - 1:], q=None, max_list=M, flags=0, count=0) == OK      # (nothing to do comes first)
    big = np.zeros(nout + M + 1, F)
    bi = big[nout:].view(np.int32)
    bi[:M], bi[M] = ind, 3
    assert call(i=bi[:M], c=bi[M:], p=big[:nout], q=None) == OK         # adjacent to indices
    assert call(i=bi[:M], c=bi[M:], p=big[1:nout + 1], q=None) == E     # out_positions overlaps indices
    assert call(i=ind, c=bi[M:], p=big[M + 1:nout + M + 1], q=None) == E        # out_positions overlaps list_count
    assert call(i=bi[:M], c=cnt, q=big[1:nout + 1]) == E                # out_normals overlaps indices
    # output sizes follow the flag: in place [count] rows, compact [max_list] rows
    assert call(flags=0, p=big[:n * V * 3], q=None, i=big[n * V * 3:].view(np.int32)[:M]) == OK
    assert call(flags=1, p=big[:n * V * 3], q=None, i=big[n * V * 3:].view(np.int32)[:M]) == E
    # nothing to do: OK whatever else is null
    assert call(count=0, i=None, c=None, s=None, p=None, q=None) == OK
    assert call(max_list=0, i=None, c=None, s=None, p=None, q=None) == OK
    assert L.mbik_skin_vertices_listed_cpu(B, 0, K, None, None, None, None, None, n, None, None, M, None, None, 0, None, None) == OK
    assert call(count=0, flags=2) == E and call(max_list=0, sw=cw) == E          # but not a bad flag or stray weights


def test_abi_version_in_the_header(mbik):
    """(mbik_plan_get_info needs a device: tests/test_gpu_skin_list.py checks the library's own number.)"""
    header = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "mbik.h")
    src = open(header).read()
    assert re.search(r"^#define MBIK_ABI_VERSION (\d+)$", src, re.M).group(1) == "15"
    assert re.search(r"^#define MBIK_SKIN_LIST_COMPACT (\w+)$", src, re.M).group(1) == "1u" and _lib.SKIN_LIST_COMPACT == 1
