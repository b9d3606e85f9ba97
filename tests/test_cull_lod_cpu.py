"""mbik_cull_lod_cpu (include/mbik.h) against tests/lod_recipe.py, bitwise: state, level,
every list, every count and the untouched tails, over seeded crowds, four-frame sequences with the
state carried along, the branch census of those inputs, the single unlimited range against
mbik_cull_boxes_cpu, the exclusive lists, the state of culled skeletons, and every refusal through
both entries (the device entry refuses before it needs a mesh, so no GPU is involved)."""
import ctypes as C
import functools
import itertools

import numpy as np
import pytest

from many_bone_ik_amd import _lib
from many_bone_ik_amd.skinning import LOD_RANGE_DTYPE, cull_boxes_cpu, cull_lod_cpu, lod_ranges

from . import lod_recipe as LR

F = np.float32
INT_SENTINEL = -777
BYTE_SENTINEL = 0xAB
N = max(LR.COUNTS)
CASES = list(itertools.product((1, 3, 8), (False, True), (0.0, 0.4)))
FRAMES = 4


def ptr(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def run_cpu(boxes, planes, camera, ranges, state, sg=None, margin=0.0, flags=0):
    """The C entry on sentinel-filled outputs -> (state, level, indices [R][count], counts [R])."""
    L = _lib.load()
    count = boxes.shape[0]
    rg, cam = lod_ranges(ranges), np.asarray(camera, F)
    st = np.array(state, np.uint8)
    level = np.full(count, BYTE_SENTINEL, np.uint8)
    indices = np.full((rg.shape[0], count), INT_SENTINEL, np.int32)
    counts = np.full(rg.shape[0], 123456789, np.int32)       # garbage: the call must not rely on cleared counts
    pl = np.ascontiguousarray(planes, F).reshape(-1, 4)
    rc = L.mbik_cull_lod_cpu(count, ptr(boxes), ptr(sg), margin, pl.shape[0], ptr(pl) if pl.shape[0] else None, ptr(cam), rg.shape[0],
                             ptr(rg), flags, ptr(st), ptr(level), ptr(indices), ptr(counts))
    assert rc == _lib.MBIK_OK, _lib.last_error()
    return st, level, indices, counts


def check_against(res, got, range_count, flags, count):
    """got (run_cpu's tuple, or the device's) against the first `count` skeletons of the recipe's result."""
    st, level, indices, counts = got
    assert np.array_equal(st, res["state"][:count]) and np.array_equal(level, res["level"][:count])
    for r, ref in enumerate(LR.lists(res, range_count, flags, count)):
        assert counts[r] == len(ref), (r, counts[r], len(ref))
        assert np.array_equal(indices[r, :len(ref)], ref)
        assert (indices[r, len(ref):] == INT_SENTINEL).all()          # the tail is not touched


def case_inputs(range_count, with_global, margin):
    seed = 1000 + range_count * 10 + with_global * 2 + (margin != 0)
    return dict(boxes=LR.crowd(seed, N, nan_every=167), planes=LR.planes(seed + 1), camera=LR.CAMERA, ranges=LR.RANGES[range_count],
                state=LR.states(seed + 2, N), sg=LR.globals_(seed + 3, N) if with_global else None, margin=margin)


@functools.lru_cache(maxsize=None)
def case_recipe(range_count, with_global, margin):
    c = case_inputs(range_count, with_global, margin)
    return LR.select(c["boxes"], c["planes"], c["camera"], c["ranges"], c["state"], c["sg"], c["margin"])


def sequence_inputs(range_count):
    """A crowd, and a camera that walks through it in FRAMES steps; the state starts strict (zeros)."""
    n = 300
    cams = [(-12.0 + 7.0 * f, 0.5 * f, 3.0 - 2.0 * f) for f in range(FRAMES)]
    return LR.crowd(2000 + range_count, n, nan_every=100), LR.planes(2100 + range_count), cams, LR.RANGES[range_count]


@functools.lru_cache(maxsize=None)
def sequence_recipe(range_count):
    boxes, planes, cams, ranges = sequence_inputs(range_count)
    state, out = np.zeros(boxes.shape[0], np.uint8), []
    for cam in cams:
        out.append(LR.select(boxes, planes, cam, ranges, state, None, 0.25))
        state = out[-1]["state"]
    return out


@pytest.mark.parametrize("range_count,with_global,margin", CASES)
def test_cpu_entry_matches_recipe(mbik, range_count, with_global, margin):
    c, res = case_inputs(range_count, with_global, margin), case_recipe(range_count, with_global, margin)
    assert 0 < res["vis"].sum() < N
    for count in LR.COUNTS:
        for flags in (0, _lib.LOD_EXCLUSIVE):
            got = run_cpu(c["boxes"][:count], c["planes"], c["camera"], c["ranges"], c["state"][:count],
                          None if c["sg"] is None else c["sg"][:count], margin, flags)
            check_against(res, got, range_count, flags, count)


@pytest.mark.parametrize("range_count", [1, 3, 8])
def test_four_frames_carry_the_state(mbik, range_count):
    boxes, planes, cams, ranges = sequence_inputs(range_count)
    refs = sequence_recipe(range_count)
    state = np.zeros(boxes.shape[0], np.uint8)
    for f, cam in enumerate(cams):
        got = run_cpu(boxes, planes, cam, ranges, state, None, 0.25, 0)
        check_against(refs[f], got, range_count, 0, boxes.shape[0])
        state = got[0]
    # the carried state matters: frame 1 from a blank state is another frame
    blank = run_cpu(boxes, planes, cams[1], ranges, np.zeros(boxes.shape[0], np.uint8), None, 0.25, 0)
    assert not np.array_equal(blank[0], refs[1]["state"])


def test_seeded_inputs_take_every_branch(mbik):
    total = dict.fromkeys(LR.BRANCHES, 0)
    for case in CASES:
        for k, v in case_recipe(*case)["stats"].items():
            total[k] += v
    for rc in (1, 3, 8):
        for res in sequence_recipe(rc):
            for k, v in res["stats"].items():
                total[k] += v
    print(total)
    assert all(total[k] >= 20 for k in LR.BRANCHES), total


@pytest.mark.parametrize("with_global,margin", [(False, 0.0), (True, 0.4)])
def test_single_unlimited_range_is_cull_boxes(mbik, with_global, margin):
    c = case_inputs(1, with_global, margin)
    vis, ind = cull_boxes_cpu(c["boxes"], c["planes"], skeleton_global=c["sg"], margin=margin)
    for state in (c["state"], np.zeros(N, np.uint8), np.full(N, 0xFF, np.uint8)):
        st, level, indices, counts = run_cpu(c["boxes"], c["planes"], c["camera"], np.zeros((1, 4), F), state, c["sg"], margin, 0)
        assert counts[0] == len(ind) and np.array_equal(indices[0, :len(ind)], ind) and (indices[0, len(ind):] == INT_SENTINEL).all()
        assert (st == 1).all() and np.array_equal(level == 0, vis == 1) and ((level == 0) | (level == _lib.LOD_NONE)).all()


@pytest.mark.parametrize("range_count", [3, 8])
def test_exclusive_lists_are_the_levels(mbik, range_count):
    c = case_inputs(range_count, False, 0.0)
    st, level, indices, counts = run_cpu(c["boxes"], c["planes"], c["camera"], c["ranges"], c["state"], None, 0.0, _lib.LOD_EXCLUSIVE)
    seen = np.zeros(N, np.int32)
    for r in range(range_count):
        assert np.array_equal(indices[r, :counts[r]], np.flatnonzero(level == r))
        seen[indices[r, :counts[r]]] += 1
    assert seen.max() == 1 and np.array_equal(seen == 0, level == _lib.LOD_NONE)
    plain = run_cpu(c["boxes"], c["planes"], c["camera"], c["ranges"], c["state"], None, 0.0, 0)
    assert plain[3].sum() > counts.sum()                              # (the overlaps: the plain lists name some twice)
    assert np.array_equal(plain[0], st) and np.array_equal(plain[1], level)
    # the Python wrapper returns the same lists
    st2, level2, lists = cull_lod_cpu(c["boxes"], c["planes"], c["camera"], c["ranges"].view(LOD_RANGE_DTYPE).reshape(-1), c["state"],
                                      flags=_lib.LOD_EXCLUSIVE)
    assert np.array_equal(st2, st) and np.array_equal(level2, level)
    assert all(np.array_equal(lists[r], indices[r, :counts[r]]) for r in range(range_count))


def test_state_advances_for_culled_skeletons(mbik):
    boxes, ranges = LR.crowd(31, 400), LR.RANGES[3]
    none_seen = np.array([[1, 0, 0, -100]], F)
    zeros = np.zeros(400, np.uint8)
    ref = LR.select(boxes, none_seen, LR.CAMERA, ranges, zeros)
    st, level, indices, counts = run_cpu(boxes, none_seen, LR.CAMERA, ranges, zeros)
    assert not ref["vis"].any() and (level == _lib.LOD_NONE).all() and not counts.any() and (indices == INT_SENTINEL).all()
    assert np.array_equal(st, ref["state"]) and np.count_nonzero(st) > 200
    # and the advanced state is what the next frame's hysteresis sees
    nxt = run_cpu(boxes, LR.planes(32), (2.5, -0.75, 2.25), ranges, st)
    assert not np.array_equal(nxt[0], run_cpu(boxes, LR.planes(32), (2.5, -0.75, 2.25), ranges, zeros)[0])
    check_against(LR.select(boxes, LR.planes(32), (2.5, -0.75, 2.25), ranges, st), nxt, 3, 0, 400)


# ---------------- refusals ----------------
def einval_cases():
    """(name, changes to a valid call's arguments).  Pointers are taken from buffers sized for count = 8, three ranges."""
    n, R = 8, 3
    buf = dict(b=np.zeros((n, 6), F), g=np.zeros((n, 12), F), pl=np.array([[1, 0, 0, 5.0], [0, 1, 0, 5.0]], F), cam=np.zeros(3, F),
               rg=LR.RANGES[3].copy(), state=np.zeros(n, np.uint8), level=np.zeros(n, np.uint8), ind=np.zeros((R, n), np.int32),
               cnt=np.zeros(R, np.int32))
    addr = {k: v.ctypes.data for k, v in buf.items()}
    base = dict(count=n, pc=2, rc=R, flags=0, **addr)
    cases = [("negative count", dict(count=-1)), ("plane_count 17", dict(pc=17)), ("plane_count -1", dict(pc=-1)),
             ("null planes", dict(pl=0)), ("null boxes", dict(b=0)), ("range_count 0", dict(rc=0)), ("range_count 9", dict(rc=9)),
             ("range_count -1", dict(rc=-1)), ("null ranges", dict(rg=0)), ("null camera", dict(cam=0)), ("unknown flags", dict(flags=2)),
             ("unknown high flag", dict(flags=0x80000001)), ("null state", dict(state=0)), ("null indices", dict(ind=0)),
             ("null list_counts", dict(cnt=0))]
    for i, bad in enumerate((np.nan, np.inf, -np.inf)):
        cam = np.zeros(3, F)
        cam[i] = bad
        buf[f"cam{i}"] = cam
        cases.append((f"camera {bad}", dict(cam=cam.ctypes.data)))
    for field, bad in itertools.product(range(4), (np.nan, np.inf, -1.0)):
        rg = LR.RANGES[3].copy()
        rg[field % 3, field] = bad
        buf[f"rg{field}{bad}"] = rg
        cases.append((f"range field {field} = {bad}", dict(rg=rg.ctypes.data)))
    rg = LR.RANGES[3].copy()
    rg[1, 0], rg[1, 1] = 9.0, 8.0
    buf["rg_order"] = rg
    cases.append(("begin behind end", dict(rg=rg.ctypes.data)))
    outs, ins = ("state", "level", "ind", "cnt"), ("b", "g", "pl", "cam", "rg")
    for o in outs:
        for i in ins:
            cases.append((f"{o} overlaps {i}", {o: addr[i]}))
    for o, q in itertools.combinations(outs, 2):
        cases.append((f"{q} overlaps {o}", {q: addr[o]}))
    cases.append(("state overlaps the last byte of boxes", dict(state=addr["b"] + n * 24 - 1)))
    cases.append(("list_counts overlaps the last entry of indices", dict(cnt=addr["ind"] + 4 * (R * n - 1))))
    return base, cases, buf


def call_both(a):
    """-> ((rc, text) of mbik_cull_lod_cpu, (rc, text) of mbik_cull_lod with a null mesh)"""
    L = _lib.load()
    vp = lambda x: C.c_void_p(x or None)
    shared = (a["count"], vp(a["b"]), vp(a["g"]), 0.0, a["pc"], vp(a["pl"]), vp(a["cam"]), a["rc"], vp(a["rg"]), a["flags"],
              vp(a["state"]), vp(a["level"]), vp(a["ind"]), vp(a["cnt"]))
    r1 = L.mbik_cull_lod_cpu(*shared)
    t1 = _lib.last_error()
    r2 = L.mbik_cull_lod(None, *shared, None)
    return (r1, t1), (r2, _lib.last_error())


def test_every_refusal_through_both_entries(mbik):
    base, cases, keep = einval_cases()
    texts = set()
    for name, change in cases:
        (r1, t1), (r2, t2) = call_both({**base, **change})
        assert r1 == _lib.MBIK_EINVAL and r2 == _lib.MBIK_EINVAL, name
        assert t1 == t2 and t1, (name, t1, t2)
        texts.add(t1)
    assert len(texts) >= 30                                            # the texts tell the cases apart
    assert not keep["state"].any() and not keep["ind"].any() and not keep["cnt"].any()      # nothing was written
    # a valid call: the host entry runs, the device entry has only the missing mesh to refuse
    (r1, _), (r2, t2) = call_both(base)
    assert r1 == _lib.MBIK_OK and r2 == _lib.MBIK_EINVAL and t2 == "null mesh"
    # the limits themselves are accepted: 16 planes, 8 ranges, begin == end, level NULL, skeleton_global NULL
    pl16 = np.tile(keep["pl"][:1], (16, 1))
    rg8 = LR.RANGES[8].copy()
    rg8[2, 0] = rg8[2, 1]
    ind8 = np.zeros((8, 8), np.int32)
    cnt8 = np.zeros(8, np.int32)
    ok = {**base, "pc": 16, "pl": pl16.ctypes.data, "rc": 8, "rg": rg8.ctypes.data, "ind": ind8.ctypes.data, "cnt": cnt8.ctypes.data,
          "level": 0, "g": 0, "flags": 1}
    assert call_both(ok)[0][0] == _lib.MBIK_OK
    # adjacent outputs do not overlap
    pool = np.zeros(8 + 8 + 3 * 8 * 4 + 3 * 4, np.uint8)
    p = pool.ctypes.data
    assert call_both({**base, "state": p, "level": p + 8, "ind": p + 16, "cnt": p + 16 + 96})[0][0] == _lib.MBIK_OK


def test_count_zero_writes_the_counts_only(mbik):
    base, _, keep = einval_cases()
    keep["cnt"][:] = 55
    (r1, _), (r2, t2) = call_both({**base, "count": 0, "b": 0, "state": 0, "ind": 0, "level": 0, "g": 0})
    assert r1 == _lib.MBIK_OK and not keep["cnt"].any()
    assert r2 == _lib.MBIK_EINVAL and t2 == "null mesh"
    assert call_both({**base, "count": 0, "cnt": 0})[0][0] == _lib.MBIK_OK      # and list_counts may be absent then
