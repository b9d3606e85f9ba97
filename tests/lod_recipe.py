"""Distance LOD lists (include/mbik.h, mbik_cull_lod) written once more without the code
under test, for tests/test_cull_lod_cpu.py and tests/test_gpu_cull_lod.py.

Everything follows the header's steps literally in numpy float32 scalars: one rounding per operation,
the compares as written (so NaN goes where they send it), the ranges in ascending order.  `select`
gives the per-skeleton results and counts which branches the inputs took; `lists` is the header's list
rule.  The seeded crowds, ranges and cameras the two test files share are here too.
"""
import numpy as np

from . import bounds_recipe as R

F = np.float32
NONE = 255
EXCLUSIVE = 1
BRANCHES = ("beyond_end", "before_begin", "inside", "margin_decides", "unlimited_side", "nan_distance", "culled_in_range",
            "in_two_ranges", "in_none_from_zero_state")


def in_range(dist, rng, prev):
    """_visibility_range_check's two compares for one range (begin, end, begin_margin, end_margin) -> (inside, which)"""
    begin, end, bm, em = (F(x) for x in rng)
    bo, eo = -bm, em
    if not prev:
        bo, eo = -bo, -eo
    if end > 0 and dist > end + eo:
        return False, "beyond_end"
    if begin > 0 and dist < begin + bo:
        return False, "before_begin"
    return True, "inside"


def select(boxes, planes, camera, ranges, state, skeleton_global=None, margin=0.0):
    """-> dict: state, level [count] uint8, vis [count] uint8, bits [count] uint8 (bit r: in range r), stats."""
    planes = np.asarray(planes, F).reshape(-1, 4)
    ranges = np.asarray(ranges, F).reshape(-1, 4)
    cam = [F(x) for x in camera]
    margin = F(margin)
    n = boxes.shape[0]
    out_state, level, vis_out = np.zeros(n, np.uint8), np.full(n, NONE, np.uint8), np.zeros(n, np.uint8)
    stats = dict.fromkeys(BRANCHES, 0)
    with np.errstate(all="ignore"):
        for s in range(n):
            b = np.array(boxes[s], F)
            if skeleton_global is not None:
                b = R.xform_aabb(skeleton_global[s], b)
            p, z = [F(b[a]) for a in range(3)], [F(b[3 + a]) for a in range(3)]
            if margin != 0:
                p = [x - margin for x in p]
                z = [x + margin * F(2.0) for x in z]
            e = [p[a] + z[a] for a in range(3)]
            vis = 1
            for pl in planes:
                c = [p[a] if pl[a] > 0 else e[a] for a in range(3)]
                if ((pl[0] * c[0] + pl[1] * c[1]) + pl[2] * c[2]) > pl[3]:
                    vis = 0
                    break
            ctr = [p[a] + z[a] * F(0.5) for a in range(3)]
            v = [ctr[a] - cam[a] for a in range(3)]
            dist = np.sqrt((v[0] * v[0] + v[1] * v[1]) + v[2] * v[2])
            assert dist.dtype == F
            if np.isnan(dist):
                stats["nan_distance"] += 1
            bits = 0
            for r, rng in enumerate(ranges):
                prev = (int(state[s]) >> r) & 1
                inside, which = in_range(dist, rng, prev)
                stats[which] += 1
                if inside != in_range(dist, rng, 1 - prev)[0]:
                    stats["margin_decides"] += 1
                if (rng[0] == 0 or rng[1] == 0) and inside:
                    stats["unlimited_side"] += 1
                if inside:
                    bits |= 1 << r
                    if vis and level[s] == NONE:
                        level[s] = r
                    if not vis:
                        stats["culled_in_range"] += 1
            if bin(bits).count("1") >= 2:
                stats["in_two_ranges"] += 1
            if bits == 0 and state[s] == 0:
                stats["in_none_from_zero_state"] += 1
            out_state[s], vis_out[s] = bits, vis
    return dict(state=out_state, level=level, vis=vis_out, bits=out_state.copy(), stats=stats)


def lists(res, range_count, flags, count=None):
    """The header's list rule for the first `count` skeletons of select()'s result: one ascending array per range."""
    count = len(res["vis"]) if count is None else count
    vis, bits, level = res["vis"][:count], res["bits"][:count], res["level"][:count]
    if flags & EXCLUSIVE:
        return [np.flatnonzero(level == r).astype(np.int32) for r in range(range_count)]
    return [np.flatnonzero((vis == 1) & (((bits >> r) & 1) == 1)).astype(np.int32) for r in range(range_count)]


# ---------------- the seeded inputs ----------------
COUNTS = (0, 1, 63, 64, 65, 255, 256, 257, 1000)
CAMERA = (1.5, -0.75, 2.25)
# (begin, end, begin_margin, end_margin).  Three ranges: 0 and 1 overlap between 6 and 8, nothing covers 16 to 18, the
# last has no far limit.  Eight: bands of 4 that overlap by 1, the first without a near limit and the last without a far one.
RANGES = {
    1: np.array([[0, 12, 0, 1.5]], F),
    3: np.array([[0, 8, 0, 1], [6, 16, 1, 1], [18, 0, 1.5, 0]], F),
    8: np.array([[4 * r, 0 if r == 7 else 4 * r + 5, 0.5, 0.5] for r in range(8)], F),
}


def crowd(seed, n, nan_every=0):
    """Boxes [n][6] scattered 20 units around the origin; every nan_every-th has a NaN coordinate."""
    rng = np.random.default_rng(seed)
    boxes = np.concatenate([rng.uniform(-20.0, 20.0, (n, 3)), rng.uniform(0.0, 1.5, (n, 3))], axis=1).astype(F)
    if nan_every:
        boxes[nan_every - 1::nan_every, rng.integers(0, 6)] = np.nan
    return boxes


def planes(seed):
    """bounds_recipe's frustum, six times as wide: about half of crowd() is inside."""
    pl = R.frustum_planes(seed).copy()
    pl[:, 3] *= F(6.0)
    return pl


def globals_(seed, n):
    """World transforms [n][12]: near-identity bases, origins within 2 units."""
    rng = np.random.default_rng(seed)
    g = np.zeros((n, 12), F)
    g[:, :9] = (np.eye(3).reshape(9) + rng.normal(0.0, 0.2, (n, 9))).astype(F)
    g[:, 9:] = rng.uniform(-2.0, 2.0, (n, 3)).astype(F)
    return g


def states(seed, n):
    return np.random.default_rng(seed).integers(0, 256, n, dtype=np.uint8)
