"""Skeleton bounds and frustum culling (include/mbik.h, ABI 14) written once more without
the code under test, for tests/test_bounds_cpu.py and tests/test_gpu_bounds.py.

Everything here follows the header's steps literally in numpy float32 scalars: one rounding per
operation, the compares as written (so NaN goes where they send it), the bones in ascending order.
`tree_bounds` is the same per-bone boxes merged as a pairwise tree: what a reduction would compute,
and what the library must NOT compute (the order pin).

`containment_tolerance` derives how far a skinned float32 vertex may lie outside its skeleton's
box, by counting roundings (u = 2^-24), for convex weights and finite transforms:

  bone box      the begin of a bone's box is always a vertex coordinate, exactly.  Its end is
                re-derived as fl(begin + fl(end - begin)) by every expand_to after the first hit and
                once more by xform_aabb: two roundings, of magnitudes <= 2A and <= A (A the largest
                |coordinate| among the bone's vertices), so after h hits the end lies at most
                d = 3 h u A below the largest coordinate.  (The first hit's size of 1e-5 only helps.)
  xform_aabb    a bound of a row is the origin plus three products: every term passes one product
                and at most three sums, 4 roundings: |error| <= 5 u T with one u of slack for the
                O(u^2) terms, T = |o_i| + sum_c |m_ic| max(|mn_c|, |mx_c|).  The box's deficit d
                reaches either bound through |m_ic|.
  merge chain   the begin is selected, never rounded.  The end is re-derived by every step, and
                once by the caller of the result (position + size): one subtraction of magnitude
                <= 2 T_box and one sum of magnitude <= T_box a step, 3 u T_box, at most U times for
                U used bones, plus one u T_box of slack; T_box the box's largest |bound| on the axis.
  skinning      the float32 vertex is within (2K + 6) u S of the exact blend (tests/skin_cases.py),
                and the exact blend is W times a convex combination of the exact images of the vertex
                under its bones' matrices, W = sum_k w_k: it leaves their hull by at most
                |W - 1| max_k T.
"""
import numpy as np

F = np.float32
U = 2.0 ** -24
TINY = F(1e-5)


def bone_boxes(B, pos, idx, w):
    """(boxes [B][6], used [B]) by RenderingServer::_surface_set_data's loop."""
    boxes = np.zeros((B, 6), F)
    used = np.zeros(B, np.uint8)
    with np.errstate(all="ignore"):
        for v in range(pos.shape[0]):
            for k in range(idx.shape[1]):
                wk, b = F(w[v, k]), int(idx[v, k])
                if wk == 0:
                    continue
                p = [F(pos[v, a]) for a in range(3)]
                if not used[b]:
                    boxes[b] = p + [TINY, TINY, TINY]
                    used[b] = 1
                    continue
                for a in range(3):
                    begin = F(boxes[b, a])
                    end = begin + F(boxes[b, 3 + a])
                    if p[a] < begin:
                        begin = p[a]
                    if p[a] > end:
                        end = p[a]
                    boxes[b, a], boxes[b, 3 + a] = begin, end - begin
    return boxes, used


def xform_aabb(m, box):
    """Transform3D::xform(AABB): m [12] basis rows then origin, box [6]."""
    with np.errstate(all="ignore"):
        mn = [F(box[a]) for a in range(3)]
        mx = [F(box[a]) + F(box[3 + a]) for a in range(3)]
        out = np.empty(6, F)
        for i in range(3):
            lo = hi = F(m[9 + i])
            for c in range(3):
                e = F(m[3 * i + c]) * mn[c]
                f = F(m[3 * i + c]) * mx[c]
                if e < f:
                    lo, hi = lo + e, hi + f
                else:
                    lo, hi = lo + f, hi + e
            out[i], out[3 + i] = lo, hi - lo
        return out


def merge(acc, t):
    """AABB::merge_with."""
    with np.errstate(all="ignore"):
        out = np.empty(6, F)
        for a in range(3):
            e1 = F(acc[3 + a]) + F(acc[a])
            e2 = F(t[3 + a]) + F(t[a])
            mn = F(acc[a]) if F(acc[a]) < F(t[a]) else F(t[a])
            mx = e1 if e1 > e2 else e2
            out[a], out[3 + a] = mn, mx - mn
        return out


def bone_images(boxes, used, skin_s):
    """The transformed boxes of one skeleton's used bones, ascending."""
    return [xform_aabb(skin_s[j], boxes[j]) for j in range(len(used)) if used[j]]


def chain_bounds(boxes, used, skin):
    """[count][6]: the ascending chain; six zeros without a used bone."""
    out = np.zeros((skin.shape[0], 6), F)
    for s in range(skin.shape[0]):
        ts = bone_images(boxes, used, skin[s])
        if ts:
            acc = ts[0]
            for t in ts[1:]:
                acc = merge(acc, t)
            out[s] = acc
    return out


def tree_bounds(boxes, used, skin):
    """[count][6]: the same boxes merged pairwise, level by level (a reduction's order)."""
    out = np.zeros((skin.shape[0], 6), F)
    for s in range(skin.shape[0]):
        ts = bone_images(boxes, used, skin[s])
        while len(ts) > 1:
            ts = [merge(ts[i], ts[i + 1]) if i + 1 < len(ts) else ts[i] for i in range(0, len(ts), 2)]
        if ts:
            out[s] = ts[0]
    return out


def cull(boxes, planes, skeleton_global=None, margin=0.0):
    """-> visible [count] uint8, by the header's five steps."""
    planes = np.asarray(planes, F).reshape(-1, 4)
    margin = F(margin)
    vis = np.zeros(boxes.shape[0], np.uint8)
    with np.errstate(all="ignore"):
        for s in range(boxes.shape[0]):
            b = np.array(boxes[s], F)
            if skeleton_global is not None:
                b = xform_aabb(skeleton_global[s], b)
            p, z = [F(b[a]) for a in range(3)], [F(b[3 + a]) for a in range(3)]
            if margin != 0:
                p = [x - margin for x in p]
                z = [x + margin * F(2.0) for x in z]
            e = [p[a] + z[a] for a in range(3)]
            seen = 1
            for n in planes:
                c = [p[a] if n[a] > 0 else e[a] for a in range(3)]
                if ((n[0] * c[0] + n[1] * c[1]) + n[2] * c[2]) > n[3]:
                    seen = 0
                    break
            vis[s] = seen
    return vis


def frustum_planes(seed):
    """Six outward planes of a box-like frustum around the origin, slightly tilted."""
    rng = np.random.default_rng(seed)
    planes = []
    for axis in range(3):
        for sign in (1.0, -1.0):
            n = rng.normal(0.0, 0.15, 3)
            n[axis] += sign
            n /= np.linalg.norm(n)
            planes.append([n[0], n[1], n[2], rng.uniform(1.0, 3.0)])
    return np.asarray(planes, F)


def containment_tolerance(K, pos, idx, w, boxes, used, skin, out_boxes, skin_scale):
    """(tol_lo, tol_hi) [count][V][3] in float64: how far below the box's begin / above its end
    (float64 position + size) a float32 skinned vertex may lie.  skin_scale is skin_cases.reference64's
    S for positions."""
    B, V = boxes.shape[0], pos.shape[0]
    p64, w64 = np.abs(pos.astype(np.float64)), w.astype(np.float64)
    hits = np.zeros(B)
    amax = np.zeros((B, 3))
    for v in range(V):
        for k in range(K):
            if w[v, k] != 0:
                hits[idx[v, k]] += 1
                amax[idx[v, k]] = np.maximum(amax[idx[v, k]], p64[v])
    deficit = 3.0 * hits[:, None] * U * amax                                      # [B][3]
    b64 = boxes.astype(np.float64)
    reach = np.maximum(np.abs(b64[:, :3]), np.abs(b64[:, :3] + b64[:, 3:]))          # [B][3]
    m = np.abs(skin.astype(np.float64))                                             # [count][B][12]
    basis, origin = m[..., :9].reshape(m.shape[:2] + (3, 3)), m[..., 9:]
    T = origin + np.einsum("sbic,bc->sbi", basis, reach + deficit)                  # [count][B][3]
    per_bone = 5.0 * U * T + np.einsum("sbic,bc->sbi", basis, deficit)              # [count][B][3]
    per_vertex = per_bone[:, idx].max(axis=2)                                       # [count][V][3]
    ymax = T[:, idx].max(axis=2)
    wsum = np.abs(w64.sum(axis=1) - 1.0)[None, :, None]
    o64 = out_boxes.astype(np.float64)
    tbox = np.maximum(np.abs(o64[:, :3]), np.abs(o64[:, :3] + o64[:, 3:]))[:, None, :]   # [count][1][3]
    n_used = int(np.count_nonzero(used))
    common = (2 * K + 6) * U * skin_scale + wsum * ymax + per_vertex
    return common, common + (3.0 * n_used + 1.0) * U * tbox
