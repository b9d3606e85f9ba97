"""mbik_bone_boxes_cpu, mbik_skin_bounds_cpu and mbik_cull_boxes_cpu (include/mbik.h, ABI 14; DESIGN.md
§18) without a device: bit for bit against tests/bounds_recipe.py's restatement in float32 scalars
(two NaNs count as equal), the pin of the merge order, what the boxes mean in float64, and the
argument checks."""
import ctypes as C

import numpy as np
import pytest

from many_bone_ik_amd import _lib
from many_bone_ik_amd import workloads as W
from many_bone_ik_amd.skinning import bone_boxes_cpu, cull_boxes_cpu, skin_bounds_cpu, skin_vertices_cpu, synthetic_mesh
from many_bone_ik_amd.solver import pose_globals_cpu

from . import bounds_recipe as R
from . import skin_cases as S

F = np.float32


def sparse_mesh(seed, B, V, K, keep=3):
    """A mesh that names every `keep`-th bone only."""
    pos, _, idx, w = S.random_mesh(seed, B, V, K)
    return pos, (idx // keep * keep).astype(np.int32), w


# ---------------- bone boxes ----------------
@pytest.mark.parametrize("K", [4, 8])
@pytest.mark.parametrize("B", [1, 3, 32, 200])
def test_bone_boxes_match_recipe(mbik, B, K):
    """Random meshes with signed weights; V small enough to leave bones of the larger rigs unused."""
    for V in (1, 7, 40):
        pos, _, idx, w = S.random_mesh(10 * B + V, B, V, K, weights="signed")
        w[::3, 1] = 0.0
        got, used = bone_boxes_cpu(B, pos, idx, w)
        ref, ref_used = R.bone_boxes(B, pos, idx, w)
        assert np.array_equal(used, ref_used) and S.same_bits(got, ref), (B, K, V)
        assert not got[used == 0].any()
    if B == 200:
        assert (ref_used == 0).any() and (ref_used == 1).any()


def test_bone_boxes_special_weights_and_vertices(mbik):
    """+0 and -0 are skipped, negative and NaN weights count; a NaN coordinate as a first hit is
    stored, as a later hit it changes nothing; a mesh of zero weights uses no bone; one used bone."""
    B, K = 4, 4
    pos = np.array([[1, 2, 3], [np.nan, 5, 6], [-1, -2, -3], [np.nan, np.nan, np.nan], [7, 8, 9]], F)
    idx = np.array([[0, 1, 2, 3], [0, 1, 2, 3], [0, 1, 2, 3], [0, 1, 2, 3], [0, 1, 2, 3]], np.int32)
    #            bone 0          bone 1      bone 2       bone 3
    w = np.array([[0.5, 0.0, -0.0, 0.0],      # bone 0: finite first hit
                  [np.nan, 1.0, 0.0, -0.0],   # bone 0: NaN x as a later hit (NaN weight counts); bone 1: NaN x as the first hit
                  [-0.25, 0.5, 0.0, 0.0],     # negative weight counts
                  [1.0, 0.0, 0.0, 0.0],       # an all-NaN vertex as a later hit of bone 0
                  [0.0, 0.25, 0.0, 0.0]], F)
    got, used = bone_boxes_cpu(B, pos, idx, w)
    ref, ref_used = R.bone_boxes(B, pos, idx, w)
    assert used.tolist() == [1, 1, 0, 0] == ref_used.tolist() and S.same_bits(got, ref)
    assert S.same_bits(got[0, :3], [-1, -2, -3]) and np.isfinite(got[0]).all()      # the NaN hits changed nothing
    assert got[0, 4] == F(F(5) - F(-2))                                             # ... but their finite coordinates did
    assert np.isnan(got[1, 0]) and np.isnan(got[1, 3]) and np.isfinite(got[1, [1, 2, 4, 5]]).all()
    zero_b, zero_u = bone_boxes_cpu(B, pos, idx, np.zeros_like(w))
    assert not zero_u.any() and not zero_b.any()
    one_b, one_u = bone_boxes_cpu(B, pos[:1], np.full((1, K), 2, np.int32), np.array([[0.25, 0, 0, 0]], F))
    assert one_u.tolist() == [0, 0, 1, 0] and S.same_bits(one_b[2], [1, 2, 3, 1e-5, 1e-5, 1e-5])


def test_bone_boxes_checks(mbik):
    L = _lib.load()
    pos, _, idx, w = S.random_mesh(1, 5, 9, 4)
    boxes, used = np.zeros((5, 6), F), np.zeros(5, np.uint8)
    call = lambda B, V, K, p, i, ww, b, u: L.mbik_bone_boxes_cpu(B, V, K, S.ptr(p), S.ptr(i), S.ptr(ww), S.ptr(b), S.ptr(u))
    E = _lib.MBIK_EINVAL
    assert call(5, 9, 4, pos, idx, w, boxes, used) == _lib.MBIK_OK
    assert call(5, 9, 3, pos, idx, w, boxes, used) == E          # influences
    assert call(-1, 9, 4, pos, idx, w, boxes, used) == E         # negative
    assert call(5, 9, 4, None, idx, w, boxes, used) == E         # null array
    assert call(4, 9, 4, pos, np.full_like(idx, 4), w, boxes, used) == E     # index out of range
    assert call(5, 9, 4, pos, idx, w, None, used) == E and call(5, 9, 4, pos, idx, w, boxes, None) == E
    assert call(5000, 9, 4, pos, idx, w, np.zeros((5000, 6), F), np.zeros(5000, np.uint8)) == _lib.MBIK_OK   # any bone count


# ---------------- one box per skeleton ----------------
@pytest.mark.parametrize("K", [4, 8])
@pytest.mark.parametrize("B", [1, 3, 32, 200])
def test_skin_bounds_match_recipe(mbik, B, K):
    skin = S.random_skin(20 + B, 3, B)
    pos, _, idx, w = S.random_mesh(30 + B, B, 40, K)
    for name, (p, i, ww) in {"dense": (pos, idx, w), "sparse": sparse_mesh(31 + B, B, 40, K), "one": (pos[:1], idx[:1] * 0 + B - 1, w[:1]),
                             "none": (pos, idx, w * 0)}.items():
        boxes, used = bone_boxes_cpu(B, p, i, ww)
        got = skin_bounds_cpu(boxes, used, skin)
        assert S.same_bits(got, R.chain_bounds(boxes, used, skin)), (B, K, name)
        if name == "none":
            assert not used.any() and not got.any()
        if name == "one":
            assert used.sum() == 1


def test_skin_bounds_non_finite(mbik):
    """A NaN and an infinity in one bone's matrix go where the compares send them: in the last bone
    they reach the result; in an earlier bone the next merge's failed compares select the finite
    operand again (AABB::merge_with's behaviour, kept)."""
    B = 8
    pos, _, idx, w = S.random_mesh(40, B, 60, 4)
    boxes, used = bone_boxes_cpu(B, pos, idx, w)
    assert used.all()
    skin = S.random_skin(41, 5, B)
    skin[1, 7, 4] = np.nan
    skin[2, 7, 9] = np.inf
    skin[3, 7, 0] = -np.inf
    skin[4, 3, 4] = np.nan
    got = skin_bounds_cpu(boxes, used, skin)
    assert S.same_bits(got, R.chain_bounds(boxes, used, skin))
    assert np.isfinite(got[0]).all() and not np.isfinite(got[1:4]).all(axis=1).any()


def test_merge_order_is_the_ascending_chain(mbik):
    """B = 32, every bone used: the library equals the ascending chain on every skeleton and, on at
    least one of them, differs from the pairwise tree a reduction would compute."""
    B, count = 32, 48
    pos, _, idx, w = S.random_mesh(50, B, 400, 4)
    boxes, used = bone_boxes_cpu(B, pos, idx, w)
    assert used.all()
    skin = S.random_skin(51, count, B)
    chain, tree = R.chain_bounds(boxes, used, skin), R.tree_bounds(boxes, used, skin)
    differs = [s for s in range(count) if not S.same_bits(chain[s], tree[s])]
    print("skeletons on which chain and tree differ:", len(differs), "of", count)
    assert differs                                     # the pin is not vacuous
    got = skin_bounds_cpu(boxes, used, skin)
    assert S.same_bits(got, chain)
    assert not S.same_bits(got[differs[0]], tree[differs[0]])


def containment_ratio(K, B, pos, idx, w, skin):
    """The worst (distance outside the box) / (derived tolerance) over every coordinate, and how many lie outside at all."""
    assert (w >= 0).all() and np.abs(w.astype(np.float64).sum(axis=1) - 1.0).max() <= K * R.U    # convex
    assert np.isfinite(skin).all()
    boxes, used = bone_boxes_cpu(B, pos, idx, w)
    out = skin_bounds_cpu(boxes, used, skin)
    verts, _ = skin_vertices_cpu(B, pos, idx, w, skin)
    _, _, scale, _ = S.reference64(pos, pos, idx, w, skin)
    tol_lo, tol_hi = R.containment_tolerance(K, pos, idx, w, boxes, used, skin, out, scale)
    o64, v64 = out.astype(np.float64), verts.astype(np.float64)
    lo, hi = o64[:, None, :3], o64[:, None, :3] + o64[:, None, 3:]
    below, above = (lo - v64) / tol_lo, (v64 - hi) / tol_hi
    return max(below.max(), above.max()), int(((below > 0) | (above > 0)).sum()), v64.size


@pytest.mark.parametrize("K", [4, 8])
def test_skinned_vertices_lie_inside_their_box(mbik, K):
    """float64 meaning: with convex weights and finite transforms every float32 skinned vertex lies in
    its skeleton's box up to the rounding bound bounds_recipe.containment_tolerance derives.
    Measured: the worst ratio is negative (-9965 for K = 4, -7312 for K = 8): blended vertices of a posed
    rig sit well inside the merged boxes of rotated boxes."""
    wl = W.generate(2, 6)
    parents, pins = wl.topo.parents.tolist(), wl.topo.pins.tolist()
    B, V = len(parents), 300
    rest, _ = pose_globals_cpu(parents, [], wl.pose[:1])
    pos, _, idx, w = synthetic_mesh(parents, rest[0], V, K, seed=7)
    inv_bind = np.random.default_rng(8).uniform(-1.0, 1.0, (B, 12)).astype(F)
    skin, _ = pose_globals_cpu(parents, pins, wl.pose, inv_bind=inv_bind)
    worst, outside, total = containment_ratio(K, B, pos, idx, w, skin)
    print(f"K={K}: worst excess / tolerance = {worst:.4f}; {outside} of {total} coordinates outside the float box at all")
    assert worst <= 1.0


@pytest.mark.parametrize("K", [4, 8])
def test_tight_boxes_hold_their_vertices(mbik, K):
    """The same bound where it binds: one bone a vertex (weight 1, the other slots 0) and axis-aligned
    transforms (signed scales and a translation), so every box is the hull of its vertices' images and
    the extreme vertices lie on its faces up to rounding.  Measured: 9 (K = 4) and 8 (K = 8) of 48,000
    coordinates lie outside the float box, the worst by 0.021 and 0.036 of the tolerance."""
    B, V, count = 32, 2000, 8
    pos, _, idx, _ = S.random_mesh(90 + K, B, V, K)
    w = np.zeros((V, K), F)
    w[:, 0] = 1.0
    rng = np.random.default_rng(91 + K)
    skin = np.zeros((count, B, 12), F)
    skin[..., 0], skin[..., 4], skin[..., 8] = (rng.uniform(0.3, 3.0, (3, count, B)) * rng.choice([-1.0, 1.0], (3, count, B))).astype(F)
    skin[..., 9:] = rng.uniform(-100.0, 100.0, (count, B, 3))
    worst, outside, total = containment_ratio(K, B, pos, idx, w, skin)
    print(f"tight K={K}: worst excess / tolerance = {worst:.4f}; {outside} of {total} coordinates outside the float box at all")
    assert worst <= 1.0


def test_skin_bounds_checks(mbik):
    L = _lib.load()
    B, n = 5, 3
    boxes, used = np.zeros((B, 6), F), np.ones(B, np.uint8)
    buf = np.zeros(n * B * 12 + n * 6, F)
    skin, out = buf[:n * B * 12], buf[n * B * 12:]
    call = lambda B, bb, u, c, s, o: L.mbik_skin_bounds_cpu(B, S.ptr(bb), S.ptr(u), c, S.ptr(s), S.ptr(o))
    E = _lib.MBIK_EINVAL
    assert call(B, boxes, used, n, skin, out) == _lib.MBIK_OK      # adjacent, not overlapping
    assert call(B, boxes, used, -1, skin, out) == E
    assert call(B, boxes, used, n, None, out) == E and call(B, boxes, used, n, skin, None) == E
    assert call(B, None, used, n, skin, out) == E and call(B, boxes, None, n, skin, out) == E
    assert call(B, boxes, used, n, skin, buf[n * B * 12 - 1:]) == E      # boxes overlaps skin
    assert call(B, boxes, used, 0, None, None) == _lib.MBIK_OK


# ---------------- culling ----------------
def test_cull_hand_made_cases(mbik):
    plane = np.array([[1, 0, 0, 2]], F)                      # visible side: x <= 2
    boxes = np.array([[3, 0, 0, 1, 1, 1],                    # wholly over
                      [-1, 0, 0, 1, 1, 1],                   # wholly under
                      [1.5, 0, 0, 1, 1, 1],                  # straddling
                      [2, 0, 0, 1, 1, 1],                    # touching: dot == d
                      [np.nextafter(F(2), F(3)), 0, 0, 1, 1, 1],
                      [np.nan, 0, 0, 1, 1, 1],               # NaN: stays visible
                      [3, 0, 0, np.nan, 1, 1]], F)           # NaN in an unused corner: culled by the finite one
    vis, ind = cull_boxes_cpu(boxes, plane)
    assert vis.tolist() == [0, 1, 1, 1, 0, 1, 0] and ind.tolist() == [1, 2, 3, 5]
    assert np.array_equal(vis, R.cull(boxes, plane))
    # the normal's sign picks the other corner
    vis, _ = cull_boxes_cpu(boxes[:4], np.array([[-1, 0, 0, -2.5]], F))          # visible side: x >= 2.5
    assert vis.tolist() == [1, 0, 1, 1]
    # margin turns a culled box visible
    assert cull_boxes_cpu(boxes[:1], plane, margin=0.5)[0].tolist() == [0]
    assert cull_boxes_cpu(boxes[:1], plane, margin=1.0)[0].tolist() == [1]      # 3 - 1 == 2: touching
    # skeleton_global moves a box across the plane, both ways
    move = np.array([[1, 0, 0, 0, 1, 0, 0, 0, 1, -2, 0, 0], [1, 0, 0, 0, 1, 0, 0, 0, 1, 5, 0, 0]], F)
    assert cull_boxes_cpu(boxes[:2], plane, skeleton_global=move)[0].tolist() == [1, 0]
    flip = np.array([[-1, 0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0]], F)                  # x -> -x: [3, 4] -> [-4, -3]
    assert cull_boxes_cpu(boxes[:1], plane, skeleton_global=flip)[0].tolist() == [1]


def test_cull_plane_counts(mbik):
    L = _lib.load()
    boxes = np.array([[5, 5, 5, 1, 1, 1], [0, 0, 0, 1, 1, 1]], F)
    vis, ind = cull_boxes_cpu(boxes, np.zeros((0, 4), F))
    assert vis.tolist() == [1, 1] and ind.tolist() == [0, 1]                    # no plane: everything visible
    planes = np.tile(np.array([[0, 0, 1, 100]], F), (16, 1))
    planes[15] = [1, 0, 0, 2]                                                   # only the sixteenth plane culls
    assert cull_boxes_cpu(boxes, planes)[0].tolist() == [0, 1]
    visible, n = np.zeros(2, np.uint8), np.zeros(1, np.int32)
    call = lambda count, pc, pl: L.mbik_cull_boxes_cpu(count, S.ptr(boxes), None, 0.0, pc, S.ptr(pl), S.ptr(visible), None, S.ptr(n))
    planes17 = np.tile(planes[:1], (17, 1))
    assert call(2, 16, planes17) == _lib.MBIK_OK
    assert call(2, 17, planes17) == _lib.MBIK_EINVAL and call(2, -1, planes17) == _lib.MBIK_EINVAL


@pytest.mark.parametrize("seed", [1, 2])
def test_cull_random_boxes_against_a_frustum(mbik, seed):
    rng = np.random.default_rng(60 + seed)
    n = 500
    boxes = np.concatenate([rng.uniform(-4.0, 4.0, (n, 3)), rng.uniform(0.0, 1.5, (n, 3))], axis=1).astype(F)
    planes = R.frustum_planes(seed)
    sg = S.random_skin(70 + seed, n, 1).reshape(n, 12)
    for kw in (dict(), dict(margin=0.75), dict(skeleton_global=sg), dict(skeleton_global=sg, margin=-0.1)):
        vis, ind = cull_boxes_cpu(boxes, planes, **kw)
        assert np.array_equal(vis, R.cull(boxes, planes, **kw)), kw
        assert np.array_equal(ind, np.flatnonzero(vis)) and (np.diff(ind) > 0).all()
        assert 0 < vis.sum() < n


def test_cull_checks(mbik):
    L = _lib.load()
    n = 4
    buf = np.zeros(n * 6 + n * 12 + 64, F)
    boxes, sg = buf[:n * 6], buf[n * 6:n * 18]
    tail = buf[n * 18:].view(np.uint8)
    visible, indices, cnt = tail[:n], tail[16:16 + 4 * n].view(np.int32), tail[64:68].view(np.int32)
    planes = np.array([[1, 0, 0, 1]], F)

    def call(count=n, b=boxes, g=sg, pc=1, pl=planes, v=visible, i=indices, c=cnt):
        return L.mbik_cull_boxes_cpu(count, S.ptr(b), S.ptr(g), 0.0, pc, S.ptr(pl), S.ptr(v), S.ptr(i), S.ptr(c))

    E = _lib.MBIK_EINVAL
    assert call() == _lib.MBIK_OK and cnt[0] == n
    assert call(b=None) == E and call(count=-1) == E and call(pl=None) == E
    assert call(v=None, i=None) == E                    # both outputs null
    assert call(c=None) == E                            # indices without visible_count
    assert call(i=None, c=None) == _lib.MBIK_OK         # visible alone
    assert call(v=None) == _lib.MBIK_OK                 # indices alone
    assert call(v=buf[n * 6 - 1:].view(np.uint8)) == E                          # visible overlaps boxes
    assert call(i=buf[n * 18 - 1:].view(np.int32)) == E                         # indices overlaps skeleton_global
    assert call(c=buf[:1].view(np.int32)) == E                                  # visible_count overlaps boxes
    assert call(i=tail[2:2 + 4 * n].view(np.int32)) == E                        # indices overlaps visible
    assert call(c=tail[16:20].view(np.int32)) == E                              # visible_count overlaps indices
    cnt[0] = 77
    assert call(count=0) == _lib.MBIK_OK and cnt[0] == 0                        # count == 0 still writes the count
