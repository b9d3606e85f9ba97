// Skeleton bounds and frustum culling (mbik_skin_bounds, mbik_cull_boxes), shared by
// the device kernels (k_bounds.hip) and the host entries (host_bounds.cpp).  The semantics are those
// of Godot 4.3's MeshStorage::mesh_get_aabb(mesh, skeleton) -- one box per bone, built when the
// surface is created, moved by the skeleton's skin transforms and merged -- and of the plane half
// of AABB::intersects_convex_shape.  A box is Godot's AABB: position, then size.
//
//     bone boxes   for v ascending, k = 0..K-1: a weight that is not +-0 puts positions[v] into the
//                  box of bone_indices[v][k]: the first hit makes { p, (1e-5, 1e-5, 1e-5) }, a later
//                  one AABB::expand_to                                          (bone_boxes_build)
//     per skeleton for the used bones j ascending: t = Transform3D::xform(AABB) of box[j] by
//                  skin[s][j]; the first t starts the chain, every later one AABB::merge_with's it
//                                                                               (box_xform, box_merge)
//     culling      the box, moved to world space and grown by a margin when asked, against outward
//                  planes: culled by the first plane whose nearest corner is over it    (cull_visible)
//
// One code path for both sides, built only from gd_math.h's primitives and compiled with
// -ffp-contract=off, so the device and the host produce the same bits.  Every compare is written
// as Godot writes it (no fminf / fmaxf, which treat NaN differently): non-finite values go where
// those compares send them.  The merge is a chain, not a reduction: each step re-derives
// end = size + position from the rounded size, so the result depends on the order, and the order
// is ascending bone index.
//
// The header also holds the box builder and the packing of the used-bone table, host code without
// a HIP call: tools/san/bounds_san.cpp runs them under ASan + UBSan.
#pragma once

#include <cstdint>
#include <cstring>

#include "skin.h"

namespace mbik {

using namespace gd;

constexpr int kCullMaxPlanes = 16; // MBIK_CULL_MAX_PLANES in mbik.h

struct Box {
	V3 p, z; // position, size
};

// ---------------- arithmetic ----------------
GDI Box box_load(const float *b) { return Box{v3(b[0], b[1], b[2]), v3(b[3], b[4], b[5])}; }
GDI void box_store(float *o, const Box &b) { o[0] = b.p.x, o[1] = b.p.y, o[2] = b.p.z, o[3] = b.z.x, o[4] = b.z.y, o[5] = b.z.z; }

// one basis element's share of a row's bounds
GDI void box_axis(float m, float mn, float mx, float &lo, float &hi) {
	const float e = m * mn, f = m * mx;
	if (e < f) lo = lo + e, hi = hi + f;
	else lo = lo + f, hi = hi + e;
}
GDI void box_row(V3 r, float o, V3 mn, V3 mx, float &lo, float &hi) {
	lo = hi = o;
	box_axis(r.x, mn.x, mx.x, lo, hi);
	box_axis(r.y, mn.y, mx.y, lo, hi);
	box_axis(r.z, mn.z, mx.z, lo, hi);
}
// Transform3D::xform(AABB)
GDI Box box_xform(const X3 &t, const Box &b) {
	const V3 mn = b.p, mx = b.p + b.z;
	V3 lo, hi;
	box_row(t.b.r[0], t.o.x, mn, mx, lo.x, hi.x);
	box_row(t.b.r[1], t.o.y, mn, mx, lo.y, hi.y);
	box_row(t.b.r[2], t.o.z, mn, mx, lo.z, hi.z);
	return Box{lo, hi - lo};
}
// AABB::merge_with, one axis: (p, z) is the accumulated box's, (tp, tz) the other's.  The axes are
// independent chains, which is what lets the device give each its own lane.
GDI void box_merge_axis(float &p, float &z, float tp, float tz) {
	const float e1 = z + p, e2 = tz + tp;
	const float mn = p < tp ? p : tp, mx = e1 > e2 ? e1 : e2;
	p = mn, z = mx - mn;
}
// AABB::merge_with
GDI Box box_merge(const Box &a, const Box &t) {
	Box r = a;
	box_merge_axis(r.p.x, r.z.x, t.p.x, t.z.x);
	box_merge_axis(r.p.y, r.z.y, t.p.y, t.z.y);
	box_merge_axis(r.p.z, r.z.z, t.p.z, t.z.z);
	return r;
}
// AABB::expand_to
GDI Box box_expand(const Box &b, V3 p) {
	V3 begin = b.p, end = b.p + b.z;
	if (p.x < begin.x) begin.x = p.x;
	if (p.y < begin.y) begin.y = p.y;
	if (p.z < begin.z) begin.z = p.z;
	if (p.x > end.x) end.x = p.x;
	if (p.y > end.y) end.y = p.y;
	if (p.z > end.z) end.z = p.z;
	return Box{begin, end - begin};
}

// One skeleton's verdict.  global: its 12 floats (basis rows, origin) or null; plane(i) gives plane i
// as (normal x, y, z, d), outward.  A NaN anywhere fails `> d`, so such a box stays visible.
template <class Plane>
GDI bool cull_visible(Box b, const float *global, float margin, int plane_count, Plane plane) {
	if (global) b = box_xform(skin_load(global), b);
	if (margin != 0) {
		const float grow = margin * 2.0f;
		b.p = v3(b.p.x - margin, b.p.y - margin, b.p.z - margin);
		b.z = v3(b.z.x + grow, b.z.y + grow, b.z.z + grow);
	}
	const V3 e = b.p + b.z;
	for (int i = 0; i < plane_count; i++) {
		float nx, ny, nz, d;
		plane(i, nx, ny, nz, d);
		const V3 c = v3(nx > 0 ? b.p.x : e.x, ny > 0 ? b.p.y : e.y, nz > 0 ? b.p.z : e.z);
		if (dot(v3(nx, ny, nz), c) > d) return false;
	}
	return true;
}

// ---------------- the bone boxes (host) ----------------
// boxes [B][6] and used [B] from a checked mesh (skin_check_mesh == SKIN_OK).  An unused bone keeps
// used = 0 and six zeros.  Blend shapes do not enter.
inline void bone_boxes_build(int32_t B, int32_t V, int32_t K, const float *positions, const int32_t *bone_indices, const float *weights,
		float *boxes, uint8_t *used) {
	for (int64_t i = 0; i < (int64_t)B * 6; i++) boxes[i] = 0.0f;
	for (int64_t b = 0; b < B; b++) used[b] = 0;
	for (int64_t v = 0; v < V; v++)
		for (int k = 0; k < K; k++) {
			const float w = weights[v * K + k];
			if (w == 0) continue; // (+-0 skipped; NaN and negative weights count)
			const int32_t b = bone_indices[v * K + k];
			const V3 p = v3(positions[v * 3], positions[v * 3 + 1], positions[v * 3 + 2]);
			float *bx = boxes + (int64_t)b * 6;
			if (!used[b]) {
				box_store(bx, Box{p, v3(1e-5f, 1e-5f, 1e-5f)});
				used[b] = 1;
			} else {
				box_store(bx, box_expand(box_load(bx), p));
			}
		}
}

// The device table: one 32-byte record per used bone, ascending --
//   bone index (int32), position x, y, z;  size x, y, z, 0
// -- read as two 16-byte quads.
constexpr int kBoneRecordBytes = 32;
inline int32_t bone_table_count(int32_t B, const uint8_t *used) {
	int32_t n = 0;
	for (int32_t b = 0; b < B; b++) n += used[b] != 0;
	return n;
}
// Fills `out` (bone_table_count() records); returns the record count.
inline int32_t bone_table_pack(int32_t B, const float *boxes, const uint8_t *used, unsigned char *out) {
	int32_t n = 0;
	for (int32_t b = 0; b < B; b++) {
		if (!used[b]) continue;
		unsigned char *r = out + (int64_t)n * kBoneRecordBytes;
		memset(r, 0, kBoneRecordBytes);
		memcpy(r, &b, 4);
		memcpy(r + 4, boxes + (int64_t)b * 6, 12);
		memcpy(r + 16, boxes + (int64_t)b * 6 + 3, 12);
		n++;
	}
	return n;
}

// ---------------- host paths ----------------
// skin [count][B][12] -> out [count][6]: the ascending chain over the used bones; six zeros without one
inline void skin_bounds_host(int32_t B, const float *boxes, const uint8_t *used, int32_t count, const float *skin, float *out) {
	for (int64_t s = 0; s < count; s++) {
		Box acc{v3(0, 0, 0), v3(0, 0, 0)};
		bool any = false;
		for (int64_t j = 0; j < B; j++) {
			if (!used[j]) continue;
			const Box t = box_xform(skin_load(skin + (s * B + j) * 12), box_load(boxes + j * 6));
			acc = any ? box_merge(acc, t) : t;
			any = true;
		}
		box_store(out + s * 6, acc);
	}
}

// boxes [count][6], skeleton_global [count][12] or null, planes [plane_count][4]; visible [count] or
// null, indices [count] or null, visible_count [1] or null
inline void cull_boxes_host(int32_t count, const float *boxes, const float *skeleton_global, float margin, int32_t plane_count,
		const float *planes, uint8_t *visible, int32_t *indices, int32_t *visible_count) {
	int32_t n = 0;
	for (int64_t s = 0; s < count; s++) {
		const bool vis = cull_visible(box_load(boxes + s * 6), skeleton_global ? skeleton_global + s * 12 : nullptr, margin, plane_count,
				[&](int i, float &nx, float &ny, float &nz, float &d) { nx = planes[i * 4], ny = planes[i * 4 + 1], nz = planes[i * 4 + 2], d = planes[i * 4 + 3]; });
		if (visible) visible[s] = vis ? 1 : 0;
		if (vis) {
			if (indices) indices[n] = (int32_t)s;
			n++;
		}
	}
	if (visible_count) *visible_count = n;
}

} // namespace mbik
