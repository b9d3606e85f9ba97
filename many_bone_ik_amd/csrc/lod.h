// Distance LOD lists (mbik_cull_lod; include/mbik.h), shared by the device kernels
// (k_bounds.hip) and the host entries (host_bounds.cpp).  The semantics are those of Godot 4.3's
// RendererSceneCull::_visibility_range_check with VISIBILITY_RANGE_FADE_DISABLED, placed in front of
// mbik_cull_boxes' plane test (bounds.h's cull_visible):
//
//     box       the skeleton's box, moved to world space and grown by the margin when asked   (lod_box)
//     verdict   that box against the planes, as mbik_cull_boxes decides it                (cull_visible)
//     distance  from the camera to the centre of that box   (AABB::get_center, Vector3::distance_to)
//     ranges    for each range ascending: inside unless beyond `end` or before `begin`, each edge
//               moved by its margin, outwards for a skeleton that was inside the range last time
//               and inwards for one that was not (the hysteresis)                          (lod_in_range)
//
// One code path for both sides, built only from gd_math.h's primitives and compiled with
// -ffp-contract=off, so the device and the host produce the same bits.  The compares are written as
// Godot writes them: a NaN distance fails both, so such a skeleton is in every range.
//
// The header also holds the host loop behind mbik_cull_lod_cpu, host code without a HIP call:
// tools/san/lod_san.cpp runs it under ASan + UBSan.
#pragma once

#include "bounds.h"

namespace mbik {

constexpr int kLodMaxRanges = 8;        // MBIK_LOD_MAX_RANGES in mbik.h
constexpr uint32_t kLodExclusive = 1u;  // MBIK_LOD_EXCLUSIVE
constexpr uint8_t kLodNone = 255;       // MBIK_LOD_NONE

struct LodRange { // mbik_lod_range
	float begin, end, begin_margin, end_margin;
};

// What one skeleton's test gives: its next state byte (bit r: in range r), its level (the least r that
// is both seen and in range, or kLodNone), and the bits that decide which lists name it.
struct LodVerdict {
	uint8_t state, level, member;
};

// The box the plane test and the distance both see: cull_visible's first two steps.
GDI Box lod_box(Box b, const float *global, float margin) {
	if (global) b = box_xform(skin_load(global), b);
	if (margin != 0) {
		const float grow = margin * 2.0f;
		b.p = v3(b.p.x - margin, b.p.y - margin, b.p.z - margin);
		b.z = v3(b.z.x + grow, b.z.y + grow, b.z.z + grow);
	}
	return b;
}

// _visibility_range_check's two compares: prev is whether the skeleton was in this range last time.
GDI bool lod_in_range(float dist, const LodRange &g, bool prev) {
	float bo = -g.begin_margin, eo = g.end_margin;
	if (!prev) bo = -bo, eo = -eo;
	if (g.end > 0 && dist > g.end + eo) return false;
	if (g.begin > 0 && dist < g.begin + bo) return false;
	return true;
}

// One skeleton.  plane(i, nx, ny, nz, d) as for cull_visible; range(r) gives range r.
template <class Plane, class Range>
GDI LodVerdict lod_select(Box b, const float *global, float margin, int plane_count, Plane plane, V3 camera, int range_count,
		Range range, uint32_t flags, uint8_t prev_state) {
	b = lod_box(b, global, margin);
	const bool vis = cull_visible(b, nullptr, 0.0f, plane_count, plane);
	const V3 c = b.p + b.z * 0.5f;
	const float dist = length(c - camera);
	LodVerdict v{0, kLodNone, 0};
	for (int r = 0; r < range_count; r++) {
		if (!lod_in_range(dist, range(r), (prev_state >> r) & 1)) continue;
		v.state |= (uint8_t)(1u << r);
		if (vis && v.level == kLodNone) v.level = (uint8_t)r;
	}
	if (flags & kLodExclusive) v.member = v.level == kLodNone ? 0 : (uint8_t)(1u << v.level);
	else v.member = vis ? v.state : 0;
	return v;
}

// ---------------- host path ----------------
// boxes [count][6], skeleton_global [count][12] or null, planes [plane_count][4], camera [3], ranges
// [range_count]; state [count] in and out, level [count] or null, indices [range_count][count],
// list_counts [range_count]
inline void cull_lod_host(int32_t count, const float *boxes, const float *skeleton_global, float margin, int32_t plane_count,
		const float *planes, const float *camera, int32_t range_count, const LodRange *ranges, uint32_t flags, uint8_t *state,
		uint8_t *level, int32_t *indices, int32_t *list_counts) {
	int32_t n[kLodMaxRanges] = {};
	const V3 cam = v3(camera[0], camera[1], camera[2]);
	for (int64_t s = 0; s < count; s++) {
		const LodVerdict v = lod_select(
				box_load(boxes + s * 6), skeleton_global ? skeleton_global + s * 12 : nullptr, margin, plane_count,
				[&](int i, float &nx, float &ny, float &nz, float &d) { nx = planes[i * 4], ny = planes[i * 4 + 1], nz = planes[i * 4 + 2], d = planes[i * 4 + 3]; },
				cam, range_count, [&](int r) { return ranges[r]; }, flags, state[s]);
		state[s] = v.state;
		if (level) level[s] = v.level;
		for (int r = 0; r < range_count; r++)
			if ((v.member >> r) & 1) indices[(int64_t)r * count + n[r]++] = (int32_t)s;
	}
	for (int r = 0; r < range_count; r++) list_counts[r] = n[r];
}

} // namespace mbik
