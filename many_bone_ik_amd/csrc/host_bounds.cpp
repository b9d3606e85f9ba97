// Skeleton bounds, frustum culling and distance LOD lists (include/mbik.h, ABI 14; bounds.h, lod.h):
// the readback of a mesh's bone boxes, mbik_skin_bounds, mbik_cull_boxes and mbik_cull_lod, which launch k_bounds.hip's
// kernels on the mesh's device, and the _cpu entries, which run the same code on the host.  A device entry and its _cpu
// form take their arguments through one check.  The boxes themselves are built with the mesh (host_skin.cpp).
#include "host.h"

#include <cmath>
#include <cstddef>

#include "bounds.h"
#include "lod.h"

using namespace mbik_host;

static_assert(sizeof(mbik_lod_range) == sizeof(mbik::LodRange) && offsetof(mbik_lod_range, end) == offsetof(mbik::LodRange, end) &&
				offsetof(mbik_lod_range, begin_margin) == offsetof(mbik::LodRange, begin_margin) &&
				offsetof(mbik_lod_range, end_margin) == offsetof(mbik::LodRange, end_margin),
		"mbik_lod_range is lod.h's LodRange");
static_assert(MBIK_LOD_MAX_RANGES == mbik::kLodMaxRanges && MBIK_LOD_EXCLUSIVE == mbik::kLodExclusive && MBIK_LOD_NONE == mbik::kLodNone,
		"mbik.h's LOD constants are lod.h's");

namespace {

// LDS a bounds block aims for, as the skinning's: eight 256-thread blocks share a CU's 160 KiB.
constexpr int64_t kBoundsBlockLdsTarget = 20 * 1024;
// Skeletons a block takes at most: one lane each in the merge chain, so one wave's worth.
constexpr int kBoundsMaxSkeletonsPerBlock = 64;

int bounds_skeletons_per_block(int32_t B, int32_t count) {
	const int64_t per = std::max<int64_t>(48, (int64_t)B * 48);
	return (int)std::max<int64_t>(1, std::min<int64_t>({kBoundsBlockLdsTarget / per, kBoundsMaxSkeletonsPerBlock, count}));
}

// 0 = go on, kNothingToDo, or the refusal
int check_bounds_call(int32_t B, int32_t count, const float *skin, const float *boxes) {
	if (int rc = check_count(count)) return rc;
	if (count == 0) return kNothingToDo;
	if (int rc = check_given(skin, "skin")) return rc;
	if (int rc = check_given(boxes, "boxes")) return rc;
	return check_apart(skin, (size_t)count * B * 12 * sizeof(float), "skin", boxes, (size_t)count * 6 * sizeof(float), "boxes");
}

// The head of both culling calls' checks: the count and the planes.
int check_planes(int32_t count, int32_t plane_count, const float *planes) {
	if (int rc = check_count(count)) return rc;
	if (plane_count < 0 || plane_count > mbik::kCullMaxPlanes) return fail(MBIK_EINVAL, "plane_count outside [0, MBIK_CULL_MAX_PLANES]");
	if (plane_count > 0 && !planes) return fail(MBIK_EINVAL, "null planes");
	return MBIK_OK;
}

int check_cull_call(int32_t count, const float *boxes, const float *skeleton_global, int32_t plane_count, const float *planes,
		const uint8_t *visible, const int32_t *indices, const int32_t *visible_count) {
	if (int rc = check_planes(count, plane_count, planes)) return rc;
	if (!visible && !indices) return fail(MBIK_EINVAL, "both visible and indices are null");
	if (indices && !visible_count) return fail(MBIK_EINVAL, "indices without visible_count");
	if (count > 0)
		if (int rc = check_given(boxes, "boxes")) return rc;
	const size_t c = (size_t)count;
	return check_disjoint({{visible, c, "visible"}, {indices, c * sizeof(int32_t), "indices"}, {visible_count, sizeof(int32_t), "visible_count"}},
			{{boxes, c * 6 * sizeof(float), "boxes"}, {skeleton_global, c * 12 * sizeof(float), "skeleton_global"}});
}

int check_lod_call(int32_t count, const float *boxes, const float *skeleton_global, int32_t plane_count, const float *planes,
		const float *camera, int32_t range_count, const mbik_lod_range *ranges, uint32_t flags, const uint8_t *state, const uint8_t *level,
		const int32_t *indices, const int32_t *list_counts) {
	if (int rc = check_planes(count, plane_count, planes)) return rc;
	if (range_count < 1 || range_count > mbik::kLodMaxRanges) return fail(MBIK_EINVAL, "range_count outside [1, MBIK_LOD_MAX_RANGES]");
	if (int rc = check_given(ranges, "ranges")) return rc;
	if (int rc = check_given(camera, "camera")) return rc;
	if (!std::isfinite(camera[0]) || !std::isfinite(camera[1]) || !std::isfinite(camera[2])) return fail(MBIK_EINVAL, "camera is not finite");
	for (int r = 0; r < range_count; r++) {
		const float f[4] = {ranges[r].begin, ranges[r].end, ranges[r].begin_margin, ranges[r].end_margin};
		for (float x : f)
			if (!std::isfinite(x) || x < 0) return fail(MBIK_EINVAL, "range " + std::to_string(r) + " has a negative or non-finite field");
		if (ranges[r].end > 0 && ranges[r].begin > ranges[r].end) return fail(MBIK_EINVAL, "range " + std::to_string(r) + " begins behind its end");
	}
	// (mbik_skin_vertices_listed's words, not check_flags')
	if (flags & ~(uint32_t)MBIK_LOD_EXCLUSIVE) return fail(MBIK_EINVAL, "unknown flag bits");
	if (count > 0) {
		if (int rc = check_given(boxes, "boxes")) return rc;
		if (int rc = check_given(state, "state")) return rc;
		if (int rc = check_given(indices, "indices")) return rc;
		if (int rc = check_given(list_counts, "list_counts")) return rc;
	}
	const size_t c = (size_t)count, rc = (size_t)range_count;
	return check_disjoint({{state, c, "state"}, {level, c, "level"}, {indices, rc * c * sizeof(int32_t), "indices"},
								  {list_counts, rc * sizeof(int32_t), "list_counts"}},
			{{boxes, c * 6 * sizeof(float), "boxes"}, {skeleton_global, c * 12 * sizeof(float), "skeleton_global"},
					{planes, (size_t)plane_count * 4 * sizeof(float), "planes"}, {camera, 3 * sizeof(float), "camera"},
					{ranges, rc * sizeof(mbik_lod_range), "ranges"}});
}

// A culling call over no skeletons on the device (the mesh's is current): its n counts become 0 in stream order.
int zero_counts(int32_t *counts, int n, const char *name, hipStream_t st) {
	if (counts && hipMemsetAsync(counts, 0, (size_t)n * sizeof(int32_t), st) != hipSuccess)
		return fail(MBIK_EHIP, std::string("hipMemsetAsync failed for ") + name);
	return MBIK_OK;
}

} // namespace

extern "C" {

int32_t mbik_mesh_bone_boxes(const mbik_mesh *m, float *boxes, uint8_t *used) {
	if (int rc = check_given(m, "mesh")) return rc;
	if (m->B > 0 && (!boxes || !used)) return fail(MBIK_EINVAL, "null boxes or used");
	if (m->B > 0) {
		memcpy(boxes, m->bone_boxes.data(), m->bone_boxes.size() * sizeof(float));
		memcpy(used, m->bone_used.data(), m->bone_used.size());
	}
	return MBIK_OK;
}

int32_t mbik_bone_boxes_cpu(int32_t bone_count, int32_t vertex_count, int32_t influences, const float *positions,
		const int32_t *bone_indices, const float *weights, float *boxes, uint8_t *used) {
	if (int rc = check_mesh(bone_count, vertex_count, influences, positions, bone_indices, weights)) return rc;
	if (bone_count > 0 && (!boxes || !used)) return fail(MBIK_EINVAL, "null boxes or used");
	mbik::bone_boxes_build(bone_count, vertex_count, influences, positions, bone_indices, weights, boxes, used);
	return MBIK_OK;
}

int32_t mbik_skin_bounds(mbik_mesh *m, int32_t count, const float *skin, float *boxes, void *hip_stream) {
	if (int rc = check_given(m, "mesh")) return rc;
	if (int rc = check_bounds_call(m->B, count, skin, boxes)) return settled(rc);
	return launched(m->device, "bounds", [&] {
		return mbik::launch_skin_bounds(reinterpret_cast<hipStream_t>(hip_stream), count, m->B, m->used_bones,
				bounds_skeletons_per_block(m->B, count), m->bone_table.as<unsigned char>(), skin, boxes);
	});
}

int32_t mbik_skin_bounds_cpu(int32_t bone_count, const float *bone_boxes, const uint8_t *used, int32_t count, const float *skin,
		float *boxes) {
	if (bone_count < 0) return fail(MBIK_EINVAL, "negative bone count");
	if (bone_count > 0 && (!bone_boxes || !used)) return fail(MBIK_EINVAL, "null bone_boxes or used");
	if (int rc = check_bounds_call(bone_count, count, skin, boxes)) return settled(rc);
	mbik::skin_bounds_host(bone_count, bone_boxes, used, count, skin, boxes);
	return MBIK_OK;
}

// (mbik_cull_boxes and mbik_cull_lod keep their own guard: the scratch and the empty call's memset need the mesh's device
// before the launch does, and launched() would take a second one)
int32_t mbik_cull_boxes(mbik_mesh *m, int32_t count, const float *boxes, const float *skeleton_global, float margin,
		int32_t plane_count, const float *planes, uint8_t *visible, int32_t *indices, int32_t *visible_count, void *hip_stream) {
	if (int rc = check_given(m, "mesh")) return rc;
	if (int rc = check_cull_call(count, boxes, skeleton_global, plane_count, planes, visible, indices, visible_count)) return rc;
	DeviceGuard guard(m->device);
	hipStream_t st = reinterpret_cast<hipStream_t>(hip_stream);
	if (count == 0) return zero_counts(visible_count, 1, "visible_count", st);
	if (indices || visible_count)
		if (int rc = m->cull_totals.reserve((size_t)mbik::cull_blocks(count) * sizeof(int32_t), "hipMalloc failed for the cull scratch")) return rc;
	return launch_result(mbik::launch_cull(st, count, boxes, skeleton_global, margin, plane_count, planes, visible, indices, visible_count,
								 m->cull_totals.as<int32_t>()),
			"cull");
}

int32_t mbik_cull_boxes_cpu(int32_t count, const float *boxes, const float *skeleton_global, float margin, int32_t plane_count,
		const float *planes, uint8_t *visible, int32_t *indices, int32_t *visible_count) {
	if (int rc = check_cull_call(count, boxes, skeleton_global, plane_count, planes, visible, indices, visible_count)) return rc;
	mbik::cull_boxes_host(count, boxes, skeleton_global, margin, plane_count, planes, visible, indices, visible_count);
	return MBIK_OK;
}

int32_t mbik_cull_lod(mbik_mesh *m, int32_t count, const float *boxes, const float *skeleton_global, float margin, int32_t plane_count,
		const float *planes, const float *camera, int32_t range_count, const mbik_lod_range *ranges, uint32_t flags, uint8_t *state,
		uint8_t *level, int32_t *indices, int32_t *list_counts, void *hip_stream) {
	// (the call's checks in front of the mesh's, unlike every other entry: kept as it has been)
	if (int rc = check_lod_call(count, boxes, skeleton_global, plane_count, planes, camera, range_count, ranges, flags, state, level, indices,
				list_counts))
		return rc;
	if (int rc = check_given(m, "mesh")) return rc;
	DeviceGuard guard(m->device);
	hipStream_t st = reinterpret_cast<hipStream_t>(hip_stream);
	if (count == 0) return zero_counts(list_counts, range_count, "list_counts", st);
	if (int rc = m->cull_totals.reserve((size_t)range_count * mbik::cull_blocks(count) * sizeof(int32_t), "hipMalloc failed for the cull scratch"))
		return rc;
	if (int rc = m->lod_member.reserve((size_t)count, "hipMalloc failed for the LOD scratch")) return rc;
	return launch_result(mbik::launch_cull_lod(st, count, boxes, skeleton_global, margin, plane_count, planes, camera, range_count,
								 reinterpret_cast<const mbik::LodRange *>(ranges), flags, state, level, indices, list_counts,
								 m->cull_totals.as<int32_t>(), m->lod_member.as<uint8_t>()),
			"cull_lod");
}

int32_t mbik_cull_lod_cpu(int32_t count, const float *boxes, const float *skeleton_global, float margin, int32_t plane_count,
		const float *planes, const float *camera, int32_t range_count, const mbik_lod_range *ranges, uint32_t flags, uint8_t *state,
		uint8_t *level, int32_t *indices, int32_t *list_counts) {
	if (int rc = check_lod_call(count, boxes, skeleton_global, plane_count, planes, camera, range_count, ranges, flags, state, level, indices,
				list_counts))
		return rc;
	if (count == 0) {
		if (list_counts)
			for (int r = 0; r < range_count; r++) list_counts[r] = 0;
		return MBIK_OK;
	}
	mbik::cull_lod_host(count, boxes, skeleton_global, margin, plane_count, planes, camera, range_count,
			reinterpret_cast<const mbik::LodRange *>(ranges), flags, state, level, indices, list_counts);
	return MBIK_OK;
}

} // extern "C"
