// Skeleton bounds and frustum culling (include/mbik.h, ABI 14; bounds.h): the
// readback of a mesh's bone boxes, mbik_skin_bounds and mbik_cull_boxes, which launch
// k_bounds.hip's kernels on the mesh's device, and the _cpu entries, which run the same code on
// the host.  The boxes themselves are built with the mesh (host_skin.cpp).
#include "host.h"

#include "bounds.h"

using namespace mbik_host;

namespace {

// LDS a bounds block aims for, as the skinning's: eight 256-thread blocks share a CU's 160 KiB.
constexpr int64_t kBoundsBlockLdsTarget = 20 * 1024;
// Skeletons a block takes at most: one lane each in the merge chain, so one wave's worth.
constexpr int kBoundsMaxSkeletonsPerBlock = 64;

int bounds_skeletons_per_block(int32_t B, int32_t count) {
	const int64_t per = std::max<int64_t>(48, (int64_t)B * 48);
	return (int)std::max<int64_t>(1, std::min<int64_t>({kBoundsBlockLdsTarget / per, kBoundsMaxSkeletonsPerBlock, count}));
}

// 0 = go on, 1 = nothing to do
int check_bounds_call(int32_t B, int32_t count, const float *skin, const float *boxes) {
	if (count < 0) return fail(MBIK_EINVAL, "negative count");
	if (count == 0) return 1;
	if (!skin) return fail(MBIK_EINVAL, "null skin");
	if (!boxes) return fail(MBIK_EINVAL, "null boxes");
	if (overlap(skin, (size_t)count * B * 12 * sizeof(float), boxes, (size_t)count * 6 * sizeof(float)))
		return fail(MBIK_EINVAL, "boxes overlaps skin");
	return 0;
}

int check_cull_call(int32_t count, const float *boxes, const float *skeleton_global, int32_t plane_count, const float *planes,
		const uint8_t *visible, const int32_t *indices, const int32_t *visible_count) {
	if (count < 0) return fail(MBIK_EINVAL, "negative count");
	if (plane_count < 0 || plane_count > mbik::kCullMaxPlanes) return fail(MBIK_EINVAL, "plane_count outside [0, MBIK_CULL_MAX_PLANES]");
	if (plane_count > 0 && !planes) return fail(MBIK_EINVAL, "null planes");
	if (!visible && !indices) return fail(MBIK_EINVAL, "both visible and indices are null");
	if (indices && !visible_count) return fail(MBIK_EINVAL, "indices without visible_count");
	if (count > 0 && !boxes) return fail(MBIK_EINVAL, "null boxes");
	struct Range {
		const void *p;
		size_t n;
		const char *name;
	};
	const size_t c = (size_t)count;
	const Range in[2] = {{boxes, c * 6 * sizeof(float), "boxes"}, {skeleton_global, c * 12 * sizeof(float), "skeleton_global"}};
	const Range out[3] = {{visible, c, "visible"}, {indices, c * sizeof(int32_t), "indices"}, {visible_count, sizeof(int32_t), "visible_count"}};
	for (int o = 0; o < 3; o++) {
		if (!out[o].p) continue;
		for (const Range &i : in)
			if (i.p && overlap(out[o].p, out[o].n, i.p, i.n)) return fail(MBIK_EINVAL, std::string(out[o].name) + " overlaps " + i.name);
		for (int q = 0; q < o; q++)
			if (out[q].p && overlap(out[o].p, out[o].n, out[q].p, out[q].n))
				return fail(MBIK_EINVAL, std::string(out[o].name) + " overlaps " + out[q].name);
	}
	return MBIK_OK;
}

} // namespace

extern "C" {

int32_t mbik_mesh_bone_boxes(const mbik_mesh *m, float *boxes, uint8_t *used) {
	if (!m) return fail(MBIK_EINVAL, "null mesh");
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
	if (!m) return fail(MBIK_EINVAL, "null mesh");
	const int rc = check_bounds_call(m->B, count, skin, boxes);
	if (rc) return rc < 0 ? rc : MBIK_OK;
	DeviceGuard guard(m->device);
	hipError_t e = mbik::launch_skin_bounds(reinterpret_cast<hipStream_t>(hip_stream), count, m->B, m->used_bones,
			bounds_skeletons_per_block(m->B, count), m->bone_table.as<unsigned char>(), skin, boxes);
	if (e != hipSuccess) return fail(MBIK_EHIP, std::string("bounds launch failed: ") + hipGetErrorString(e));
	return MBIK_OK;
}

int32_t mbik_skin_bounds_cpu(int32_t bone_count, const float *bone_boxes, const uint8_t *used, int32_t count, const float *skin,
		float *boxes) {
	if (bone_count < 0) return fail(MBIK_EINVAL, "negative bone count");
	if (bone_count > 0 && (!bone_boxes || !used)) return fail(MBIK_EINVAL, "null bone_boxes or used");
	const int rc = check_bounds_call(bone_count, count, skin, boxes);
	if (rc) return rc < 0 ? rc : MBIK_OK;
	mbik::skin_bounds_host(bone_count, bone_boxes, used, count, skin, boxes);
	return MBIK_OK;
}

int32_t mbik_cull_boxes(mbik_mesh *m, int32_t count, const float *boxes, const float *skeleton_global, float margin,
		int32_t plane_count, const float *planes, uint8_t *visible, int32_t *indices, int32_t *visible_count, void *hip_stream) {
	if (!m) return fail(MBIK_EINVAL, "null mesh");
	if (int rc = check_cull_call(count, boxes, skeleton_global, plane_count, planes, visible, indices, visible_count)) return rc;
	DeviceGuard guard(m->device);
	hipStream_t st = reinterpret_cast<hipStream_t>(hip_stream);
	if (count == 0) {
		if (visible_count && hipMemsetAsync(visible_count, 0, sizeof(int32_t), st) != hipSuccess)
			return fail(MBIK_EHIP, "hipMemsetAsync failed for visible_count");
		return MBIK_OK;
	}
	if (indices || visible_count)
		if (int rc = m->cull_totals.reserve((size_t)mbik::cull_blocks(count) * sizeof(int32_t), "hipMalloc failed for the cull scratch")) return rc;
	hipError_t e = mbik::launch_cull(st, count, boxes, skeleton_global, margin, plane_count, planes, visible, indices, visible_count,
			m->cull_totals.as<int32_t>());
	if (e != hipSuccess) return fail(MBIK_EHIP, std::string("cull launch failed: ") + hipGetErrorString(e));
	return MBIK_OK;
}

int32_t mbik_cull_boxes_cpu(int32_t count, const float *boxes, const float *skeleton_global, float margin, int32_t plane_count,
		const float *planes, uint8_t *visible, int32_t *indices, int32_t *visible_count) {
	if (int rc = check_cull_call(count, boxes, skeleton_global, plane_count, planes, visible, indices, visible_count)) return rc;
	mbik::cull_boxes_host(count, boxes, skeleton_global, margin, plane_count, planes, visible, indices, visible_count);
	return MBIK_OK;
}

} // extern "C"
