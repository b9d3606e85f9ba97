// Distance LOD lists (include/mbik.h; lod.h): mbik_cull_lod, which launches
// k_cull_lod.hip's kernels on the mesh's device, and mbik_cull_lod_cpu, which runs the same code on
// the host.  Both take their arguments through check_lod_call.
#include "host.h"

#include <cmath>
#include <cstddef>

#include "lod.h"

using namespace mbik_host;

static_assert(sizeof(mbik_lod_range) == sizeof(mbik::LodRange) && offsetof(mbik_lod_range, end) == offsetof(mbik::LodRange, end) &&
				offsetof(mbik_lod_range, begin_margin) == offsetof(mbik::LodRange, begin_margin) &&
				offsetof(mbik_lod_range, end_margin) == offsetof(mbik::LodRange, end_margin),
		"mbik_lod_range is lod.h's LodRange");
static_assert(MBIK_LOD_MAX_RANGES == mbik::kLodMaxRanges && MBIK_LOD_EXCLUSIVE == mbik::kLodExclusive && MBIK_LOD_NONE == mbik::kLodNone,
		"mbik.h's LOD constants are lod.h's");

namespace {

int check_lod_call(int32_t count, const float *boxes, const float *skeleton_global, int32_t plane_count, const float *planes,
		const float *camera, int32_t range_count, const mbik_lod_range *ranges, uint32_t flags, const uint8_t *state, const uint8_t *level,
		const int32_t *indices, const int32_t *list_counts) {
	if (count < 0) return fail(MBIK_EINVAL, "negative count");
	if (plane_count < 0 || plane_count > mbik::kCullMaxPlanes) return fail(MBIK_EINVAL, "plane_count outside [0, MBIK_CULL_MAX_PLANES]");
	if (plane_count > 0 && !planes) return fail(MBIK_EINVAL, "null planes");
	if (range_count < 1 || range_count > mbik::kLodMaxRanges) return fail(MBIK_EINVAL, "range_count outside [1, MBIK_LOD_MAX_RANGES]");
	if (!ranges) return fail(MBIK_EINVAL, "null ranges");
	if (!camera) return fail(MBIK_EINVAL, "null camera");
	if (!std::isfinite(camera[0]) || !std::isfinite(camera[1]) || !std::isfinite(camera[2])) return fail(MBIK_EINVAL, "camera is not finite");
	for (int r = 0; r < range_count; r++) {
		const float f[4] = {ranges[r].begin, ranges[r].end, ranges[r].begin_margin, ranges[r].end_margin};
		for (float x : f)
			if (!std::isfinite(x) || x < 0) return fail(MBIK_EINVAL, "range " + std::to_string(r) + " has a negative or non-finite field");
		if (ranges[r].end > 0 && ranges[r].begin > ranges[r].end) return fail(MBIK_EINVAL, "range " + std::to_string(r) + " begins behind its end");
	}
	if (flags & ~(uint32_t)MBIK_LOD_EXCLUSIVE) return fail(MBIK_EINVAL, "unknown flag bits");
	if (count > 0 && !boxes) return fail(MBIK_EINVAL, "null boxes");
	if (count > 0 && !state) return fail(MBIK_EINVAL, "null state");
	if (count > 0 && !indices) return fail(MBIK_EINVAL, "null indices");
	if (count > 0 && !list_counts) return fail(MBIK_EINVAL, "null list_counts");
	struct Range {
		const void *p;
		size_t n;
		const char *name;
	};
	const size_t c = (size_t)count, rc = (size_t)range_count;
	const Range in[5] = {{boxes, c * 6 * sizeof(float), "boxes"}, {skeleton_global, c * 12 * sizeof(float), "skeleton_global"},
			{planes, (size_t)plane_count * 4 * sizeof(float), "planes"}, {camera, 3 * sizeof(float), "camera"},
			{ranges, rc * sizeof(mbik_lod_range), "ranges"}};
	const Range out[4] = {{state, c, "state"}, {level, c, "level"}, {indices, rc * c * sizeof(int32_t), "indices"},
			{list_counts, rc * sizeof(int32_t), "list_counts"}};
	for (int o = 0; o < 4; o++) {
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

int32_t mbik_cull_lod(mbik_mesh *m, int32_t count, const float *boxes, const float *skeleton_global, float margin, int32_t plane_count,
		const float *planes, const float *camera, int32_t range_count, const mbik_lod_range *ranges, uint32_t flags, uint8_t *state,
		uint8_t *level, int32_t *indices, int32_t *list_counts, void *hip_stream) {
	// (the shared checks first: they read host memory only, so both entries refuse a call in the same words)
	if (int rc = check_lod_call(count, boxes, skeleton_global, plane_count, planes, camera, range_count, ranges, flags, state, level, indices,
				list_counts))
		return rc;
	if (!m) return fail(MBIK_EINVAL, "null mesh");
	DeviceGuard guard(m->device);
	hipStream_t st = reinterpret_cast<hipStream_t>(hip_stream);
	if (count == 0) {
		if (list_counts && hipMemsetAsync(list_counts, 0, (size_t)range_count * sizeof(int32_t), st) != hipSuccess)
			return fail(MBIK_EHIP, "hipMemsetAsync failed for list_counts");
		return MBIK_OK;
	}
	if (int rc = m->cull_totals.reserve((size_t)range_count * mbik::cull_blocks(count) * sizeof(int32_t), "hipMalloc failed for the cull scratch"))
		return rc;
	if (int rc = m->lod_member.reserve((size_t)count, "hipMalloc failed for the LOD scratch")) return rc;
	hipError_t e = mbik::launch_cull_lod(st, count, boxes, skeleton_global, margin, plane_count, planes, camera, range_count,
			reinterpret_cast<const mbik::LodRange *>(ranges), flags, state, level, indices, list_counts, m->cull_totals.as<int32_t>(),
			m->lod_member.as<uint8_t>());
	if (e != hipSuccess) return fail(MBIK_EHIP, std::string("cull_lod launch failed: ") + hipGetErrorString(e));
	return MBIK_OK;
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
