// Modifier influence (include/mbik.h, ABI 11): the blend Skeleton3D::_process_modifiers applies
// around a SkeletonModifier3D when its `influence` is below 1, between the solve and
// mbik_pose_globals.  mbik_pose_blend launches k_blend.hip's kernel on the plan's device;
// mbik_pose_blend_cpu runs the same per-bone code (blend.h) on the host.  DESIGN.md §15.
#include "host.h"

#include "blend.h"

using namespace mbik_host;

namespace {

// The checks both entry points share, for count > 0 and B > 0.  Returns 0, or the error code.
int check_args(int32_t count, int B, const float *pose_in, const float *pose_mod, const float *pose_out) {
	if (!pose_in) return fail(MBIK_EINVAL, "null pose_in");
	if (!pose_mod) return fail(MBIK_EINVAL, "null pose_mod");
	if (!pose_out) return fail(MBIK_EINVAL, "null pose_out");
	const size_t n = (size_t)count * B * 10 * sizeof(float);
	if (pose_out != pose_in && overlap(pose_out, n, pose_in, n)) return fail(MBIK_EINVAL, "pose_out overlaps pose_in without being pose_in");
	if (pose_out != pose_mod && overlap(pose_out, n, pose_mod, n))
		return fail(MBIK_EINVAL, "pose_out overlaps pose_mod without being pose_mod");
	return MBIK_OK;
}

} // namespace

extern "C" {

int32_t mbik_pose_blend(mbik_plan *p, int32_t count, const float *pose_in, const float *pose_mod, float influence,
		const float *influence_per_skeleton, float *pose_out, void *hip_stream) {
	if (!p) return fail(MBIK_EINVAL, "null plan");
	if (count < 0) return fail(MBIK_EINVAL, "negative count");
	const int B = p->host.B;
	if (count == 0 || B == 0) return MBIK_OK;
	if (int rc = check_args(count, B, pose_in, pose_mod, pose_out)) return rc;
	if ((int64_t)count * B > (int64_t)INT32_MAX * 256) return fail(MBIK_EUNSUPPORTED, "more than 2^39 bones in one call");
	return launched(p->device, "pose blend", [&] {
		return mbik::launch_blend(reinterpret_cast<hipStream_t>(hip_stream), (int64_t)count * B, B, p->host.libm_variant, influence,
				influence_per_skeleton, pose_in, pose_mod, pose_out);
	});
}

int32_t mbik_pose_blend_cpu(int32_t bone_count, int32_t libm_variant, int32_t count, const float *pose_in, const float *pose_mod,
		float influence, const float *influence_per_skeleton, float *pose_out) {
	if (count < 0 || bone_count < 0) return fail(MBIK_EINVAL, "negative count");
	if (libm_variant != MBIK_LIBM_VARIANT_FMA && libm_variant != MBIK_LIBM_VARIANT_SSE2) return fail(MBIK_EINVAL, "unknown libm_variant");
	const int B = bone_count;
	if (count == 0 || B == 0) return MBIK_OK;
	if (int rc = check_args(count, B, pose_in, pose_mod, pose_out)) return rc;
	for (int64_t s = 0; s < count; s++) {
		const float w = influence_per_skeleton ? influence_per_skeleton[s] : influence;
		for (int64_t i = s * B; i < (s + 1) * B; i++) mbik::blend_bone(pose_in + i * 10, pose_mod + i * 10, w, libm_variant, pose_out + i * 10);
	}
	return MBIK_OK;
}

} // extern "C"
