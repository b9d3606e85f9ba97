// The back half of a frame (include/mbik.h): skeleton-space bone transforms, skin transforms and
// pin-to-target distances from solved poses.  mbik_pose_globals launches k_fk.hip's kernel on the
// plan's device; mbik_pose_globals_cpu runs the same per-bone code (fk.h) on the host.
// Replaces Skeleton3D::get_bone_global_pose as the reference calls it (ik_bone_3d.cpp:71);
// DESIGN.md §13.
#include "host.h"

#include "fk.h"

using namespace mbik_host;

namespace {

// LDS a block aims for: eight 256-thread blocks (all 32 wave slots) share a CU's 160 KiB.
constexpr int64_t kFkBlockLdsTarget = 20 * 1024;
constexpr int kFkMaxSkeletonsPerBlock = 64;

// The checks both entry points share; P = the rig's pin count.  Returns 0, or the error code.
int check_args(int32_t count, int B, int P, const float *pose, const float *globals, const float *targets,
		const float *pin_distance) {
	if (!globals && !pin_distance) return fail(MBIK_EINVAL, "globals and pin_distance are both null");
	if (pin_distance && P > 0 && !targets) return fail(MBIK_EINVAL, "pin_distance needs targets");
	if (!pose) return fail(MBIK_EINVAL, "null pose");
	if (globals && overlap(pose, (size_t)count * B * 10 * sizeof(float), globals, (size_t)count * B * 12 * sizeof(float)))
		return fail(MBIK_EINVAL, "pose overlaps globals");
	return MBIK_OK;
}

// Builds the plan's schedule and uploads it (kernels.h launch_fk's layout); once per plan.
int ensure_fk_schedule(mbik_plan *p) {
	if (p->fk_sched) return MBIK_OK;
	const int B = p->host.B, P = p->host.P;
	if ((int)p->src_parents.size() != B || (int)p->src_pins.size() != P) return fail(MBIK_EINVAL, "plan without its rig description");
	std::vector<int32_t> depth(B), order(B), level_off(B + 1);
	const int levels = mbik::fk_build_schedule(B, p->src_parents.data(), depth.data(), order.data(), level_off.data());
	if (levels < 0) return fail(MBIK_EINVAL, levels == -1 ? "parent index out of range" : "parent cycle");
	std::vector<int32_t> blob(level_off.begin(), level_off.begin() + levels + 1);
	if (blob.size() & 1) blob.push_back(0);
	for (int i = 0; i < B; i++) {
		blob.push_back(order[i]);
		blob.push_back(p->src_parents[order[i]]);
	}
	for (int e = 0; e < P; e++) {
		if (p->src_pins[e].bone < 0 || p->src_pins[e].bone >= B) return fail(MBIK_EINVAL, "pin bone out of range");
		blob.push_back(p->src_pins[e].bone);
	}
	// published only once the copy succeeded: a failed call leaves nothing behind
	DevBuf d;
	if (int rc = d.upload(blob.data(), blob.size() * sizeof(int32_t), "the bone schedule")) return rc;
	p->device_bytes += (int64_t)d.bytes();
	p->fk_levels = levels;
	p->fk_sched = std::move(d);
	return MBIK_OK;
}

} // namespace

extern "C" {

int32_t mbik_pose_globals(mbik_plan *p, int32_t count, const float *pose, const float *inv_bind, float *globals,
		const float *targets, float *pin_distance, void *hip_stream) {
	if (!p) return fail(MBIK_EINVAL, "null plan");
	if (count < 0) return fail(MBIK_EINVAL, "negative count");
	const int B = p->host.B, P = p->host.P;
	if (count == 0 || B == 0) return MBIK_OK;
	if (int rc = check_args(count, B, P, pose, globals, targets, pin_distance)) return rc;
	if (P == 0) pin_distance = nullptr;
	if (!globals && !pin_distance) return MBIK_OK; // a pinless plan asked for distances only
	if (B > mbik::kFkMaxBones)
		return fail(MBIK_EUNSUPPORTED, "rig has " + std::to_string(B) + " bones; mbik_pose_globals supports at most " +
				std::to_string(mbik::kFkMaxBones) + " (MBIK_FK_MAX_BONES: one skeleton's poses and globals must fit 160 KiB of LDS)");
	DeviceGuard guard(p->device);
	if (int rc = ensure_fk_schedule(p)) return rc;
	const int64_t per = mbik::fk_lds_floats(B, 1) * (int64_t)sizeof(float);
	const int S = (int)std::max<int64_t>(1, std::min<int64_t>({kFkBlockLdsTarget / per, kFkMaxSkeletonsPerBlock, count}));
	// (the guard is this entry's own: the schedule's upload needs it too, and launched() would take a second one)
	return launch_result(mbik::launch_fk(reinterpret_cast<hipStream_t>(hip_stream), count, B, P, S, p->fk_levels, p->fk_sched.as<int>(), pose,
								 inv_bind, globals, targets, pin_distance),
			"pose globals");
}

int32_t mbik_pose_globals_cpu(const mbik_skeleton_desc *desc, int32_t count, const float *pose, const float *inv_bind,
		float *globals, const float *targets, float *pin_distance) {
	if (!desc) return fail(MBIK_EINVAL, "null description");
	if (count < 0 || desc->bone_count < 0 || desc->pin_count < 0) return fail(MBIK_EINVAL, "negative count");
	const int B = desc->bone_count, P = desc->pin_count;
	if ((B > 0 && !desc->parents) || (P > 0 && !desc->pins)) return fail(MBIK_EINVAL, "null rig arrays");
	std::vector<int32_t> depth(B), order(B), level_off(B + 1), pin_bone(P);
	const int levels = mbik::fk_build_schedule(B, desc->parents, depth.data(), order.data(), level_off.data());
	if (levels < 0) return fail(MBIK_EINVAL, levels == -1 ? "parent index out of range" : "parent cycle");
	for (int e = 0; e < P; e++) {
		if (desc->pins[e].bone < 0 || desc->pins[e].bone >= B) return fail(MBIK_EINVAL, "pin bone out of range");
		pin_bone[e] = desc->pins[e].bone;
	}
	if (count == 0 || B == 0) return MBIK_OK;
	if (int rc = check_args(count, B, P, pose, globals, targets, pin_distance)) return rc;
	if (P == 0) pin_distance = nullptr;
	std::vector<float> scratch;
	if (inv_bind || !globals) scratch.resize((size_t)B * 12);
	for (int64_t s = 0; s < count; s++) {
		float *out = globals ? globals + s * B * 12 : nullptr;
		mbik::fk_skeleton(B, desc->parents, order.data(), P, pin_bone.data(), pose + s * B * 10, inv_bind,
				targets ? targets + s * P * 12 : nullptr, scratch.empty() ? out : scratch.data(), out,
				pin_distance ? pin_distance + s * P : nullptr);
	}
	return MBIK_OK;
}

} // extern "C"
