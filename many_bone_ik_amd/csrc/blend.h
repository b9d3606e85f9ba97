// Modifier influence, shared by the device kernel (k_blend.hip) and the host entry
// mbik_pose_blend_cpu (host_blend.cpp): what Skeleton3D::_process_modifiers does around a
// SkeletonModifier3D's _process_modification when the modifier's `influence` is below 1 -- per
// bone, old_pose.interpolate_with(new_pose, influence) written back with set_bone_pose.  Godot
// 4.3's sequence (Transform3D::interpolate_with, Basis::get_scale / get_rotation_quaternion,
// Quaternion::slerp, Vector3::lerp, Basis::set_quaternion_scale, Skeleton3D::set_bone_pose) in
// gd_math.h's operation order, float32 and unfused; one code path for both sides, made of
// IEEE-exact operations only, so the device and the host produce the same bits.  DESIGN.md §15.
#pragma once

#include <cstdint>
#include <cstring>

#include "gd_math.h"

namespace mbik {

using namespace gd;

// Quaternion::slerp at a general weight in [0, 1) (oracle/godot_math.h q_slerp restates it).
// The coefficient of `from` is a double sine over the float sinom: gd_math.h's sin_taylor on
// both sides (argument in [0, pi/2] once the weight is in [0, 1]), a double quotient, one
// rounding to float.  omega is an acosf of a cosine in [0, 1), so every sine argument is finite.
GDI Q blend_slerp(Q from, Q to, float w, int lv) {
	float cosom = dot(from, to);
	if (cosom < 0.0f) {
		cosom = -cosom;
		to = q4(-to.x, -to.y, -to.z, -to.w);
	}
	float scale0, scale1;
	if ((1.0f - cosom) > (float)CMP_EPSILON) {
		const float omega = acos_f(cosom);
		const float sinom = sin_f(omega, lv);
		scale0 = (float)(sin_taylor((1.0 - (double)w) * (double)omega) / (double)sinom);
		scale1 = gd_div(sin_f(w * omega, lv), sinom);
	} else {
		scale0 = 1.0f - w;
		scale1 = w;
	}
	return q4(scale0 * from.x + scale1 * to.x, scale0 * from.y + scale1 * to.y, scale0 * from.z + scale1 * to.z,
			scale0 * from.w + scale1 * to.w);
}

// A NaN result is stored as the one quiet NaN 0x7fc00000: x86 and gfx950 give generated and
// propagated NaNs different signs and payloads, and the output is specified bit for bit.
// Nothing else about non-finite values is special.
GDI float blend_canon(float x) {
	union {
		uint32_t u;
		float f;
	} c{0x7fc00000u};
	return x != x ? c.f : x;
}

// True when Godot blends this bone: the weight is below 1 (a NaN weight is not) and the two
// poses' transforms differ in at least one of their 12 floats (float ==: +0 equals -0, NaN
// differs from itself).  Otherwise the modifier's pose stands, bit for bit.
GDI bool blend_needed(const X3 &A, const X3 &M, float w) { return w < 1.0f && !eq(A, M); }

// The blend of one bone whose blend_needed() holds: A / M are pose_to_xform of the input and of
// the modifier's pose.  A negative weight counts as 0 (the property's range is 0..1; Godot would
// extrapolate, and the double sine's argument would leave its range); -0 stays -0.
GDI void blend_xforms(const X3 &A, const X3 &M, float w, int lv, float *out10) {
	if (w < 0.0f) w = 0.0f;
	const V3 sa = get_scale(A.b), sm = get_scale(M.b);
	const Q qa = get_rotation_quaternion(A.b), qm = get_rotation_quaternion(M.b);
	const Q q = normalized(blend_slerp(qa, qm, w, lv));
	const V3 sc = sa + (sm - sa) * w;
	const V3 o = A.o + (M.o - A.o) * w;
	// Basis::set_quaternion_scale, then Skeleton3D::set_bone_pose's decomposition
	const B3 T = from_quat(q) * bset(sc.x, 0, 0, 0, sc.y, 0, 0, 0, sc.z);
	const Q r = get_rotation_quaternion(T);
	const V3 s = get_scale(T);
	out10[0] = blend_canon(r.x), out10[1] = blend_canon(r.y), out10[2] = blend_canon(r.z), out10[3] = blend_canon(r.w);
	out10[4] = blend_canon(o.x), out10[5] = blend_canon(o.y), out10[6] = blend_canon(o.z);
	out10[7] = blend_canon(s.x), out10[8] = blend_canon(s.y), out10[9] = blend_canon(s.z);
}

// One bone on the host: a / m / out are [10] (quaternion xyzw, position, scale); out may be a or m.
inline void blend_bone(const float *a, const float *m, float w, int lv, float *out) {
	const X3 A = pose_to_xform(a), M = pose_to_xform(m);
	if (blend_needed(A, M, w)) {
		blend_xforms(A, M, w, lv, out);
	} else if (out != m) {
		std::memcpy(out, m, 10 * sizeof(float));
	}
}

} // namespace mbik
