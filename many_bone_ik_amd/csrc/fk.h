// Forward kinematics of solved poses, shared by the device kernel (k_fk.hip) and the host entry
// mbik_pose_globals_cpu (host_fk.cpp): Skeleton3D::get_bone_global_pose for every bone of a
// skeleton (the reference calls it at ik_bone_3d.cpp:71), the skin transform global *
// bind_inverse, and each pin's distance to its target.  One code path for both sides, built on
// gd_math.h's pose_to_xform and Transform3D product in Godot's operation order, so the device
// and the host produce the same bits (-ffp-contract=off).
//
// Parents may come in any order: fk_build_schedule sorts the bones by depth, and a bone's parent
// is then always finished one level earlier -- the kernel's level-synchronous loop and the host
// walk both follow that order.
#pragma once

#include <cstdint>

#include "gd_math.h"

namespace mbik {

using namespace gd;

// LDS of one kernel block: the block's poses as they are in memory ([S][B][10]) and its
// globals, [S][fk_gstride(B)].  The globals' per-skeleton stride is odd: the lanes of a level
// are consecutive skeletons at one bone, so their dword accesses at stride * s + const fall on
// 32 different banks (an unpadded C2 skeleton, 32 bones x 12 floats = 384 dwords, would put
// them all on one).
GDI int fk_gstride(int B) { return (B * 12) | 1; }
GDI int64_t fk_lds_floats(int B, int S) { return (int64_t)S * ((int64_t)B * 10 + fk_gstride(B)); }
// The largest rig whose single skeleton fits the LDS budget (MBIK_FK_MAX_BONES in mbik.h).
constexpr int kFkMaxBones = 1861;
constexpr int kFkMaxLdsBytes = 160 * 1024;
static_assert((kFkMaxBones * 22 + 1) * 4 <= kFkMaxLdsBytes && ((kFkMaxBones + 1) * 22 + 1) * 4 > kFkMaxLdsBytes,
		"kFkMaxBones is the largest B with fk_lds_floats(B, 1) * 4 <= 160 KiB");

// Depth-ordered schedule of a rig: order[B] lists the bones level by level (a level = the bones
// of one depth, ascending bone index), level_off[levels + 1] the levels' offsets into it (level
// 0 = the parentless bones); depth[B] is scratch.  level_off needs room for B + 1 entries.
// Returns the number of levels (0 for an empty rig), -1 for a parent index outside [-1, B) and
// -2 for a parent cycle.
GDI int fk_build_schedule(int B, const int32_t *parents, int32_t *depth, int32_t *order, int32_t *level_off) {
	for (int b = 0; b < B; b++) {
		if (parents[b] < -1 || parents[b] >= B) return -1;
		depth[b] = -1;
	}
	int levels = 0;
	for (int b = 0; b < B; b++) {
		// walk up to the first ancestor of known depth (or a root), then number the path downwards
		int k = 0, a = b;
		while (depth[a] < 0 && parents[a] >= 0) {
			a = parents[a];
			if (++k > B) return -2;
		}
		int d = (depth[a] < 0 ? 0 : depth[a]) + k;
		for (a = b; depth[a] < 0; a = parents[a]) {
			depth[a] = d--;
			if (parents[a] < 0) break;
		}
		if (depth[b] + 1 > levels) levels = depth[b] + 1;
	}
	for (int l = 0; l <= levels; l++) level_off[l] = 0;
	for (int b = 0; b < B; b++) level_off[depth[b] + 1]++;
	for (int l = 0; l < levels; l++) level_off[l + 1] += level_off[l];
	for (int b = 0; b < B; b++) order[level_off[depth[b]]++] = b; // (level_off[l] is now level l's end)
	for (int l = levels; l > 0; l--) level_off[l] = level_off[l - 1];
	level_off[0] = 0;
	return levels;
}

// Transform3D <-> 12 floats: basis rows, then origin (the layout of `targets`).
GDI X3 fk_load(const float *p) { return X3{bset(p[0], p[1], p[2], p[3], p[4], p[5], p[6], p[7], p[8]), v3(p[9], p[10], p[11])}; }
GDI void fk_store(float *p, const X3 &t) {
	p[0] = t.b.r[0].x, p[1] = t.b.r[0].y, p[2] = t.b.r[0].z;
	p[3] = t.b.r[1].x, p[4] = t.b.r[1].y, p[5] = t.b.r[1].z;
	p[6] = t.b.r[2].x, p[7] = t.b.r[2].y, p[8] = t.b.r[2].z;
	p[9] = t.o.x, p[10] = t.o.y, p[11] = t.o.z;
}

// The per-bone steps.  A bone's slot g (12 floats) first holds its local pose, then its global.
// local(b) = pose_to_xform(pose[b])
GDI void fk_local(const float *pose10, float *g) { fk_store(g, pose_to_xform(pose10)); }
// global(b) = global(parent) * local(b); a parentless bone's global is its local, already in place
GDI void fk_compose(const float *g_parent, float *g) { fk_store(g, fk_load(g_parent) * fk_load(g)); }
// skin(b) = global(b) * X(inv_bind[b])
GDI void fk_skin(const float *g, const float *inv_bind12, float *out) { fk_store(out, fk_load(g) * fk_load(inv_bind12)); }
// |global(pin bone).origin - target.origin|
GDI float fk_pin_distance(const float *g, const float *target12) {
	return length(v3(g[9], g[10], g[11]) - v3(target12[9], target12[10], target12[11]));
}

// One skeleton on the host: G is [B][12] scratch (it may be `globals` itself when inv_bind is
// null).  globals / dist may be null; dist needs targets.
inline void fk_skeleton(int B, const int32_t *parents, const int32_t *order, int P, const int32_t *pin_bone, const float *pose,
		const float *inv_bind, const float *targets, float *G, float *globals, float *dist) {
	for (int b = 0; b < B; b++) fk_local(pose + (int64_t)b * 10, G + (int64_t)b * 12);
	for (int i = 0; i < B; i++) {
		const int b = order[i];
		if (parents[b] >= 0) fk_compose(G + (int64_t)parents[b] * 12, G + (int64_t)b * 12);
	}
	if (dist)
		for (int e = 0; e < P; e++) dist[e] = fk_pin_distance(G + (int64_t)pin_bone[e] * 12, targets + (int64_t)e * 12);
	if (!globals) return;
	for (int b = 0; b < B; b++) {
		if (inv_bind) fk_skin(G + (int64_t)b * 12, inv_bind + (int64_t)b * 12, globals + (int64_t)b * 12);
		else if (globals != G) fk_store(globals + (int64_t)b * 12, fk_load(G + (int64_t)b * 12));
	}
}

} // namespace mbik
