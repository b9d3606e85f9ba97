// Linear blend skinning of a mesh from skin transforms (mbik_skin_vertices),
// shared by the device kernel (k_skin.hip) and the host entry mbik_skin_vertices_cpu
// (host_skin.cpp).  The semantics are those of Godot's skeleton compute shader -- blend the bone
// matrices, then transform -- on ArrayMesh surface arrays (ARRAY_VERTEX, ARRAY_NORMAL,
// ARRAY_BONES, ARRAY_WEIGHTS; 4 or 8 influences a vertex).  With X_k = skin[bones[v][k]] (12
// floats: basis rows, then origin, as mbik_pose_globals writes them) and w_k = weights[v][k]:
//
//     M    = X_0 * w_0                     every element (V3 * float on the three rows and the origin)
//     M    = M + X_k * w_k   k = 1..K-1    in influence order; every influence, weight 0 included
//     pos' = xform(M, pos)                 ((r.x*v.x + r.y*v.y) + r.z*v.z) + o per row
//     nrm' = xform(M.b, nrm)               same matrix, no origin, not renormalised
//     tan' = xform(M.b, tan.xyz), tan.w    the normal's transform on ARRAY_TANGENT's xyz; the binormal
//                                          sign w is copied, its bits untouched (mbik_skin_vertices_call,
//                                          DESIGN.md §22)
//
// One code path for both sides, built only from gd_math.h's primitives and compiled with
// -ffp-contract=off, so the device and the host produce the same bits.  Weights are used as
// given (no normalisation, no sorting), and non-finite values propagate: a NaN in one bone's
// matrix reaches exactly the vertices that list that bone, weight 0 included (0 * NaN = NaN).
// A renderer fixes no float order, so this header's host function is the specification.
//
// The header also holds the mesh validation and the device mesh layout with its packing, which
// are host code without a HIP call: tools/san/skin_san.cpp runs them under ASan + UBSan.
#pragma once

#include <cstdint>
#include <cstring>

#include "gd_math.h"

namespace mbik {

using namespace gd;

// One skeleton's matrices, 48 bytes a bone, are staged in LDS: the largest rig that fits the
// 160 KiB budget with nothing else there (MBIK_SKIN_MAX_BONES in mbik.h).
constexpr int kSkinMaxBones = 3413;
constexpr int kSkinMaxLdsBytes = 160 * 1024;
static_assert(kSkinMaxBones * 48 <= kSkinMaxLdsBytes && (kSkinMaxBones + 1) * 48 > kSkinMaxLdsBytes,
		"kSkinMaxBones is the largest B with B * 48 <= 160 KiB");
static_assert(kSkinMaxBones <= 65536, "the device mesh keeps bone indices in 16 bits");

// ---------------- arithmetic ----------------
GDI X3 skin_load(const float *p) { return X3{bset(p[0], p[1], p[2], p[3], p[4], p[5], p[6], p[7], p[8]), v3(p[9], p[10], p[11])}; }
// X * w, every element
GDI X3 skin_scaled(const X3 &x, float w) {
	X3 r;
	r.b.r[0] = x.b.r[0] * w, r.b.r[1] = x.b.r[1] * w, r.b.r[2] = x.b.r[2] * w;
	r.o = x.o * w;
	return r;
}
// M + X * w
GDI X3 skin_accumulate(const X3 &m, const X3 &x, float w) {
	const X3 t = skin_scaled(x, w);
	X3 r;
	r.b.r[0] = m.b.r[0] + t.b.r[0], r.b.r[1] = m.b.r[1] + t.b.r[1], r.b.r[2] = m.b.r[2] + t.b.r[2];
	r.o = m.o + t.o;
	return r;
}
GDI V3 skin_position(const X3 &m, V3 pos) { return xform(m, pos); }
GDI V3 skin_normal(const X3 &m, V3 nrm) { return xform(m.b, nrm); }

// What a call writes for a vertex: the attribute tier of the kernels and of the host path.
enum SkinTier { SKIN_POSITIONS = 0, SKIN_NORMALS = 1, SKIN_TANGENTS = 2 };
constexpr int skin_tier(bool normals, bool tangents) { return tangents ? SKIN_TANGENTS : (normals ? SKIN_NORMALS : SKIN_POSITIONS); }

// ---------------- validation (the checks mbik_mesh_create and mbik_skin_vertices_cpu share) ----------------
enum SkinCheck { SKIN_OK = 0, SKIN_BAD_INFLUENCES, SKIN_NEGATIVE, SKIN_NULL, SKIN_BAD_INDEX, SKIN_TANGENTS_WITHOUT_NORMALS };
// bad_vertex / bad_slot: where the first index outside [0, B) is (SKIN_BAD_INDEX)
inline SkinCheck skin_check_mesh(int32_t B, int32_t V, int32_t K, const float *positions, const int32_t *bone_indices,
		const float *weights, int64_t *bad_vertex = nullptr, int *bad_slot = nullptr) {
	if (K != 4 && K != 8) return SKIN_BAD_INFLUENCES;
	if (B < 0 || V < 0) return SKIN_NEGATIVE;
	if (V > 0 && (!positions || !bone_indices || !weights)) return SKIN_NULL;
	for (int64_t v = 0; v < V; v++)
		for (int k = 0; k < K; k++) {
			const int32_t b = bone_indices[v * K + k];
			if (b < 0 || b >= B) {
				if (bad_vertex) *bad_vertex = v;
				if (bad_slot) *bad_slot = k;
				return SKIN_BAD_INDEX;
			}
		}
	return SKIN_OK;
}
// a mesh's tangents ([V][4]: xyz and the binormal sign) come with its normals
inline SkinCheck skin_check_tangents(const float *normals, const float *tangents) {
	return tangents && !normals ? SKIN_TANGENTS_WITHOUT_NORMALS : SKIN_OK;
}
inline const char *skin_check_text(SkinCheck c) {
	switch (c) {
		case SKIN_BAD_INFLUENCES: return "influences must be 4 or 8";
		case SKIN_NEGATIVE: return "negative bone or vertex count";
		case SKIN_NULL: return "null mesh array";
		case SKIN_BAD_INDEX: return "bone index outside [0, bone_count)";
		case SKIN_TANGENTS_WITHOUT_NORMALS: return "tangents given for a mesh without normals";
		default: return "ok";
	}
}

// ---------------- device mesh layout ----------------
// Planes of per-vertex records, each plane contiguous over the vertices so that consecutive
// lanes load consecutive 8 or 16 bytes:
//   positions  [V] 16 B   x, y, z, 0
//   normals    [V] 16 B   x, y, z, 0                 (meshes with normals)
//   indices    [V] 2 B x K  bone indices, 16 bits each in influence order (8 B for K = 4, 16 B for K = 8)
//   weights    [K / 4][V] 16 B   influences 4q .. 4q + 3 of plane q
// Every plane starts at a multiple of 16 bytes.  Offsets are in bytes from the mesh's base.
// A mesh with tangents keeps them in one more plane behind these and behind morph.h's shape planes
// (tangent_layout there), so that no offset here depends on them.
struct SkinLayout {
	int64_t pos, nrm, idx, wgt, bytes; // nrm = -1 for a mesh without normals
};
inline SkinLayout skin_layout(int32_t V, int32_t K, bool normals) {
	const int64_t n = ((int64_t)V + 1) & ~(int64_t)1; // (K = 4: the 8-byte index plane ends on 16 bytes)
	SkinLayout l;
	int64_t at = 0;
	l.pos = at, at += n * 16;
	l.nrm = normals ? at : -1;
	if (normals) at += n * 16;
	l.idx = at, at += n * 2 * K;
	l.wgt = at, at += (int64_t)(K / 4) * n * 16;
	l.bytes = at;
	return l;
}
// Fills `out` (skin_layout().bytes bytes) from a checked mesh (skin_check_mesh == SKIN_OK, B <= 65536).
inline void skin_pack(int32_t V, int32_t K, const float *positions, const float *normals, const int32_t *bone_indices,
		const float *weights, unsigned char *out) {
	const SkinLayout l = skin_layout(V, K, normals != nullptr);
	if (l.bytes == 0) return; // (a mesh without vertices: `out` may be null)
	memset(out, 0, (size_t)l.bytes);
	const int64_t n = ((int64_t)V + 1) & ~(int64_t)1;
	for (int64_t v = 0; v < V; v++) {
		memcpy(out + l.pos + v * 16, positions + v * 3, 12);
		if (normals) memcpy(out + l.nrm + v * 16, normals + v * 3, 12);
		for (int k = 0; k < K; k++) {
			const uint16_t b = (uint16_t)bone_indices[v * K + k];
			memcpy(out + l.idx + (v * K + k) * 2, &b, 2);
		}
		for (int q = 0; q < K / 4; q++) memcpy(out + l.wgt + (q * n + v) * 16, weights + v * K + 4 * q, 16);
	}
}

// ---------------- host path ----------------
// One vertex of one skeleton: skin = that skeleton's [B][12] matrices, idx / w the vertex's K
// influences; out_n (and nrm) may be null; tan [4] and out_t [4] likewise (given with out_n only).
inline void skin_vertex_host(int K, const float *skin, const int32_t *idx, const float *w, const float *pos, const float *nrm,
		float *out_p, float *out_n, const float *tan = nullptr, float *out_t = nullptr) {
	X3 m = skin_scaled(skin_load(skin + (int64_t)idx[0] * 12), w[0]);
	for (int k = 1; k < K; k++) m = skin_accumulate(m, skin_load(skin + (int64_t)idx[k] * 12), w[k]);
	const V3 p = skin_position(m, v3(pos[0], pos[1], pos[2]));
	out_p[0] = p.x, out_p[1] = p.y, out_p[2] = p.z;
	if (out_n) {
		const V3 q = skin_normal(m, v3(nrm[0], nrm[1], nrm[2]));
		out_n[0] = q.x, out_n[1] = q.y, out_n[2] = q.z;
	}
	if (out_t) {
		const V3 t = skin_normal(m, v3(tan[0], tan[1], tan[2]));
		out_t[0] = t.x, out_t[1] = t.y, out_t[2] = t.z;
		memcpy(out_t + 3, tan + 3, 4); // (the sign's bits: never a float in a register)
	}
}
// count skeletons of a checked mesh: skin [count][B][12], out_positions / out_normals [count][V][3];
// tangents [V][4] and out_tangents [count][V][4], or null
inline void skin_vertices_host(int32_t B, int32_t V, int32_t K, const float *positions, const float *normals,
		const int32_t *bone_indices, const float *weights, int32_t count, const float *skin, float *out_positions,
		float *out_normals, const float *tangents = nullptr, float *out_tangents = nullptr) {
	for (int64_t s = 0; s < count; s++)
		for (int64_t v = 0; v < V; v++)
			skin_vertex_host(K, skin + s * B * 12, bone_indices + v * K, weights + v * K, positions + v * 3,
					out_normals ? normals + v * 3 : nullptr, out_positions + (s * V + v) * 3,
					out_normals ? out_normals + (s * V + v) * 3 : nullptr, out_tangents ? tangents + v * 4 : nullptr,
					out_tangents ? out_tangents + (s * V + v) * 4 : nullptr);
}

} // namespace mbik
