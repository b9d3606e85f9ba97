// Blend shapes (morph targets) in front of linear blend skinning (mbik_skin_vertices_shaped,
// DESIGN.md §17), shared by the device kernel (k_skin.hip) and the host entry
// mbik_skin_vertices_shaped_cpu (host_skin.cpp).  The semantics are the first half of Godot 4.3's
// skeleton compute shader, BLEND_SHAPE_MODE_RELATIVE and BLEND_SHAPE_MODE_NORMALIZED, on float32
// arrays.  For vertex v of skeleton s with c_j = shape_weights[s][j], float32, unfused:
//
//     bp = bn = (0,0,0); total = 0
//     for j = 0 .. P-1 ascending, where fabsf(c_j) > 0.0001f (false for NaN: such a weight is skipped):
//         bp = bp + shape_pos[j][v] * c_j;  bn = bn + shape_nrm[j][v] * c_j;  total = total + c_j
//     normalized mode: base_w = 1.0f - total; pos = pos * base_w; nrm = nrm * base_w
//     pos = pos + bp;  nrm = normalized(nrm + bn)        (the zero vector stays zero)
//
// and skin.h's blend and transform then run on pos and nrm.  One code path for both sides
// (morph_vertex), built only from gd_math.h's primitives, so the device and the host produce
// the same bits; the two sides differ in how they fetch a weight and a shape record only.
//
// The header also holds the shape validation and the device layout of the shape planes with its
// packing, host code without a HIP call: tools/san/morph_san.cpp runs them under ASan + UBSan.
// A mesh's tangents take the normal's steps on records of their own (morph_vertex_tier; their
// validation, layout and packing are further down; tools/san/skin_tangent_san.cpp).
#pragma once

#include "skin.h"

namespace mbik {

enum MorphMode { MORPH_RELATIVE = 0, MORPH_NORMALIZED = 1 };

// One skeleton's matrices and shape weights are staged together (MBIK_MAX_LDS_BYTES in mbik.h).
constexpr int64_t morph_lds_bytes(int64_t B, int64_t P) { return B * 48 + P * 4; }
static_assert(morph_lds_bytes(kSkinMaxBones, 4) <= kSkinMaxLdsBytes && morph_lds_bytes(kSkinMaxBones, 5) > kSkinMaxLdsBytes,
		"the largest rig leaves room for four shape weights");

// ---------------- arithmetic ----------------
// the shader's test; false for NaN
GDI bool morph_active(float c) { return fabsf(c) > 0.0001f; }

// pos and nrm come in as the base vertex and leave as the morphed one.  weight(j) is c_j,
// shape_pos(j) / shape_nrm(j) the vertex's record of shape j; a skipped shape's records are not
// fetched.  after_skipped(j, c) is the next shape to look at behind a skipped one: j + 1 on the
// host; the device has turned every skipped weight into a link to the next active shape
// (morph_link_skipped), so that a run of skipped shapes costs one step.  On the device weight(j)
// is the same in every lane of a wave, so the branch is uniform.
//
// TIER is a SkinTier.  With SKIN_TANGENTS the tangent's xyz goes through the normal's steps on its own
// records, shape_tan(j), inside the same loop (mbik_skin_vertices_call):
//     bt = bt + shape_tan[j][v] * c_j;  normalized mode: tan = tan * base_w;  tan = normalized(tan + bt)
// The binormal sign is not this function's business.
template <int TIER, class Weight, class AfterSkipped, class ShapePos, class ShapeNrm, class ShapeTan>
GDI void morph_vertex_tier(int mode, int P, Weight weight, AfterSkipped after_skipped, ShapePos shape_pos, ShapeNrm shape_nrm,
		ShapeTan shape_tan, V3 &pos, V3 &nrm, V3 &tan) {
	constexpr bool NRM = TIER >= SKIN_NORMALS, TAN = TIER >= SKIN_TANGENTS;
	V3 bp = v3(0, 0, 0), bn = v3(0, 0, 0), bt = v3(0, 0, 0);
	float total = 0.0f;
	for (int j = 0; j < P;) {
		const float c = weight(j);
		if (!morph_active(c)) {
			j = after_skipped(j, c);
		} else {
			const V3 dp = shape_pos(j); // (every record fetched before any is used)
			V3 dn = v3(0, 0, 0), dt = v3(0, 0, 0);
			if constexpr (NRM) dn = shape_nrm(j);
			if constexpr (TAN) dt = shape_tan(j);
			bp = bp + dp * c;
			if constexpr (NRM) bn = bn + dn * c;
			if constexpr (TAN) bt = bt + dt * c;
			total = total + c;
			j++;
		}
	}
	if (mode == MORPH_NORMALIZED) {
		const float base_w = 1.0f - total;
		pos = pos * base_w;
		if constexpr (NRM) nrm = nrm * base_w;
		if constexpr (TAN) tan = tan * base_w;
	}
	pos = pos + bp;
	if constexpr (NRM) nrm = normalized(nrm + bn);
	if constexpr (TAN) tan = normalized(tan + bt);
}
// The tiers without tangents, as every caller before the tangent stream spells them.
template <bool NRM, class Weight, class AfterSkipped, class ShapePos, class ShapeNrm>
GDI void morph_vertex(int mode, int P, Weight weight, AfterSkipped after_skipped, ShapePos shape_pos, ShapeNrm shape_nrm, V3 &pos,
		V3 &nrm) {
	V3 none = v3(0, 0, 0);
	morph_vertex_tier<NRM ? SKIN_NORMALS : SKIN_POSITIONS>(mode, P, weight, after_skipped, shape_pos, shape_nrm,
			[](int) { return v3(0, 0, 0); }, pos, nrm, none);
}

// One skeleton's staged weights c[0..P), rewritten in place: a skipped weight becomes the index of
// the next active shape behind it (P if there is none), stored as an integer's bits.  Such a value
// is itself a skipped weight -- an index up to P is a denormal far below 0.0001f, P being at most
// 40,960 -- so morph_vertex needs no second array to tell a link from a weight, and the LDS holds
// what it held.  after_skipped is then morph_link(c).
GDI void morph_link_skipped(float *c, int P) {
	int next = P;
	for (int j = P - 1; j >= 0; j--) {
		if (morph_active(c[j])) next = j;
		else __builtin_memcpy(&c[j], &next, 4);
	}
}
GDI int morph_link(float c) {
	int next;
	__builtin_memcpy(&next, &c, 4);
	return next;
}

// ---------------- validation (the checks mbik_mesh_create_shaped and mbik_skin_vertices_shaped_cpu share) ----------------
enum MorphCheck { MORPH_OK = 0, MORPH_BAD_COUNT, MORPH_BAD_MODE, MORPH_NULL, MORPH_NORMALS_MISMATCH, MORPH_TOO_LARGE };
// lds_limit: morph_lds_bytes(B, P) may not exceed it (< 0: no limit, the host entry takes any rig)
inline MorphCheck morph_check(int32_t B, int32_t V, bool mesh_normals, int32_t P, int32_t mode, const float *shape_positions,
		const float *shape_normals, int64_t lds_limit) {
	if (P < 1) return MORPH_BAD_COUNT;
	if (mode != MORPH_RELATIVE && mode != MORPH_NORMALIZED) return MORPH_BAD_MODE;
	if (V > 0 && !shape_positions) return MORPH_NULL;
	if (mesh_normals != (shape_normals != nullptr)) return MORPH_NORMALS_MISMATCH;
	if (lds_limit >= 0 && morph_lds_bytes(B, P) > lds_limit) return MORPH_TOO_LARGE;
	return MORPH_OK;
}
inline const char *morph_check_text(MorphCheck c) {
	switch (c) {
		case MORPH_BAD_COUNT: return "shape_count must be at least 1";
		case MORPH_BAD_MODE: return "shape mode must be 0 (relative) or 1 (normalized)";
		case MORPH_NULL: return "null shape positions";
		case MORPH_NORMALS_MISMATCH: return "the mesh and its shapes must both have normals or both have none";
		case MORPH_TOO_LARGE: return "bone_count * 48 + shape_count * 4 exceeds 160 KiB of LDS";
		default: return "ok";
	}
}

// ---------------- device layout ----------------
// Behind skin_layout()'s planes, whose offsets do not move:
//   shape positions  [P][V] 16 B   x, y, z, 0
//   shape normals    [P][V] 16 B   x, y, z, 0      (meshes with normals)
// Every plane holds `stride` records (V rounded up to even, as skin.h's planes) and starts at a
// multiple of 16 bytes.  Offsets are in bytes from the mesh's base.
struct MorphLayout {
	int64_t pos, nrm, stride, bytes; // nrm = -1 without normals; bytes = the whole mesh, skin_layout()'s planes included
};
inline MorphLayout morph_layout(int32_t V, int32_t K, bool normals, int32_t P) {
	const int64_t n = ((int64_t)V + 1) & ~(int64_t)1;
	MorphLayout l;
	int64_t at = skin_layout(V, K, normals).bytes;
	l.stride = n;
	l.pos = at, at += (int64_t)P * n * 16;
	l.nrm = normals ? at : -1;
	if (normals) at += (int64_t)P * n * 16;
	l.bytes = at;
	return l;
}
// Fills the shape planes of `out` (morph_layout().bytes bytes; skin_pack fills the planes in front)
// from checked shapes: shape_positions / shape_normals [P][V][3].
inline void morph_pack(int32_t V, int32_t K, int32_t P, const float *shape_positions, const float *shape_normals, unsigned char *out) {
	const MorphLayout l = morph_layout(V, K, shape_normals != nullptr, P);
	if (V == 0) return; // (a mesh without vertices: `out` may be null)
	memset(out + l.pos, 0, (size_t)(l.bytes - l.pos));
	for (int64_t j = 0; j < P; j++)
		for (int64_t v = 0; v < V; v++) {
			memcpy(out + l.pos + (j * l.stride + v) * 16, shape_positions + (j * V + v) * 3, 12);
			if (shape_normals) memcpy(out + l.nrm + (j * l.stride + v) * 16, shape_normals + (j * V + v) * 3, 12);
		}
}

// ---------------- tangents (mbik_mesh_create_desc) ----------------
// Shape tangents [P][V][3] are given exactly when the mesh has both shapes and tangents.
enum TangentCheck { TANGENT_OK = 0, TANGENT_SHAPES_MISMATCH };
inline TangentCheck tangent_check_shapes(bool shapes, bool tangents, const float *shape_tangents) {
	return (shapes && tangents) != (shape_tangents != nullptr) ? TANGENT_SHAPES_MISMATCH : TANGENT_OK;
}
inline const char *tangent_check_text(TangentCheck c) {
	return c == TANGENT_SHAPES_MISMATCH ? "shape_tangents must be given exactly when the mesh has both shapes and tangents" : "ok";
}
// Behind everything skin_layout() and morph_layout() place, so that a mesh without tangents is the
// image it always was and no existing offset moves:
//   base tangents   [stride] 16 B   x, y, z, w       (w: the binormal sign's bits; no plane of its own)
//   shape tangents  [P][stride] 16 B   x, y, z, 0    (shaped meshes)
struct TangentLayout {
	int64_t tan, stan, stride, bytes; // tan = -1 without tangents, stan = -1 without shapes; bytes = the whole mesh
};
inline TangentLayout tangent_layout(int32_t V, int32_t K, bool normals, int32_t P, bool tangents) {
	const MorphLayout ml = morph_layout(V, K, normals, P); // (P == 0: skin_layout()'s bytes)
	TangentLayout l;
	int64_t at = ml.bytes;
	l.stride = ml.stride;
	l.tan = tangents ? at : -1;
	if (tangents) at += ml.stride * 16;
	l.stan = tangents && P > 0 ? at : -1;
	if (tangents) at += (int64_t)P * ml.stride * 16;
	l.bytes = at;
	return l;
}
// Fills the tangent planes of `out` (tangent_layout().bytes bytes; skin_pack and morph_pack fill the
// planes in front): tangents [V][4], shape_tangents [P][V][3] or null when P == 0.
inline void tangent_pack(int32_t V, int32_t K, int32_t P, const float *tangents, const float *shape_tangents, unsigned char *out) {
	const TangentLayout l = tangent_layout(V, K, true, P, true);
	if (V == 0) return; // (a mesh without vertices: `out` may be null)
	memset(out + l.tan, 0, (size_t)(l.bytes - l.tan));
	for (int64_t v = 0; v < V; v++) memcpy(out + l.tan + v * 16, tangents + v * 4, 16);
	for (int64_t j = 0; j < P; j++)
		for (int64_t v = 0; v < V; v++) memcpy(out + l.stan + (j * l.stride + v) * 16, shape_tangents + (j * V + v) * 3, 12);
}

// ---------------- host path ----------------
// count skeletons of a checked mesh with checked shapes: shape_weights [count][P]; the rest as skin_vertices_host
// (tangents [V][4], shape_tangents [P][V][3] and out_tangents [count][V][4] all given, with out_normals, or all null)
inline void morph_skin_vertices_host(int32_t B, int32_t V, int32_t K, const float *positions, const float *normals,
		const int32_t *bone_indices, const float *weights, int32_t P, int32_t mode, const float *shape_positions,
		const float *shape_normals, int32_t count, const float *skin, const float *shape_weights, float *out_positions,
		float *out_normals, const float *tangents = nullptr, const float *shape_tangents = nullptr, float *out_tangents = nullptr) {
	for (int64_t s = 0; s < count; s++)
		for (int64_t v = 0; v < V; v++) {
			const float *c = shape_weights + s * P;
			const auto weight = [&](int j) { return c[j]; };
			const auto next = [](int j, float) { return j + 1; };
			const auto spos = [&](int j) { const float *p = shape_positions + ((int64_t)j * V + v) * 3; return v3(p[0], p[1], p[2]); };
			const auto snrm = [&](int j) { const float *p = shape_normals + ((int64_t)j * V + v) * 3; return v3(p[0], p[1], p[2]); };
			const auto stan = [&](int j) { const float *p = shape_tangents + ((int64_t)j * V + v) * 3; return v3(p[0], p[1], p[2]); };
			V3 pos = v3(positions[v * 3], positions[v * 3 + 1], positions[v * 3 + 2]), nrm = v3(0, 0, 0), tan = v3(0, 0, 0);
			if (out_tangents) {
				nrm = v3(normals[v * 3], normals[v * 3 + 1], normals[v * 3 + 2]);
				tan = v3(tangents[v * 4], tangents[v * 4 + 1], tangents[v * 4 + 2]);
				morph_vertex_tier<SKIN_TANGENTS>(mode, P, weight, next, spos, snrm, stan, pos, nrm, tan);
			} else if (out_normals) {
				nrm = v3(normals[v * 3], normals[v * 3 + 1], normals[v * 3 + 2]);
				morph_vertex<true>(mode, P, weight, next, spos, snrm, pos, nrm);
			} else {
				morph_vertex<false>(mode, P, weight, next, spos, snrm, pos, nrm);
			}
			const float p3[3] = {pos.x, pos.y, pos.z}, n3[3] = {nrm.x, nrm.y, nrm.z};
			float t4[4] = {tan.x, tan.y, tan.z, 0.0f};
			if (out_tangents) memcpy(t4 + 3, tangents + v * 4 + 3, 4); // (the sign's bits)
			skin_vertex_host(K, skin + s * B * 12, bone_indices + v * K, weights + v * K, p3, out_normals ? n3 : nullptr,
					out_positions + (s * V + v) * 3, out_normals ? out_normals + (s * V + v) * 3 : nullptr, out_tangents ? t4 : nullptr,
					out_tangents ? out_tangents + (s * V + v) * 4 : nullptr);
		}
}

} // namespace mbik
