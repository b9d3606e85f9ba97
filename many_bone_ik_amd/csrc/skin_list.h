// List-driven skinning (mbik_skin_vertices_listed): the skeletons a list names, e.g.
// mbik_cull_boxes' visible list, skinned with mbik_skin_vertices' or mbik_skin_vertices_shaped's bits.
//
//     n = min(max(list_count[0], 0), max_list)
//     for r = 0 .. n-1:  s = indices[r]
//         if (s < 0 || s >= count) continue          nothing is read or written for the entry
//         row = compact ? r : s
//         out[row] = what the plain (shape_weights == null) or the shaped call writes to row s
//     every other row of the outputs is not touched
//
// This header is the host path, host code without a HIP call: one skeleton a call through
// skin_vertices_host / morph_skin_vertices_host, which do not change, so the bits are theirs by
// construction.  tools/san/skin_list_san.cpp runs it under ASan + UBSan.  The device path is
// k_skin_list.hip.
#pragma once

#include <algorithm>

#include "morph.h"
#include "skin.h"

namespace mbik {

constexpr uint32_t kSkinListCompact = 1u; // MBIK_SKIN_LIST_COMPACT
constexpr uint32_t kSkinListFlags = kSkinListCompact;

// The entries the call looks at.
inline int32_t skin_list_length(const int32_t *list_count, int32_t max_list) { return std::min(std::max(list_count[0], 0), max_list); }

// A checked mesh (and checked shapes when shape_weights is given; P, mode, shape_positions and
// shape_normals are not looked at otherwise); skin [count][B][12], shape_weights [count][P] or null,
// indices [max_list], list_count [1]; out_positions / out_normals [compact ? max_list : count][V][3].
// out_tangents (the same rows, [V][4]) with the mesh's tangents [V][4], and shape_tangents when
// shape_weights is given, or null.
inline void skin_vertices_listed_host(int32_t B, int32_t V, int32_t K, const float *positions, const float *normals,
		const int32_t *bone_indices, const float *weights, int32_t P, int32_t mode, const float *shape_positions,
		const float *shape_normals, int32_t count, const int32_t *indices, const int32_t *list_count, int32_t max_list, const float *skin,
		const float *shape_weights, bool compact, float *out_positions, float *out_normals, const float *tangents = nullptr,
		const float *shape_tangents = nullptr, float *out_tangents = nullptr) {
	const int32_t n = skin_list_length(list_count, max_list);
	for (int64_t r = 0; r < n; r++) {
		const int64_t s = indices[r];
		if (s < 0 || s >= count) continue;
		const int64_t at = (compact ? r : s) * V * 3;
		float *out_n = out_normals ? out_normals + at : nullptr;
		float *out_t = out_tangents ? out_tangents + (compact ? r : s) * V * 4 : nullptr;
		if (shape_weights)
			morph_skin_vertices_host(B, V, K, positions, normals, bone_indices, weights, P, mode, shape_positions, shape_normals, 1,
					skin + s * B * 12, shape_weights + s * P, out_positions + at, out_n, tangents, shape_tangents, out_t);
		else
			skin_vertices_host(B, V, K, positions, normals, bone_indices, weights, 1, skin + s * B * 12, out_positions + at, out_n, tangents,
					out_t);
	}
}

} // namespace mbik
