// What the skinning kernel TUs (k_skin.hip, k_skin_list.hip) share on the device side: the block
// size, a bone's matrix read from its LDS image and the 12-byte output store.  Device code only.
#pragma once
#include <hip/hip_runtime.h>

#include "skin.h"

namespace mbik {

constexpr int kSkinThreads = 256;

__device__ __forceinline__ X3 skin_load_lds(const float4 *m) {
	const float4 a = m[0], b = m[1], c = m[2];
	return X3{bset(a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w, c.x), v3(c.y, c.z, c.w)};
}

__device__ __forceinline__ void skin_store3(float *o, V3 p) {
#ifdef MBIK_SKIN_NT // A/B build: the outputs are written once and not read here
	__builtin_nontemporal_store(p.x, o), __builtin_nontemporal_store(p.y, o + 1), __builtin_nontemporal_store(p.z, o + 2);
#else
	o[0] = p.x, o[1] = p.y, o[2] = p.z;
#endif
}

} // namespace mbik
