// The lane arithmetic of the kernels that give a block 256 consecutive items of a batch of skeletons, whatever skeletons
// they belong to (k_clip.hip: bones; k_clip_shapes.hip: shape weights).
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace mbik {

// The skeleton and the item (bone, shape) of element b0 + t of a batch with `per` items a skeleton: the block's first
// skeleton (uniform, one 64-bit division) plus a 32-bit quotient per lane.
struct BatchLane {
	int64_t s;
	int item;
};
__device__ __forceinline__ BatchLane batch_lane(int per, int64_t b0, int t) {
	const uint32_t pu = (uint32_t)per;
	const int64_t s0 = b0 / per;
	const uint32_t r = (uint32_t)(b0 - s0 * per) + (uint32_t)t, q = r / pu;
	return BatchLane{s0 + q, (int)(r - q * pu)};
}

} // namespace mbik
