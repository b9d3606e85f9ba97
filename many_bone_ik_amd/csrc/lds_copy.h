// Block-wide copies between contiguous runs of device memory and LDS, shared by the kernels
// that stage whole skeletons (k_fk.hip, k_skin.hip): consecutive lanes move consecutive
// addresses, 16 bytes a lane from the first 16-byte boundary of the device address and dwords
// for the head, the tail and whatever a float-aligned run leaves over.  Device code only.
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>
#include <type_traits>

namespace mbik {

// run r (of `runs`, `len` floats each) lies at g + r * len in device memory and at l + r * lstride
// in LDS.  With several runs len is a multiple of 4, so every run has the head of the first.
// Every thread of the THREADS-wide block calls it; the caller places the barriers.
template <bool TO_LDS, int THREADS>
__device__ __forceinline__ void lds_copy_runs(float *l, int lstride, typename std::conditional<TO_LDS, const float, float>::type *g,
		int len, int runs) {
	const int mis = (int)((reinterpret_cast<uintptr_t>(g) >> 2) & 3); // floats past a 16-byte boundary
	const int head = min(len, (4 - mis) & 3);
	const int nvec = (len - head) >> 2;
	const int edge = len - 4 * nvec; // head + tail floats of a run
	for (int i = threadIdx.x; i < runs * nvec; i += THREADS) {
		const int r = i / nvec, k = head + 4 * (i - r * nvec);
		float *lp = l + r * lstride + k;
		if constexpr (TO_LDS) {
			const float4 v = *reinterpret_cast<const float4 *>(g + (size_t)r * len + k);
			lp[0] = v.x, lp[1] = v.y, lp[2] = v.z, lp[3] = v.w;
		} else {
			*reinterpret_cast<float4 *>(g + (size_t)r * len + k) = make_float4(lp[0], lp[1], lp[2], lp[3]);
		}
	}
	for (int i = threadIdx.x; i < runs * edge; i += THREADS) {
		const int r = i / edge, j = i - r * edge;
		const int k = j < head ? j : j + 4 * nvec;
		if constexpr (TO_LDS) l[r * lstride + k] = g[(size_t)r * len + k];
		else g[(size_t)r * len + k] = l[r * lstride + k];
	}
}

} // namespace mbik
