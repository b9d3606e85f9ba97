// Block-wide copies between contiguous runs of device memory and LDS, shared by the kernels
// that stage whole skeletons (k_fk.hip, k_skin.hip, k_skin_list.hip): consecutive lanes move consecutive
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

// The gathered form, device memory to LDS (k_skin_list.hip): run r still lands at l + r * lstride, but
// comes from g + src(r) * len, and a run with src(r) < 0 is left out (its LDS is not written).  With
// len a multiple of 4 every run has the head of g, whichever run number it has, and moves 16 bytes a
// lane as above; any other len moves dwords (the runs' heads differ).  kGatherDepth loads of a lane
// are issued before the first is waited for, across runs: a run is often shorter than the block.
// Every thread calls src() in every pass, lanes without an item with r = 0, so src may use
// cross-lane operations.
// (-DMBIK_GATHER_DEPTH=n: A/B builds of the loads in flight)
#ifndef MBIK_GATHER_DEPTH
#define MBIK_GATHER_DEPTH 4
#endif
constexpr int kGatherDepth = MBIK_GATHER_DEPTH;
template <int THREADS, class Src>
__device__ __forceinline__ void lds_gather_runs(float *l, int lstride, const float *g, int len, int runs, Src src) {
	const int mis = (int)((reinterpret_cast<uintptr_t>(g) >> 2) & 3);
	const bool quads = (len & 3) == 0;
	const int head = quads ? min(len, (4 - mis) & 3) : 0;
	const int nvec = quads ? (len - head) >> 2 : 0;
	const int edge = len - 4 * nvec;
	for (int base = 0; base < runs * nvec; base += kGatherDepth * THREADS) {
		float4 v[kGatherDepth];
		int at[kGatherDepth]; // the item's LDS float offset; -1: no item, or a run left out
#pragma unroll
		for (int u = 0; u < kGatherDepth; u++) {
			const int i = base + u * THREADS + (int)threadIdx.x;
			const bool item = i < runs * nvec;
			const int r = item ? i / nvec : 0, k = head + 4 * (i - r * nvec);
			const int64_t s = src(r);
			at[u] = item && s >= 0 ? r * lstride + k : -1;
			if (at[u] >= 0) v[u] = *reinterpret_cast<const float4 *>(g + s * len + k);
		}
#pragma unroll
		for (int u = 0; u < kGatherDepth; u++)
			if (at[u] >= 0) {
				float *lp = l + at[u];
				lp[0] = v[u].x, lp[1] = v[u].y, lp[2] = v[u].z, lp[3] = v[u].w;
			}
	}
	for (int base = 0; base < runs * edge; base += THREADS) {
		const int i = base + (int)threadIdx.x;
		const bool item = i < runs * edge;
		const int r = item ? i / edge : 0, j = i - r * edge;
		const int k = j < head ? j : j + 4 * nvec;
		const int64_t s = src(r);
		if (item && s >= 0) l[r * lstride + k] = g[s * len + k];
	}
}

} // namespace mbik
