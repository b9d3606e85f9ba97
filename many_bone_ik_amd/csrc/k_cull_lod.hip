// mbik_cull_lod's kernels (lod.h).
//
// k_bounds.hip's culling, once per range: one thread per skeleton, 256 a block, the planes, the
// camera and the ranges in the kernel's arguments.  Every list needs each of its skeletons' rank, so
// there are three launches in stream order and no block waits for another inside one:
//
//   mbik_lod_select_kernel   runs lod_select, writes state and level and, to the mesh's scratch, one
//                            member byte a skeleton (bit r: list r names it), and counts each range's
//                            members in the block: a ballot and pop-count a wave, the wave counts
//                            through LDS, totals[r][block]
//   mbik_lod_scan_kernel     block r turns row r of the totals into exclusive offsets and writes
//                            list_counts[r]: mbik_cull_scan_kernel's loop with its carry, a row a block
//   mbik_lod_place_kernel    reads the member bytes back and places the indices: ballot prefix inside
//                            a wave, wave counts through LDS, the block's offset from the scan
//
// The placement does not run lod_select again: the first kernel has already advanced `state`, so the
// verdict it would reach is no longer the one the counts were taken from by construction.  The member
// byte carries the verdict across instead, and the placement reads one byte a skeleton, not a box.
// The loops over the ranges are launch-uniform, so every lane meets every ballot and barrier.
#include "kernels.h"
#include "lod.h"

namespace {
using namespace mbik;

constexpr int kThreads = 256, kWaves = kThreads / 64;

struct LodPlanes {
	float4 p[kCullMaxPlanes];
};
struct LodRanges {
	float4 r[kLodMaxRanges]; // begin, end, begin_margin, end_margin
};

__global__ __launch_bounds__(kThreads) void mbik_lod_select_kernel(int count, const float *__restrict__ boxes,
		const float *__restrict__ global, float margin, int plane_count, LodPlanes planes, float cx, float cy, float cz, int range_count,
		LodRanges ranges, uint32_t flags, uint8_t *__restrict__ state, uint8_t *__restrict__ level, uint8_t *__restrict__ member,
		int32_t *__restrict__ totals, int blocks) {
	__shared__ int wave_count[kLodMaxRanges][kWaves];
	const int64_t s = (int64_t)blockIdx.x * kThreads + threadIdx.x;
	LodVerdict v{0, kLodNone, 0};
	if (s < count) {
		v = lod_select(
				box_load(boxes + s * 6), global ? global + s * 12 : nullptr, margin, plane_count,
				[&](int i, float &nx, float &ny, float &nz, float &d) {
					const float4 q = planes.p[i];
					nx = q.x, ny = q.y, nz = q.z, d = q.w;
				},
				v3(cx, cy, cz), range_count,
				[&](int r) {
					const float4 q = ranges.r[r];
					return LodRange{q.x, q.y, q.z, q.w};
				},
				flags, state[s]);
		state[s] = v.state;
		if (level) level[s] = v.level;
		member[s] = v.member;
	}
	const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
	for (int r = 0; r < range_count; r++) { // (uniform)
		const unsigned long long ballot = __ballot((v.member >> r) & 1);
		if (lane == 0) wave_count[r][wave] = __popcll(ballot);
	}
	__syncthreads();
	if ((int)threadIdx.x < range_count) {
		const int *w = wave_count[threadIdx.x];
		totals[(size_t)threadIdx.x * blocks + blockIdx.x] = w[0] + w[1] + w[2] + w[3];
	}
}

// Block r: totals[r][0 .. n) become their exclusive prefix sums, list_counts[r] their sum.
__global__ __launch_bounds__(kThreads) void mbik_lod_scan_kernel(int n, int32_t *__restrict__ totals, int32_t *__restrict__ list_counts) {
	__shared__ int wave_sum[kWaves];
	int32_t *row = totals + (size_t)blockIdx.x * n;
	const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
	int carry = 0;
	for (int base = 0; base < n; base += kThreads) { // (uniform)
		const int i = base + (int)threadIdx.x;
		const int v = i < n ? row[i] : 0;
		int incl = v;
		for (int d = 1; d < 64; d <<= 1) {
			const int up = __shfl_up(incl, d, 64);
			if (lane >= d) incl += up;
		}
		if (lane == 63) wave_sum[wave] = incl;
		__syncthreads();
		int before = 0;
		for (int w = 0; w < wave; w++) before += wave_sum[w];
		if (i < n) row[i] = carry + before + incl - v;
		carry += wave_sum[0] + wave_sum[1] + wave_sum[2] + wave_sum[3];
		__syncthreads();
	}
	if (threadIdx.x == 0) list_counts[blockIdx.x] = carry;
}

__global__ __launch_bounds__(kThreads) void mbik_lod_place_kernel(int count, int range_count, const uint8_t *__restrict__ member,
		const int32_t *__restrict__ totals, int blocks, int32_t *__restrict__ indices) {
	__shared__ int wave_count[kLodMaxRanges][kWaves];
	const int64_t s = (int64_t)blockIdx.x * kThreads + threadIdx.x;
	const unsigned m = s < count ? member[s] : 0u;
	const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
	for (int r = 0; r < range_count; r++) { // (uniform)
		const unsigned long long ballot = __ballot((m >> r) & 1);
		if (lane == 0) wave_count[r][wave] = __popcll(ballot);
	}
	__syncthreads();
	for (int r = 0; r < range_count; r++) { // (uniform)
		const bool in = (m >> r) & 1;
		const unsigned long long ballot = __ballot(in);
		int at = totals[(size_t)r * blocks + blockIdx.x] + __popcll(ballot & ((1ull << lane) - 1ull));
		for (int w = 0; w < wave; w++) at += wave_count[r][w];
		if (in) indices[(int64_t)r * count + at] = (int32_t)s;
	}
}

} // namespace

namespace mbik {

hipError_t launch_cull_lod(hipStream_t st, int count, const float *boxes, const float *skeleton_global, float margin, int plane_count,
		const float *planes, const float *camera, int range_count, const LodRange *ranges, uint32_t flags, uint8_t *state, uint8_t *level,
		int32_t *indices, int32_t *list_counts, int32_t *totals, uint8_t *member) {
	LodPlanes lp;
	for (int i = 0; i < kCullMaxPlanes; i++)
		lp.p[i] = i < plane_count ? make_float4(planes[i * 4], planes[i * 4 + 1], planes[i * 4 + 2], planes[i * 4 + 3]) : make_float4(0, 0, 0, 0);
	LodRanges lr;
	for (int r = 0; r < kLodMaxRanges; r++)
		lr.r[r] = r < range_count ? make_float4(ranges[r].begin, ranges[r].end, ranges[r].begin_margin, ranges[r].end_margin) : make_float4(0, 0, 0, 0);
	const int blocks = cull_blocks(count);
	hipLaunchKernelGGL(mbik_lod_select_kernel, dim3(blocks), dim3(kThreads), 0, st, count, boxes, skeleton_global, margin, plane_count, lp,
			camera[0], camera[1], camera[2], range_count, lr, flags, state, level, member, totals, blocks);
	hipLaunchKernelGGL(mbik_lod_scan_kernel, dim3(range_count), dim3(kThreads), 0, st, blocks, totals, list_counts);
	hipLaunchKernelGGL(mbik_lod_place_kernel, dim3(blocks), dim3(kThreads), 0, st, count, range_count, member, totals, blocks, indices);
	return hipGetLastError();
}

} // namespace mbik
