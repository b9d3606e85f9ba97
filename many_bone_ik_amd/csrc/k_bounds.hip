// mbik_skin_bounds', mbik_cull_boxes' and mbik_cull_lod's kernels (bounds.h, lod.h).
//
// Bounds.  A block owns S consecutive skeletons.  Their matrices are one contiguous run of `skin`
// (S x B x 12 floats) and go into LDS as k_skin.hip's do (lds_copy.h).  Phase 1 is parallel: one
// thread per (skeleton, used bone) item, 256 items a pass, reads its bone's record from the mesh's
// table (two quads) and its matrix from LDS (three quads) and computes t = xform_aabb.  Phase 2 is
// the merge chain, which fixes the order and is therefore not a reduction: the three axes of a box
// are independent chains, so one lane per (skeleton, axis) walks its t's in ascending order with
// compares and selects and stores its two floats.
//
// The t's live in the LDS the matrices came in: item u of a skeleton writes floats [6u, 6u + 6) of
// that skeleton's image.  Bone indices ascend with u, so bone(u) >= u, and the floats an item
// overwrites belong to the matrix of bone u / 2 -- needed only by an item u' <= u / 2, of this pass
// or an earlier one.  A barrier between a pass's reads and its writes is therefore all the order
// the passes need, a rig of MBIK_SKIN_MAX_BONES bones fits with one skeleton a block, and the block
// needs no LDS beyond the matrices'.
//
// Culling.  One thread per skeleton, 256 a block, the planes in the kernel's arguments.  The
// ordered list needs each visible skeleton's rank: mbik_cull_flags_kernel writes the verdicts and
// each block's count of visible skeletons, mbik_cull_scan_kernel (one block) turns the counts into
// exclusive offsets and writes the total, and mbik_cull_flags_kernel runs again to place the indices
// (ballot prefix inside a wave, wave counts through LDS, the block's offset from the scan).  Three
// launches in stream order; no block waits for another inside a launch.
//
// LOD lists.  The culling once per range, with the camera and the ranges in the kernel's arguments as
// well, and the same three launches, since every list needs each of its skeletons' rank:
//
//   mbik_lod_select_kernel   runs lod_select, writes state and level and, to the mesh's scratch, one
//                            member byte a skeleton (bit r: list r names it), and counts each range's
//                            members in the block into totals[r][block]
//   mbik_cull_scan_kernel    a block a range: block r turns row r of the totals into exclusive offsets
//                            and writes list_counts[r]
//   mbik_lod_place_kernel    reads the member bytes back and places the indices
//
// The placement does not run lod_select again: the first kernel has already advanced `state`, so the
// verdict it would reach is no longer the one the counts were taken from by construction.  The member
// byte carries the verdict across instead, and the placement reads one byte a skeleton, not a box.
//
// The counting and the ranking are wave_vote, block_votes and rank_in_block below.  Every lane of a
// block meets every ballot and every barrier: the loops over the ranges around them are
// launch-uniform (range_count is a kernel argument), and so is the scan's loop over n.
#include <mutex>

#include "bounds.h"
#include "kernels.h"
#include "lds_copy.h"
#include "lod.h"

namespace {
using namespace mbik;

constexpr int kThreads = 256, kWaves = kThreads / 64;

__global__ __launch_bounds__(kThreads) void mbik_skin_bounds_kernel(int count, int B, int U, int S, const float4 *__restrict__ table,
		const float *__restrict__ skin, float *__restrict__ boxes) {
	extern __shared__ __attribute__((aligned(16))) float bounds_lds[];
	const int64_t s0 = (int64_t)blockIdx.x * S;
	const int ns = (int)min((int64_t)S, (int64_t)count - s0);
	if (ns <= 0) return;
	lds_copy_runs<true, kThreads>(bounds_lds, 0, skin + s0 * B * 12, ns * B * 12, 1);
	__syncthreads();
	const int items = ns * U;
	for (int base = 0; base < items; base += kThreads) { // (uniform: every thread meets the barrier)
		const int i = base + (int)threadIdx.x;
		const int s = i / U, u = i - s * U;
		Box t;
		if (i < items) {
			const float4 r0 = table[2 * u], r1 = table[2 * u + 1];
			const float4 *m = reinterpret_cast<const float4 *>(bounds_lds + (s * B + __builtin_bit_cast(int, r0.x)) * 12);
			const float4 a = m[0], b = m[1], c = m[2];
			t = box_xform(X3{bset(a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w, c.x), v3(c.y, c.z, c.w)},
					Box{v3(r0.y, r0.z, r0.w), v3(r1.x, r1.y, r1.z)});
		}
		__syncthreads();
		if (i < items) box_store(bounds_lds + s * B * 12 + u * 6, t);
	}
	__syncthreads();
#ifndef MBIK_BOUNDS_ONE_LANE
	for (int i = threadIdx.x; i < ns * 3; i += kThreads) {
		const int s = i / 3, a = i - s * 3;
		const float *ts = bounds_lds + s * B * 12 + a;
		float p = 0.0f, z = 0.0f;
		if (U > 0) p = ts[0], z = ts[3];
		for (int u = 1; u < U; u++) box_merge_axis(p, z, ts[u * 6], ts[u * 6 + 3]);
		float *o = boxes + (s0 + s) * 6 + a;
		o[0] = p, o[3] = z;
	}
#else // A/B build: one lane a skeleton walks all three axes
	for (int s = threadIdx.x; s < ns; s += kThreads) {
		const float *ts = bounds_lds + s * B * 12;
		Box acc{v3(0, 0, 0), v3(0, 0, 0)};
		if (U > 0) acc = box_load(ts);
		for (int u = 1; u < U; u++) acc = box_merge(acc, box_load(ts + u * 6));
		box_store(boxes + (s0 + s) * 6, acc);
	}
#endif
}

// The planes of a call as a kernel argument: read from host memory at the launch, the unused ones zero.
struct CullPlanes {
	float4 p[kCullMaxPlanes];
	CullPlanes(int plane_count, const float *planes) {
		for (int i = 0; i < kCullMaxPlanes; i++)
			p[i] = i < plane_count ? make_float4(planes[i * 4], planes[i * 4 + 1], planes[i * 4 + 2], planes[i * 4 + 3]) : make_float4(0, 0, 0, 0);
	}
};
struct LodRanges {
	float4 r[kLodMaxRanges]; // begin, end, begin_margin, end_margin
};

// Counting and ranking the lanes of a block that vote in a ballot.  Every lane of the block takes the ballot and calls
// publish_votes, a barrier follows, then block_votes and rank_in_block read the counts.  lane and wave are the kernel's
// threadIdx.x & 63 and threadIdx.x >> 6.
// The wave's first lane writes the ballot's count to *count, the wave's place in the block's counts.
__device__ inline void publish_votes(unsigned long long ballot, int lane, int *count) {
	if (lane == 0) *count = __popcll(ballot);
}
__device__ inline int block_votes(const int *counts) { return counts[0] + counts[1] + counts[2] + counts[3]; }
// base + the voting lanes of the block in front of this one: in its wave by the ballot, the waves in front by their counts.
__device__ inline int rank_in_block(int base, unsigned long long ballot, int lane, int wave, const int *counts) {
	int at = base + __popcll(ballot & ((1ull << lane) - 1ull));
	for (int w = 0; w < wave; w++) at += counts[w];
	return at;
}

// PLACE false: visible[] (when given) and totals[block] (when given).  PLACE true: totals holds the
// blocks' exclusive offsets; the visible skeletons' indices go to indices[offset + rank in the block].
template <bool PLACE>
__global__ __launch_bounds__(kThreads) void mbik_cull_flags_kernel(int count, const float *__restrict__ boxes,
		const float *__restrict__ global, float margin, int plane_count, CullPlanes planes, uint8_t *__restrict__ visible,
		int32_t *__restrict__ totals, int32_t *__restrict__ indices) {
	__shared__ int wave_count[kWaves];
	const int64_t s = (int64_t)blockIdx.x * kThreads + threadIdx.x;
	bool vis = false;
	if (s < count)
		vis = cull_visible(box_load(boxes + s * 6), global ? global + s * 12 : nullptr, margin, plane_count,
				[&](int i, float &nx, float &ny, float &nz, float &d) {
					const float4 q = planes.p[i];
					nx = q.x, ny = q.y, nz = q.z, d = q.w;
				});
	if constexpr (!PLACE) {
		if (visible && s < count) visible[s] = vis ? 1 : 0;
		if (!totals) return; // (uniform)
	}
	const unsigned long long ballot = __ballot(vis);
	const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
	publish_votes(ballot, lane, &wave_count[wave]);
	__syncthreads();
	if constexpr (!PLACE) {
		if (threadIdx.x == 0) totals[blockIdx.x] = block_votes(wave_count);
	} else {
		const int at = rank_in_block(totals[blockIdx.x], ballot, lane, wave, wave_count);
		if (vis) indices[at] = (int32_t)s;
	}
}

// Block r: totals[r][0 .. n) become their exclusive prefix sums, counts[r] their sum.  mbik_cull_boxes has one row and
// one count; it launches the scan only for a call with a visible_count (indices come with one), so counts is never null.
__global__ __launch_bounds__(kThreads) void mbik_cull_scan_kernel(int n, int32_t *__restrict__ totals, int32_t *__restrict__ counts) {
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
		carry += block_votes(wave_sum);
		__syncthreads();
	}
	if (threadIdx.x == 0) counts[blockIdx.x] = carry;
}

__global__ __launch_bounds__(kThreads) void mbik_lod_select_kernel(int count, const float *__restrict__ boxes,
		const float *__restrict__ global, float margin, int plane_count, CullPlanes planes, float cx, float cy, float cz, int range_count,
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
	for (int r = 0; r < range_count; r++) publish_votes(__ballot((v.member >> r) & 1), lane, &wave_count[r][wave]); // (uniform)
	__syncthreads();
	if ((int)threadIdx.x < range_count) totals[(size_t)threadIdx.x * blocks + blockIdx.x] = block_votes(wave_count[threadIdx.x]);
}

__global__ __launch_bounds__(kThreads) void mbik_lod_place_kernel(int count, int range_count, const uint8_t *__restrict__ member,
		const int32_t *__restrict__ totals, int blocks, int32_t *__restrict__ indices) {
	__shared__ int wave_count[kLodMaxRanges][kWaves];
	const int64_t s = (int64_t)blockIdx.x * kThreads + threadIdx.x;
	const unsigned m = s < count ? member[s] : 0u;
	const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
	for (int r = 0; r < range_count; r++) publish_votes(__ballot((m >> r) & 1), lane, &wave_count[r][wave]); // (uniform)
	__syncthreads();
	for (int r = 0; r < range_count; r++) { // (uniform)
		const bool in = (m >> r) & 1;
		const unsigned long long ballot = __ballot(in);
		const int at = rank_in_block(totals[(size_t)r * blocks + blockIdx.x], ballot, lane, wave, wave_count[r]);
		if (in) indices[(int64_t)r * count + at] = (int32_t)s;
	}
}

} // namespace

namespace mbik {

hipError_t launch_skin_bounds(hipStream_t st, int count, int B, int U, int S, const unsigned char *table, const float *skin,
		float *boxes) {
	static std::once_flag once;
	std::call_once(once, [] {
		(void)hipFuncSetAttribute((const void *)mbik_skin_bounds_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, kSkinMaxLdsBytes);
	});
	const size_t lds = (size_t)S * (size_t)max(B, 1) * 12 * sizeof(float);
	const dim3 grid((unsigned)(((int64_t)count + S - 1) / S));
	hipLaunchKernelGGL(mbik_skin_bounds_kernel, grid, dim3(kThreads), lds, st, count, B, U, S, reinterpret_cast<const float4 *>(table), skin,
			boxes);
	return hipGetLastError();
}

hipError_t launch_cull(hipStream_t st, int count, const float *boxes, const float *skeleton_global, float margin, int plane_count,
		const float *planes, uint8_t *visible, int32_t *indices, int32_t *visible_count, int32_t *totals) {
	const CullPlanes cp(plane_count, planes);
	const int blocks = cull_blocks(count);
	const bool rank = indices || visible_count;
	hipLaunchKernelGGL(mbik_cull_flags_kernel<false>, dim3(blocks), dim3(kThreads), 0, st, count, boxes, skeleton_global, margin, plane_count,
			cp, visible, rank ? totals : nullptr, (int32_t *)nullptr);
	if (rank) hipLaunchKernelGGL(mbik_cull_scan_kernel, dim3(1), dim3(kThreads), 0, st, blocks, totals, visible_count);
	if (indices)
		hipLaunchKernelGGL(mbik_cull_flags_kernel<true>, dim3(blocks), dim3(kThreads), 0, st, count, boxes, skeleton_global, margin,
				plane_count, cp, (uint8_t *)nullptr, totals, indices);
	return hipGetLastError();
}

hipError_t launch_cull_lod(hipStream_t st, int count, const float *boxes, const float *skeleton_global, float margin, int plane_count,
		const float *planes, const float *camera, int range_count, const LodRange *ranges, uint32_t flags, uint8_t *state, uint8_t *level,
		int32_t *indices, int32_t *list_counts, int32_t *totals, uint8_t *member) {
	const CullPlanes cp(plane_count, planes);
	LodRanges lr;
	for (int r = 0; r < kLodMaxRanges; r++)
		lr.r[r] = r < range_count ? make_float4(ranges[r].begin, ranges[r].end, ranges[r].begin_margin, ranges[r].end_margin) : make_float4(0, 0, 0, 0);
	const int blocks = cull_blocks(count);
	hipLaunchKernelGGL(mbik_lod_select_kernel, dim3(blocks), dim3(kThreads), 0, st, count, boxes, skeleton_global, margin, plane_count, cp,
			camera[0], camera[1], camera[2], range_count, lr, flags, state, level, member, totals, blocks);
	hipLaunchKernelGGL(mbik_cull_scan_kernel, dim3(range_count), dim3(kThreads), 0, st, blocks, totals, list_counts);
	hipLaunchKernelGGL(mbik_lod_place_kernel, dim3(blocks), dim3(kThreads), 0, st, count, range_count, member, totals, blocks, indices);
	return hipGetLastError();
}

} // namespace mbik
