// mbik_pose_globals' kernel: skeleton-space bone transforms (Skeleton3D::get_bone_global_pose),
// skin transforms and pin-to-target distances for a batch of solved poses (fk.h).
//
// A block owns S consecutive skeletons.  Their poses are one contiguous run of `pose` and their
// globals one contiguous run of `globals`, so both go through LDS: the run is read and written by
// consecutive lanes at consecutive addresses (16 bytes a lane where the address is 16-byte
// aligned, dwords for the head, the tail and unaligned runs), whatever the (skeleton, bone)
// mapping of the arithmetic in between.  The parent dependency is level-synchronous: the threads
// cover the (skeleton, bone of the level) pairs, read the parent's global from LDS and meet at
// one block barrier per level.
#include <mutex>

#include "fk.h"
#include "kernels.h"
#include "lds_copy.h"

namespace {
using namespace mbik;

constexpr int kFkThreads = 256;

// sched: [levels + 1] level offsets, then [B] (bone, parent) pairs in schedule order, then [P] pin bones.
__global__ __launch_bounds__(kFkThreads) void mbik_fk_kernel(int count, int B, int P, int S, int levels,
		const int *__restrict__ sched, const float *__restrict__ pose, const float *__restrict__ inv_bind,
		float *__restrict__ globals, const float *__restrict__ targets, float *__restrict__ pin_distance) {
	extern __shared__ __attribute__((aligned(16))) float fk_lds[];
	const int64_t s0 = (int64_t)blockIdx.x * S;
	const int ns = (int)min((int64_t)S, (int64_t)count - s0);
	if (ns <= 0) return;
	const int gs = fk_gstride(B);
	float *Pl = fk_lds;                  // [ns][B][10]
	float *G = fk_lds + (size_t)S * B * 10; // [ns][gs]
	const int *level_off = sched;
	const int2 *pairs = reinterpret_cast<const int2 *>(sched + levels + 1 + ((levels + 1) & 1));
	const int *pin_bone = reinterpret_cast<const int *>(pairs + B);

	lds_copy_runs<true, kFkThreads>(Pl, 0, pose + s0 * B * 10, ns * B * 10, 1);
	__syncthreads();
	// locals of every (skeleton, bone); the roots' are their globals
	for (int i = threadIdx.x; i < ns * B; i += kFkThreads) {
		const int s = i / B, b = i - s * B;
		fk_local(Pl + (size_t)i * 10, G + s * gs + b * 12);
	}
	__syncthreads();
	for (int l = 1; l < levels; l++) {
		const int lo = level_off[l], w = level_off[l + 1] - lo;
		for (int i = threadIdx.x; i < ns * w; i += kFkThreads) {
			const int j = i / ns, s = i - j * ns; // consecutive lanes: consecutive skeletons
			const int2 bp = pairs[lo + j];
			fk_compose(G + s * gs + bp.y * 12, G + s * gs + bp.x * 12);
		}
		__syncthreads();
	}
	if (pin_distance) {
		for (int i = threadIdx.x; i < ns * P; i += kFkThreads) {
			const int s = i / P, e = i - s * P;
			pin_distance[s0 * P + i] = fk_pin_distance(G + s * gs + pin_bone[e] * 12, targets + (s0 * P + i) * 12);
		}
	}
	if (!globals) return;
	if (inv_bind) {
		__syncthreads(); // the distances read the unskinned globals
		for (int i = threadIdx.x; i < ns * B; i += kFkThreads) {
			const int b = i / ns, s = i - b * ns;
			float *g = G + s * gs + b * 12;
			fk_skin(g, inv_bind + b * 12, g);
		}
		__syncthreads();
	}
	lds_copy_runs<false, kFkThreads>(G, gs, globals + s0 * B * 12, B * 12, ns);
}
} // namespace

namespace mbik {

hipError_t launch_fk(hipStream_t st, int count, int B, int P, int S, int levels, const int *sched, const float *pose,
		const float *inv_bind, float *globals, const float *targets, float *pin_distance) {
	static std::once_flag once;
	std::call_once(once, [] {
		(void)hipFuncSetAttribute((const void *)mbik_fk_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, kFkMaxLdsBytes);
	});
	const size_t lds = (size_t)fk_lds_floats(B, S) * sizeof(float);
	const unsigned blocks = (unsigned)(((int64_t)count + S - 1) / S);
	hipLaunchKernelGGL(mbik_fk_kernel, dim3(blocks), dim3(kFkThreads), lds, st, count, B, P, S, levels, sched, pose, inv_bind,
			globals, targets, pin_distance);
	return hipGetLastError();
}

} // namespace mbik
