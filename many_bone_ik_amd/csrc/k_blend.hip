// mbik_pose_blend's kernel: the modifier influence of Skeleton3D::_process_modifiers for a batch of
// skeletons (blend.h).
//
// One thread per bone; a block owns kBlendThreads consecutive bones of the batch, whatever
// skeletons they belong to.  Their records are one contiguous run of 10 floats a bone in pose_in,
// pose_mod and pose_out, so all three go through LDS (lds_copy_runs): consecutive lanes move
// consecutive addresses, 16 bytes a lane where the address allows, instead of ten dword accesses
// 40 bytes apart per lane and array.  A lane then reads its own two records from LDS at a stride
// of 10 dwords: lanes i and i + 32 share a bank (10 * 32 = 5 * 64), a 2-way conflict on 30 dword
// accesses a lane, against well over a thousand arithmetic instructions.  A stride of 11 would be
// conflict-free but turns the one run into 256 runs of 10 floats, which lds_copy_runs' 16-byte
// path cannot move (several runs need a length that is a multiple of 4).
//
// The result is written over the block's copy of pose_mod: a bone that is not blended keeps the
// modifier's bits without touching them, and a wave none of whose lanes blends (influence >= 1,
// or equal transforms) branches around the arithmetic.  The block has read both of its runs
// before the barrier and writes only its own run of pose_out after it, so pose_out may be
// pose_mod or pose_in.
#include "blend.h"
#include "kernels.h"
#include "lds_copy.h"

namespace {
using namespace mbik;

constexpr int kBlendThreads = 256;

// LV: the plan's libm_variant (gd::LIBM_FMA / LIBM_SSE2), a compile-time constant of sin_f.
template <int LV>
__global__ __launch_bounds__(kBlendThreads) void mbik_blend_kernel(int64_t total, int B, float influence,
		const float *influence_per_skeleton, const float *pose_in, const float *pose_mod, float *pose_out) {
	__shared__ __attribute__((aligned(16))) float Al[kBlendThreads * 10];
	__shared__ __attribute__((aligned(16))) float Ml[kBlendThreads * 10];
	const int64_t b0 = (int64_t)blockIdx.x * kBlendThreads;
	const int n = (int)min((int64_t)kBlendThreads, total - b0);
	if (n <= 0) return;
	lds_copy_runs<true, kBlendThreads>(Al, 0, pose_in + b0 * 10, n * 10, 1);
	lds_copy_runs<true, kBlendThreads>(Ml, 0, pose_mod + b0 * 10, n * 10, 1);
	__syncthreads();
	const int t = threadIdx.x;
	if (t < n) {
		float w = influence;
		if (influence_per_skeleton) {
			// the skeleton of bone b0 + t: the block's first skeleton (uniform) plus a 32-bit quotient
			const int64_t s0 = b0 / B;
			const int r = (int)(b0 - s0 * B) + t;
			w = influence_per_skeleton[s0 + r / B];
		}
		float *m = Ml + t * 10;
		const X3 A = pose_to_xform(Al + t * 10), M = pose_to_xform(m);
		if (blend_needed(A, M, w)) blend_xforms(A, M, w, LV, m);
	}
	__syncthreads();
	lds_copy_runs<false, kBlendThreads>(Ml, 0, pose_out + b0 * 10, n * 10, 1);
}
} // namespace

namespace mbik {

hipError_t launch_blend(hipStream_t st, int64_t total_bones, int B, int libm, float influence, const float *influence_per_skeleton,
		const float *pose_in, const float *pose_mod, float *pose_out) {
	const unsigned blocks = (unsigned)((total_bones + kBlendThreads - 1) / kBlendThreads);
	const auto kernel = libm == LIBM_SSE2 ? mbik_blend_kernel<LIBM_SSE2> : mbik_blend_kernel<LIBM_FMA>;
	hipLaunchKernelGGL(kernel, dim3(blocks), dim3(kBlendThreads), 0, st, total_bones, B, influence, influence_per_skeleton,
			pose_in, pose_mod, pose_out);
	return hipGetLastError();
}

} // namespace mbik
