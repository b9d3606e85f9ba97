// mbik_clip_sample's kernel: Godot's Animation track interpolation for a batch of skeletons, each
// at its own time in its own clip (clip.h).
//
// One thread per bone; a block owns kClipThreads consecutive bones of the batch, whatever
// skeletons they belong to, as k_blend.hip does.  A lane builds its bone's 10 floats in LDS, and
// the block's records leave as one contiguous run of pose_out through lds_copy_runs: consecutive
// lanes store consecutive addresses, 16 bytes a lane where the address allows.  The inputs are 12
// bytes a skeleton (time, clip index) and the clip set's tables, which every skeleton shares and
// which stay in L2.  A lane's loads are arranged in as few dependent rounds as the data allows
// (clip.h clip_sample_bone): the three channels of a bone search in step, three independent loads
// in flight, and the key times and values of all three channels are then loaded at once.  Every
// probe of every lane is its own L2 request, and their rate is what bounds the kernel (§16).
// The slerp and the lerps sit behind per-lane branches: a wave whose lanes are all untracked,
// clamped or nearest skips them.
//
// The kernel tests no key index: mbik_clipset_create has checked every table (host_clip.cpp).
#include "clip.h"
#include "kernels.h"
#include "lds_copy.h"

namespace {
using namespace mbik;

constexpr int kClipThreads = 256;

// LV: the set's libm_variant (gd::LIBM_FMA / LIBM_SSE2), a compile-time constant of sin_f.
template <int LV>
__global__ __launch_bounds__(kClipThreads) void mbik_clip_kernel(ClipView v, int64_t total, const double *time, const int32_t *clip_index,
		int clip, float *pose_out) {
	__shared__ __attribute__((aligned(16))) float Pl[kClipThreads * 10];
	const int64_t b0 = (int64_t)blockIdx.x * kClipThreads;
	const int n = (int)min((int64_t)kClipThreads, total - b0);
	if (n <= 0) return;
	const int t = threadIdx.x;
	if (t < n) {
		// the skeleton of bone b0 + t: the block's first skeleton (uniform) plus a 32-bit quotient
		const uint32_t B = (uint32_t)v.B;
		const int64_t s0 = b0 / v.B;
		const uint32_t r = (uint32_t)(b0 - s0 * v.B) + (uint32_t)t, q = r / B;
		const int64_t s = s0 + q;
		clip_sample_bone(v, clip_index ? clip_index[s] : clip, (int)(r - q * B), time[s], LV, Pl + t * 10);
	}
	__syncthreads();
	lds_copy_runs<false, kClipThreads>(Pl, 0, pose_out + b0 * 10, n * 10, 1);
}
} // namespace

namespace mbik {

hipError_t launch_clip(hipStream_t st, const ClipView &v, int libm, int64_t total_bones, const double *time, const int32_t *clip_index,
		int clip, float *pose_out) {
	const unsigned blocks = (unsigned)((total_bones + kClipThreads - 1) / kClipThreads);
	const auto kernel = libm == LIBM_SSE2 ? mbik_clip_kernel<LIBM_SSE2> : mbik_clip_kernel<LIBM_FMA>;
	hipLaunchKernelGGL(kernel, dim3(blocks), dim3(kClipThreads), 0, st, v, total_bones, time, clip_index, clip, pose_out);
	return hipGetLastError();
}

} // namespace mbik
