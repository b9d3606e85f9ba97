// mbik_clip_sample_layers' kernel: AnimationMixer's blend of up to 8 clips a skeleton, each at its
// own time with its own weight, accumulated onto the rest pose (clip_layers.h).
//
// k_clip.hip's shape: one thread per bone; a block owns kClipLayersThreads consecutive bones of the
// batch, whatever skeletons they belong to.  A lane builds its bone's 10 floats in LDS, and the
// block's records leave as one contiguous run of pose_out through lds_copy_runs.  The inputs are
// 16 bytes a layer and the clip set's tables, which stay in L2.  The layers are walked in a loop
// over named state -- K is uniform over the launch but not a compile-time constant, and a
// per-thread array indexed by it would live in scratch.  The loop loads layer l + 1's record, clip
// info and three headers before it consumes layer l's search steps, so a lane has two layers'
// loads in flight; what bounds the sampler is the rate of its own L2 requests (§16), not
// arithmetic.  The slerp, the lerps and every key load sit behind per-lane branches: a layer that
// is off, untracked or weighted zero -- most layers of a crowd that is not mid-transition -- costs
// its record and headers only.
//
// The kernel tests every clip index before it touches a table (the records are device data the
// host never sees), and no key index: mbik_clipset_create has checked every table (host_clip.cpp).
#include "clip_layers.h"
#include "kernels.h"
#include "lds_copy.h"

namespace {
using namespace mbik;

constexpr int kClipLayersThreads = 256;

// LV: the set's libm_variant (gd::LIBM_FMA / LIBM_SSE2), a compile-time constant of sin_f.
// (An occupancy target of 4 waves a SIMD holds the allocation at 128 VGPRs without a spill, and
// measured the same time as the 136-140 VGPRs and 3 waves the compiler picks on its own: §20.)
template <int LV>
__global__ __launch_bounds__(kClipLayersThreads) void mbik_clip_layers_kernel(ClipView v, int64_t total, const ClipLayer *layers, int K,
		uint32_t flags, float *pose_out) {
	__shared__ __attribute__((aligned(16))) float Pl[kClipLayersThreads * 10];
	const int64_t b0 = (int64_t)blockIdx.x * kClipLayersThreads;
	const int n = (int)min((int64_t)kClipLayersThreads, total - b0);
	if (n <= 0) return;
	const int t = threadIdx.x;
	if (t < n) {
		// the skeleton of bone b0 + t: the block's first skeleton (uniform) plus a 32-bit quotient
		const uint32_t B = (uint32_t)v.B;
		const int64_t s0 = b0 / v.B;
		const uint32_t r = (uint32_t)(b0 - s0 * v.B) + (uint32_t)t, q = r / B;
		const int64_t s = s0 + q;
		clip_layers_bone(v, layers + s * K, K, flags, (int)(r - q * B), LV, Pl + t * 10);
	}
	__syncthreads();
	lds_copy_runs<false, kClipLayersThreads>(Pl, 0, pose_out + b0 * 10, n * 10, 1);
}
} // namespace

namespace mbik {

hipError_t launch_clip_layers(hipStream_t st, const ClipView &v, int libm, int64_t total_bones, const ClipLayer *layers, int layer_count,
		uint32_t flags, float *pose_out) {
	const unsigned blocks = (unsigned)((total_bones + kClipLayersThreads - 1) / kClipLayersThreads);
	const auto kernel = libm == LIBM_SSE2 ? mbik_clip_layers_kernel<LIBM_SSE2> : mbik_clip_layers_kernel<LIBM_FMA>;
	hipLaunchKernelGGL(kernel, dim3(blocks), dim3(kClipLayersThreads), 0, st, v, total_bones, layers, layer_count, flags, pose_out);
	return hipGetLastError();
}

} // namespace mbik
