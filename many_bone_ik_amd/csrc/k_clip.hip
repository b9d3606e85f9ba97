// mbik_clip_sample's and mbik_clip_sample_layers' kernels, two per-bone calls in one frame.
//
// mbik_clip_sample: Godot's Animation track interpolation for a batch of skeletons, each at its own
// time in its own clip (clip.h).
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
//
// mbik_clip_sample_layers: AnimationMixer's blend of up to 8 clips a skeleton, each at its own time
// with its own weight, accumulated onto the rest pose (clip_layers.h).
//
// The same frame.  The inputs are 16 bytes a layer and the clip set's tables, which stay in L2.
// The layers are walked in a loop over named state -- K is uniform over the launch but not a
// compile-time constant, and a per-thread array indexed by it would live in scratch.  The loop
// loads layer l + 1's record, clip info and three headers before it consumes layer l's search
// steps, so a lane has two layers' loads in flight; what bounds the sampler is the rate of its own
// L2 requests (§16), not arithmetic.  The slerp, the lerps and every key load sit behind per-lane
// branches: a layer that is off, untracked or weighted zero -- most layers of a crowd that is not
// mid-transition -- costs its record and headers only.
//
// The layered kernel tests every clip index before it touches a table (the records are device data
// the host never sees), and no key index either.
#include "batch_lane.h"
#include "clip_layers.h"
#include "kernels.h"
#include "lds_copy.h"

namespace {
using namespace mbik;

constexpr int kClipThreads = 256;

// The frame: per_bone(skeleton, bone, out) builds one bone's record in the block's LDS tile.
template <class PerBone>
__device__ __forceinline__ void clip_frame(int B, int64_t total, float *pose_out, PerBone per_bone) {
	__shared__ __attribute__((aligned(16))) float Pl[kClipThreads * 10];
	const int64_t b0 = (int64_t)blockIdx.x * kClipThreads;
	const int n = (int)min((int64_t)kClipThreads, total - b0);
	if (n <= 0) return;
	const int t = threadIdx.x;
	if (t < n) {
		const BatchLane ln = batch_lane(B, b0, t);
		per_bone(ln.s, ln.item, Pl + t * 10);
	}
	__syncthreads();
	lds_copy_runs<false, kClipThreads>(Pl, 0, pose_out + b0 * 10, n * 10, 1);
}

// LV: the set's libm_variant (gd::LIBM_FMA / LIBM_SSE2), a compile-time constant of sin_f.
// CUBIC: the set has a cubic pose track (clip.h); a set without runs the <LV, false>
// kernels, which are what they were before cubic tracks existed.
template <int LV, bool CUBIC>
__global__ __launch_bounds__(kClipThreads) void mbik_clip_kernel(ClipView v, int64_t total, const double *time, const int32_t *clip_index,
		int clip, float *pose_out) {
	clip_frame(v.B, total, pose_out,
			[&](int64_t s, int bone, float *out) { clip_sample_bone<CUBIC>(v, clip_index ? clip_index[s] : clip, bone, time[s], LV, out); });
}

// (An occupancy target of 4 waves a SIMD holds the allocation at 128 VGPRs without a spill, and
// measured the same time as the 136-140 VGPRs and 3 waves the compiler picks on its own: §20.)
template <int LV, bool CUBIC>
__global__ __launch_bounds__(kClipThreads) void mbik_clip_layers_kernel(ClipView v, int64_t total, const ClipLayer *layers, int K,
		uint32_t flags, float *pose_out) {
	clip_frame(v.B, total, pose_out, [&](int64_t s, int bone, float *out) { clip_layers_bone<CUBIC>(v, layers + s * K, K, flags, bone, LV, out); });
}
} // namespace

namespace mbik {

hipError_t launch_clip(hipStream_t st, const ClipView &v, int libm, bool cubic, int64_t total_bones, const double *time, const int32_t *clip_index,
		int clip, float *pose_out) {
	const unsigned blocks = (unsigned)((total_bones + kClipThreads - 1) / kClipThreads);
	const auto kernel = cubic ? (libm == LIBM_SSE2 ? mbik_clip_kernel<LIBM_SSE2, true> : mbik_clip_kernel<LIBM_FMA, true>)
							  : (libm == LIBM_SSE2 ? mbik_clip_kernel<LIBM_SSE2, false> : mbik_clip_kernel<LIBM_FMA, false>);
	hipLaunchKernelGGL(kernel, dim3(blocks), dim3(kClipThreads), 0, st, v, total_bones, time, clip_index, clip, pose_out);
	return hipGetLastError();
}

hipError_t launch_clip_layers(hipStream_t st, const ClipView &v, int libm, bool cubic, int64_t total_bones, const ClipLayer *layers, int layer_count,
		uint32_t flags, float *pose_out) {
	const unsigned blocks = (unsigned)((total_bones + kClipThreads - 1) / kClipThreads);
	const auto kernel = cubic ? (libm == LIBM_SSE2 ? mbik_clip_layers_kernel<LIBM_SSE2, true> : mbik_clip_layers_kernel<LIBM_FMA, true>)
							  : (libm == LIBM_SSE2 ? mbik_clip_layers_kernel<LIBM_SSE2, false> : mbik_clip_layers_kernel<LIBM_FMA, false>);
	hipLaunchKernelGGL(kernel, dim3(blocks), dim3(kClipThreads), 0, st, v, total_bones, layers, layer_count, flags, pose_out);
	return hipGetLastError();
}

} // namespace mbik
