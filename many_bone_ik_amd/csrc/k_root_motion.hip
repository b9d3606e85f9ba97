// mbik_clip_root_motion[_layers]' and mbik_root_motion_apply's kernels: AnimationMixer's root motion
// for a crowd -- the root bone's change over the frame per skeleton, and its composition into the
// skeleton's world transform (root_motion.h).
//
// Extraction, the plain call and a layered call with one layer: one thread per skeleton,
// kRootThreads skeletons a block (two or more layers: the lanes kernel below).  A block is one wave, so a
// crowd of a few thousand skeletons still spreads over as many compute units as it has waves.
// Unlike the pose samplers every lane reads the same bone's few tracks: the header, key-time and
// key-value loads of a wave fall into a handful of cache lines.  The layers are walked in a loop
// over named state (K is a run-time value; a per-thread array indexed by it would live in
// scratch), layer l + 1's record, previous time, clip info and headers are loaded before layer
// l's keys are searched, both ends of a segment search in step and load their keys together, and
// the second segment of a layer that crossed the seam sits behind a per-lane branch -- few lanes
// wrap in any one frame.  A lane builds its 10 floats in LDS and the block's records leave as one
// contiguous run of motion_out through lds_copy_runs.  The same lane puts the rest pose's root
// record into `pose`, when given, for a skeleton whose clip indices are valid.
//
// The kernels test every clip index before they touch a table (the records are device data the
// host never sees), and no key index: mbik_clipset_create has checked every table (host_clip.cpp).
#include "kernels.h"
#include "lds_copy.h"
#include "root_motion.h"

#include <type_traits>

namespace {
using namespace mbik;

constexpr int kRootThreads = 64;

// LV: the set's libm_variant, a compile-time constant of sin_f.  PLAIN: one (time, clip, 1.0f)
// record a skeleton from time / clip_index / clip, flags 0; else [count][K] records.  CUBIC: the
// set has a cubic pose track (clip.h); a set without runs the <.., false> kernels.
template <int LV, bool PLAIN, bool CUBIC>
__global__ __launch_bounds__(kRootThreads) void mbik_root_motion_kernel(ClipView v, int count, int K, int root, const ClipLayer *layers,
		const double *time_prev, const double *time, const int32_t *clip_index, int clip, uint32_t flags, float *motion_out, float *pose) {
	__shared__ __attribute__((aligned(16))) float Ml[kRootThreads * 10];
	const int64_t s0 = (int64_t)blockIdx.x * kRootThreads;
	const int n = (int)min((int64_t)kRootThreads, (int64_t)count - s0);
	if (n <= 0) return;
	const int t = threadIdx.x;
	if (t < n) {
		const int64_t s = s0 + t;
		float *pose_s = pose ? pose + s * v.B * 10 : nullptr;
		if constexpr (PLAIN) {
			const RootPlain src{ClipLayer{time[s], clip_index ? clip_index[s] : clip, 1.0f}, time_prev[s]};
			root_motion_skeleton<CUBIC>(v, src, 1, 0u, root, LV, Ml + t * 10, pose_s);
		} else {
			const RootLayers src{layers + s * K, time_prev + s * K};
			root_motion_skeleton<CUBIC>(v, src, K, flags, root, LV, Ml + t * 10, pose_s);
		}
	}
	__syncthreads();
	lds_copy_runs<false, kRootThreads>(Ml, 0, motion_out + s0 * 10, n * 10, 1);
}

// The layered form with a lane per (skeleton, layer): a block owns 64 / K skeletons, lane t layer
// t % K of skeleton t / K.  What a lane of the form above waits for is the chain of dependent loads
// of one layer after the other -- record, headers, the search steps, the keys -- so K layers cost K
// chains; here the K chains of a skeleton run side by side.  A lane publishes its layer's validity,
// clamped weight and tracked channels in LDS; after a barrier every lane adds up its skeleton's
// totals from them (ascending, as the spec orders the sum), computes its layer's one or two steps
// (root_layer_steps: the searches, the lerps and all three slerps) and leaves them in LDS; after a
// second barrier the skeleton's first lane adds the steps up in layer order -- the order is part of
// the spec, so the sums stay on one lane: two products and a normalisation a step -- and stores the
// record.  20 floats and a word of LDS a lane.  (-DMBIK_ROOT_LANE_PER_LAYER=0: A/B builds, §24.)
#ifndef MBIK_ROOT_LANE_PER_LAYER
#define MBIK_ROOT_LANE_PER_LAYER 1
#endif
constexpr int kStepFloats = 21; // meta word, then two steps of e (4), dp (3), ds (3); odd, so lanes fall into distinct banks

__device__ __forceinline__ void put_step(float *p, const RootStep &r) {
	p[0] = r.e.x, p[1] = r.e.y, p[2] = r.e.z, p[3] = r.e.w;
	p[4] = r.dp.x, p[5] = r.dp.y, p[6] = r.dp.z, p[7] = r.ds.x, p[8] = r.ds.y, p[9] = r.ds.z;
}
__device__ __forceinline__ RootStep get_step(const float *p) {
	return RootStep{q4(p[0], p[1], p[2], p[3]), v3(p[4], p[5], p[6]), v3(p[7], p[8], p[9])};
}

template <int LV, bool CUBIC>
__global__ __launch_bounds__(kRootThreads) void mbik_root_motion_lanes_kernel(ClipView v, int count, int K, int root, const ClipLayer *layers,
		const double *time_prev, uint32_t flags, float *motion_out, float *pose) {
	__shared__ __attribute__((aligned(16))) float Ml[kRootThreads * 10];
	__shared__ float Wl[kRootThreads];        // the layer's clamped weight
	__shared__ int Fl[kRootThreads];          // 1 position, 2 rotation, 4 scale tracked; 8: an index outside the set
	__shared__ float Sl[kRootThreads * kStepFloats];
	const int per_block = kRootThreads / K;
	const int64_t s0 = (int64_t)blockIdx.x * per_block;
	const int n = (int)min((int64_t)per_block, (int64_t)count - s0);
	if (n <= 0) return;
	const int t = threadIdx.x, sl = t / K, l = t - sl * K;
	const bool active = sl < n;
	const int64_t s = s0 + sl;
	ClipLayer rec{0.0, kClipLayerOff, 0.0f};
	double t0 = 0.0;
	ClipLayerHeaders h = clip_layer_headers(v, kClipLayerOff, root);
	ClipInfo info{1.0, 0, 0};
	bool on = false;
	if (active) {
		rec = layers[s * K + l];
		t0 = time_prev[s * K + l];
		const bool outside = rec.clip != kClipLayerOff && (rec.clip < 0 || rec.clip >= v.clip_count);
		on = rec.clip != kClipLayerOff && !outside;
		if (on) { // the index is tested: the tables may be read
			h = clip_layer_headers(v, rec.clip, root);
			info = v.clips[rec.clip];
		}
		Wl[t] = clip_layer_weight(rec.weight);
		Fl[t] = outside ? 8 : (h.pos.key_count ? 1 : 0) | (h.rot.key_count ? 2 : 0) | (h.scl.key_count ? 4 : 0);
	}
	__syncthreads();
	bool valid = true;
	if (active) {
		const bool normalize = (flags & kClipLayersNormalize) != 0;
		float tot_pos = 0.0f, tot_rot = 0.0f, tot_scl = 0.0f;
		for (int j = 0; j < K; j++) {
			const int f = Fl[sl * K + j];
			const float w = Wl[sl * K + j];
			valid = valid && !(f & 8);
			if (normalize && (f & 1)) tot_pos = tot_pos + w;
			if (normalize && (f & 2)) tot_rot = tot_rot + w;
			if (normalize && (f & 4)) tot_scl = tot_scl + w;
		}
		float *mine = Sl + t * kStepFloats;
		int meta = 0;
		if (valid && on) {
			const RootLayerSteps ls = root_layer_steps<CUBIC>(v, info, h, t0, rec.time, rec.weight, normalize, tot_pos, tot_rot, tot_scl, LV);
			meta = ls.segments | (ls.do_pos ? 4 : 0) | (ls.do_rot ? 8 : 0) | (ls.do_scl ? 16 : 0);
			if (ls.segments > 0) put_step(mine + 1, ls.first);
			if (ls.segments > 1) put_step(mine + 11, ls.second);
		}
		mine[0] = __int_as_float(meta);
	}
	__syncthreads();
	if (active && l == 0) {
		float *out10 = Ml + sl * 10;
		if (!valid) {
			for (int f = 0; f < 10; f++) out10[f] = clip_nan();
		} else {
			RootAcc a = root_acc_start();
			for (int j = 0; j < K; j++) {
				const float *theirs = Sl + (sl * K + j) * kStepFloats;
				const int meta = __float_as_int(theirs[0]);
				const bool do_pos = meta & 4, do_rot = meta & 8, do_scl = meta & 16;
				if ((meta & 3) > 0) root_add(a, get_step(theirs + 1), do_pos, do_rot, do_scl);
				if ((meta & 3) > 1) root_add(a, get_step(theirs + 11), do_pos, do_rot, do_scl);
			}
			root_store(a, out10);
			if (pose) {
				const float *rest = v.rest + (int64_t)root * 10;
				float *p = pose + (s * v.B + root) * 10;
#pragma unroll
				for (int f = 0; f < 10; f++) p[f] = rest[f];
			}
		}
	}
	__syncthreads();
	lds_copy_runs<false, kRootThreads>(Ml, 0, motion_out + s0 * 10, n * 10, 1);
}

constexpr int kApplyThreads = 64;

// One thread per skeleton: 40 bytes in, 48 bytes in and out.
__global__ __launch_bounds__(kApplyThreads) void mbik_root_apply_kernel(int count, const float *motion, uint32_t flags, float *skeleton_global) {
	const int64_t s = (int64_t)blockIdx.x * kApplyThreads + (int64_t)threadIdx.x;
	if (s >= count) return;
	float m[10], G[12];
	const float *mp = motion + s * 10;
	float *gp = skeleton_global + s * 12;
#pragma unroll
	for (int f = 0; f < 10; f++) m[f] = mp[f];
#pragma unroll
	for (int f = 0; f < 12; f++) G[f] = gp[f];
	root_motion_apply(m, flags, G);
#pragma unroll
	for (int f = 0; f < 12; f++) gp[f] = G[f];
}
} // namespace

namespace mbik {

hipError_t launch_root_motion(hipStream_t st, const ClipView &v, int libm, bool cubic, int count, int layer_count, int root, const ClipLayer *layers,
		const double *time_prev, const double *time, const int32_t *clip_index, int clip, uint32_t flags, float *motion_out, float *pose) {
	const bool sse2 = libm == LIBM_SSE2;
	if (MBIK_ROOT_LANE_PER_LAYER && layers && layer_count > 1) {
		const int per_block = kRootThreads / layer_count;
		const unsigned blocks = (unsigned)(((int64_t)count + per_block - 1) / per_block);
		const auto kernel = cubic ? (sse2 ? mbik_root_motion_lanes_kernel<LIBM_SSE2, true> : mbik_root_motion_lanes_kernel<LIBM_FMA, true>)
								  : (sse2 ? mbik_root_motion_lanes_kernel<LIBM_SSE2, false> : mbik_root_motion_lanes_kernel<LIBM_FMA, false>);
		hipLaunchKernelGGL(kernel, dim3(blocks), dim3(kRootThreads), 0, st, v, count, layer_count, root, layers, time_prev, flags, motion_out, pose);
		return hipGetLastError();
	}
	const unsigned blocks = (unsigned)(((int64_t)count + kRootThreads - 1) / kRootThreads);
	const auto plain = [&](auto c) {
		constexpr bool CUBIC = decltype(c)::value;
		return layers ? (sse2 ? mbik_root_motion_kernel<LIBM_SSE2, false, CUBIC> : mbik_root_motion_kernel<LIBM_FMA, false, CUBIC>)
					  : (sse2 ? mbik_root_motion_kernel<LIBM_SSE2, true, CUBIC> : mbik_root_motion_kernel<LIBM_FMA, true, CUBIC>);
	};
	const auto kernel = cubic ? plain(std::true_type{}) : plain(std::false_type{});
	hipLaunchKernelGGL(kernel, dim3(blocks), dim3(kRootThreads), 0, st, v, count, layer_count, root, layers, time_prev, time, clip_index, clip,
			flags, motion_out, pose);
	return hipGetLastError();
}

hipError_t launch_root_apply(hipStream_t st, int count, const float *motion, uint32_t flags, float *skeleton_global) {
	const unsigned blocks = (unsigned)(((int64_t)count + kApplyThreads - 1) / kApplyThreads);
	hipLaunchKernelGGL(mbik_root_apply_kernel, dim3(blocks), dim3(kApplyThreads), 0, st, count, motion, flags, skeleton_global);
	return hipGetLastError();
}

} // namespace mbik
