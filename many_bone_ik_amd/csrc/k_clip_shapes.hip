// mbik_clip_sample_shapes' and mbik_clip_sample_shapes_layers' kernels: the blend-shape tracks of a
// clip set sampled -- and layered as AnimationMixer layers them -- for a batch of skeletons, into
// the [count][P] weights mbik_skin_vertices_shaped reads (clip_shapes.h).
//
// One thread per (skeleton, shape); a block owns kShapeThreads consecutive weights of the batch,
// whatever skeletons they belong to, as k_clip.hip's blocks own bones.  A lane's result is one
// float at the lane's own consecutive address, so the store is a plain coalesced vector store and
// there is no LDS.  The inputs are 12 bytes a skeleton (or 16 bytes a layer) and the set's shape
// tables, which every skeleton shares and which stay in L2.  A lane's dependent rounds of loads:
// the time and clip index (or the layer record); the clip's info and the shape's header; the
// search, one 8-byte load a step; two 16-byte key records that carry both times and both values.
// The layered kernel walks its K layers in a loop over named state -- K is uniform over the launch
// but not a compile-time constant -- and loads layer l + 1's record, info and header before it
// searches layer l's keys.  There is no slerp, so no libm variant.
//
// The kernels test every clip index before they touch a table (the indices are device data the
// host never sees), and no key index: mbik_clipset_create_shaped has checked every table.
#include "batch_lane.h"
#include "clip_shapes.h"
#include "kernels.h"

namespace {
using namespace mbik;

constexpr int kShapeThreads = 256;

// CUBIC: the set has a cubic shape track (clip_shapes.h); a set without runs the
// <false> kernels, which are what they were before cubic tracks existed.
template <bool CUBIC>
__global__ __launch_bounds__(kShapeThreads) void mbik_clip_shapes_kernel(ShapeView v, int64_t total, const double *time,
		const int32_t *clip_index, int clip, float *weights_out) {
	const int64_t b0 = (int64_t)blockIdx.x * kShapeThreads;
	const int t = threadIdx.x;
	if (b0 + t >= total) return;
	const BatchLane ln = batch_lane(v.P, b0, t);
	weights_out[b0 + t] = shape_sample<CUBIC>(v, clip_index ? clip_index[ln.s] : clip, ln.item, time[ln.s]);
}

template <bool CUBIC>
__global__ __launch_bounds__(kShapeThreads) void mbik_clip_shapes_layers_kernel(ShapeView v, int64_t total, const ClipLayer *layers, int K,
		uint32_t flags, float *weights_out) {
	const int64_t b0 = (int64_t)blockIdx.x * kShapeThreads;
	const int t = threadIdx.x;
	if (b0 + t >= total) return;
	const BatchLane ln = batch_lane(v.P, b0, t);
	weights_out[b0 + t] = shape_layers<CUBIC>(v, layers + ln.s * K, K, flags, ln.item);
}
} // namespace

namespace mbik {

hipError_t launch_clip_shapes(hipStream_t st, const ShapeView &v, bool cubic, int64_t total_weights, const double *time, const int32_t *clip_index,
		int clip, float *weights_out) {
	const unsigned blocks = (unsigned)((total_weights + kShapeThreads - 1) / kShapeThreads);
	hipLaunchKernelGGL(cubic ? mbik_clip_shapes_kernel<true> : mbik_clip_shapes_kernel<false>, dim3(blocks), dim3(kShapeThreads), 0, st, v, total_weights, time, clip_index, clip,
			weights_out);
	return hipGetLastError();
}

hipError_t launch_clip_shapes_layers(hipStream_t st, const ShapeView &v, bool cubic, int64_t total_weights, const ClipLayer *layers, int layer_count,
		uint32_t flags, float *weights_out) {
	const unsigned blocks = (unsigned)((total_weights + kShapeThreads - 1) / kShapeThreads);
	hipLaunchKernelGGL(cubic ? mbik_clip_shapes_layers_kernel<true> : mbik_clip_shapes_layers_kernel<false>, dim3(blocks), dim3(kShapeThreads), 0, st, v, total_weights, layers, layer_count, flags,
			weights_out);
	return hipGetLastError();
}

} // namespace mbik
