// mbik_playback_advance's kernel: AnimationPlayer for a crowd -- every skeleton's playback
// positions, cross-fades and clip-to-clip transitions one frame on, and the layer records and
// previous times the layered samplers and root motion read (playback.h).
//
// One thread per skeleton, kPlaybackThreads skeletons a block.  A block is one wave, so a crowd
// of a few thousand skeletons still spreads over as many compute units as it has waves.  The
// state is a structure of arrays in the object's memory ([K][capacity] a field), read and written
// in place: lane t's slot j lies next to lane t + 1's, so every load and store of a field is one
// run of the wave.  The slots are walked in a loop over named state (K is a run-time value; a
// per-thread array indexed by it would live in scratch), with a write cursor for the compaction.
// With more than one layer a lane builds its K records and K previous times in LDS and the
// block's [64][K] of each leave as one contiguous run through lds_copy_runs; with one layer
// consecutive lanes already store consecutive records.
//
// The kernel tests every field of a command before it uses it (the commands are device data the
// host never sees) and trusts the state, which only mbik_playback_write's checks and this kernel
// produce.
#include "kernels.h"
#include "lds_copy.h"
#include "playback.h"

namespace {
using namespace mbik;

constexpr int kPlaybackThreads = 64;

// A lane's K records and previous times in the block's LDS staging.
struct PlaybackStaged {
	ClipLayer *layers;
	double *prev;
	__device__ __forceinline__ void put(int j, const ClipLayer &rec, double time_prev) const { layers[j] = rec, prev[j] = time_prev; }
};

template <bool STAGED>
__global__ __launch_bounds__(kPlaybackThreads) void mbik_playback_kernel(PlaybackTables T, PlaybackState st, int count, int K, double delta,
		float speed_scale, const PlaybackCmd *cmds, int cmd_count, ClipLayer *layers_out, double *time_prev_out, uint8_t *events_out) {
	__shared__ __attribute__((aligned(16))) float Ll[STAGED ? kPlaybackThreads * kClipMaxLayers * 4 : 4];
	__shared__ __attribute__((aligned(16))) float Pl[STAGED ? kPlaybackThreads * kClipMaxLayers * 2 : 4];
	const int64_t s0 = (int64_t)blockIdx.x * kPlaybackThreads;
	const int n = (int)min((int64_t)kPlaybackThreads, (int64_t)count - s0);
	if (n <= 0) return;
	const int t = threadIdx.x;
	if (t < n) {
		const int64_t s = s0 + t;
		const PlaybackLane lane{st, s};
		uint32_t events;
		if constexpr (STAGED) {
			const PlaybackStaged out{reinterpret_cast<ClipLayer *>(Ll) + t * K, reinterpret_cast<double *>(Pl) + t * K};
			events = playback_skeleton(T, lane, K, (int)s, delta, speed_scale, cmds, cmd_count, out);
		} else {
			const PlaybackDirect out{layers_out + s, time_prev_out + s};
			events = playback_skeleton(T, lane, 1, (int)s, delta, speed_scale, cmds, cmd_count, out);
		}
		if (events_out) events_out[s] = (uint8_t)events;
	}
	if constexpr (STAGED) {
		__syncthreads();
		lds_copy_runs<false, kPlaybackThreads>(Ll, 0, reinterpret_cast<float *>(layers_out + s0 * K), n * K * 4, 1);
		lds_copy_runs<false, kPlaybackThreads>(Pl, 0, reinterpret_cast<float *>(time_prev_out + s0 * K), n * K * 2, 1);
	}
}
} // namespace

namespace mbik {

hipError_t launch_playback(hipStream_t st, const PlaybackTables &T, const PlaybackState &state, int count, int layer_count, double delta,
		float speed_scale, const PlaybackCmd *cmds, int cmd_count, ClipLayer *layers_out, double *time_prev_out, uint8_t *events_out) {
	const unsigned blocks = (unsigned)(((int64_t)count + kPlaybackThreads - 1) / kPlaybackThreads);
	const auto kernel = layer_count > 1 ? mbik_playback_kernel<true> : mbik_playback_kernel<false>;
	hipLaunchKernelGGL(kernel, dim3(blocks), dim3(kPlaybackThreads), 0, st, T, state, count, layer_count, delta, speed_scale, cmds, cmd_count,
			layers_out, time_prev_out, events_out);
	return hipGetLastError();
}

} // namespace mbik
