// mbik_skin_vertices' and mbik_skin_vertices_shaped's kernels: linear blend skinning of a mesh for a
// batch of skeletons (skin.h), with each skeleton's blend shapes applied to the vertex
// first in the shaped form (morph.h).
//
// The block's body is skin_dev.h's skin_block, shared with k_skin_list.hip; this file says what a tile
// is here.  A block owns S consecutive skeletons and one chunk of the vertex range.  The skeletons'
// matrices are one contiguous run of `skin` (S x B x 12 floats) and go into LDS as k_fk.hip's runs do
// (lds_copy.h); the tile's S x P shape weights are one contiguous run of `shape_weights` likewise.  At
// 12 dwords a bone the quads of any bone start on a multiple of 4 banks and 3 is coprime to 16, so the
// bones spread over all sixteen 4-bank slots without padding; lanes that name the same bone broadcast.
//
// A thread loops over the block's skeletons with one vertex in registers: the shape walk, K matrix
// reads, the blend, the transform, one 12-byte store per output (consecutive lanes are consecutive
// vertices: 768 contiguous bytes a wave), and in the tangent tier one 16-byte store more.  Meshes with fewer vertices in a chunk than the block has
// threads give the spare waves other skeletons of the tile.
#include <mutex>

#include "skin_dev.h"

namespace {
using namespace mbik;

// S consecutive skeletons from s0, the last tile fewer; none is skipped and a skeleton writes its own row
struct RangeTile {
	int64_t s0;
	int ns;
	__device__ __forceinline__ int slots() const { return ns; }
	__device__ __forceinline__ static int entry_of(int s) { return s; }
	__device__ __forceinline__ static bool skipped(int) { return false; }
	__device__ __forceinline__ int64_t row(int s, int) const { return s0 + s; }
	__device__ __forceinline__ void stage(float *lds, const float *__restrict__ g, int items, int width) const {
		lds_copy_runs<true, kSkinThreads>(lds, 0, g + s0 * items * width, ns * items * width, 1);
	}
	__device__ __forceinline__ void link(float *wlds, int P) const {
		for (int s = threadIdx.x; s < ns; s += kSkinThreads) morph_link_skipped(wlds + s * P, P);
	}
};

__device__ __forceinline__ RangeTile range_tile(int count, int S) {
	const int64_t s0 = (int64_t)blockIdx.x * S;
	return RangeTile{s0, (int)min((int64_t)S, (int64_t)count - s0)};
}

// Two entry points, for their argument lists: the plain kernels take no shape arguments (with the
// shaped list they compile to the same loop behind 32 more bytes of arguments, and the plain call at
// C2 measured 0.8 % slower).
template <int K, bool NRM>
__global__ __launch_bounds__(kSkinThreads) void mbik_skin_kernel(int count, int B, int V, int S, int chunk, int vshift,
		const float4 *__restrict__ m_pos, const float4 *__restrict__ m_nrm, const uint2 *__restrict__ m_idx,
		const float4 *__restrict__ m_wgt, int64_t wplane, const float *__restrict__ skin, float *__restrict__ out_p,
		float *__restrict__ out_n) {
	extern __shared__ __attribute__((aligned(16))) float skin_lds[];
	skin_block<K, skin_tier(NRM, false), kNoShapes>(range_tile(count, S), skin_lds, B, V, 0, S, chunk, vshift, m_pos, m_nrm, m_idx, m_wgt, nullptr, nullptr,
			wplane, skin, nullptr, out_p, out_n);
}

template <int K, bool NRM, int MODE>
__global__ __launch_bounds__(kSkinThreads) void mbik_skin_shaped_kernel(int count, int B, int V, int P, int S, int chunk, int vshift,
		const float4 *__restrict__ m_pos, const float4 *__restrict__ m_nrm, const uint2 *__restrict__ m_idx,
		const float4 *__restrict__ m_wgt, const float4 *__restrict__ m_spos, const float4 *__restrict__ m_snrm, int64_t wplane,
		const float *__restrict__ skin, const float *__restrict__ shape_weights, float *__restrict__ out_p,
		float *__restrict__ out_n) {
	extern __shared__ __attribute__((aligned(16))) float skin_lds[];
	skin_block<K, skin_tier(NRM, false), MODE>(range_tile(count, S), skin_lds, B, V, P, S, chunk, vshift, m_pos, m_nrm, m_idx, m_wgt, m_spos, m_snrm, wplane,
			skin, shape_weights, out_p, out_n);
}

// The tangent tier (mbik_skin_vertices_call with out_tangents): the same two argument lists with
// the tangent planes behind the normals' and the third output last.
template <int K>
__global__ __launch_bounds__(kSkinThreads) void mbik_skin_tan_kernel(int count, int B, int V, int S, int chunk, int vshift,
		const float4 *__restrict__ m_pos, const float4 *__restrict__ m_nrm, const float4 *__restrict__ m_tan,
		const uint2 *__restrict__ m_idx, const float4 *__restrict__ m_wgt, int64_t wplane, const float *__restrict__ skin,
		float *__restrict__ out_p, float *__restrict__ out_n, float *__restrict__ out_t) {
	extern __shared__ __attribute__((aligned(16))) float skin_lds[];
	skin_block<K, SKIN_TANGENTS, kNoShapes>(range_tile(count, S), skin_lds, B, V, 0, S, chunk, vshift, m_pos, m_nrm, m_idx, m_wgt, nullptr,
			nullptr, wplane, skin, nullptr, out_p, out_n, SkinTangents{m_tan, nullptr, out_t});
}

template <int K, int MODE>
__global__ __launch_bounds__(kSkinThreads) void mbik_skin_tan_shaped_kernel(int count, int B, int V, int P, int S, int chunk, int vshift,
		const float4 *__restrict__ m_pos, const float4 *__restrict__ m_nrm, const float4 *__restrict__ m_tan,
		const uint2 *__restrict__ m_idx, const float4 *__restrict__ m_wgt, const float4 *__restrict__ m_spos,
		const float4 *__restrict__ m_snrm, const float4 *__restrict__ m_stan, int64_t wplane, const float *__restrict__ skin,
		const float *__restrict__ shape_weights, float *__restrict__ out_p, float *__restrict__ out_n, float *__restrict__ out_t) {
	extern __shared__ __attribute__((aligned(16))) float skin_lds[];
	skin_block<K, SKIN_TANGENTS, MODE>(range_tile(count, S), skin_lds, B, V, P, S, chunk, vshift, m_pos, m_nrm, m_idx, m_wgt, m_spos, m_snrm,
			wplane, skin, shape_weights, out_p, out_n, SkinTangents{m_tan, m_stan, out_t});
}

struct RangeKernels {
	template <int K, int TIER, int MODE>
	static auto kernel() {
		if constexpr (TIER == SKIN_TANGENTS) {
			if constexpr (MODE == kNoShapes) return &mbik_skin_tan_kernel<K>;
			else return &mbik_skin_tan_shaped_kernel<K, MODE>;
		} else {
			constexpr bool NRM = TIER == SKIN_NORMALS;
			if constexpr (MODE == kNoShapes) return &mbik_skin_kernel<K, NRM>;
			else return &mbik_skin_shaped_kernel<K, NRM, MODE>;
		}
	}
};
} // namespace

namespace mbik {

hipError_t launch_skin(const SkinLaunch &a) {
	static std::once_flag once;
	std::call_once(once, skin_set_lds_limits<RangeKernels>);
	return skin_launch<RangeKernels>(a, a.count);
}

} // namespace mbik
