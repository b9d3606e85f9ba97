// mbik_skin_vertices_listed's kernels: k_skin.hip's driven by a device-resident list of skeletons and
// its device-resident count (skin_list.h).
//
// The block's body is the same skin_dev.h's skin_block: 256 threads, `vlanes` vertex lanes by 256 / vlanes
// slot groups, one vertex in registers looped over the tile's slots, the same per-vertex calls into skin.h
// and morph.h.  What differs is what a tile is: a block owns S consecutive list ENTRIES, r0 .. r0 + S.
//   - Every block reads list_count[0] first, at a uniform address, and a block whose first entry is
//     at or past n = min(max(list_count[0], 0), max_list) returns before it touches LDS: the grid is
//     sized on the host from max_list, and a short list costs those exits only.
//   - Lane l of every wave loads entry r0 + l (S <= 64) and tests it against [0, count) itself -- the
//     list is device data no host has seen; an entry that fails becomes -1.  The entries stay in that
//     register: the staging asks for them by __shfl, the skinning loop, whose tile slot is uniform
//     in a wave, by v_readlane.  No LDS is spent on them, so the per-skeleton footprint is k_skin.hip's
//     and MBIK_SKIN_MAX_BONES and the shaped limit hold unchanged.
//   - Staging is a gather (lds_gather_runs): entry r's matrices are the run skin + indices[r] * B * 12,
//     its shape weights the run shape_weights + indices[r] * P, landing where k_skin.hip puts them.  P
//     floats of shape weights a run have no alignment of their own; lds_gather_runs moves them as quads
//     when P is a multiple of 4 and as dwords otherwise.
//   - An entry outside [0, count) is neither staged nor linked (morph_link_skipped) nor skinned.
//   - The output row is the entry's skeleton, or with `compact` its place in the list: a select on
//     wave-uniform values by a kernel argument, not a template parameter.
#include <mutex>

#include "skin_dev.h"

namespace {
using namespace mbik;

struct ListTile {
	int64_t r0;  // the tile's first list entry
	int nt;      // its entries, 0: nothing to do
	int entry;   // lane l of every wave: the skeleton of entry r0 + l, or -1 (past the tile, or outside [0, count))
	int compact; // the kernel argument

	__device__ __forceinline__ int slots() const { return nt; }
	// (s uniform in the wave)
	__device__ __forceinline__ int entry_of(int s) const { return __builtin_amdgcn_readlane(entry, __builtin_amdgcn_readfirstlane(s)); }
	__device__ __forceinline__ static bool skipped(int e) { return e < 0; }
	__device__ __forceinline__ int64_t row(int s, int e) const { return compact ? r0 + s : (int64_t)e; }
	__device__ __forceinline__ void stage(float *lds, const float *__restrict__ g, int items, int width) const {
		const int n = items * width;
#ifdef MBIK_LIST_CONTIGUOUS // A/B build: k_skin.hip's copy of one run; right for the list 0, 1, 2, ... only.
		// (Since the kernels share this stage() the switch also reaches the shaped kernels' weights, which always gathered before.)
		lds_copy_runs<true, kSkinThreads>(lds, 0, g + r0 * n, nt * n, 1);
#else
		lds_gather_runs<kSkinThreads>(lds, n, g, n, nt, [&](int r) { return (int64_t)__shfl(entry, r); });
#endif
	}
	// (S <= 64: thread s of the first wave holds slot s's entry; an unstaged slot is not linked)
	__device__ __forceinline__ void link(float *wlds, int P) const {
		if ((int)threadIdx.x < nt && entry >= 0) morph_link_skipped(wlds + threadIdx.x * P, P);
	}
};

// (every thread of the block, before any divergence)
__device__ __forceinline__ ListTile list_tile(int count, int S, const int32_t *__restrict__ indices,
		const int32_t *__restrict__ list_count, int max_list, int compact) {
	ListTile t;
	const int n = min(max(list_count[0], 0), max_list);
	t.r0 = (int64_t)blockIdx.x * S;
	t.nt = (int)max((int64_t)0, min((int64_t)S, (int64_t)n - t.r0));
	t.entry = -1;
	t.compact = compact;
	const int lane = threadIdx.x & 63;
	if (lane < t.nt) {
		const int s = indices[t.r0 + lane];
		if (s >= 0 && s < count) t.entry = s;
	}
	return t;
}

// The waves a SIMD each kernel is compiled for.  Left to itself the scheduler settles on 65 / 103 VGPRs (plain, K = 4 / 8)
// and up to 130 (shaped, K = 8) -- 4 waves where k_skin.hip's kernels run 7 -- although nothing here needs them; with the
// target stated it stays within it without scratch.  The targets are k_skin.hip's occupancies, one wave fewer for the
// plain kernels: the entry register, the list position and the skip branch cost a few registers, and at 8 / 7 waves the
// plain kernels spill.
constexpr int list_waves(int K, bool nrm, bool shaped) { return shaped ? (K == 4 ? (nrm ? 6 : 7) : 5) : (K == 4 ? 7 : 6); }

// k_skin.hip's two argument lists with the list's in front of the outputs
template <int K, bool NRM>
__global__ __launch_bounds__(kSkinThreads) __attribute__((amdgpu_waves_per_eu(list_waves(K, NRM, false))))
void mbik_skin_list_kernel(int count, int B, int V, int S, int chunk, int vshift,
		const float4 *__restrict__ m_pos, const float4 *__restrict__ m_nrm, const uint2 *__restrict__ m_idx,
		const float4 *__restrict__ m_wgt, int64_t wplane, const float *__restrict__ skin, const int32_t *__restrict__ indices,
		const int32_t *__restrict__ list_count, int max_list, int compact, float *__restrict__ out_p, float *__restrict__ out_n) {
	extern __shared__ __attribute__((aligned(16))) float skin_lds[];
	skin_block<K, skin_tier(NRM, false), kNoShapes>(list_tile(count, S, indices, list_count, max_list, compact), skin_lds, B, V, 0, S, chunk, vshift, m_pos,
			m_nrm, m_idx, m_wgt, nullptr, nullptr, wplane, skin, nullptr, out_p, out_n);
}

template <int K, bool NRM, int MODE>
__global__ __launch_bounds__(kSkinThreads) __attribute__((amdgpu_waves_per_eu(list_waves(K, NRM, true))))
void mbik_skin_list_shaped_kernel(int count, int B, int V, int P, int S, int chunk, int vshift,
		const float4 *__restrict__ m_pos, const float4 *__restrict__ m_nrm, const uint2 *__restrict__ m_idx,
		const float4 *__restrict__ m_wgt, const float4 *__restrict__ m_spos, const float4 *__restrict__ m_snrm, int64_t wplane,
		const float *__restrict__ skin, const float *__restrict__ shape_weights, const int32_t *__restrict__ indices,
		const int32_t *__restrict__ list_count, int max_list, int compact, float *__restrict__ out_p, float *__restrict__ out_n) {
	extern __shared__ __attribute__((aligned(16))) float skin_lds[];
	skin_block<K, skin_tier(NRM, false), MODE>(list_tile(count, S, indices, list_count, max_list, compact), skin_lds, B, V, P, S, chunk, vshift, m_pos, m_nrm,
			m_idx, m_wgt, m_spos, m_snrm, wplane, skin, shape_weights, out_p, out_n);
}

// The tangent tier: k_skin.hip's two tangent argument lists with the list's in front of the outputs.
// The plain kernels' targets are one wave under the normals tier's: the tangent and its sign are four registers more.  The
// shaped ones are compiled for 4 waves: with 5 the relative K = 4 kernel came out at 96 VGPRs and one spilled register, with 4
// it takes 97 and none; the normalized K = 4 one stays at 83, which runs 5 waves all the same.
constexpr int list_tan_waves(int K, bool shaped) { return shaped ? 4 : list_waves(K, true, shaped) - 1; }

template <int K>
__global__ __launch_bounds__(kSkinThreads) __attribute__((amdgpu_waves_per_eu(list_tan_waves(K, false))))
void mbik_skin_list_tan_kernel(int count, int B, int V, int S, int chunk, int vshift,
		const float4 *__restrict__ m_pos, const float4 *__restrict__ m_nrm, const float4 *__restrict__ m_tan,
		const uint2 *__restrict__ m_idx, const float4 *__restrict__ m_wgt, int64_t wplane, const float *__restrict__ skin,
		const int32_t *__restrict__ indices, const int32_t *__restrict__ list_count, int max_list, int compact,
		float *__restrict__ out_p, float *__restrict__ out_n, float *__restrict__ out_t) {
	extern __shared__ __attribute__((aligned(16))) float skin_lds[];
	skin_block<K, SKIN_TANGENTS, kNoShapes>(list_tile(count, S, indices, list_count, max_list, compact), skin_lds, B, V, 0, S, chunk, vshift,
			m_pos, m_nrm, m_idx, m_wgt, nullptr, nullptr, wplane, skin, nullptr, out_p, out_n, SkinTangents{m_tan, nullptr, out_t});
}

template <int K, int MODE>
__global__ __launch_bounds__(kSkinThreads) __attribute__((amdgpu_waves_per_eu(list_tan_waves(K, true))))
void mbik_skin_list_tan_shaped_kernel(int count, int B, int V, int P, int S, int chunk, int vshift,
		const float4 *__restrict__ m_pos, const float4 *__restrict__ m_nrm, const float4 *__restrict__ m_tan,
		const uint2 *__restrict__ m_idx, const float4 *__restrict__ m_wgt, const float4 *__restrict__ m_spos,
		const float4 *__restrict__ m_snrm, const float4 *__restrict__ m_stan, int64_t wplane, const float *__restrict__ skin,
		const float *__restrict__ shape_weights, const int32_t *__restrict__ indices, const int32_t *__restrict__ list_count,
		int max_list, int compact, float *__restrict__ out_p, float *__restrict__ out_n, float *__restrict__ out_t) {
	extern __shared__ __attribute__((aligned(16))) float skin_lds[];
	skin_block<K, SKIN_TANGENTS, MODE>(list_tile(count, S, indices, list_count, max_list, compact), skin_lds, B, V, P, S, chunk, vshift, m_pos,
			m_nrm, m_idx, m_wgt, m_spos, m_snrm, wplane, skin, shape_weights, out_p, out_n, SkinTangents{m_tan, m_stan, out_t});
}

struct ListKernels {
	template <int K, int TIER, int MODE>
	static auto kernel() {
		if constexpr (TIER == SKIN_TANGENTS) {
			if constexpr (MODE == kNoShapes) return &mbik_skin_list_tan_kernel<K>;
			else return &mbik_skin_list_tan_shaped_kernel<K, MODE>;
		} else {
			constexpr bool NRM = TIER == SKIN_NORMALS;
			if constexpr (MODE == kNoShapes) return &mbik_skin_list_kernel<K, NRM>;
			else return &mbik_skin_list_shaped_kernel<K, NRM, MODE>;
		}
	}
};
} // namespace

namespace mbik {

hipError_t launch_skin_listed(const SkinLaunch &a) {
	static std::once_flag once;
	std::call_once(once, skin_set_lds_limits<ListKernels>);
	if (a.S < 1 || a.S > 64 || a.max_list < 1) return hipErrorInvalidValue; // (a wave's lanes hold the tile's entries)
	return skin_launch<ListKernels>(a, a.max_list, a.indices, a.list_count, a.max_list, a.compact ? 1 : 0);
}

} // namespace mbik
