// mbik_skin_vertices_listed's kernels: k_skin.hip's two kernels driven by a device-resident list of
// skeletons and its device-resident count (skin_list.h).
//
// The block is k_skin.hip's: 256 threads, `vlanes` vertex lanes by 256 / vlanes skeleton groups, one
// vertex in registers looped over the tile's skeletons, the same per-vertex calls into skin.h and
// morph.h.  What differs is what a tile is: a block owns S consecutive list ENTRIES, r0 .. r0 + S.
//   - Every block reads list_count[0] first, at a uniform address, and a block whose first entry is
//     at or past n = min(max(list_count[0], 0), max_list) returns before it touches LDS: the grid is
//     sized on the host from max_list, and a short list costs those exits only.
//   - Lane l of every wave loads entry r0 + l (S <= 64) and tests it against [0, count) itself -- the
//     list is device data no host has seen; an entry that fails becomes -1.  The entries stay in that
//     register: the staging asks for them by __shfl, the skinning loop, whose tile slot is uniform
//     in a wave, by v_readlane.  No LDS is spent on them, so the per-skeleton footprint is k_skin.hip's
//     and MBIK_SKIN_MAX_BONES and the shaped limit hold unchanged.
//   - Staging is a gather (lds_gather_runs): entry r's matrices are the run skin + indices[r] * B * 12,
//     its shape weights the run shape_weights + indices[r] * P, landing where k_skin.hip puts them.
//   - An entry outside [0, count) is neither staged nor linked (morph_link_skipped) nor skinned.
//   - The output row is the entry's skeleton, or with `compact` its place in the list: a select on
//     wave-uniform values by a kernel argument, not a template parameter.
#include <mutex>

#include "kernels.h"
#include "lds_copy.h"
#include "morph.h"
#include "skin.h"
#include "skin_dev.h"

namespace {
using namespace mbik;

struct ListTile {
	int64_t r0; // the tile's first list entry
	int nt;     // its entries, 0: nothing to do
	int entry;  // lane l of every wave: the skeleton of entry r0 + l, or -1 (past the tile, or outside [0, count))
};

// (every thread of the block, before any divergence)
__device__ __forceinline__ ListTile list_tile(int count, int S, const int32_t *__restrict__ indices,
		const int32_t *__restrict__ list_count, int max_list) {
	ListTile t;
	const int n = min(max(list_count[0], 0), max_list);
	t.r0 = (int64_t)blockIdx.x * S;
	t.nt = (int)max((int64_t)0, min((int64_t)S, (int64_t)n - t.r0));
	t.entry = -1;
	const int lane = threadIdx.x & 63;
	if (lane < t.nt) {
		const int s = indices[t.r0 + lane];
		if (s >= 0 && s < count) t.entry = s;
	}
	return t;
}

// the skeleton of tile slot s, s uniform in the wave (-1: skipped)
__device__ __forceinline__ int list_entry(const ListTile &t, int s) {
	return __builtin_amdgcn_readlane(t.entry, __builtin_amdgcn_readfirstlane(s));
}

// The waves a SIMD each kernel is compiled for.  Left to itself the scheduler settles on 65 / 103 VGPRs (plain, K = 4 / 8)
// and up to 130 (shaped, K = 8) -- 4 waves where k_skin.hip's kernels run 7 -- although nothing here needs them; with the
// target stated it stays within it without scratch.  The targets are k_skin.hip's occupancies, one wave fewer for the
// plain kernels: the entry register, the list position and the skip branch cost a few registers, and at 8 / 7 waves the
// plain kernels spill.
constexpr int list_waves(int K, bool nrm, bool shaped) { return shaped ? (K == 4 ? (nrm ? 6 : 7) : 5) : (K == 4 ? 7 : 6); }

template <int K, bool NRM>
__global__ __launch_bounds__(kSkinThreads) __attribute__((amdgpu_waves_per_eu(list_waves(K, NRM, false))))
void mbik_skin_list_kernel(int count, int B, int V, int S, int chunk, int vshift,
		const float4 *__restrict__ m_pos, const float4 *__restrict__ m_nrm, const uint2 *__restrict__ m_idx,
		const float4 *__restrict__ m_wgt, int64_t wplane, const float *__restrict__ skin, const int32_t *__restrict__ indices,
		const int32_t *__restrict__ list_count, int max_list, int compact, float *__restrict__ out_p, float *__restrict__ out_n) {
	extern __shared__ __attribute__((aligned(16))) float skin_lds[];
	const ListTile t = list_tile(count, S, indices, list_count, max_list);
	const int v0 = (int)min((int64_t)blockIdx.y * chunk, (int64_t)V);
	const int v1 = (int)min((int64_t)v0 + chunk, (int64_t)V);
	if (t.nt <= 0 || v0 >= v1) return;
#ifdef MBIK_LIST_CONTIGUOUS // A/B build: k_skin.hip's copy of one run; right for the list 0, 1, 2, ... only
	lds_copy_runs<true, kSkinThreads>(skin_lds, 0, skin + t.r0 * B * 12, t.nt * B * 12, 1);
#else
	lds_gather_runs<kSkinThreads>(skin_lds, B * 12, skin, B * 12, t.nt, [&](int r) { return (int64_t)__shfl(t.entry, r); });
#endif
	__syncthreads();

	const int vlanes = 1 << vshift, sgroups = kSkinThreads >> vshift;
	const int vt = threadIdx.x & (vlanes - 1), sg = threadIdx.x >> vshift;
	const float4 *lds4 = reinterpret_cast<const float4 *>(skin_lds);
	for (int v = v0 + vt; v < v1; v += vlanes) {
		const float4 p4 = m_pos[v];
		const V3 pos = v3(p4.x, p4.y, p4.z);
		V3 nrm = v3(0, 0, 0);
		if constexpr (NRM) {
			const float4 n4 = m_nrm[v];
			nrm = v3(n4.x, n4.y, n4.z);
		}
		int q[K];
		float w[K];
#pragma unroll
		for (int h = 0; h < K / 4; h++) {
			const uint2 iv = m_idx[(int64_t)v * (K / 4) + h];
			q[4 * h + 0] = (int)(iv.x & 0xffffu) * 3, q[4 * h + 1] = (int)(iv.x >> 16) * 3;
			q[4 * h + 2] = (int)(iv.y & 0xffffu) * 3, q[4 * h + 3] = (int)(iv.y >> 16) * 3;
			const float4 wv = m_wgt[h * wplane + v];
			w[4 * h + 0] = wv.x, w[4 * h + 1] = wv.y, w[4 * h + 2] = wv.z, w[4 * h + 3] = wv.w;
		}
		for (int s = sg; s < t.nt; s += sgroups) {
			const int e = list_entry(t, s);
			if (e < 0) continue;
			const float4 *ms = lds4 + s * B * 3;
			X3 m = skin_scaled(skin_load_lds(ms + q[0]), w[0]);
#pragma unroll
			for (int k = 1; k < K; k++) m = skin_accumulate(m, skin_load_lds(ms + q[k]), w[k]);
			const int64_t row = compact ? t.r0 + s : (int64_t)e;
			const int64_t at = (row * V + v) * 3;
			skin_store3(out_p + at, skin_position(m, pos));
			if constexpr (NRM) skin_store3(out_n + at, skin_normal(m, nrm));
		}
	}
}

// The shaped form: k_skin.hip's mbik_skin_shaped_kernel on the same tile.  P floats of shape weights a
// run have no alignment of their own; lds_gather_runs moves them as quads when P is a multiple of 4
// and as dwords otherwise.
template <int K, bool NRM, int MODE>
__global__ __launch_bounds__(kSkinThreads) __attribute__((amdgpu_waves_per_eu(list_waves(K, NRM, true))))
void mbik_skin_list_shaped_kernel(int count, int B, int V, int P, int S, int chunk, int vshift, const float4 *__restrict__ m_pos, const float4 *__restrict__ m_nrm, const uint2 *__restrict__ m_idx,
		const float4 *__restrict__ m_wgt, const float4 *__restrict__ m_spos, const float4 *__restrict__ m_snrm, int64_t wplane,
		const float *__restrict__ skin, const float *__restrict__ shape_weights, const int32_t *__restrict__ indices,
		const int32_t *__restrict__ list_count, int max_list, int compact, float *__restrict__ out_p, float *__restrict__ out_n) {
	extern __shared__ __attribute__((aligned(16))) float skin_lds[];
	const ListTile t = list_tile(count, S, indices, list_count, max_list);
	const int v0 = (int)min((int64_t)blockIdx.y * chunk, (int64_t)V);
	const int v1 = (int)min((int64_t)v0 + chunk, (int64_t)V);
	if (t.nt <= 0 || v0 >= v1) return;
	float *wlds = skin_lds + S * B * 12;
	const auto src = [&](int r) { return (int64_t)__shfl(t.entry, r); };
	lds_gather_runs<kSkinThreads>(skin_lds, B * 12, skin, B * 12, t.nt, src);
	lds_gather_runs<kSkinThreads>(wlds, P, shape_weights, P, t.nt, src);
	__syncthreads();
	// (S <= 64: thread s of the first wave holds slot s's entry; an unstaged slot is not linked)
	if ((int)threadIdx.x < t.nt && t.entry >= 0) morph_link_skipped(wlds + threadIdx.x * P, P);
	__syncthreads();

	const int vlanes = 1 << vshift, sgroups = kSkinThreads >> vshift;
	const int vt = threadIdx.x & (vlanes - 1), sg = threadIdx.x >> vshift;
	const float4 *lds4 = reinterpret_cast<const float4 *>(skin_lds);
	for (int v = v0 + vt; v < v1; v += vlanes) {
		const float4 p4 = m_pos[v];
		const V3 pos0 = v3(p4.x, p4.y, p4.z);
		V3 nrm0 = v3(0, 0, 0);
		if constexpr (NRM) {
			const float4 n4 = m_nrm[v];
			nrm0 = v3(n4.x, n4.y, n4.z);
		}
		int q[K];
		float w[K];
#pragma unroll
		for (int h = 0; h < K / 4; h++) {
			const uint2 iv = m_idx[(int64_t)v * (K / 4) + h];
			q[4 * h + 0] = (int)(iv.x & 0xffffu) * 3, q[4 * h + 1] = (int)(iv.x >> 16) * 3;
			q[4 * h + 2] = (int)(iv.y & 0xffffu) * 3, q[4 * h + 3] = (int)(iv.y >> 16) * 3;
			const float4 wv = m_wgt[h * wplane + v];
			w[4 * h + 0] = wv.x, w[4 * h + 1] = wv.y, w[4 * h + 2] = wv.z, w[4 * h + 3] = wv.w;
		}
		const float4 *sp = m_spos + v, *sn = m_snrm + v;
		for (int s = sg; s < t.nt; s += sgroups) {
			const int e = list_entry(t, s);
			if (e < 0) continue;
			const float *cs = wlds + s * P;
			V3 pos = pos0, nrm = nrm0;
			float4 rn = make_float4(0, 0, 0, 0);
			morph_vertex<NRM>(
					MODE, P, [&](int j) { return __builtin_bit_cast(float, __builtin_amdgcn_readfirstlane(__builtin_bit_cast(int, cs[j]))); },
					[](int, float c) { return morph_link(c); },
					// (both records are requested before the first is waited for, as in k_skin.hip)
					[&](int j) {
						const float4 r = sp[j * wplane];
						if constexpr (NRM) {
							rn = sn[j * wplane];
							__builtin_amdgcn_sched_barrier(0);
						}
						return v3(r.x, r.y, r.z);
					},
					[&](int) { return v3(rn.x, rn.y, rn.z); },
					pos, nrm);
			const float4 *ms = lds4 + s * B * 3;
			X3 m = skin_scaled(skin_load_lds(ms + q[0]), w[0]);
#pragma unroll
			for (int k = 1; k < K; k++) m = skin_accumulate(m, skin_load_lds(ms + q[k]), w[k]);
			const int64_t row = compact ? t.r0 + s : (int64_t)e;
			const int64_t at = (row * V + v) * 3;
			skin_store3(out_p + at, skin_position(m, pos));
			if constexpr (NRM) skin_store3(out_n + at, skin_normal(m, nrm));
		}
	}
}

template <int K, bool NRM>
void set_lds_limit() {
	(void)hipFuncSetAttribute((const void *)mbik_skin_list_kernel<K, NRM>, hipFuncAttributeMaxDynamicSharedMemorySize, kSkinMaxLdsBytes);
}
template <int K, bool NRM, int MODE>
void set_shaped_lds_limit() {
	(void)hipFuncSetAttribute((const void *)mbik_skin_list_shaped_kernel<K, NRM, MODE>, hipFuncAttributeMaxDynamicSharedMemorySize,
			kSkinMaxLdsBytes);
}

struct ListArgs {
	hipStream_t st;
	dim3 grid;
	size_t lds;
	int count, B, V, P, S, chunk, vshift;
	const unsigned char *mesh;
	SkinLayout l;
	MorphLayout ml;
	const float *skin, *shape_weights;
	const int32_t *indices, *list_count;
	int max_list, compact;
	float *out_p, *out_n;
};

template <int K, bool NRM>
void list_launch(const ListArgs &a) {
	const int64_t wplane = ((int64_t)a.V + 1) & ~(int64_t)1;
	hipLaunchKernelGGL((mbik_skin_list_kernel<K, NRM>), a.grid, dim3(kSkinThreads), a.lds, a.st, a.count, a.B, a.V, a.S, a.chunk,
			a.vshift, reinterpret_cast<const float4 *>(a.mesh + a.l.pos), NRM ? reinterpret_cast<const float4 *>(a.mesh + a.l.nrm) : nullptr,
			reinterpret_cast<const uint2 *>(a.mesh + a.l.idx), reinterpret_cast<const float4 *>(a.mesh + a.l.wgt), wplane, a.skin,
			a.indices, a.list_count, a.max_list, a.compact, a.out_p, a.out_n);
}
template <int K, bool NRM, int MODE>
void list_shaped_launch(const ListArgs &a) {
	hipLaunchKernelGGL((mbik_skin_list_shaped_kernel<K, NRM, MODE>), a.grid, dim3(kSkinThreads), a.lds, a.st, a.count, a.B, a.V, a.P,
			a.S, a.chunk, a.vshift, reinterpret_cast<const float4 *>(a.mesh + a.l.pos),
			NRM ? reinterpret_cast<const float4 *>(a.mesh + a.l.nrm) : nullptr, reinterpret_cast<const uint2 *>(a.mesh + a.l.idx),
			reinterpret_cast<const float4 *>(a.mesh + a.l.wgt), reinterpret_cast<const float4 *>(a.mesh + a.ml.pos),
			NRM ? reinterpret_cast<const float4 *>(a.mesh + a.ml.nrm) : nullptr, a.ml.stride, a.skin, a.shape_weights, a.indices,
			a.list_count, a.max_list, a.compact, a.out_p, a.out_n);
}
template <int K, bool NRM>
void list_launch_any(int mode, const ListArgs &a) {
	if (!a.shape_weights) list_launch<K, NRM>(a);
	else if (mode == MORPH_NORMALIZED) list_shaped_launch<K, NRM, MORPH_NORMALIZED>(a);
	else list_shaped_launch<K, NRM, MORPH_RELATIVE>(a);
}
} // namespace

namespace mbik {

hipError_t launch_skin_listed(hipStream_t st, int K, int mode, int count, int B, int V, int P, int S, int chunk, int chunks, int vshift,
		const unsigned char *mesh, bool mesh_normals, const float *skin, const float *shape_weights, const int32_t *indices,
		const int32_t *list_count, int max_list, bool compact, float *out_p, float *out_n) {
	static std::once_flag once;
	std::call_once(once, [] {
		set_lds_limit<4, false>(), set_lds_limit<4, true>(), set_lds_limit<8, false>(), set_lds_limit<8, true>();
		set_shaped_lds_limit<4, false, 0>(), set_shaped_lds_limit<4, true, 0>(), set_shaped_lds_limit<8, false, 0>();
		set_shaped_lds_limit<8, true, 0>(), set_shaped_lds_limit<4, false, 1>(), set_shaped_lds_limit<4, true, 1>();
		set_shaped_lds_limit<8, false, 1>(), set_shaped_lds_limit<8, true, 1>();
	});
	if (S < 1 || S > 64 || max_list < 1) return hipErrorInvalidValue; // (a wave's lanes hold the tile's entries)
	ListArgs a;
	a.st = st, a.grid = dim3((unsigned)(((int64_t)max_list + S - 1) / S), (unsigned)chunks);
	a.lds = shape_weights ? (size_t)S * (size_t)morph_lds_bytes(B, P) : (size_t)S * B * 12 * sizeof(float);
	a.count = count, a.B = B, a.V = V, a.P = P, a.S = S, a.chunk = chunk, a.vshift = vshift, a.mesh = mesh;
	a.l = skin_layout(V, K, mesh_normals), a.ml = shape_weights ? morph_layout(V, K, mesh_normals, P) : MorphLayout{};
	a.skin = skin, a.shape_weights = shape_weights, a.indices = indices, a.list_count = list_count;
	a.max_list = max_list, a.compact = compact ? 1 : 0, a.out_p = out_p, a.out_n = out_n;
	if (K == 4) {
		if (out_n) list_launch_any<4, true>(mode, a);
		else list_launch_any<4, false>(mode, a);
	} else {
		if (out_n) list_launch_any<8, true>(mode, a);
		else list_launch_any<8, false>(mode, a);
	}
	return hipGetLastError();
}

} // namespace mbik
