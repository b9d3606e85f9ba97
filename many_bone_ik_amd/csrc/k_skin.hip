// mbik_skin_vertices' kernel: linear blend skinning of a mesh for a batch of skeletons (skin.h;
// DESIGN.md §14).
//
// A block owns S consecutive skeletons and one chunk of the vertex range.  The skeletons'
// matrices are one contiguous run of `skin` (S x B x 12 floats) and go into LDS as k_fk.hip's
// runs do (lds_copy.h); a bone's matrix then sits at 48 * b bytes, 16-byte aligned, and is read
// as three 16-byte quads.  At 12 dwords a bone the quads of any bone start on a multiple of 4
// banks and 3 is coprime to 16, so the bones spread over all sixteen 4-bank slots without padding;
// lanes that name the same bone broadcast.
//
// A thread keeps one vertex -- position, normal, K indices (as LDS quad offsets) and K weights --
// in registers and loops over the block's skeletons: K matrix reads, the blend, the transform,
// one 12-byte store per output (consecutive lanes are consecutive vertices: 768 contiguous
// bytes a wave).  Meshes with fewer vertices in a chunk than the block has threads give the
// spare waves other skeletons of the tile: the block is `vlanes` vertex lanes by 256 / vlanes
// skeleton groups, vlanes a multiple of the wave size, so a wave's skeleton is uniform.
//
// mbik_skin_vertices_shaped's kernel follows it: the same block with each skeleton's blend shapes
// applied to the vertex first (morph.h).
#include <mutex>

#include "kernels.h"
#include "lds_copy.h"
#include "morph.h"
#include "skin.h"
#include "skin_dev.h"

namespace {
using namespace mbik;

template <int K, bool NRM>
__global__ __launch_bounds__(kSkinThreads) void mbik_skin_kernel(int count, int B, int V, int S, int chunk, int vshift,
		const float4 *__restrict__ m_pos, const float4 *__restrict__ m_nrm, const uint2 *__restrict__ m_idx,
		const float4 *__restrict__ m_wgt, int64_t wplane, const float *__restrict__ skin, float *__restrict__ out_p,
		float *__restrict__ out_n) {
	extern __shared__ __attribute__((aligned(16))) float skin_lds[];
	const int64_t s0 = (int64_t)blockIdx.x * S;
	const int ns = (int)min((int64_t)S, (int64_t)count - s0);
	const int v0 = (int)min((int64_t)blockIdx.y * chunk, (int64_t)V);
	const int v1 = (int)min((int64_t)v0 + chunk, (int64_t)V);
	if (ns <= 0 || v0 >= v1) return;
	lds_copy_runs<true, kSkinThreads>(skin_lds, 0, skin + s0 * B * 12, ns * B * 12, 1);
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
		// the bones' quad offsets inside one skeleton's LDS image, and the weights
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
		for (int s = sg; s < ns; s += sgroups) {
			const float4 *ms = lds4 + s * B * 3;
			X3 m = skin_scaled(skin_load_lds(ms + q[0]), w[0]);
#pragma unroll
			for (int k = 1; k < K; k++) m = skin_accumulate(m, skin_load_lds(ms + q[k]), w[k]);
			const int64_t at = ((s0 + s) * V + v) * 3;
			skin_store3(out_p + at, skin_position(m, pos));
			if constexpr (NRM) skin_store3(out_n + at, skin_normal(m, nrm));
		}
	}
}

// mbik_skin_vertices_shaped's kernel: blend shapes in front of the same blend and transform
// (morph.h).  Block and grid as above.  The tile's S x P shape weights are one
// contiguous run of `shape_weights` and are staged behind the S x B x 12 matrices.  Per vertex and
// skeleton the shapes are walked in ascending order in registers; a wave's skeleton is uniform, so
// the weight is read through readfirstlane and `fabsf(c) > 0.0001f` is a scalar branch that skips
// the shape's loads with its arithmetic.  Once staged, a skipped weight is overwritten by the index
// of the next active shape (morph_link_skipped), so the walk steps from active shape to active
// shape and a skeleton pays for its active shapes only, whatever P is.  Shape
// records are 16 bytes a lane, consecutive lanes consecutive vertices, shared by every skeleton.
template <int K, bool NRM, int MODE>
__global__ __launch_bounds__(kSkinThreads) void mbik_skin_shaped_kernel(int count, int B, int V, int P, int S, int chunk, int vshift,
		const float4 *__restrict__ m_pos, const float4 *__restrict__ m_nrm, const uint2 *__restrict__ m_idx,
		const float4 *__restrict__ m_wgt, const float4 *__restrict__ m_spos, const float4 *__restrict__ m_snrm, int64_t wplane,
		const float *__restrict__ skin, const float *__restrict__ shape_weights, float *__restrict__ out_p,
		float *__restrict__ out_n) {
	extern __shared__ __attribute__((aligned(16))) float skin_lds[];
	const int64_t s0 = (int64_t)blockIdx.x * S;
	const int ns = (int)min((int64_t)S, (int64_t)count - s0);
	const int v0 = (int)min((int64_t)blockIdx.y * chunk, (int64_t)V);
	const int v1 = (int)min((int64_t)v0 + chunk, (int64_t)V);
	if (ns <= 0 || v0 >= v1) return;
	float *wlds = skin_lds + S * B * 12;
	lds_copy_runs<true, kSkinThreads>(skin_lds, 0, skin + s0 * B * 12, ns * B * 12, 1);
	lds_copy_runs<true, kSkinThreads>(wlds, 0, shape_weights + s0 * P, ns * P, 1);
	__syncthreads();
#ifndef MBIK_MORPH_SCAN // A/B build: every vertex walks all P weights of its skeleton
	for (int s = threadIdx.x; s < ns; s += kSkinThreads) morph_link_skipped(wlds + s * P, P);
	__syncthreads();
#endif

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
		for (int s = sg; s < ns; s += sgroups) {
			const float *cs = wlds + s * P;
			V3 pos = pos0, nrm = nrm0;
			float4 rn = make_float4(0, 0, 0, 0);
			morph_vertex<NRM>(
					MODE, P, [&](int j) { return __builtin_bit_cast(float, __builtin_amdgcn_readfirstlane(__builtin_bit_cast(int, cs[j]))); },
#ifndef MBIK_MORPH_SCAN
					[](int, float c) { return morph_link(c); },
#else
					[](int j, float) { return j + 1; },
#endif
					// (both records are requested before the first is waited for: the scheduler otherwise
					// puts the position's arithmetic, and its wait, in front of the normal's load)
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
			const int64_t at = ((s0 + s) * V + v) * 3;
			skin_store3(out_p + at, skin_position(m, pos));
			if constexpr (NRM) skin_store3(out_n + at, skin_normal(m, nrm));
		}
	}
}

template <int K, bool NRM>
void skin_set_lds_limit() {
	(void)hipFuncSetAttribute((const void *)mbik_skin_kernel<K, NRM>, hipFuncAttributeMaxDynamicSharedMemorySize, kSkinMaxLdsBytes);
}

template <int K, bool NRM>
void skin_launch(hipStream_t st, dim3 grid, size_t lds, int count, int B, int V, int S, int chunk, int vshift, const unsigned char *mesh,
		const SkinLayout &l, const float *skin, float *out_p, float *out_n) {
	const int64_t wplane = ((int64_t)V + 1) & ~(int64_t)1;
	hipLaunchKernelGGL((mbik_skin_kernel<K, NRM>), grid, dim3(kSkinThreads), lds, st, count, B, V, S, chunk, vshift,
			reinterpret_cast<const float4 *>(mesh + l.pos), NRM ? reinterpret_cast<const float4 *>(mesh + l.nrm) : nullptr,
			reinterpret_cast<const uint2 *>(mesh + l.idx), reinterpret_cast<const float4 *>(mesh + l.wgt), wplane, skin, out_p, out_n);
}

template <int K, bool NRM, int MODE>
void skin_shaped_set_lds_limit() {
	(void)hipFuncSetAttribute((const void *)mbik_skin_shaped_kernel<K, NRM, MODE>, hipFuncAttributeMaxDynamicSharedMemorySize,
			kSkinMaxLdsBytes);
}

struct ShapedArgs {
	hipStream_t st;
	dim3 grid;
	size_t lds;
	int count, B, V, P, S, chunk, vshift;
	const unsigned char *mesh;
	SkinLayout l;
	MorphLayout ml;
	const float *skin, *shape_weights;
	float *out_p, *out_n;
};

template <int K, bool NRM, int MODE>
void skin_shaped_launch(const ShapedArgs &a) {
	hipLaunchKernelGGL((mbik_skin_shaped_kernel<K, NRM, MODE>), a.grid, dim3(kSkinThreads), a.lds, a.st, a.count, a.B, a.V, a.P, a.S,
			a.chunk, a.vshift, reinterpret_cast<const float4 *>(a.mesh + a.l.pos),
			NRM ? reinterpret_cast<const float4 *>(a.mesh + a.l.nrm) : nullptr, reinterpret_cast<const uint2 *>(a.mesh + a.l.idx),
			reinterpret_cast<const float4 *>(a.mesh + a.l.wgt), reinterpret_cast<const float4 *>(a.mesh + a.ml.pos),
			NRM ? reinterpret_cast<const float4 *>(a.mesh + a.ml.nrm) : nullptr, a.ml.stride, a.skin, a.shape_weights, a.out_p, a.out_n);
}
template <int K, bool NRM>
void skin_shaped_launch_mode(int mode, const ShapedArgs &a) {
	if (mode == MORPH_NORMALIZED) skin_shaped_launch<K, NRM, MORPH_NORMALIZED>(a);
	else skin_shaped_launch<K, NRM, MORPH_RELATIVE>(a);
}
} // namespace

namespace mbik {

hipError_t launch_skin(hipStream_t st, int K, int count, int B, int V, int S, int chunk, int chunks, int vshift,
		const unsigned char *mesh, bool mesh_normals, const float *skin, float *out_p, float *out_n) {
	static std::once_flag once;
	std::call_once(once, [] {
		skin_set_lds_limit<4, false>(), skin_set_lds_limit<4, true>(), skin_set_lds_limit<8, false>(), skin_set_lds_limit<8, true>();
	});
	const SkinLayout l = skin_layout(V, K, mesh_normals);
	const size_t lds = (size_t)S * B * 12 * sizeof(float);
	const dim3 grid((unsigned)(((int64_t)count + S - 1) / S), (unsigned)chunks);
	if (K == 4) {
		if (out_n) skin_launch<4, true>(st, grid, lds, count, B, V, S, chunk, vshift, mesh, l, skin, out_p, out_n);
		else skin_launch<4, false>(st, grid, lds, count, B, V, S, chunk, vshift, mesh, l, skin, out_p, out_n);
	} else {
		if (out_n) skin_launch<8, true>(st, grid, lds, count, B, V, S, chunk, vshift, mesh, l, skin, out_p, out_n);
		else skin_launch<8, false>(st, grid, lds, count, B, V, S, chunk, vshift, mesh, l, skin, out_p, out_n);
	}
	return hipGetLastError();
}

hipError_t launch_skin_shaped(hipStream_t st, int K, int mode, int count, int B, int V, int P, int S, int chunk, int chunks, int vshift,
		const unsigned char *mesh, bool mesh_normals, const float *skin, const float *shape_weights, float *out_p, float *out_n) {
	static std::once_flag once;
	std::call_once(once, [] {
		skin_shaped_set_lds_limit<4, false, 0>(), skin_shaped_set_lds_limit<4, true, 0>(), skin_shaped_set_lds_limit<8, false, 0>();
		skin_shaped_set_lds_limit<8, true, 0>(), skin_shaped_set_lds_limit<4, false, 1>(), skin_shaped_set_lds_limit<4, true, 1>();
		skin_shaped_set_lds_limit<8, false, 1>(), skin_shaped_set_lds_limit<8, true, 1>();
	});
	ShapedArgs a;
	a.st = st, a.grid = dim3((unsigned)(((int64_t)count + S - 1) / S), (unsigned)chunks);
	a.lds = (size_t)S * (size_t)morph_lds_bytes(B, P);
	a.count = count, a.B = B, a.V = V, a.P = P, a.S = S, a.chunk = chunk, a.vshift = vshift, a.mesh = mesh;
	a.l = skin_layout(V, K, mesh_normals), a.ml = morph_layout(V, K, mesh_normals, P);
	a.skin = skin, a.shape_weights = shape_weights, a.out_p = out_p, a.out_n = out_n;
	if (K == 4) {
		if (out_n) skin_shaped_launch_mode<4, true>(mode, a);
		else skin_shaped_launch_mode<4, false>(mode, a);
	} else {
		if (out_n) skin_shaped_launch_mode<8, true>(mode, a);
		else skin_shaped_launch_mode<8, false>(mode, a);
	}
	return hipGetLastError();
}

} // namespace mbik
