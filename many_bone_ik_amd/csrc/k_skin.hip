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
#include <mutex>

#include "kernels.h"
#include "lds_copy.h"
#include "skin.h"

namespace {
using namespace mbik;

constexpr int kSkinThreads = 256;

__device__ __forceinline__ X3 skin_load_lds(const float4 *m) {
	const float4 a = m[0], b = m[1], c = m[2];
	return X3{bset(a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w, c.x), v3(c.y, c.z, c.w)};
}

__device__ __forceinline__ void skin_store3(float *o, V3 p) {
#ifdef MBIK_SKIN_NT // A/B build: the outputs are written once and not read here
	__builtin_nontemporal_store(p.x, o), __builtin_nontemporal_store(p.y, o + 1), __builtin_nontemporal_store(p.z, o + 2);
#else
	o[0] = p.x, o[1] = p.y, o[2] = p.z;
#endif
}

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

} // namespace mbik
