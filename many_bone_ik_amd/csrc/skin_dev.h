// What the skinning kernel TUs (k_skin.hip, k_skin_list.hip) share, which is everything but what a
// tile is: the block size, one vertex in registers and its load, the shape step, and the block's body
// from the early return to the vertex loop with the blend and its 12-byte stores (skin_block); on the
// host side the K x tier x mode dispatch with the launch built on it.  The tier (skin.h's SkinTier) says
// what a vertex carries: the position, the normal with it, or the tangent with both.  A TU adds its tile policy
// and its __global__ entry points, which form the tile, call skin_block and carry the attributes that
// differ.
//
// A tile policy says
//   slots()            how many slots the tile has (<= 0: the block returns);
//   entry_of(s)        what the tile keeps for slot s, s uniform in the wave, and skipped(e) whether that
//                      says to leave the slot out (ListTile: the listed skeleton or -1; RangeTile keeps
//                      nothing, answers s and skips none);
//   row(s, e)          the output row slot s writes, asked behind the blend;
//   stage(lds, g, items, width)
//                      how the slots' runs of n = items x width floats (a slot's: g + its skeleton * n)
//                      get to lds + s * n;
//   link(wlds, P)      the link pass over the staged slots' weights (morph_link_skipped), a slot a
//                      thread; a slot that was not staged is not linked.
// Everything here is forced inline, and the 24 kernels of the first two tiers keep the registers of the
// hand-written loops they replace (profiles/skin_refactor_regs.json); the shaped ones keep their instruction
// counts too.  The tangent tier's 12 kernels are `if constexpr` additions to the same body and leave the 24
// as they were, instruction for instruction (profiles/skin_tangent_regs.json).
// Four things sit where they do for that (DESIGN.md §19 has the figures): a run's length comes as its
// two factors (RangeTile multiplies s0 * items * width in the hand-written order; the same loop three
// instructions further up measured 1.4 % slower at C5), the link pass is the tile's (shared as one
// counted loop it is 27 instructions more in the listed kernels), the row is asked for behind the blend
// (in front of it RangeTile's 64-bit sum costs the plain K = 8 normals kernel 2 VGPRs and a wave), and
// the blend stands in the loop itself (as a function of its own it costs the shaped K = 8 normalized
// positions-only kernel 5 VGPRs and a wave).
#pragma once
#include <hip/hip_runtime.h>

#include <type_traits>

#include "kernels.h"
#include "lds_copy.h"
#include "morph.h"
#include "skin.h"

namespace mbik {

constexpr int kSkinThreads = 256;
// MODE of the kernels without blend shapes; the others' is a MorphMode
constexpr int kNoShapes = -1;

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

// The tangent's 16 bytes a lane: x, y, z and the binormal sign, whose bits are only moved.  Four dword
// stores in the source, as skin_store3's three: the outputs need float alignment only, and the backend
// merges them into one global_store_dwordx4, 1,024 contiguous bytes a wave.
__device__ __forceinline__ void skin_store4(float *o, V3 p, float w) {
#ifdef MBIK_SKIN_NT
	__builtin_nontemporal_store(p.x, o), __builtin_nontemporal_store(p.y, o + 1), __builtin_nontemporal_store(p.z, o + 2);
	__builtin_nontemporal_store(w, o + 3);
#else
	o[0] = p.x, o[1] = p.y, o[2] = p.z, o[3] = w;
#endif
}

// The tangent tier's planes and output, null in the other tiers: m_tan the base tangents (x, y, z, w a
// vertex), m_stan the shape tangents of shape 0 (the next shape's wplane records on), out_t [rows][V][4].
struct SkinTangents {
	const float4 *__restrict__ m_tan = nullptr, *__restrict__ m_stan = nullptr;
	float *__restrict__ out_t = nullptr;
};

// One vertex as a thread keeps it: position, normal (zero without NRM), the bones' quad offsets inside
// one skeleton's LDS image, and the weights.
template <int K>
struct SkinVertex {
	V3 pos, nrm;
	int q[K];
	float w[K];
};

template <int K, bool NRM>
__device__ __forceinline__ SkinVertex<K> skin_load_vertex(const float4 *__restrict__ m_pos, const float4 *__restrict__ m_nrm,
		const uint2 *__restrict__ m_idx, const float4 *__restrict__ m_wgt, int64_t wplane, int v) {
	SkinVertex<K> x;
	const float4 p4 = m_pos[v];
	x.pos = v3(p4.x, p4.y, p4.z);
	x.nrm = v3(0, 0, 0);
	if constexpr (NRM) {
		const float4 n4 = m_nrm[v];
		x.nrm = v3(n4.x, n4.y, n4.z);
	}
#pragma unroll
	for (int h = 0; h < K / 4; h++) {
		const uint2 iv = m_idx[(int64_t)v * (K / 4) + h];
		x.q[4 * h + 0] = (int)(iv.x & 0xffffu) * 3, x.q[4 * h + 1] = (int)(iv.x >> 16) * 3;
		x.q[4 * h + 2] = (int)(iv.y & 0xffffu) * 3, x.q[4 * h + 3] = (int)(iv.y >> 16) * 3;
		const float4 wv = m_wgt[h * wplane + v];
		x.w[4 * h + 0] = wv.x, x.w[4 * h + 1] = wv.y, x.w[4 * h + 2] = wv.z, x.w[4 * h + 3] = wv.w;
	}
	return x;
}

// The shape step (morph.h): one skeleton's staged weights cs[0..P) walked in ascending
// order in registers, pos and nrm morphed in place.  A wave's skeleton is uniform, so the weight is
// read through readfirstlane and `fabsf(c) > 0.0001f` is a scalar branch that skips the shape's loads
// with its arithmetic; skin_link_weights has turned every skipped weight into the index of the next
// active shape, so the walk steps from active shape to active shape.  sp / sn: the vertex's record of
// shape 0, 16 bytes a lane, the next shape's wplane records on.
// st: the shape tangents likewise (tangent tier), requested with the other two records in front of the one barrier.
template <int TIER, int MODE>
__device__ __forceinline__ void skin_shape_vertex(int P, const float *cs, const float4 *__restrict__ sp, const float4 *__restrict__ sn,
		const float4 *__restrict__ st, int64_t wplane, V3 &pos, V3 &nrm, V3 &tan) {
	constexpr bool NRM = TIER >= SKIN_NORMALS, TAN = TIER >= SKIN_TANGENTS;
	float4 rn = make_float4(0, 0, 0, 0), rt = make_float4(0, 0, 0, 0);
	morph_vertex_tier<TIER>(
			MODE, P, [&](int j) { return __builtin_bit_cast(float, __builtin_amdgcn_readfirstlane(__builtin_bit_cast(int, cs[j]))); },
#ifndef MBIK_MORPH_SCAN
			[](int, float c) { return morph_link(c); },
#else // A/B build: every vertex walks all P weights of its skeleton
			[](int j, float) { return j + 1; },
#endif
			// (every record is requested before the first is waited for: the scheduler otherwise
			// puts the position's arithmetic, and its wait, in front of the normal's load)
			[&](int j) {
				const float4 r = sp[j * wplane];
				if constexpr (NRM) {
					rn = sn[j * wplane];
					if constexpr (TAN) rt = st[j * wplane];
					__builtin_amdgcn_sched_barrier(0);
				}
				return v3(r.x, r.y, r.z);
			},
			[&](int) { return v3(rn.x, rn.y, rn.z); }, [&](int) { return v3(rt.x, rt.y, rt.z); }, pos, nrm, tan);
}

// The staged weights of the tile's slots, P a slot, linked for skin_shape_vertex.  Every thread of the
// block calls it.
template <class Tile>
__device__ __forceinline__ void skin_link_weights(const Tile &t, float *wlds, int P) {
#ifndef MBIK_MORPH_SCAN
	t.link(wlds, P);
	__syncthreads();
#endif
}

// What a block does with its tile `t` and vertex chunk blockIdx.y.  The tile's matrices (B x 12 floats
// a slot) go into LDS, a bone's matrix then sits at 48 * b bytes, 16-byte aligned, and is read as three
// 16-byte quads; with shapes the tile's weights (P a slot) are staged behind the S x B x 12 matrices.
// The block is `vlanes` vertex lanes by 256 / vlanes slot groups, vlanes a multiple of the wave size,
// so a wave's slot is uniform; a thread keeps one vertex in registers and loops over its group's slots.
// tg: the tangent tier's planes and output; such a thread also keeps the base tangent, w in one register across the slot loop.
template <int K, int TIER, int MODE, class Tile>
__device__ __forceinline__ void skin_block(const Tile &t, float *skin_lds, int B, int V, int P, int S, int chunk, int vshift,
		const float4 *__restrict__ m_pos, const float4 *__restrict__ m_nrm, const uint2 *__restrict__ m_idx,
		const float4 *__restrict__ m_wgt, const float4 *__restrict__ m_spos, const float4 *__restrict__ m_snrm, int64_t wplane,
		const float *__restrict__ skin, const float *__restrict__ shape_weights, float *__restrict__ out_p, float *__restrict__ out_n,
		const SkinTangents tg = SkinTangents{}) {
	constexpr bool kShaped = MODE != kNoShapes, NRM = TIER >= SKIN_NORMALS, TAN = TIER >= SKIN_TANGENTS;
	const int v0 = (int)min((int64_t)blockIdx.y * chunk, (int64_t)V);
	const int v1 = (int)min((int64_t)v0 + chunk, (int64_t)V);
	if (t.slots() <= 0 || v0 >= v1) return;
	float *const wlds = kShaped ? skin_lds + S * B * 12 : nullptr;
	t.stage(skin_lds, skin, B, 12);
	if constexpr (kShaped) t.stage(wlds, shape_weights, P, 1);
	__syncthreads();
	if constexpr (kShaped) skin_link_weights(t, wlds, P);

	const int vlanes = 1 << vshift, sgroups = kSkinThreads >> vshift;
	const int vt = threadIdx.x & (vlanes - 1), sg = threadIdx.x >> vshift;
	const float4 *lds4 = reinterpret_cast<const float4 *>(skin_lds);
	for (int v = v0 + vt; v < v1; v += vlanes) {
		const SkinVertex<K> x = skin_load_vertex<K, NRM>(m_pos, m_nrm, m_idx, m_wgt, wplane, v);
		const float4 *const sp = kShaped ? m_spos + v : nullptr, *const sn = kShaped && NRM ? m_snrm + v : nullptr;
		float4 t4 = make_float4(0, 0, 0, 0);
		if constexpr (TAN) t4 = tg.m_tan[v];
		const float4 *st = nullptr;
		if constexpr (kShaped && TAN) st = tg.m_stan + v;
		for (int s = sg; s < t.slots(); s += sgroups) {
			const int e = t.entry_of(s);
			if (t.skipped(e)) continue;
			V3 pos = x.pos, nrm = x.nrm, tan = v3(t4.x, t4.y, t4.z);
			if constexpr (kShaped) skin_shape_vertex<TIER, MODE>(P, wlds + s * P, sp, sn, st, wplane, pos, nrm, tan);
			// K matrix reads from the slot's LDS image, the blend, the transform, one 12-byte store an output
			const float4 *ms = lds4 + s * B * 3;
			X3 m = skin_scaled(skin_load_lds(ms + x.q[0]), x.w[0]);
#pragma unroll
			for (int k = 1; k < K; k++) m = skin_accumulate(m, skin_load_lds(ms + x.q[k]), x.w[k]);
			const int64_t rv = t.row(s, e) * V + v, at = rv * 3;
			skin_store3(out_p + at, skin_position(m, pos));
			if constexpr (NRM) skin_store3(out_n + at, skin_normal(m, nrm));
			if constexpr (TAN) skin_store4(tg.out_t + rv * 4, skin_normal(m, tan), t4.w);
		}
	}
}

// ---------------- host side ----------------
template <int N>
using SkinInt = std::integral_constant<int, N>;

// The one K x tier x mode ladder: f(K, TIER, MODE) with the three as integral constants.
// tier: a SkinTier; mode: kNoShapes or a MorphMode.
template <class F>
void skin_dispatch(int K, int tier, int mode, F f) {
	const auto with_mode = [&](auto k, auto n) {
		if (mode == kNoShapes) f(k, n, SkinInt<kNoShapes>());
		else if (mode == MORPH_NORMALIZED) f(k, n, SkinInt<MORPH_NORMALIZED>());
		else f(k, n, SkinInt<MORPH_RELATIVE>());
	};
	const auto with_tier = [&](auto k) {
		if (tier == SKIN_TANGENTS) with_mode(k, SkinInt<SKIN_TANGENTS>());
		else if (tier == SKIN_NORMALS) with_mode(k, SkinInt<SKIN_NORMALS>());
		else with_mode(k, SkinInt<SKIN_POSITIONS>());
	};
	if (K == 4) with_tier(SkinInt<4>());
	else with_tier(SkinInt<8>());
}

// Kernels::kernel<K, TIER, MODE>() is a TU's __global__ entry point.  Every one of them may use the
// whole LDS (each TU, once, before its first launch).
template <class Kernels>
void skin_set_lds_limits() {
	for (int K : {4, 8})
		for (int tier : {(int)SKIN_POSITIONS, (int)SKIN_NORMALS, (int)SKIN_TANGENTS})
			for (int mode : {kNoShapes, (int)MORPH_RELATIVE, (int)MORPH_NORMALIZED})
				skin_dispatch(K, tier, mode, [](auto k, auto n, auto m) {
					(void)hipFuncSetAttribute((const void *)Kernels::template kernel<decltype(k)::value, decltype(n)::value, decltype(m)::value>(),
							hipFuncAttributeMaxDynamicSharedMemorySize, kSkinMaxLdsBytes);
				});
}

// The launch of `a` (kernels.h) over ceil(tiled / a.S) tiles x a.chunks vertex chunks: shaped when a.shape_weights is
// given, normals when a.out_n is, tangents when a.out_t is.  A TU's entry points take the plain or the shaped argument
// list, then `extra`, then the outputs; the tangent tier's have the tangent planes behind the normals' and out_t last.
template <class Kernels, class... Extra>
hipError_t skin_launch(const SkinLaunch &a, int64_t tiled, Extra... extra) {
	const bool shaped = a.shape_weights != nullptr;
	const SkinLayout l = skin_layout(a.V, a.K, a.mesh_normals);
	const MorphLayout ml = morph_layout(a.V, a.K, a.mesh_normals, shaped ? a.P : 0); // (its stride is every plane's)
	const TangentLayout tl = tangent_layout(a.V, a.K, a.mesh_normals, a.P, a.mesh_tangents); // (behind all the mesh's shapes)
	if (a.out_t && (!a.out_n || !a.mesh_tangents)) return hipErrorInvalidValue;
	const dim3 grid((unsigned)((tiled + a.S - 1) / a.S), (unsigned)a.chunks);
	const size_t lds = (size_t)a.S * (size_t)morph_lds_bytes(a.B, shaped ? a.P : 0);
	const auto plane = [&](bool have, int64_t at) { return have ? reinterpret_cast<const float4 *>(a.mesh + at) : nullptr; };
	skin_dispatch(a.K, skin_tier(a.out_n != nullptr, a.out_t != nullptr), shaped ? a.mode : kNoShapes, [&](auto k, auto n, auto m) {
		constexpr int TIER = decltype(n)::value;
		constexpr bool NRM = TIER >= SKIN_NORMALS, TAN = TIER >= SKIN_TANGENTS;
		constexpr int MODE = decltype(m)::value;
		const auto kernel = Kernels::template kernel<decltype(k)::value, TIER, MODE>();
		const auto idx = reinterpret_cast<const uint2 *>(a.mesh + l.idx);
		if constexpr (MODE == kNoShapes && !TAN)
			hipLaunchKernelGGL(kernel, grid, dim3(kSkinThreads), lds, a.st, a.count, a.B, a.V, a.S, a.chunk, a.vshift, plane(true, l.pos),
					plane(NRM, l.nrm), idx, plane(true, l.wgt), ml.stride, a.skin, extra..., a.out_p, a.out_n);
		else if constexpr (!TAN)
			hipLaunchKernelGGL(kernel, grid, dim3(kSkinThreads), lds, a.st, a.count, a.B, a.V, a.P, a.S, a.chunk, a.vshift, plane(true, l.pos),
					plane(NRM, l.nrm), idx, plane(true, l.wgt), plane(true, ml.pos), plane(NRM, ml.nrm), ml.stride, a.skin, a.shape_weights,
					extra..., a.out_p, a.out_n);
		else if constexpr (MODE == kNoShapes)
			hipLaunchKernelGGL(kernel, grid, dim3(kSkinThreads), lds, a.st, a.count, a.B, a.V, a.S, a.chunk, a.vshift, plane(true, l.pos),
					plane(true, l.nrm), plane(true, tl.tan), idx, plane(true, l.wgt), ml.stride, a.skin, extra..., a.out_p, a.out_n, a.out_t);
		else
			hipLaunchKernelGGL(kernel, grid, dim3(kSkinThreads), lds, a.st, a.count, a.B, a.V, a.P, a.S, a.chunk, a.vshift, plane(true, l.pos),
					plane(true, l.nrm), plane(true, tl.tan), idx, plane(true, l.wgt), plane(true, ml.pos), plane(true, ml.nrm),
					plane(true, tl.stan), ml.stride, a.skin, a.shape_weights, extra..., a.out_p, a.out_n, a.out_t);
	});
	return hipGetLastError();
}

} // namespace mbik
