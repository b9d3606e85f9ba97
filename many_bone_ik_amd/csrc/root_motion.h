// Root motion, shared by the device kernels (k_root_motion.hip) and the host entries
// mbik_clip_root_motion[_layers]_cpu and mbik_root_motion_apply_cpu (host_clip.cpp): what Godot
// 4.3's AnimationMixer::_blend_process does for the track named by root_motion_track.  Per
// skeleton, the root bone's tracks are not written into the pose; the change of each channel over
// the frame -- from the layer's previous time to its time, split at the loop seam -- is accumulated
// over the layers with clip_layers.h's blend factors into a motion record of 10 floats (rotation
// delta xyzw, position delta, scale delta), and root_motion_apply composes that record into the
// skeleton's world transform.  One code path for both sides, made of clip.h's, clip_layers.h's and
// gd_math.h's IEEE-exact operations only, so the device and the host produce the same bits.
// include/mbik.h states the semantics; DESIGN.md §24.
#pragma once

#include "clip_layers.h"

namespace mbik {

constexpr uint32_t kRootMotionOrthonormalize = 1u;

// Where a skeleton's layer records and previous times come from.  The layered call reads
// [K] records and [K] previous times; the plain call is one record of weight 1.
struct RootLayers {
	const ClipLayer *L;
	const double *prev;
	GDI ClipLayer rec(int l) const { return L[l]; }
	GDI double time_prev(int l) const { return prev[l]; }
};
struct RootPlain {
	ClipLayer one;
	double prev;
	GDI ClipLayer rec(int) const { return one; }
	GDI double time_prev(int) const { return prev; }
};

// The root's channels at both ends of one segment (u0, u1) of already mapped times, or NaN for a
// layer whose times are not finite.  Both ends search in step -- six independent loads a step --
// and their twenty-four key loads (forty-eight with CUBIC) are issued before either end is evaluated.
template <bool CUBIC = false>
GDI void root_segment(const ClipView &v, const ClipInfo &info, const ClipLayerHeaders &h, bool finite, double u0, double u1, int lv,
		ClipSampled &x0, ClipSampled &x1) {
	if (!finite) { // no key is read
		const float nan = clip_nan();
		x0.rot = x1.rot = q4(nan, nan, nan, nan);
		x0.pos = x1.pos = x0.scl = x1.scl = v3(nan, nan, nan);
		return;
	}
	ClipChan p0 = clip_chan(v, h.pos), r0 = clip_chan(v, h.rot), s0 = clip_chan(v, h.scl);
	ClipChan p1 = p0, r1 = r0, s1 = s0;
	const int nrs = r0.n > s0.n ? r0.n : s0.n, nmax = p0.n > nrs ? p0.n : nrs;
	int step = 1;
	while (step <= (nmax >> 1)) step <<= 1;
	for (; step > 0; step >>= 1) {
		clip_search_step(p0, r0, s0, step, u0);
		clip_search_step(p1, r1, s1, step, u1);
	}
	if constexpr (CUBIC) {
		const ClipLoadedCubic k0 = clip_load_cubic(p0, r0, s0), k1 = clip_load_cubic(p1, r1, s1);
		clip_eval_cubic(k0, r0.n, u0, info.length, lv, x0);
		clip_eval_cubic(k1, r1.n, u1, info.length, lv, x1);
	} else {
		const ClipLoaded k0 = clip_load(p0, r0, s0), k1 = clip_load(p1, r1, s1);
		clip_eval(k0, r0.n, u0, info.length, lv, x0);
		clip_eval(k1, r1.n, u1, info.length, lv, x1);
	}
}

// What one layer adds over one segment: the position and scale differences times their blend
// factors, and the rotation from identity towards inverse(X(u0)) * X(u1).
struct RootStep {
	Q e;
	V3 dp, ds;
};
GDI RootStep root_step(const ClipSampled &x0, const ClipSampled &x1, bool do_pos, bool do_rot, bool do_scl, float bp, float br, float bs,
		int lv) {
	RootStep r{qid(), v3(0.0f, 0.0f, 0.0f), v3(0.0f, 0.0f, 0.0f)};
	if (do_pos) r.dp = (x1.pos - x0.pos) * bp;
	if (do_scl) r.ds = (x1.scl - x0.scl) * bs;
	if (do_rot) r.e = blend_slerp(qid(), inverse(x0.rot) * x1.rot, br, lv);
	return r;
}

// Steps 2 to 4 and the products of step 5 for one layer that is on, from its record, previous time,
// clip info and headers and the channels' totals: which channels it is accumulated into, and its
// one or two segments' steps.  segments == 0: nothing of the layer is accumulated and no key was
// read.  The second segment of a layer that crossed its clip's seam sits behind a per-lane branch.
struct RootLayerSteps {
	int segments;
	bool do_pos, do_rot, do_scl;
	RootStep first, second;
};
template <bool CUBIC = false>
GDI RootLayerSteps root_layer_steps(const ClipView &v, const ClipInfo &info, ClipLayerHeaders h, double t0, double t1, float weight,
		bool normalize, float tot_pos, float tot_rot, float tot_scl, int lv) {
	RootLayerSteps out;
	const float w = clip_layer_weight(weight);
	float bp, br, bs;
	out.do_pos = clip_layer_blend(normalize, h.pos.key_count, w, tot_pos, bp);
	out.do_rot = clip_layer_blend(normalize, h.rot.key_count, w, tot_rot, br);
	out.do_scl = clip_layer_blend(normalize, h.scl.key_count, w, tot_scl, bs);
	out.segments = 0;
	if (!(out.do_pos || out.do_rot || out.do_scl)) return out; // no key load; the layer's times are not looked at
	// a channel that is not accumulated searches nothing: it becomes a channel without keys
	const ClipHeader none{0, 0, 0, 0};
	if (!out.do_pos) h.pos = none;
	if (!out.do_rot) h.rot = none;
	if (!out.do_scl) h.scl = none;
	const bool finite = clip_finite(t0) && clip_finite(t1);
	double p0 = 0.0, p1 = 0.0;
	if (finite) p0 = clip_time(t0, info.length, info.loop_mode), p1 = clip_time(t1, info.length, info.loop_mode);
	const bool looped = finite && info.loop_mode == 1 && p0 > p1;
	ClipSampled x0, x1;
	root_segment<CUBIC>(v, info, h, finite, p0, looped ? info.length : p1, lv, x0, x1);
	out.first = root_step(x0, x1, out.do_pos, out.do_rot, out.do_scl, bp, br, bs, lv);
	out.segments = 1;
	if (looped) {
		root_segment<CUBIC>(v, info, h, true, 0.0, p1, lv, x0, x1);
		out.second = root_step(x0, x1, out.do_pos, out.do_rot, out.do_scl, bp, br, bs, lv);
		out.segments = 2;
	}
	return out;
}

// The accumulators of one skeleton's record, and step 5's sums: the layers' steps are added
// ascending, each layer's segments in order.
struct RootAcc {
	Q rot;
	V3 pos, scl;
	bool any_pos, any_rot, any_scl;
};
GDI RootAcc root_acc_start() { return RootAcc{qid(), v3(0.0f, 0.0f, 0.0f), v3(0.0f, 0.0f, 0.0f), false, false, false}; }
GDI void root_add(RootAcc &a, const RootStep &r, bool do_pos, bool do_rot, bool do_scl) {
	if (do_pos) a.pos = a.pos + r.dp, a.any_pos = true;
	if (do_scl) a.scl = a.scl + r.ds, a.any_scl = true;
	if (do_rot) a.rot = normalized(a.rot * r.e), a.any_rot = true;
}
// Step 6.
GDI void root_store(const RootAcc &a, float *out10) {
	out10[0] = a.any_rot ? blend_canon(a.rot.x) : 0.0f, out10[1] = a.any_rot ? blend_canon(a.rot.y) : 0.0f;
	out10[2] = a.any_rot ? blend_canon(a.rot.z) : 0.0f, out10[3] = a.any_rot ? blend_canon(a.rot.w) : 1.0f;
	out10[4] = a.any_pos ? blend_canon(a.pos.x) : 0.0f, out10[5] = a.any_pos ? blend_canon(a.pos.y) : 0.0f;
	out10[6] = a.any_pos ? blend_canon(a.pos.z) : 0.0f;
	out10[7] = a.any_scl ? blend_canon(a.scl.x) : 0.0f, out10[8] = a.any_scl ? blend_canon(a.scl.y) : 0.0f;
	out10[9] = a.any_scl ? blend_canon(a.scl.z) : 0.0f;
}

// Step 1 for one skeleton, from the records alone: no clip index but -1 lies outside the set.
template <class Src>
GDI bool root_motion_valid(const Src &src, int K, int clip_count) {
	for (int l = 0; l < K; l++) {
		const int c = src.rec(l).clip;
		if (c != kClipLayerOff && (c < 0 || c >= clip_count)) return false;
	}
	return true;
}

// One valid skeleton: out10 = the motion record of bone `root` over the frame of the skeleton's K
// layers.  The layers are walked in loops over named state, as in clip_layers_bone: the channels'
// totals in normalize mode, then the accumulation, which loads layer l + 1's record, previous
// time, clip info and headers before layer l's keys are searched.
// (k_root_motion.hip also has a form that gives each layer a lane of its own: the same
// root_layer_steps, root_add and root_store, the totals and the sums in the same order.)
template <bool CUBIC = false, class Src>
GDI void root_motion_record(const ClipView &v, const Src &src, int K, uint32_t flags, int root, int lv, float *out10) {
	const bool normalize = (flags & kClipLayersNormalize) != 0;
	float tot_pos = 0.0f, tot_rot = 0.0f, tot_scl = 0.0f;
	if (normalize) {
		for (int l = 0; l < K; l++) {
			const ClipLayer rec = src.rec(l);
			if (rec.clip == kClipLayerOff) continue;
			const ClipHeader *h = v.headers + ((int64_t)rec.clip * v.B + root) * 3;
			const int np = h[0].key_count, nr = h[1].key_count, ns = h[2].key_count;
			const float w = clip_layer_weight(rec.weight);
			if (np) tot_pos = tot_pos + w;
			if (nr) tot_rot = tot_rot + w;
			if (ns) tot_scl = tot_scl + w;
		}
	}
	RootAcc a = root_acc_start();

	ClipLayer next = src.rec(0);
	double next_prev = src.time_prev(0);
	ClipLayerHeaders next_h = clip_layer_headers(v, next.clip, root);
	ClipInfo next_info = v.clips[next.clip == kClipLayerOff ? 0 : next.clip];
	for (int l = 0; l < K; l++) {
		const ClipLayer rec = next;
		const double t0 = next_prev;
		const ClipLayerHeaders h = next_h;
		const ClipInfo info = next_info;
		if (l + 1 < K) {
			next = src.rec(l + 1);
			next_prev = src.time_prev(l + 1);
			next_h = clip_layer_headers(v, next.clip, root);
			next_info = v.clips[next.clip == kClipLayerOff ? 0 : next.clip];
		}
		if (rec.clip == kClipLayerOff) continue;
		const RootLayerSteps ls = root_layer_steps<CUBIC>(v, info, h, t0, rec.time, rec.weight, normalize, tot_pos, tot_rot, tot_scl, lv);
		if (ls.segments > 0) root_add(a, ls.first, ls.do_pos, ls.do_rot, ls.do_scl);
		if (ls.segments > 1) root_add(a, ls.second, ls.do_pos, ls.do_rot, ls.do_scl);
	}
	root_store(a, out10);
}

// One skeleton, steps 1 to 7: its record, ten NaNs for an invalid one, and the rest pose's root
// record into pose_s ([B][10], or null) for a valid one.
template <bool CUBIC = false, class Src>
GDI void root_motion_skeleton(const ClipView &v, const Src &src, int K, uint32_t flags, int root, int lv, float *out10, float *pose_s) {
	if (!root_motion_valid(src, K, v.clip_count)) {
		for (int f = 0; f < 10; f++) out10[f] = clip_nan();
		return;
	}
	if (pose_s) {
		const float *rest = v.rest + (int64_t)root * 10;
		for (int f = 0; f < 10; f++) pose_s[(int64_t)root * 10 + f] = rest[f];
	}
	root_motion_record<CUBIC>(v, src, K, flags, root, lv, out10);
}

// One skeleton's world transform G [12] (basis rows, then origin) times the motion record's
// Transform3D(Basis(q), p), in place: Transform3D::operator*=.  The record's scale is not applied.
GDI void root_motion_apply(const float *motion10, uint32_t flags, float *G12) {
	const X3 G{bset(G12[0], G12[1], G12[2], G12[3], G12[4], G12[5], G12[6], G12[7], G12[8]), v3(G12[9], G12[10], G12[11])};
	const X3 T{from_quat(q4(motion10[0], motion10[1], motion10[2], motion10[3])), v3(motion10[4], motion10[5], motion10[6])};
	X3 R = G * T;
	if (flags & kRootMotionOrthonormalize) R.b = orthonormalized(R.b);
	for (int i = 0; i < 3; i++) {
		G12[3 * i + 0] = blend_canon(R.b.r[i].x), G12[3 * i + 1] = blend_canon(R.b.r[i].y), G12[3 * i + 2] = blend_canon(R.b.r[i].z);
	}
	G12[9] = blend_canon(R.o.x), G12[10] = blend_canon(R.o.y), G12[11] = blend_canon(R.o.z);
}

} // namespace mbik
