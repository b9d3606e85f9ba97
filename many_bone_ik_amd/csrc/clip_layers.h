// Layered clip sampling, shared by the device kernel (k_clip_layers.hip) and the host entry
// mbik_clip_sample_layers_cpu (host_clip.cpp): up to kClipMaxLayers (time, clip, weight) records a
// skeleton, each sampled as mbik_clip_sample samples it (clip.h clip_sample_channels) and
// accumulated onto the rest pose in the order of Godot 4.3's AnimationMixer::_blend_process:
// loc += (x - init) * blend, rot = (rot * slerp(identity, init^-1 * x, blend)).normalized().
// One code path for both sides, made of clip.h's and blend.h's IEEE-exact operations only, so the
// device and the host produce the same bits.  include/mbik.h states the semantics; DESIGN.md §20.
#pragma once

#include "clip.h"

namespace mbik {

// mbik_clip_layer: 16 bytes.
struct ClipLayer {
	double time;
	int32_t clip;
	float weight;
};
static_assert(sizeof(ClipLayer) == 16, "a layer record is 16 bytes");
constexpr int kClipMaxLayers = 8;
constexpr uint32_t kClipLayersNormalize = 1u;
constexpr int kClipLayerOff = -1;

// Step 2: the weight clamped into [0, 1]; a NaN passes both compares.
GDI float clip_layer_weight(float w) {
	if (w < 0.0f) w = 0.0f;
	if (w > 1.0f) w = 1.0f;
	return w;
}

// The three headers of `bone` in a layer's clip, or three empty ones for a layer that is off:
// an empty header is a channel without keys, which takes no part in anything below.
struct ClipLayerHeaders {
	ClipHeader pos, rot, scl;
};
GDI ClipLayerHeaders clip_layer_headers(const ClipView &v, int clip, int bone) {
	const ClipHeader none{0, 0, 0, 0};
	if (clip == kClipLayerOff) return ClipLayerHeaders{none, none, none};
	const ClipHeader *h = v.headers + ((int64_t)clip * v.B + bone) * 3;
	return ClipLayerHeaders{h[0], h[1], h[2]};
}

// Step 4 for one channel of one layer: the blend factor, and whether the layer is accumulated
// (the channel has keys, its total is not zero, and the factor is not is_zero_approx).
GDI bool clip_layer_blend(bool normalize, int key_count, float w, float total, float &blend) {
	blend = w;
	if (key_count == 0) return false;
	if (normalize) {
		if (fabsf(total) < (float)CMP_EPSILON) return false;
		blend = gd_div(w, total);
	}
	return !(fabsf(blend) < (float)CMP_EPSILON);
}

// One bone of one skeleton: out10 = the blend of the skeleton's K layers L[0..K-1] for `bone`.
// The layers are walked in loops over named state (K is a run-time value; there is no array of
// per-layer values).  Three passes over the records: validity (records only, so an invalid index
// is found before any table is touched); in normalize mode the channels' totals, which need the
// K x 3 key counts; then the accumulation, which loads layer l + 1's record and headers before
// layer l's keys are searched, so that a lane has two layers' loads in flight.  A layer whose
// three channels are all off, untracked or skipped by weight reads no key.
template <bool CUBIC = false>
GDI void clip_layers_bone(const ClipView &v, const ClipLayer *L, int K, uint32_t flags, int bone, int lv, float *out10) {
	for (int l = 0; l < K; l++) {
		const int c = L[l].clip;
		if (c != kClipLayerOff && (c < 0 || c >= v.clip_count)) {
			for (int f = 0; f < 10; f++) out10[f] = clip_nan();
			return;
		}
	}
	const bool normalize = (flags & kClipLayersNormalize) != 0;
	float tot_pos = 0.0f, tot_rot = 0.0f, tot_scl = 0.0f;
	if (normalize) {
		for (int l = 0; l < K; l++) {
			const ClipLayer rec = L[l];
			if (rec.clip == kClipLayerOff) continue;
			const ClipHeader *h = v.headers + ((int64_t)rec.clip * v.B + bone) * 3;
			const int np = h[0].key_count, nr = h[1].key_count, ns = h[2].key_count;
			const float w = clip_layer_weight(rec.weight);
			if (np) tot_pos = tot_pos + w;
			if (nr) tot_rot = tot_rot + w;
			if (ns) tot_scl = tot_scl + w;
		}
	}
	const float *rest = v.rest + (int64_t)bone * 10;
	const Q Ir = q4(rest[0], rest[1], rest[2], rest[3]);
	const V3 Ip = v3(rest[4], rest[5], rest[6]), Is = v3(rest[7], rest[8], rest[9]);
	Q rot = Ir;
	V3 pos = Ip, scl = Is;
	bool any_pos = false, any_rot = false, any_scl = false;

	ClipLayer next = L[0];
	ClipLayerHeaders next_h = clip_layer_headers(v, next.clip, bone);
	ClipInfo next_info = v.clips[next.clip == kClipLayerOff ? 0 : next.clip];
	for (int l = 0; l < K; l++) {
		const ClipLayer rec = next;
		ClipLayerHeaders h = next_h;
		const ClipInfo info = next_info;
		if (l + 1 < K) {
			next = L[l + 1];
			next_h = clip_layer_headers(v, next.clip, bone);
			next_info = v.clips[next.clip == kClipLayerOff ? 0 : next.clip];
		}
		const float w = clip_layer_weight(rec.weight);
		float bp, br, bs;
		const bool do_pos = clip_layer_blend(normalize, h.pos.key_count, w, tot_pos, bp);
		const bool do_rot = clip_layer_blend(normalize, h.rot.key_count, w, tot_rot, br);
		const bool do_scl = clip_layer_blend(normalize, h.scl.key_count, w, tot_scl, bs);
		if (!(do_pos || do_rot || do_scl)) continue; // no key load
		// a channel that is not accumulated searches nothing: it becomes a channel without keys
		const ClipHeader none{0, 0, 0, 0};
		if (!do_pos) h.pos = none;
		if (!do_rot) h.rot = none;
		if (!do_scl) h.scl = none;
		const ClipSampled x = clip_sample_channels<CUBIC>(v, info, h.pos, h.rot, h.scl, rec.time, lv);
		if (do_pos) pos = pos + (x.pos - Ip) * bp, any_pos = true;
		if (do_scl) scl = scl + (x.scl - Is) * bs, any_scl = true;
		if (do_rot) {
			const Q d = inverse(Ir) * x.rot;
			const Q e = blend_slerp(qid(), d, br, lv);
			rot = normalized(rot * e), any_rot = true;
		}
	}
	out10[0] = any_rot ? blend_canon(rot.x) : rest[0], out10[1] = any_rot ? blend_canon(rot.y) : rest[1];
	out10[2] = any_rot ? blend_canon(rot.z) : rest[2], out10[3] = any_rot ? blend_canon(rot.w) : rest[3];
	out10[4] = any_pos ? blend_canon(pos.x) : rest[4], out10[5] = any_pos ? blend_canon(pos.y) : rest[5];
	out10[6] = any_pos ? blend_canon(pos.z) : rest[6];
	out10[7] = any_scl ? blend_canon(scl.x) : rest[7], out10[8] = any_scl ? blend_canon(scl.y) : rest[8];
	out10[9] = any_scl ? blend_canon(scl.z) : rest[9];
}

} // namespace mbik
