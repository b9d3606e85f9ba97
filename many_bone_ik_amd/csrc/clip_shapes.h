// Blend-shape tracks of animation clips, shared by the device kernels (k_clip_shapes.hip) and the
// host entries mbik_clip_sample_shapes_cpu / mbik_clip_sample_shapes_layers_cpu (host_clip.cpp):
// Godot 4.3's Animation::blend_shape_track_interpolate for one (skeleton, shape), and the
// TYPE_BLEND_SHAPE case of AnimationMixer::_blend_process for up to kClipMaxLayers layers of it.
// The time mapping, the pick of the two keys and their weight are clip.h's (clip_time, clip_pick,
// clip_weight), the layer rules clip_layers.h's (clip_layer_weight, clip_layer_blend); what is new
// is the value type -- one float -- and the table layout.  One code path for both sides, made of
// IEEE-exact operations only, so the device and the host produce the same bits.  include/mbik.h
// states the semantics; DESIGN.md §23.
#pragma once

#include "clip_layers.h"

namespace mbik {

// ---- the repacked shape tracks: one blob, on the device for mbik_clipset, on the host for the CPU entries ----
// A key is one 16-byte record, time and value together, so the two keys a sample is made of are
// two 16-byte loads -- one 32-byte run for an interior pick -- where clip.h's split layout needs
// four loads from two arrays (§16's "not tried": key times and values in one line).  One header
// per (clip, shape); key_count == 0: the shape is untracked in that clip (key_off 0).  The key
// array ends with one record that belongs to no track, so index key_off + 0 exists for every
// header: the search loads at a clamped index and selects.
struct ShapeKey {
	double time;
	float value, pad;
};
static_assert(sizeof(ShapeKey) == 16, "a shape key is 16 bytes");
struct ShapeHeader {
	int32_t key_off, key_count, flags, reserved; // flags: kClipLinear, kClipWrap, kClipCubic
};
struct ShapeView {
	int32_t P, clip_count;
	const ClipInfo *clips;      // [clip_count]
	const ShapeHeader *headers; // [clip_count][P]
	const ShapeKey *keys;       // [keys + 1]
	const float *init;          // [P]
};

// A tracked shape (h.key_count != 0) at raw time t in the clip `info`: mbik_clip_sample's steps 2,
// 3, 5 and 6 on one float.  The dependent rounds of loads: the search, one 8-byte load a step;
// then the two key records, 16 bytes each, which bring both times and both values.
// CUBIC (a set with a cubic shape track): four key records, the ones before a and after b as well,
// all loaded before any is used; a pick that is not cubic repeats a's and b's addresses.
template <bool CUBIC = false>
GDI float shape_sample_keys(const ShapeView &v, const ClipInfo &info, const ShapeHeader &h, double t) {
	if (!clip_finite(t)) return clip_nan(); // no key is read
	const double tp = clip_time(t, info.length, info.loop_mode);
	const ShapeKey *keys = v.keys + h.key_off;
	const int n = h.key_count;
	int pos = 0, step = 1;
	while (step <= (n >> 1)) step <<= 1; // the highest power of two <= n
	for (; step > 0; step >>= 1) {
		const int k = pos + step - 1;
		const bool in = k < n;
		const double tk = keys[in ? k : 0].time;
		pos += in && tk <= tp ? step : 0;
	}
	if constexpr (CUBIC) {
		const ClipPickCubic p = clip_pick_cubic(ClipChan{nullptr, nullptr, n, h.flags, pos});
		const ShapeKey a = keys[p.a], b = keys[p.b], pre = keys[p.pre], post = keys[p.post];
		if (p.mode == kClipCopy) return a.value;
		const float c = clip_weight(p.mode, a.time, b.time, tp, info.length);
		if (!p.cubic) return blend_canon(a.value + (b.value - a.value) * c);
		if (c == 0.0f) return a.value; // on a key: the key's bits (clip.h clip_value_vec_cubic)
		// Math::cubic_interpolate_in_time
		const ClipCubicW w = clip_cubic_weights(c, clip_span(p, pre.time, a.time, b.time, post.time, info.length));
		return blend_canon(clip_cubic(a.value, b.value, pre.value, post.value, w));
	}
	const ClipPick p = clip_pick(ClipChan{nullptr, nullptr, n, h.flags, pos});
	const ShapeKey a = keys[p.a], b = keys[p.b];
	if (p.mode == kClipCopy) return a.value;
	const float c = clip_weight(p.mode, a.time, b.time, tp, info.length);
	return blend_canon(a.value + (b.value - a.value) * c); // Math::lerp
}

// mbik_clip_sample_shapes for one (skeleton, shape).
template <bool CUBIC = false>
GDI float shape_sample(const ShapeView &v, int clip, int shape, double t) {
	if (clip < 0 || clip >= v.clip_count) return clip_nan();
	const ClipInfo info = v.clips[clip];
	const ShapeHeader h = v.headers[(int64_t)clip * v.P + shape];
	if (h.key_count == 0) return v.init[shape];
	return shape_sample_keys<CUBIC>(v, info, h, t);
}

GDI ShapeHeader shape_layer_header(const ShapeView &v, int clip, int shape) {
	if (clip == kClipLayerOff) return ShapeHeader{0, 0, 0, 0};
	return v.headers[(int64_t)clip * v.P + shape];
}

// mbik_clip_sample_shapes_layers for one (skeleton, shape): the blend of the skeleton's K layers
// L[0..K-1].  clip_layers_bone's three passes over named state (K is a run-time value; there is no
// array of per-layer values): validity from the records alone, before any table is touched; in
// normalize mode the shape's total; then the accumulation, which loads layer l + 1's record, clip
// info and header before layer l's keys are searched.
template <bool CUBIC = false>
GDI float shape_layers(const ShapeView &v, const ClipLayer *L, int K, uint32_t flags, int shape) {
	for (int l = 0; l < K; l++) {
		const int c = L[l].clip;
		if (c != kClipLayerOff && (c < 0 || c >= v.clip_count)) return clip_nan();
	}
	const bool normalize = (flags & kClipLayersNormalize) != 0;
	float total = 0.0f;
	if (normalize) {
		for (int l = 0; l < K; l++) {
			const ClipLayer rec = L[l];
			if (rec.clip == kClipLayerOff) continue;
			if (v.headers[(int64_t)rec.clip * v.P + shape].key_count) total = total + clip_layer_weight(rec.weight);
		}
	}
	const float I = v.init[shape];
	float acc = I;
	bool any = false;

	ClipLayer next = L[0];
	ShapeHeader next_h = shape_layer_header(v, next.clip, shape);
	ClipInfo next_info = v.clips[next.clip == kClipLayerOff ? 0 : next.clip];
	for (int l = 0; l < K; l++) {
		const ClipLayer rec = next;
		const ShapeHeader h = next_h;
		const ClipInfo info = next_info;
		if (l + 1 < K) {
			next = L[l + 1];
			next_h = shape_layer_header(v, next.clip, shape);
			next_info = v.clips[next.clip == kClipLayerOff ? 0 : next.clip];
		}
		float blend;
		if (!clip_layer_blend(normalize, h.key_count, clip_layer_weight(rec.weight), total, blend)) continue; // no key load
		const float x = shape_sample_keys<CUBIC>(v, info, h, rec.time);
		acc = acc + (x - I) * blend, any = true;
	}
	return any ? blend_canon(acc) : I;
}

} // namespace mbik
