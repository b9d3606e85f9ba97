// Animation clip sampling, shared by the device kernel (k_clip.hip) and the host entry
// mbik_clip_sample_cpu (host_clip.cpp): Godot 4.3's Animation::position_track_interpolate,
// rotation_track_interpolate and scale_track_interpolate (Animation::_interpolate) for
// INTERPOLATION_NEAREST / INTERPOLATION_LINEAR / INTERPOLATION_CUBIC (the samplers' CUBIC forms,
// DESIGN.md §26), LOOP_NONE / LOOP_LINEAR, forward playback and key transitions of 1, for every
// bone of a skeleton at that skeleton's time in that skeleton's clip.
// One code path for both sides, made of IEEE-exact operations only (double compares, differences
// and sums, an integer fmod, gd_math.h's float arithmetic and blend.h's slerp), so the device and
// the host produce the same bits.  include/mbik.h (ABI 12) states the semantics; DESIGN.md §16.
// clip_layers.h blends several such samples a skeleton (mbik_clip_sample_layers).
#pragma once

#include <cstdint>
#include <cstring>

#include "blend.h"

namespace mbik {

// ---- the repacked clip set: one blob, on the device for mbik_clipset, on the host for the CPU entry ----
// One header per (clip, bone, channel), channel 0 position, 1 rotation, 2 scale.  The keys of a
// channel are key_count consecutive entries of `times` and of `values` from key_off; a value is
// 4 floats whatever the channel (a position or scale key leaves the fourth 0), so a key is one
// 16-byte load.  key_count == 0: the channel is untracked (key_off 0).  Both arrays end with one
// entry that belongs to no track, so index key_off + 0 exists for every header: the per-bone code
// loads at a clamped index and selects, instead of branching around each load.
struct ClipHeader {
	int32_t key_off, key_count, flags, reserved;
};
constexpr int kClipLinear = 1; // flags: INTERPOLATION_LINEAR (else nearest)
constexpr int kClipWrap = 2;   //        loop_mode == LOOP_LINEAR && loop_wrap
constexpr int kClipCubic = 4;  //        INTERPOLATION_CUBIC (never with kClipLinear); sets of mbik_clipset_create_desc only
struct ClipInfo {
	double length;
	int32_t loop_mode, reserved;
};
struct ClipValue {
	float x, y, z, w;
};
struct ClipView {
	int32_t B, clip_count;
	const ClipInfo *clips;     // [clip_count]
	const ClipHeader *headers; // [clip_count][B][3]
	const double *times;       // [keys + 1]
	const ClipValue *values;   // [keys + 1]
	const float *rest;         // [B][10]
};

GDI uint64_t clip_bits(double x) {
	union {
		double d;
		uint64_t u;
	} c{x};
	return c.u;
}
GDI bool clip_finite(double x) { return (clip_bits(x) & 0x7ff0000000000000ull) != 0x7ff0000000000000ull; }

// fmod(x, y) for finite x and finite y > 0: the remainder of the integer significands, shifted one
// bit at a time, so it is exact -- C's fmod, whose result is always representable -- and made of
// integer operations and one exact scaling only.  ex - ey iterations: 30 for a time of 1e9 s.
GDI double clip_fmod(double x, double y) {
	const double ax = x < 0 ? -x : x;
	if (ax < y) return x; // (-0 stays -0)
	uint64_t mx = clip_bits(ax) & 0x000fffffffffffffull, my = clip_bits(y) & 0x000fffffffffffffull;
	int ex = (int)(clip_bits(ax) >> 52), ey = (int)(clip_bits(y) >> 52);
	// significands with the leading bit at 52; a subnormal is shifted up, its exponent going below 1
	if (ex) mx |= 1ull << 52;
	else
		for (ex = 1; !(mx >> 52); ex--) mx <<= 1;
	if (ey) my |= 1ull << 52;
	else
		for (ey = 1; !(my >> 52); ey--) my <<= 1;
	for (int n = ex - ey; n > 0; n--) {
		if (mx >= my) mx -= my;
		mx <<= 1;
	}
	if (mx >= my) mx -= my;
	const double r = ldexp((double)(int64_t)mx, ey - 1075); // mx < 2^53 and r < y is a multiple of x's and y's last bits: exact
	return x < 0 ? -r : r;
}

// Step 3: the time a clip is sampled at.  LOOP_NONE clamps to [0, length]; LOOP_LINEAR is
// Math::fposmod.  t is finite.
GDI double clip_time(double t, double length, int loop_mode) {
	if (loop_mode == 0) return t < 0 ? 0.0 : (t > length ? length : t);
	double v = clip_fmod(t, length);
	if (v < 0) v += length;
	v += 0.0;
	return v;
}

// One channel of one bone: its keys (T = times + key_off, V likewise), and `pos`, the number of
// keys the search knows to be <= the time.
struct ClipChan {
	const double *T;
	const ClipValue *V;
	int n, flags, pos;
};
GDI ClipChan clip_chan(const ClipView &v, const ClipHeader &h) { return ClipChan{v.times + h.key_off, v.values + h.key_off, h.key_count, h.flags, 0}; }

// One step of the three channels' searches for their last key <= tp: pos grows by `step` when the
// key that would then be the last one is <= tp.  Over step = 2^k ... 1 with 2^k the highest power
// of two <= n (a larger first step changes nothing), pos ends as the count of keys <= tp.  The
// three loads are issued before any of them is used, at an index clamped into the channel's keys
// (0 for a channel without keys: the arrays' spare entry at worst), so a lane has three
// independent loads in flight per step, not three round trips one after the other.
GDI void clip_search_step(ClipChan &a, ClipChan &b, ClipChan &c, int step, double tp) {
	const int ka = a.pos + step - 1, kb = b.pos + step - 1, kc = c.pos + step - 1;
	const bool ia = ka < a.n, ib = kb < b.n, ic = kc < c.n;
	const double ta = a.T[ia ? ka : 0], tb = b.T[ib ? kb : 0], tc = c.T[ic ? kc : 0];
	a.pos += ia && ta <= tp ? step : 0;
	b.pos += ib && tb <= tp ? step : 0;
	c.pos += ic && tc <= tp ? step : 0;
}

// Step 5 up to the loads: the keys a and b a channel's value comes from, and how.  i = pos - 1 is
// the last key <= tp, or -1.  A channel without keys picks index 0 as a copy (its value is not used).
enum ClipMode : int {
	kClipCopy = 0,       // V[a]
	kClipInterior = 1,   // delta = T[b] - T[a], from = tp - T[a]
	kClipWrapAfter = 2,  // a = n-1, b = 0: delta = (length - T[a]) + T[b], from = tp - T[a]
	kClipWrapBefore = 3, //                 the same delta,                 from = (length - T[a]) + tp
};
struct ClipPick {
	int a, b, mode;
};
GDI ClipPick clip_pick(const ClipChan &ch) {
	const int n = ch.n, i = ch.pos - 1;
	const bool wrap = (ch.flags & kClipWrap) != 0;
	if (n <= 1) return ClipPick{0, 0, kClipCopy};
	if (!wrap && i < 0) return ClipPick{0, 0, kClipCopy};
	if (!wrap && i == n - 1) return ClipPick{n - 1, n - 1, kClipCopy};
	const bool linear = (ch.flags & kClipLinear) != 0;
	if (i >= 0 && i < n - 1) return ClipPick{i, i + 1, linear ? kClipInterior : kClipCopy};
	return ClipPick{n - 1, 0, linear ? (i < 0 ? kClipWrapBefore : kClipWrapAfter) : kClipCopy};
}
// The pick of a sampler's CUBIC form (a set that has a cubic track).  A cubic channel's pick that
// is not one of the copies above also names the keys before a and after b -- clamped into the
// track, or going round it with wrap -- and says so in `cubic`; every other pick is clip_pick's
// with pre = a and post = b, so that its two further loads repeat addresses it loads anyway.
struct ClipPickCubic : ClipPick {
	int pre, post;
	bool cubic;
};
GDI ClipPickCubic clip_pick_cubic(const ClipChan &ch) {
	const ClipPick p = clip_pick(ch);
	const int n = ch.n, i = ch.pos - 1;
	const bool wrap = (ch.flags & kClipWrap) != 0;
	const bool copied = n <= 1 || (!wrap && (i < 0 || i == n - 1));
	if (!(ch.flags & kClipCubic) || copied) return ClipPickCubic{p, p.a, p.b, false};
	if (!wrap) return ClipPickCubic{ClipPick{i, i + 1, kClipInterior}, i > 0 ? i - 1 : 0, i + 2 < n ? i + 2 : n - 1, true};
	const int a = i < 0 ? n - 1 : i, b = a + 1 < n ? a + 1 : 0;
	return ClipPickCubic{ClipPick{a, b, i < 0 ? kClipWrapBefore : (i == n - 1 ? kClipWrapAfter : kClipInterior)}, a > 0 ? a - 1 : n - 1,
			b + 1 < n ? b + 1 : 0, true};
}
// The weight c between the two keys of a pick that is not a copy.  Every difference and sum in
// double, rounded once to float; the quotient is IEEE float division.
GDI float clip_weight(int mode, double Ta, double Tb, double tp, double length) {
	float delta, from;
	if (mode == kClipInterior) {
		delta = (float)(Tb - Ta);
		from = (float)(tp - Ta);
	} else {
		const double end = length - Ta;
		delta = (float)(end + Tb);
		from = mode == kClipWrapBefore ? (float)(end + tp) : (float)(tp - Ta);
	}
	return fabsf(delta) < (float)CMP_EPSILON ? 0.0f : gd_div(from, delta);
}

GDI float clip_nan() {
	union {
		uint32_t u;
		float f;
	} c{0x7fc00000u};
	return c.f;
}

// A tracked position or scale channel from its loaded keys.
GDI V3 clip_value_vec(const ClipPick &p, float c, const ClipValue &a, const ClipValue &b) {
	if (p.mode == kClipCopy) return v3(a.x, a.y, a.z);
	const V3 r = v3(a.x, a.y, a.z) + (v3(b.x, b.y, b.z) - v3(a.x, a.y, a.z)) * c; // Vector3::lerp
	return v3(blend_canon(r.x), blend_canon(r.y), blend_canon(r.z));
}

// ---- INTERPOLATION_CUBIC (include/mbik.h, the continuation of step 5) ----
// The times of the keys before a, at b and after b, relative to key a's, as Animation::_interpolate
// hands them to the *_in_time interpolators: a key that the pick reached by going round the clip
// counts a length earlier or later.  Sums and differences in double, rounded once.  (A pick that
// does not wrap has pre <= a < b <= post, so the one form serves both.)
struct ClipSpan {
	float pre_t, to_t, post_t;
};
GDI ClipSpan clip_span(const ClipPickCubic &p, double Tpre, double Ta, double Tb, double Tpost, double length) {
	ClipSpan s;
	s.pre_t = p.pre > p.a ? (float)((-length + Tpre) - Ta) : (float)(Tpre - Ta);
	s.to_t = p.b < p.a ? (float)((length + Tb) - Ta) : (float)(Tb - Ta);
	s.post_t = (p.b < p.a || p.post <= p.a) ? (float)((length + Tpost) - Ta) : (float)(Tpost - Ta);
	return s;
}
GDI float clip_lerp(float a, float b, float w) { return a + (b - a) * w; } // Math::lerp
// Math::cubic_interpolate_in_time (Barry-Goldman): its six lerp weights depend on the times alone,
// so a channel computes them once for all its components.
struct ClipCubicW {
	float a1, a2, a3, b1, b2;
};
GDI ClipCubicW clip_cubic_weights(float c, const ClipSpan &s) {
	const float t = clip_lerp(0.0f, s.to_t, c);
	ClipCubicW w;
	w.a1 = s.pre_t == 0.0f ? 0.0f : gd_div(t - s.pre_t, -s.pre_t);
	w.a2 = s.to_t == 0.0f ? 0.5f : gd_div(t, s.to_t);
	const float d3 = s.post_t - s.to_t, d1 = s.to_t - s.pre_t;
	w.a3 = d3 == 0.0f ? 1.0f : gd_div(t - s.to_t, d3);
	w.b1 = d1 == 0.0f ? 0.0f : gd_div(t - s.pre_t, d1);
	w.b2 = s.post_t == 0.0f ? 1.0f : gd_div(t, s.post_t);
	return w;
}
GDI float clip_cubic(float from, float to, float pre, float post, const ClipCubicW &w) {
	const float a1 = clip_lerp(pre, from, w.a1), a2 = clip_lerp(from, to, w.a2), a3 = clip_lerp(to, post, w.a3);
	const float b1 = clip_lerp(a1, a2, w.b1), b2 = clip_lerp(a2, a3, w.b2);
	return clip_lerp(b1, b2, w.a2);
}
GDI V3 clip_cubic_vec(const ClipValue &a, const ClipValue &b, const ClipValue &pre, const ClipValue &post, const ClipCubicW &w) {
	return v3(blend_canon(clip_cubic(a.x, b.x, pre.x, post.x, w)), blend_canon(clip_cubic(a.y, b.y, pre.y, post.y, w)),
			blend_canon(clip_cubic(a.z, b.z, pre.z, post.z, w)));
}
// Quaternion::log and Quaternion::exp.
GDI V3 clip_quat_log(Q q) { return get_axis(q) * get_angle_clamped(q); }
GDI Q clip_quat_exp(V3 v, int lv) {
	const float theta = length(v);
	const V3 u = normalized(v);
	const float ls = length_sq(u);
	const bool unit = ls == 1.0f || fabsf(ls - 1.0f) < 0.001f; // Vector3::is_normalized: is_equal_approx(length_squared(), 1, UNIT_EPSILON)
	if (theta < (float)CMP_EPSILON || !unit) return qid();
	return axis_angle(u, theta, lv);
}
GDI Q clip_quat_neg(Q q) { return q4(-q.x, -q.y, -q.z, -q.w); }
GDI bool clip_signbit(float x) {
	union {
		float f;
		uint32_t u;
	} c{x};
	return (c.u >> 31) != 0;
}
// One of the two expmap halves: base * exp(cubic(log(base^-1 * from), log(base^-1 * to), log(base^-1
// * pre), log(base^-1 * post))), where the log of base^-1 * base is the zero vector as written.
GDI Q clip_cubic_half(Q base, bool base_is_from, Q other, Q pre, Q post, const ClipCubicW &w, int lv) {
	const Q inv = inverse(base);
	const V3 zero = v3(0.0f, 0.0f, 0.0f), lo = clip_quat_log(inv * other);
	const V3 lf = base_is_from ? zero : lo, lt = base_is_from ? lo : zero;
	const V3 lp = clip_quat_log(inv * pre), lq = clip_quat_log(inv * post);
	const V3 ln = v3(clip_cubic(lf.x, lt.x, lp.x, lq.x, w), clip_cubic(lf.y, lt.y, lp.y, lq.y, w), clip_cubic(lf.z, lt.z, lp.z, lq.z, w));
	return base * clip_quat_exp(ln, lv);
}
// Quaternion::spherical_cubic_interpolate_in_time, not renormalised.
GDI Q clip_cubic_rot(const ClipValue &a, const ClipValue &b, const ClipValue &vpre, const ClipValue &vpost, float c, const ClipCubicW &w,
		int lv) {
	const Q from = get_rotation_quaternion(from_quat(q4(a.x, a.y, a.z, a.w)));
	Q pre = get_rotation_quaternion(from_quat(q4(vpre.x, vpre.y, vpre.z, vpre.w)));
	Q to = get_rotation_quaternion(from_quat(q4(b.x, b.y, b.z, b.w)));
	Q post = get_rotation_quaternion(from_quat(q4(vpost.x, vpost.y, vpost.z, vpost.w)));
	if (clip_signbit(dot(from, pre))) pre = clip_quat_neg(pre);
	const bool flip2 = clip_signbit(dot(from, to));
	if (flip2) to = clip_quat_neg(to);
	const float dp = dot(to, post);
	if (flip2 ? dp <= 0.0f : clip_signbit(dp)) post = clip_quat_neg(post);
	const Q q1 = clip_cubic_half(from, true, to, pre, post, w, lv);
	const Q q2 = clip_cubic_half(to, false, from, pre, post, w, lv);
	const Q r = blend_slerp(q1, q2, c, lv);
	return q4(blend_canon(r.x), blend_canon(r.y), blend_canon(r.z), blend_canon(r.w));
}

// The three channels of one bone at one time in one clip, before they become a pose: steps 2 to 6
// of mbik_clip_sample for the channels that have keys.  has_* is false for a channel without keys,
// whose value is then unspecified (step 4 belongs to the caller: clip_sample_bone stores the rest
// pose, clip_layers.h leaves the channel out of the blend).
struct ClipSampled {
	Q rot;
	V3 pos, scl;
	bool has_pos, has_rot, has_scl;
};
// The three channels' searches for their last key <= tp, in step: pos ends as the count of keys <= tp.
GDI void clip_search(ClipChan &pos, ClipChan &rot, ClipChan &scl, double tp) {
	const int nrs = rot.n > scl.n ? rot.n : scl.n, nmax = pos.n > nrs ? pos.n : nrs;
	int step = 1;
	while (step <= (nmax >> 1)) step <<= 1; // the highest power of two <= nmax
	for (; step > 0; step >>= 1) clip_search_step(pos, rot, scl, step, tp);
}
// The picks of three searched channels, and the two key times and the two key values of each:
// twelve independent loads.
struct ClipLoaded {
	ClipPick pp, pr, ps;
	double pTa, pTb, rTa, rTb, sTa, sTb;
	ClipValue pVa, pVb, rVa, rVb, sVa, sVb;
};
GDI ClipLoaded clip_load(const ClipChan &pos, const ClipChan &rot, const ClipChan &scl) {
	ClipLoaded k;
	k.pp = clip_pick(pos), k.pr = clip_pick(rot), k.ps = clip_pick(scl);
	k.pTa = pos.T[k.pp.a], k.pTb = pos.T[k.pp.b], k.rTa = rot.T[k.pr.a], k.rTb = rot.T[k.pr.b], k.sTa = scl.T[k.ps.a], k.sTb = scl.T[k.ps.b];
	k.pVa = pos.V[k.pp.a], k.pVb = pos.V[k.pp.b], k.rVa = rot.V[k.pr.a], k.rVb = rot.V[k.pr.b], k.sVa = scl.V[k.ps.a], k.sVb = scl.V[k.ps.b];
	return k;
}
// Steps 5 and 6 from the loaded keys; rot_n is the rotation channel's key count.
GDI void clip_eval(const ClipLoaded &k, int rot_n, double tp, double length, int lv, ClipSampled &out) {
	const float pc = clip_weight(k.pp.mode, k.pTa, k.pTb, tp, length), rc = clip_weight(k.pr.mode, k.rTa, k.rTb, tp, length),
				sc = clip_weight(k.ps.mode, k.sTa, k.sTb, tp, length);
	if (rot_n == 0 || k.pr.mode == kClipCopy) {
		out.rot = q4(k.rVa.x, k.rVa.y, k.rVa.z, k.rVa.w);
	} else {
		// Quaternion::slerp, not renormalised; a wave none of whose lanes gets here skips it
		const Q r = blend_slerp(q4(k.rVa.x, k.rVa.y, k.rVa.z, k.rVa.w), q4(k.rVb.x, k.rVb.y, k.rVb.z, k.rVb.w), rc, lv);
		out.rot = q4(blend_canon(r.x), blend_canon(r.y), blend_canon(r.z), blend_canon(r.w));
	}
	out.pos = clip_value_vec(k.pp, pc, k.pVa, k.pVb);
	out.scl = clip_value_vec(k.ps, sc, k.sVa, k.sVb);
}
// The same for a sampler's CUBIC form: four key times and four key values a channel, the keys
// before a and after b as well -- twenty-four loads, all issued before any is used.
struct ClipChanKeys {
	ClipPickCubic p;
	double Ta, Tb, Tpre, Tpost;
	ClipValue Va, Vb, Vpre, Vpost;
};
struct ClipLoadedCubic {
	ClipChanKeys pos, rot, scl;
};
GDI ClipLoadedCubic clip_load_cubic(const ClipChan &pos, const ClipChan &rot, const ClipChan &scl) {
	ClipLoadedCubic k;
	const ClipPickCubic pp = clip_pick_cubic(pos), pr = clip_pick_cubic(rot), ps = clip_pick_cubic(scl);
	k.pos.p = pp, k.rot.p = pr, k.scl.p = ps;
	k.pos.Ta = pos.T[pp.a], k.pos.Tb = pos.T[pp.b], k.pos.Tpre = pos.T[pp.pre], k.pos.Tpost = pos.T[pp.post];
	k.rot.Ta = rot.T[pr.a], k.rot.Tb = rot.T[pr.b], k.rot.Tpre = rot.T[pr.pre], k.rot.Tpost = rot.T[pr.post];
	k.scl.Ta = scl.T[ps.a], k.scl.Tb = scl.T[ps.b], k.scl.Tpre = scl.T[ps.pre], k.scl.Tpost = scl.T[ps.post];
	k.pos.Va = pos.V[pp.a], k.pos.Vb = pos.V[pp.b], k.pos.Vpre = pos.V[pp.pre], k.pos.Vpost = pos.V[pp.post];
	k.rot.Va = rot.V[pr.a], k.rot.Vb = rot.V[pr.b], k.rot.Vpre = rot.V[pr.pre], k.rot.Vpost = rot.V[pr.post];
	k.scl.Va = scl.V[ps.a], k.scl.Vb = scl.V[ps.b], k.scl.Vpre = scl.V[ps.pre], k.scl.Vpost = scl.V[ps.post];
	return k;
}
// On a key (c == 0, -0 included) the value is V[a]'s bits: the scheme's own result there,
// lerp(pre + (from - pre), from, w), is `from` only when from - pre is representable.
GDI V3 clip_value_vec_cubic(const ClipChanKeys &k, float c, double length) {
	if (!k.p.cubic) return clip_value_vec(k.p, c, k.Va, k.Vb);
	if (c == 0.0f) return v3(k.Va.x, k.Va.y, k.Va.z);
	return clip_cubic_vec(k.Va, k.Vb, k.Vpre, k.Vpost, clip_cubic_weights(c, clip_span(k.p, k.Tpre, k.Ta, k.Tb, k.Tpost, length)));
}
GDI void clip_eval_cubic(const ClipLoadedCubic &k, int rot_n, double tp, double length, int lv, ClipSampled &out) {
	const float pc = clip_weight(k.pos.p.mode, k.pos.Ta, k.pos.Tb, tp, length), rc = clip_weight(k.rot.p.mode, k.rot.Ta, k.rot.Tb, tp, length),
				sc = clip_weight(k.scl.p.mode, k.scl.Ta, k.scl.Tb, tp, length);
	const ClipChanKeys &r = k.rot;
	if (rot_n == 0 || r.p.mode == kClipCopy) {
		out.rot = q4(r.Va.x, r.Va.y, r.Va.z, r.Va.w);
	} else if (r.p.cubic) {
		// the spherical cubic, behind a per-lane branch as the slerp is
		out.rot = clip_cubic_rot(r.Va, r.Vb, r.Vpre, r.Vpost, rc, clip_cubic_weights(rc, clip_span(r.p, r.Tpre, r.Ta, r.Tb, r.Tpost, length)), lv);
	} else {
		const Q q = blend_slerp(q4(r.Va.x, r.Va.y, r.Va.z, r.Va.w), q4(r.Vb.x, r.Vb.y, r.Vb.z, r.Vb.w), rc, lv);
		out.rot = q4(blend_canon(q.x), blend_canon(q.y), blend_canon(q.z), blend_canon(q.w));
	}
	out.pos = clip_value_vec_cubic(k.pos, pc, length);
	out.scl = clip_value_vec_cubic(k.scl, sc, length);
}
// One end: the loads and the evaluation of three searched channels, in the sampler's form.
template <bool CUBIC>
GDI void clip_load_eval(const ClipChan &pos, const ClipChan &rot, const ClipChan &scl, double tp, double length, int lv, ClipSampled &out) {
	if constexpr (CUBIC) clip_eval_cubic(clip_load_cubic(pos, rot, scl), rot.n, tp, length, lv, out);
	else clip_eval(clip_load(pos, rot, scl), rot.n, tp, length, lv, out);
}
// hp / hr / hs: the bone's three headers in `info`'s clip, already loaded -- a caller that samples
// several clips loads the next one's while this one's keys are searched.  What a lane waits for is
// memory, so the loads are arranged in as few dependent rounds as the data allows: the search
// steps, three loads each; then the two key times and the two key values of all three channels at
// once.  clip_sample_channels_at starts from tp, a finite time step 3 has already mapped into the
// clip (root_motion.h samples the ends of a frame's segments, the clip's end among them);
// clip_sample_channels maps the raw time t and calls it.
template <bool CUBIC = false>
GDI ClipSampled clip_sample_channels_at(const ClipView &v, const ClipInfo &info, const ClipHeader &hp, const ClipHeader &hr,
		const ClipHeader &hs, double tp, int lv) {
	ClipChan pos = clip_chan(v, hp), rot = clip_chan(v, hr), scl = clip_chan(v, hs);
	ClipSampled out;
	out.has_pos = pos.n != 0, out.has_rot = rot.n != 0, out.has_scl = scl.n != 0;
	clip_search(pos, rot, scl, tp);
	clip_load_eval<CUBIC>(pos, rot, scl, tp, info.length, lv, out);
	return out;
}
template <bool CUBIC = false>
GDI ClipSampled clip_sample_channels(const ClipView &v, const ClipInfo &info, const ClipHeader &hp, const ClipHeader &hr,
		const ClipHeader &hs, double t, int lv) {
	if (!clip_finite(t)) { // no key is read
		ClipSampled out;
		out.has_pos = hp.key_count != 0, out.has_rot = hr.key_count != 0, out.has_scl = hs.key_count != 0;
		const float nan = clip_nan();
		out.rot = q4(nan, nan, nan, nan), out.pos = v3(nan, nan, nan), out.scl = v3(nan, nan, nan);
		return out;
	}
	return clip_sample_channels_at<CUBIC>(v, info, hp, hr, hs, clip_time(t, info.length, info.loop_mode), lv);
}

// One bone of one skeleton: out10 = the pose (quaternion xyzw, position, scale) of `bone` at raw
// time t in clip `clip`: the sampled channels, and the rest pose's bits where a channel has no keys.
template <bool CUBIC = false>
GDI void clip_sample_bone(const ClipView &v, int clip, int bone, double t, int lv, float *out10) {
	if (clip < 0 || clip >= v.clip_count) {
		for (int f = 0; f < 10; f++) out10[f] = clip_nan();
		return;
	}
	const ClipInfo info = v.clips[clip];
	const ClipHeader *h = v.headers + ((int64_t)clip * v.B + bone) * 3;
	const float *rest = v.rest + (int64_t)bone * 10;
	const ClipSampled s = clip_sample_channels<CUBIC>(v, info, h[0], h[1], h[2], t, lv);
	out10[0] = s.has_rot ? s.rot.x : rest[0], out10[1] = s.has_rot ? s.rot.y : rest[1];
	out10[2] = s.has_rot ? s.rot.z : rest[2], out10[3] = s.has_rot ? s.rot.w : rest[3];
	out10[4] = s.has_pos ? s.pos.x : rest[4], out10[5] = s.has_pos ? s.pos.y : rest[5], out10[6] = s.has_pos ? s.pos.z : rest[6];
	out10[7] = s.has_scl ? s.scl.x : rest[7], out10[8] = s.has_scl ? s.scl.y : rest[8], out10[9] = s.has_scl ? s.scl.z : rest[9];
}

} // namespace mbik
