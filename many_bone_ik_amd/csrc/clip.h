// Animation clip sampling, shared by the device kernel (k_clip.hip) and the host entry
// mbik_clip_sample_cpu (host_clip.cpp): Godot 4.3's Animation::position_track_interpolate,
// rotation_track_interpolate and scale_track_interpolate (Animation::_interpolate) for
// INTERPOLATION_NEAREST / INTERPOLATION_LINEAR, LOOP_NONE / LOOP_LINEAR, forward playback and key
// transitions of 1, for every bone of a skeleton at that skeleton's time in that skeleton's clip.
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
// hp / hr / hs: the bone's three headers in `info`'s clip, already loaded -- a caller that samples
// several clips loads the next one's while this one's keys are searched.  What a lane waits for is
// memory, so the loads are arranged in as few dependent rounds as the data allows: the search
// steps, three loads each; then the two key times and the two key values of all three channels at
// once.  clip_sample_channels_at starts from tp, a finite time step 3 has already mapped into the
// clip (root_motion.h samples the ends of a frame's segments, the clip's end among them);
// clip_sample_channels maps the raw time t and calls it.
GDI ClipSampled clip_sample_channels_at(const ClipView &v, const ClipInfo &info, const ClipHeader &hp, const ClipHeader &hr,
		const ClipHeader &hs, double tp, int lv) {
	ClipChan pos = clip_chan(v, hp), rot = clip_chan(v, hr), scl = clip_chan(v, hs);
	ClipSampled out;
	out.has_pos = pos.n != 0, out.has_rot = rot.n != 0, out.has_scl = scl.n != 0;
	clip_search(pos, rot, scl, tp);
	clip_eval(clip_load(pos, rot, scl), rot.n, tp, info.length, lv, out);
	return out;
}
GDI ClipSampled clip_sample_channels(const ClipView &v, const ClipInfo &info, const ClipHeader &hp, const ClipHeader &hr,
		const ClipHeader &hs, double t, int lv) {
	if (!clip_finite(t)) { // no key is read
		ClipSampled out;
		out.has_pos = hp.key_count != 0, out.has_rot = hr.key_count != 0, out.has_scl = hs.key_count != 0;
		const float nan = clip_nan();
		out.rot = q4(nan, nan, nan, nan), out.pos = v3(nan, nan, nan), out.scl = v3(nan, nan, nan);
		return out;
	}
	return clip_sample_channels_at(v, info, hp, hr, hs, clip_time(t, info.length, info.loop_mode), lv);
}

// One bone of one skeleton: out10 = the pose (quaternion xyzw, position, scale) of `bone` at raw
// time t in clip `clip`: the sampled channels, and the rest pose's bits where a channel has no keys.
GDI void clip_sample_bone(const ClipView &v, int clip, int bone, double t, int lv, float *out10) {
	if (clip < 0 || clip >= v.clip_count) {
		for (int f = 0; f < 10; f++) out10[f] = clip_nan();
		return;
	}
	const ClipInfo info = v.clips[clip];
	const ClipHeader *h = v.headers + ((int64_t)clip * v.B + bone) * 3;
	const float *rest = v.rest + (int64_t)bone * 10;
	const ClipSampled s = clip_sample_channels(v, info, h[0], h[1], h[2], t, lv);
	out10[0] = s.has_rot ? s.rot.x : rest[0], out10[1] = s.has_rot ? s.rot.y : rest[1];
	out10[2] = s.has_rot ? s.rot.z : rest[2], out10[3] = s.has_rot ? s.rot.w : rest[3];
	out10[4] = s.has_pos ? s.pos.x : rest[4], out10[5] = s.has_pos ? s.pos.y : rest[5], out10[6] = s.has_pos ? s.pos.z : rest[6];
	out10[7] = s.has_scl ? s.scl.x : rest[7], out10[8] = s.has_scl ? s.scl.y : rest[8], out10[9] = s.has_scl ? s.scl.z : rest[9];
}

} // namespace mbik
