// Playback, shared by the device kernel (k_playback.hip) and the host entry
// mbik_playback_advance_cpu (host_playback.cpp): Godot 4.3's AnimationPlayer for a crowd.  Per
// skeleton a current animation (slot 0) and up to K - 1 clips fading out behind it (slots 1..);
// one advance applies the frame's commands (play, stop), moves every slot's position by the
// frame's step, lets the fades run down, writes the (time, clip, weight) records and previous
// times the layered samplers and root motion read, and starts the clip that follows one that
// ended.  One code path for both sides, made of IEEE-exact operations only -- double add,
// multiply, divide and compare, float subtract and add, clip.h's clip_time -- with nothing fused,
// so the device and the host produce the same bits.  include/mbik.h states the semantics;
// DESIGN.md §25.
#pragma once

#include "clip_layers.h"

namespace mbik {

// mbik_playback_slot and mbik_playback_cmd: 24 bytes each.
struct PlaybackSlot {
	double pos;
	int32_t clip;
	float speed, blend_left, blend_time;
};
struct PlaybackCmd {
	double start;
	int32_t skeleton, clip;
	float blend_time, speed;
};
static_assert(sizeof(PlaybackSlot) == 24 && sizeof(PlaybackCmd) == 24, "the public records are 24 bytes");

constexpr uint32_t kPlaybackStarted = 1u, kPlaybackEnded = 2u; // a skeleton's flags; events as well
constexpr uint32_t kPlaybackLooped = 4u, kPlaybackTransitioned = 8u, kPlaybackBadCommand = 16u, kPlaybackFadeDropped = 32u;

// What an object takes from its set and its desc: on the device for mbik_playback, host memory for
// the CPU entry.  next and blend_times may be null.
struct PlaybackTables {
	int32_t clip_count;
	float default_blend_time;
	const ClipInfo *clips;    // [clip_count]
	const int32_t *next;      // [clip_count], -1 none
	const float *blend_times; // [clip_count][clip_count] from, to
};

// One skeleton's state in the object's device memory: structure of arrays, slot j of skeleton s at
// [j * stride + s] of each field, so a wave's loads and stores of a field are one run.  One
// allocation: pos [K][stride] doubles, then clip, speed, blend_left, blend_time [K][stride] and
// flags [stride], 4 bytes each; stride is the capacity rounded up to a multiple of 4, so every
// plane starts on a 16-byte boundary.  One base pointer instead of six keeps the kernel's
// scalar registers free of spills.
struct PlaybackState {
	unsigned char *base;
	int64_t stride;
	int32_t K;
	GDI double *pos(int j, int64_t s) const { return reinterpret_cast<double *>(base) + (int64_t)j * stride + s; }
	// plane 0 clip, 1 speed, 2 blend_left, 3 blend_time; plane 4, j 0: flags
	GDI uint32_t *word(int plane, int j, int64_t s) const {
		return reinterpret_cast<uint32_t *>(base + (int64_t)K * stride * 8) + ((int64_t)plane * K + j) * stride + s;
	}
	GDI int32_t *clip(int j, int64_t s) const { return reinterpret_cast<int32_t *>(word(0, j, s)); }
	GDI float *speed(int j, int64_t s) const { return reinterpret_cast<float *>(word(1, j, s)); }
	GDI float *blend_left(int j, int64_t s) const { return reinterpret_cast<float *>(word(2, j, s)); }
	GDI float *blend_time(int j, int64_t s) const { return reinterpret_cast<float *>(word(3, j, s)); }
	GDI uint32_t *flags(int64_t s) const { return word(4, 0, s); }
	GDI size_t bytes() const { return (size_t)stride * ((size_t)K * 24 + 4); }
};
struct PlaybackLane {
	PlaybackState st;
	int64_t s;
	GDI PlaybackSlot get(int j) const { return PlaybackSlot{*st.pos(j, s), *st.clip(j, s), *st.speed(j, s), *st.blend_left(j, s), *st.blend_time(j, s)}; }
	GDI void put(int j, const PlaybackSlot &v) const {
		*st.pos(j, s) = v.pos, *st.clip(j, s) = v.clip, *st.speed(j, s) = v.speed, *st.blend_left(j, s) = v.blend_left, *st.blend_time(j, s) = v.blend_time;
	}
	// a slot that stays where it is changes its position and what is left of its fade only
	GDI void put_advanced(int j, const PlaybackSlot &v) const { *st.pos(j, s) = v.pos, *st.blend_left(j, s) = v.blend_left; }
	GDI void put_pos(int j, double pos) const { *st.pos(j, s) = pos; }
	GDI uint32_t flags() const { return *st.flags(s); }
	GDI void set_flags(uint32_t f) const { *st.flags(s) = f; }
};
// The same for the CPU entry's [K] public records.
struct PlaybackRecords {
	PlaybackSlot *slots;
	uint32_t *flag;
	GDI PlaybackSlot get(int j) const { return slots[j]; }
	GDI void put(int j, const PlaybackSlot &v) const { slots[j] = v; }
	GDI void put_advanced(int j, const PlaybackSlot &v) const { slots[j] = v; }
	GDI void put_pos(int j, double pos) const { slots[j].pos = pos; }
	GDI uint32_t flags() const { return *flag; }
	GDI void set_flags(uint32_t f) const { *flag = f; }
};
// Where a skeleton's K records and previous times go: straight to the output arrays.
struct PlaybackDirect {
	ClipLayer *layers;
	double *prev;
	GDI void put(int j, const ClipLayer &rec, double time_prev) const { layers[j] = rec, prev[j] = time_prev; }
};

GDI PlaybackSlot playback_off() { return PlaybackSlot{0.0, kClipLayerOff, 0.0f, 0.0f, 0.0f}; }
GDI bool playback_finite(float x) {
	union {
		float f;
		uint32_t u;
	} c{x};
	return (c.u & 0x7f800000u) != 0x7f800000u;
}
GDI bool playback_signbit(float x) {
	union {
		float f;
		uint32_t u;
	} c{x};
	return (c.u >> 31) != 0;
}
// A start that is not finite: the clip's own start.
GDI double playback_no_start() {
	union {
		uint64_t u;
		double d;
	} c{0x7ff8000000000000ull};
	return c.d;
}
// max(0, 1 - sum): the weight that is left for the current animation.
GDI float playback_rest_weight(float sum) {
	const float w = 1.0f - sum;
	return w > 0.0f ? w : 0.0f;
}

// Rule A's play: the current animation, if there is one and the blend time is positive, becomes
// the newest fade, and slot 0 starts `clip`.  The state is changed in place through `st`.
template <class St>
GDI void playback_play(const PlaybackTables &T, const St &st, int K, int clip, double start, float speed, float blend_time, uint32_t &flags,
		uint32_t &events) {
	const PlaybackSlot cur = st.get(0);
	const bool playing = cur.clip != kClipLayerOff;
	float bt = T.default_blend_time;
	if (blend_time >= 0.0f) bt = blend_time;
	else if (playing && T.blend_times) bt = T.blend_times[(int64_t)cur.clip * T.clip_count + clip];
	if (playing && bt > 0.0f) {
		float sum = 0.0f;
		int fades = 0;
		for (int j = 1; j < K; j++) {
			const PlaybackSlot f = st.get(j);
			if (f.clip == kClipLayerOff) break;
			sum = sum + f.blend_left;
			fades++;
		}
		const PlaybackSlot fade{cur.pos, cur.clip, cur.speed, playback_rest_weight(sum), bt};
		if (fades + 1 < K) {
			st.put(fades + 1, fade);
		} else { // no free slot: the oldest fade leaves; with one layer, the new one
			events |= kPlaybackFadeDropped;
			for (int j = 1; j + 1 < K; j++) st.put(j, st.get(j + 1));
			if (K > 1) st.put(K - 1, fade);
		}
	} else {
		for (int j = 1; j < K; j++) {
			if (st.get(j).clip == kClipLayerOff) break;
			st.put(j, playback_off());
		}
	}
	const ClipInfo info = T.clips[clip];
	const double at = clip_finite(start) ? clip_time(start, info.length, info.loop_mode) : (playback_signbit(speed) ? info.length : 0.0);
	st.put(0, PlaybackSlot{at, clip, speed, 0.0f, 0.0f});
	flags = kPlaybackStarted;
}

// The first command with skeleton >= s: the search include/mbik.h writes out.  It reads entries
// of [0, cmd_count) only, whatever their order.
GDI int playback_first_command(const PlaybackCmd *cmds, int cmd_count, int s) {
	int lo = 0, hi = cmd_count;
	while (lo < hi) {
		const int mid = lo + ((hi - lo) >> 1);
		if (cmds[mid].skeleton < s) lo = mid + 1;
		else hi = mid;
	}
	return lo;
}

// A slot's position one frame on: pos + step mapped into its clip; a sum that is not finite
// leaves the position where it is.  n is the sum.
GDI double playback_step(double pos, double step, const ClipInfo &info, double &n) {
	n = pos + step;
	return clip_finite(n) ? clip_time(n, info.length, info.loop_mode) : pos;
}

// One skeleton, rules A to D: its state through `st`, its K records and previous times through
// `out`; returns its events.  The slots are walked in loops over named state (K is a run-time
// value; there is no array of per-slot values), with a write cursor for the compaction.
template <class St, class Out>
GDI uint32_t playback_skeleton(const PlaybackTables &T, const St &st, int K, int s, double delta, float speed_scale, const PlaybackCmd *cmds,
		int cmd_count, const Out &out) {
	const uint32_t flags_in = st.flags();
	uint32_t flags = flags_in, events = 0;
	// A. commands
	for (int i = playback_first_command(cmds, cmd_count, s); i < cmd_count; i++) {
		const PlaybackCmd c = cmds[i];
		if (c.skeleton != s) break;
		if (c.clip == kClipLayerOff) {
			for (int j = 0; j < K; j++) {
				if (st.get(j).clip == kClipLayerOff) break;
				st.put(j, playback_off());
			}
			flags = 0;
		} else if (c.clip < 0 || c.clip >= T.clip_count || !playback_finite(c.speed)) {
			events |= kPlaybackBadCommand;
		} else {
			playback_play(T, st, K, c.clip, c.start, c.speed, c.blend_time, flags, events);
		}
	}
	// B. advance
	const double g = (double)speed_scale * delta;
	const double ag = g < 0 ? -g : g;
	PlaybackSlot cur = st.get(0);
	const bool playing = cur.clip != kClipLayerOff;
	const double prev0 = cur.pos;
	bool ended = false;
	if (playing) {
		if (flags & kPlaybackStarted) {
			flags &= ~kPlaybackStarted, events |= kPlaybackStarted; // the first frame of a clip shows its start
		} else if (!(flags & kPlaybackEnded)) {
			const ClipInfo info = T.clips[cur.clip];
			const double step = g * (double)cur.speed;
			double n;
			cur.pos = playback_step(cur.pos, step, info, n);
			st.put_pos(0, cur.pos);
			if (info.loop_mode == 0) {
				ended = (step > 0 && n >= info.length) || (step < 0 && n <= 0);
				if (ended) flags |= kPlaybackEnded, events |= kPlaybackEnded;
			} else if (cur.pos != n) {
				events |= kPlaybackLooped;
			}
		}
	}
	// the fades, compacted as they go; C. their records
	float sum = 0.0f;
	int w = 1, j = 1;
	for (; j < K; j++) {
		PlaybackSlot f = st.get(j);
		if (f.clip == kClipLayerOff) break; // an off slot is followed only by off slots
		const double prev = f.pos;
		if (!ended) { // a clip that ends takes its fades with it
			const ClipInfo info = T.clips[f.clip];
			double n;
			f.pos = playback_step(f.pos, g * (double)f.speed, info, n);
			f.blend_left = f.blend_left - (float)(ag / (double)f.blend_time);
		}
		if (ended || !(f.blend_left > 0.0f)) continue;
		sum = sum + f.blend_left;
		if (w == j) st.put_advanced(w, f);
		else st.put(w, f);
		out.put(w, ClipLayer{f.pos, f.clip, f.blend_left}, prev);
		w++;
	}
	for (int k = w; k < j; k++) st.put(k, playback_off());
	for (int k = w; k < K; k++) out.put(k, ClipLayer{0.0, kClipLayerOff, 0.0f}, 0.0);
	if (playing) out.put(0, ClipLayer{cur.pos, cur.clip, playback_rest_weight(sum)}, prev0);
	else out.put(0, ClipLayer{0.0, kClipLayerOff, 0.0f}, 0.0);
	// D. the clip that follows the one that ended
	if (ended && T.next) {
		const int next = T.next[cur.clip];
		if (next >= 0) {
			playback_play(T, st, K, next, playback_no_start(), cur.speed, -1.0f, flags, events);
			events |= kPlaybackTransitioned;
		}
	}
	if (flags != flags_in) st.set_flags(flags);
	return events;
}

} // namespace mbik
