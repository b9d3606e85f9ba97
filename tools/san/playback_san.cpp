// playback.h under ASan + UBSan: the host path behind mbik_playback_advance_cpu (the kernel runs
// the same per-skeleton code) on built-in crowds: empty and full fade lists, 1 and 8 slots, no
// command and one command, aimed at the first and at the last skeleton, plays that overflow the
// fade list, stops, transitions and commands with fields outside every table.  Every array is a
// heap block of exactly its size -- the clip infos, next, the blend times, the [count][K] slots,
// the flag words, the commands, the records, the previous times and the events -- so a slot, a
// command or a table entry read or written out of range is a sanitizer report; what each case must
// leave behind (a compact fade list, off slots all +0, weights in [0, 1], positions inside their
// clips) is checked as well.
//   playback_san   -> exit 0 and one line per case, or a sanitizer report
#include <cmath>
#include <cstdio>
#include <memory>
#include <vector>

#include "../../many_bone_ik_amd/csrc/playback.h"

namespace {
using namespace mbik;

constexpr int kClips = 4;
constexpr int kCount = 70;

struct Tables {
	std::unique_ptr<ClipInfo[]> clips{new ClipInfo[kClips]};
	std::unique_ptr<int32_t[]> next{new int32_t[kClips]};
	std::unique_ptr<float[]> blend{new float[kClips * kClips]};
	Tables() {
		const double length[kClips] = {0.7, 1.0, 3.0, 0.5};
		const int32_t follow[kClips] = {-1, 3, -1, 1};
		for (int c = 0; c < kClips; c++) clips[c] = ClipInfo{length[c], c % 2 == 0 ? 1 : 0, 0}, next[c] = follow[c];
		for (int i = 0; i < kClips * kClips; i++) blend[i] = 0.1f * (float)(i % 5);
	}
	PlaybackTables view(bool desc) const { return PlaybackTables{kClips, desc ? 0.25f : 0.0f, clips.get(), desc ? next.get() : nullptr, desc ? blend.get() : nullptr}; }
};

struct Crowd {
	int K;
	std::unique_ptr<PlaybackSlot[]> slots;
	std::unique_ptr<uint32_t[]> flags;
	// full: every fade slot on; else slot 0 only (every seventh skeleton off)
	Crowd(int K, bool full, const Tables &t) : K(K), slots(new PlaybackSlot[(size_t)kCount * K]), flags(new uint32_t[kCount]) {
		for (int s = 0; s < kCount; s++) {
			flags[s] = s % 9 == 3 ? kPlaybackStarted : 0u;
			for (int j = 0; j < K; j++) {
				const int c = (s + j) % kClips;
				const bool on = s % 7 != 6 && (j == 0 || full);
				slots[(size_t)s * K + j] = on ? PlaybackSlot{t.clips[c].length * ((s * 13 + j * 5) % 17) / 16.0, c, s % 4 == 1 ? -1.0f : 1.5f,
													  j ? 0.9f / (float)K : 0.0f, j ? 4.0f + (float)j : 0.0f}
											  : playback_off();
			}
		}
	}
};

uint32_t fbits(float x) {
	uint32_t u;
	std::memcpy(&u, &x, 4);
	return u;
}

// Frames of one crowd with the same command list each frame; returns false when a state or a record breaks an invariant.
bool run(const Tables &t, bool desc, Crowd &c, const std::vector<PlaybackCmd> &cmds, int frames, double delta, long &events_seen, long &on_fades) {
	const PlaybackTables T = t.view(desc);
	const int K = c.K;
	std::unique_ptr<ClipLayer[]> layers(new ClipLayer[(size_t)kCount * K]);
	std::unique_ptr<double[]> prev(new double[(size_t)kCount * K]);
	std::unique_ptr<uint8_t[]> events(new uint8_t[kCount]);
	std::unique_ptr<PlaybackCmd[]> list(cmds.empty() ? nullptr : new PlaybackCmd[cmds.size()]);
	for (size_t i = 0; i < cmds.size(); i++) list[i] = cmds[i];
	for (int frame = 0; frame < frames; frame++) {
		for (int s = 0; s < kCount; s++) {
			const uint32_t ev = playback_skeleton(T, PlaybackRecords{c.slots.get() + (size_t)s * K, c.flags.get() + s}, K, s, delta, 1.0f, list.get(),
					(int)cmds.size(), PlaybackDirect{layers.get() + (size_t)s * K, prev.get() + (size_t)s * K});
			events[s] = (uint8_t)ev;
			events_seen |= ev;
		}
		for (int s = 0; s < kCount; s++) {
			if (c.flags[s] & ~(kPlaybackStarted | kPlaybackEnded)) return false;
			bool off_seen = false;
			float sum = 0.0f;
			for (int j = 0; j < K; j++) {
				const PlaybackSlot &r = c.slots[(size_t)s * K + j];
				const ClipLayer &l = layers[(size_t)s * K + j];
				if (r.clip == kClipLayerOff) {
					off_seen = true;
					if (fbits(r.speed) | fbits(r.blend_left) | fbits(r.blend_time) | clip_bits(r.pos)) return false;
					continue;
				}
				if (off_seen || r.clip < 0 || r.clip >= kClips) return false;
				if (!(r.pos >= 0 && r.pos <= t.clips[r.clip].length)) return false;
				if (j == 0 && (fbits(r.blend_left) | fbits(r.blend_time))) return false;
				if (j > 0 && !(r.blend_time > 0)) return false;
				on_fades += j > 0;
				if (!(events[s] & kPlaybackTransitioned) && l.clip != kClipLayerOff) {
					if (!(l.weight >= 0 && l.weight <= 1) || !(l.time >= 0 && l.time <= t.clips[l.clip].length)) return false;
					sum += l.weight;
				}
			}
			if (sum > 1.0001f) return false;
		}
	}
	return true;
}

int report(const char *name, int K, size_t cmds, bool ok, long events, long fades) {
	std::printf("%s: %s K=%d count=%d cmds=%zu events=%ld fades=%ld\n", name, ok ? "ok" : "FAILED", K, kCount, cmds, events, fades);
	return ok ? 0 : 1;
}

} // namespace

int main() {
	int bad = 0;
	const Tables t;
	const double nan = std::nan("");
	for (int K : {1, 8})
		for (int full = 0; full < 2; full++) {
			char name[64];
			const char *fill = full ? "full" : "empty";
			struct Case {
				const char *what;
				std::vector<PlaybackCmd> cmds;
			};
			const Case cases[] = {
					{"no_cmds", {}},
					{"first", {PlaybackCmd{nan, 0, 2, 0.5f, 1.0f}}},
					{"last", {PlaybackCmd{0.3, kCount - 1, 1, -1.0f, -1.0f}}},
					{"stop_last", {PlaybackCmd{nan, kCount - 1, kClipLayerOff, 0.0f, 1.0f}}},
					{"past_the_crowd", {PlaybackCmd{nan, kCount, 1, 0.5f, 1.0f}}},
					{"before_the_crowd", {PlaybackCmd{nan, -1, 1, 0.5f, 1.0f}}},
					{"bad_clip", {PlaybackCmd{nan, 5, INT32_MAX, 0.5f, 1.0f}}},
					{"bad_clip_low", {PlaybackCmd{nan, 5, INT32_MIN, 0.5f, 1.0f}}},
					{"bad_speed", {PlaybackCmd{nan, 0, 1, 0.5f, INFINITY}}},
					{"overflow", std::vector<PlaybackCmd>(12, PlaybackCmd{1e9, 33, 3, 5.0f, 2.0f})},
					{"unsorted", {PlaybackCmd{nan, 40, 1, 0.5f, 1.0f}, PlaybackCmd{nan, 2, 0, 0.5f, 1.0f}, PlaybackCmd{nan, 69, 2, 0.5f, 1.0f},
										 PlaybackCmd{nan, 0, 3, 0.5f, 1.0f}}},
			};
			for (const Case &c : cases)
				for (int desc = 0; desc < 2; desc++) {
					Crowd crowd(K, full != 0, t);
					long events = 0, fades = 0;
					const bool ok = run(t, desc != 0, crowd, c.cmds, 6, 0.11, events, fades);
					std::snprintf(name, sizeof name, "%s_%s_k%d_%s", c.what, fill, K, desc ? "desc" : "plain");
					bad += report(name, K, c.cmds.size(), ok, events, fades);
				}
		}
	return bad ? 1 : 0;
}
