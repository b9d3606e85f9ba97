// root_motion.h under ASan + UBSan: the host paths behind mbik_clip_root_motion[_layers]_cpu and
// mbik_root_motion_apply_cpu (the kernels run the same per-skeleton code) on built-in clip sets: an
// untracked root, single keys, frame ends exactly on keys, on 0 and on the length, both seam
// branches, layers that are off or invalid, 1 and 8 layers, both modes, and the apply with and
// without orthonormalisation.  Every table is a heap block of exactly its size -- headers
// [clips][bones][3], times and values keys + 1 (the spare entry), the rest pose, the layer records,
// the previous times, the poses and the outputs -- so a key index, a header or a record read out of
// range is a sanitizer report; what each case must produce (start bits, NaN bits, finite values,
// the rest pose's root record) is checked as well.
//   root_motion_san   -> exit 0 and one line per case, or a sanitizer report
#include <cmath>
#include <cstdio>
#include <vector>

#include "../../many_bone_ik_amd/csrc/root_motion.h"

namespace {
using namespace mbik;

uint32_t g_state = 20261022u;
float rnd(float lo, float hi) { // LCG, top 24 bits
	g_state = g_state * 1664525u + 1013904223u;
	return lo + (hi - lo) * (float)(g_state >> 8) * (1.0f / 16777216.0f);
}

uint32_t bits(float x) {
	uint32_t u;
	std::memcpy(&u, &x, 4);
	return u;
}

constexpr float kUnwritten = -12345.678f;
const float kStart[10] = {0, 0, 0, 1, 0, 0, 0, 0, 0, 0};

// A clip set in clip.h's repacked form.  keys_of(c, bone, channel) decides each channel's key count.
struct Set {
	int B, clip_count;
	std::vector<ClipInfo> clips;
	std::vector<ClipHeader> headers;
	std::vector<double> times;
	std::vector<ClipValue> values;
	std::vector<float> rest;
	ClipView view() const { return ClipView{B, clip_count, clips.data(), headers.data(), times.data(), values.data(), rest.data()}; }
};

template <typename KeysOf>
Set make_set(int B, int clip_count, bool inside, KeysOf keys_of) {
	Set s{B, clip_count, {}, {}, {}, {}, {}};
	s.rest.resize((size_t)B * 10);
	for (float &r : s.rest) r = rnd(2.0f, 3.0f); // no motion record holds a value in [2, 3]
	for (int c = 0; c < clip_count; c++) {
		const double length = 1.0 + c;
		s.clips.push_back(ClipInfo{length, c % 2 == 0 ? 1 : 0, 0});
		for (int b = 0; b < B; b++)
			for (int ch = 0; ch < 3; ch++) {
				const int n = keys_of(c, b, ch);
				if (n == 0) {
					s.headers.push_back(ClipHeader{0, 0, 0, 0});
					continue;
				}
				s.headers.push_back(ClipHeader{(int32_t)s.times.size(), n, ((b + ch) % 3 ? kClipLinear : 0) | (c % 2 == 0 ? kClipWrap : 0), 0});
				for (int k = 0; k < n; k++) {
					// inside: keys strictly inside (0, length), so both ends of the clip interpolate across the seam
					const double lo = inside ? 0.1 : 0.0, hi = inside ? 0.9 : 1.0;
					s.times.push_back(n == 1 ? lo * length : length * (lo + (hi - lo) * k / (n - 1)));
					float q[4], l = 0;
					for (float &v : q) v = rnd(-1.0f, 1.0f), l += v * v;
					if (ch == 1) s.values.push_back(ClipValue{q[0] / std::sqrt(l), q[1] / std::sqrt(l), q[2] / std::sqrt(l), q[3] / std::sqrt(l)});
					else s.values.push_back(ClipValue{q[0], q[1], q[2], 0.0f});
				}
			}
	}
	s.times.push_back(0.0);
	s.values.push_back(ClipValue{0.0f, 0.0f, 0.0f, 0.0f});
	s.clips.shrink_to_fit(), s.times.shrink_to_fit(), s.values.shrink_to_fit(), s.headers.shrink_to_fit();
	return s;
}

struct Tally {
	long floats = 0, nan = 0, start = 0, fixed = 0; // fixed: skeletons whose root record in the pose is the rest pose's
};

// Runs [count][K] records (or, with K == 0, the plain form on `time` / `clip`) with a pose buffer.
Tally run(const Set &s, int root, const std::vector<ClipLayer> &layers, const std::vector<double> &prev, int K, uint32_t flags,
		const std::vector<double> &time, const std::vector<int32_t> &clip) {
	const int count = (int)prev.size() / (K ? K : 1);
	std::vector<float> out((size_t)count * 10, kUnwritten), pose((size_t)count * s.B * 10, kUnwritten);
	out.shrink_to_fit(), pose.shrink_to_fit();
	const ClipView v = s.view();
	for (int i = 0; i < count; i++) {
		float *pose_s = pose.data() + (size_t)i * s.B * 10;
		if (K) root_motion_skeleton(v, RootLayers{layers.data() + (size_t)i * K, prev.data() + (size_t)i * K}, K, flags, root, 0, out.data() + (size_t)i * 10, pose_s);
		else root_motion_skeleton(v, RootPlain{ClipLayer{time[i], clip[i], 1.0f}, prev[i]}, 1, 0u, root, 0, out.data() + (size_t)i * 10, pose_s);
	}
	Tally t;
	for (int i = 0; i < count; i++) {
		for (int f = 0; f < 10; f++) {
			const float x = out[(size_t)i * 10 + f];
			t.floats++;
			if (x != x) {
				if (bits(x) != 0x7fc00000u) return Tally{-1, 0, 0, 0}; // a NaN that is not the canonical one
				t.nan++;
				continue;
			}
			if (x == kUnwritten) return Tally{-1, 0, 0, 0};
			if (bits(x) == bits(kStart[f])) t.start++;
		}
		bool fixed = true, touched = false;
		for (int b = 0; b < s.B; b++)
			for (int f = 0; f < 10; f++) {
				const float p = pose[((size_t)i * s.B + b) * 10 + f];
				if (b == root) fixed = fixed && bits(p) == bits(s.rest[(size_t)b * 10 + f]), touched = touched || p != kUnwritten;
				else if (p != kUnwritten) return Tally{-1, 0, 0, 0}; // another bone written
			}
		if (touched && !fixed) return Tally{-1, 0, 0, 0}; // a root record written in part
		t.fixed += fixed;
	}
	return t;
}

int report(const char *name, const Set &s, const Tally &t, int count, int K, bool ok) {
	std::printf("%s: %s B=%d clips=%d count=%d K=%d floats=%ld nan=%ld start=%ld fixed=%ld\n", name, t.floats < 0 || !ok ? "FAILED" : "ok", s.B,
			s.clip_count, count, K, t.floats, t.nan, t.start, t.fixed);
	return t.floats < 0 || !ok ? 1 : 0;
}

// Frames (t0, t1) of interest in a clip of `length` whose keys lie as make_set lays them out: inside one
// pass, across the seam, a whole loop and more, of no length, backwards, ends exactly on keys, on 0 and on
// the length, far from 0.
void frames_for(double length, bool inside, std::vector<double> &t0, std::vector<double> &t1) {
	const double lo = inside ? 0.1 : 0.0, hi = inside ? 0.9 : 1.0;
	std::vector<double> marks{0.0, -0.0, length, 0.05 * length, 0.5 * length, 0.95 * length};
	for (int n : {2, 3, 17})
		for (int k = 0; k < n; k++) marks.push_back(length * (lo + (hi - lo) * k / (n - 1)));
	for (size_t i = 0; i < marks.size(); i++) {
		const double a = marks[i], b = marks[(i * 7 + 3) % marks.size()];
		for (double shift : {0.0, length, -length, 1e6 * length}) t0.push_back(a + shift), t1.push_back(b + shift);
		t0.push_back(a), t1.push_back(b + length);       // one loop on
		t0.push_back(a), t1.push_back(a);                 // no length
		t0.push_back(a + 0.9 * length), t1.push_back(a + 1.1 * length); // across the seam, whatever a is
	}
}

} // namespace

int main() {
	int bad = 0;
	const int kinds[] = {0, 1, 2, 3, 17};
	const auto mixed = [&](int c, int b, int ch) { return kinds[(c * 7 + b * 3 + ch) % 5]; };
	const auto tracked = [&](int c, int b, int ch) { return kinds[1 + (c * 7 + b * 3 + ch) % 4]; };
	struct Case {
		const char *name;
		Set set;
		bool inside;
		int root;
		bool still; // a root without keys, or with one key a channel: nothing changes over a frame, every record is the start values
	};
	Case cases[] = {
			{"untracked_root", make_set(3, 2, false, [&](int c, int b, int ch) { return b == 1 ? 0 : mixed(c, b, ch); }), false, 1, true},
			{"single_keys", make_set(3, 2, false, [](int, int, int) { return 1; }), false, 0, true},
			{"times_on_keys", make_set(3, 2, false, tracked), false, 2, false},
			{"seam_branches", make_set(3, 2, true, tracked), true, 0, false},
	};
	for (const Case &c : cases) {
		std::vector<double> t0, t1;
		std::vector<int32_t> clip;
		for (int k = 0; k < c.set.clip_count; k++) {
			const size_t before = t0.size();
			frames_for(c.set.clips[k].length, c.inside, t0, t1);
			clip.insert(clip.end(), t0.size() - before, k);
		}
		t0.shrink_to_fit(), t1.shrink_to_fit(), clip.shrink_to_fit();
		const int count = (int)t0.size();
		char name[64];
		{
			const Tally t = run(c.set, c.root, {}, t0, 0, 0u, t1, clip);
			std::snprintf(name, sizeof name, "plain_%s", c.name);
			bad += report(name, c.set, t, count, 0, t.nan == 0 && t.fixed == count && (c.still ? t.start == t.floats : t.start < t.floats));
		}
		for (uint32_t flags = 0; flags < 2; flags++)
			for (int K : {1, 8}) {
				std::vector<ClipLayer> L;
				std::vector<double> prev;
				for (int i = 0; i < count; i++)
					for (int l = 0; l < K; l++) {
						const int j = (i + l * 5) % count;
						L.push_back(ClipLayer{t1[j], K == 8 && l % 3 == 2 ? kClipLayerOff : clip[j], 1.0f / (float)K});
						prev.push_back(K == 8 && l % 3 == 2 ? std::nan("") : t0[j]);
					}
				L.shrink_to_fit(), prev.shrink_to_fit();
				const Tally t = run(c.set, c.root, L, prev, K, flags, {}, {});
				std::snprintf(name, sizeof name, "layers_%s_k%d_%s", c.name, K, flags ? "normalize" : "plain");
				bad += report(name, c.set, t, count, K, t.nan == 0 && t.fixed == count && (c.still ? t.start == t.floats : t.start < t.floats));
			}
	}
	const Set set = make_set(3, 3, true, tracked);
	std::vector<double> t0, t1;
	frames_for(1.0, true, t0, t1);
	const int count = (int)t0.size();
	for (uint32_t flags = 0; flags < 2; flags++) {
		const char *mode = flags ? "normalize" : "plain";
		char name[64];
		{ // every layer off, times and weights NaN: the start values, the pose fixed up
			std::vector<ClipLayer> L((size_t)count * 3, ClipLayer{std::nan(""), kClipLayerOff, std::nanf("")});
			std::vector<double> prev((size_t)count * 3, std::nan(""));
			L.shrink_to_fit(), prev.shrink_to_fit();
			const Tally t = run(set, 0, L, prev, 3, flags, {}, {});
			std::snprintf(name, sizeof name, "off_layers_%s", mode);
			bad += report(name, set, t, count, 3, t.start == t.floats && t.fixed == count);
		}
		{ // one invalid index among valid ones: all NaN, no table read (indices far outside every table), the pose untouched
			std::vector<ClipLayer> L;
			std::vector<double> prev;
			const int32_t invalid[] = {3, INT32_MIN, -2, INT32_MAX};
			for (int i = 0; i < count; i++)
				for (int l = 0; l < 3; l++) L.push_back(ClipLayer{t1[i], l == i % 3 ? invalid[i % 4] : l, 0.5f}), prev.push_back(t0[i]);
			L.shrink_to_fit(), prev.shrink_to_fit();
			const Tally t = run(set, 0, L, prev, 3, flags, {}, {});
			std::snprintf(name, sizeof name, "invalid_layers_%s", mode);
			bad += report(name, set, t, count, 3, t.nan == t.floats && t.fixed == 0);
		}
		{ // non-finite times: NaN records, no key read, the pose fixed up
			std::vector<ClipLayer> L;
			std::vector<double> prev;
			const double nf[] = {std::nan(""), INFINITY, -INFINITY};
			for (int i = 0; i < count; i++)
				for (int l = 0; l < 2; l++) L.push_back(ClipLayer{l ? t1[i] : nf[i % 3], l, 0.5f}), prev.push_back(l ? nf[i % 3] : t0[i]);
			L.shrink_to_fit(), prev.shrink_to_fit();
			const Tally t = run(set, 0, L, prev, 2, flags, {}, {});
			std::snprintf(name, sizeof name, "nonfinite_times_%s", mode);
			bad += report(name, set, t, count, 2, t.nan == t.floats && t.fixed == count);
		}
	}
	{ // the plain form's invalid indices
		std::vector<int32_t> clip;
		const int32_t invalid[] = {3, INT32_MIN, -2, INT32_MAX};
		for (int i = 0; i < count; i++) clip.push_back(invalid[i % 4]);
		clip.shrink_to_fit();
		const Tally t = run(set, 0, {}, t0, 0, 0u, t1, clip);
		bad += report("plain_invalid", set, t, count, 0, t.nan == t.floats && t.fixed == 0);
	}
	for (uint32_t flags = 0; flags < 2; flags++) { // the apply, in place on exact-size blocks
		const int n = 64;
		std::vector<float> motion((size_t)n * 10), G((size_t)n * 12);
		motion.shrink_to_fit(), G.shrink_to_fit();
		for (int i = 0; i < n; i++) {
			float q[4], l = 0;
			for (float &v : q) v = rnd(-1.0f, 1.0f), l += v * v;
			for (int f = 0; f < 4; f++) motion[(size_t)i * 10 + f] = q[f] / std::sqrt(l);
			for (int f = 4; f < 10; f++) motion[(size_t)i * 10 + f] = rnd(-1.0f, 1.0f);
			for (int f = 0; f < 12; f++) G[(size_t)i * 12 + f] = rnd(-1.0f, 1.0f) + (f % 4 == 0 && f < 9 ? 2.0f : 0.0f);
		}
		for (int f = 0; f < 10; f++) motion[f] = std::nanf(""); // a NaN record
		for (int f = 0; f < 4; f++) motion[10 + f] = 0.0f;       // a zero quaternion
		for (int f = 0; f < 9; f++) G[24 + f] = 0.0f;            // a zero basis
		long nan = 0, bad_nan = 0;
		for (int i = 0; i < n; i++) root_motion_apply(motion.data() + (size_t)i * 10, flags, G.data() + (size_t)i * 12);
		for (float x : G)
			if (x != x) nan++, bad_nan += bits(x) != 0x7fc00000u;
		const bool ok = bad_nan == 0 && nan >= 12 && nan <= 36;
		std::printf("apply_%s: %s count=%d nan=%ld\n", flags ? "orthonormalize" : "plain", ok ? "ok" : "FAILED", n, nan);
		bad += ok ? 0 : 1;
	}
	return bad ? 1 : 0;
}
