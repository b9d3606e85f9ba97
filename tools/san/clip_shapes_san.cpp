// clip_shapes.h under ASan + UBSan: the host paths behind mbik_clip_sample_shapes_cpu and
// mbik_clip_sample_shapes_layers_cpu (the kernels run the same per-shape code) on built-in sets:
// untracked shapes, single keys, times exactly on keys, both wrap branches, and for the layered
// path layers that are off, invalid, weighted to a zero total or NaN, with 1 and with 8 layers.
// Every table is a heap block of exactly its size -- clip infos, headers [clips][shapes], key
// records keys + 1 (the spare record), init, the layer records and the output -- so a key index, a
// header or a record read out of range is a sanitizer report; what each case must produce (init
// bits, NaN bits, finite values) is checked as well.
//   clip_shapes_san   -> exit 0 and one line per case, or a sanitizer report
#include <cmath>
#include <cstdio>
#include <vector>

#include "../../many_bone_ik_amd/csrc/clip_shapes.h"

namespace {
using namespace mbik;

uint32_t g_state = 20261021u;
float rnd(float lo, float hi) { // LCG, top 24 bits
	g_state = g_state * 1664525u + 1013904223u;
	return lo + (hi - lo) * (float)(g_state >> 8) * (1.0f / 16777216.0f);
}

uint32_t bits(float x) {
	uint32_t u;
	std::memcpy(&u, &x, 4);
	return u;
}

// A set of shape tracks in clip_shapes.h's repacked form.  keys_of(c, shape) decides each key count.
struct Set {
	int P, clip_count;
	std::vector<ClipInfo> clips;
	std::vector<ShapeHeader> headers;
	std::vector<ShapeKey> keys;
	std::vector<float> init;
	ShapeView view() const { return ShapeView{P, clip_count, clips.data(), headers.data(), keys.data(), init.data()}; }
};

template <typename KeysOf>
Set make_set(int P, int clip_count, bool inside, KeysOf keys_of) {
	Set s{P, clip_count, {}, {}, {}, {}};
	for (int j = 0; j < P; j++) s.init.push_back(rnd(2.0f, 3.0f)); // no key value is in [2, 3]
	for (int c = 0; c < clip_count; c++) {
		const double length = 1.0 + c;
		s.clips.push_back(ClipInfo{length, c % 2 == 0 ? 1 : 0, 0});
		for (int j = 0; j < P; j++) {
			const int n = keys_of(c, j);
			if (n == 0) {
				s.headers.push_back(ShapeHeader{0, 0, 0, 0});
				continue;
			}
			s.headers.push_back(ShapeHeader{(int32_t)s.keys.size(), n, (j % 3 ? kClipLinear : 0) | (c % 2 == 0 ? kClipWrap : 0), 0});
			for (int k = 0; k < n; k++) {
				// inside: keys strictly inside (0, length), so times before the first and after the last key wrap
				const double lo = inside ? 0.1 : 0.0, hi = inside ? 0.9 : 1.0;
				s.keys.push_back(ShapeKey{n == 1 ? lo * length : length * (lo + (hi - lo) * k / (n - 1)), rnd(-0.25f, 1.25f), 0.0f});
			}
		}
	}
	s.keys.push_back(ShapeKey{0.0, 0.0f, 0.0f});
	s.clips.shrink_to_fit(), s.headers.shrink_to_fit(), s.keys.shrink_to_fit(), s.init.shrink_to_fit();
	return s;
}

struct Tally {
	long floats = 0, nan = 0, init = 0;
};
Tally tally(const Set &s, const std::vector<float> &out, int count) {
	Tally t;
	for (int i = 0; i < count; i++)
		for (int j = 0; j < s.P; j++) {
			const float x = out[(size_t)i * s.P + j];
			t.floats++;
			if (x != x) {
				if (bits(x) != 0x7fc00000u) return Tally{-1, 0, 0}; // a NaN that is not the canonical one
				t.nan++;
			} else if (bits(x) == bits(s.init[j])) {
				t.init++;
			} else if (x == -12345.678f) {
				return Tally{-1, 0, 0}; // left unwritten
			}
		}
	return t;
}

int report(const char *name, const Set &s, const Tally &t, int count, int K, bool ok) {
	std::printf("%s: %s P=%d clips=%d count=%d K=%d floats=%ld nan=%ld init=%ld\n", name, t.floats < 0 || !ok ? "FAILED" : "ok", s.P,
			s.clip_count, count, K, t.floats, t.nan, t.init);
	return t.floats < 0 || !ok ? 1 : 0;
}

// The plain path: every skeleton at time[i] in clip clip[i].
Tally plain(const Set &s, const std::vector<double> &time, const std::vector<int32_t> &clip) {
	const int count = (int)time.size();
	std::vector<float> out((size_t)count * s.P, -12345.678f);
	const ShapeView v = s.view();
	for (int i = 0; i < count; i++)
		for (int j = 0; j < s.P; j++) out[(size_t)i * s.P + j] = shape_sample(v, clip[i], j, time[i]);
	return tally(s, out, count);
}

// The layered path: [count][K] records.
Tally layered(const Set &s, const std::vector<ClipLayer> &layers, int K, uint32_t flags) {
	const int count = (int)(layers.size() / K);
	std::vector<float> out((size_t)count * s.P, -12345.678f);
	const ShapeView v = s.view();
	for (int i = 0; i < count; i++)
		for (int j = 0; j < s.P; j++) out[(size_t)i * s.P + j] = shape_layers(v, layers.data() + (size_t)i * K, K, flags, j);
	return tally(s, out, count);
}

// The times of interest of a clip of `length` with n keys laid out as make_set lays them out.
std::vector<double> times_for(double length, bool inside) {
	std::vector<double> t{0.0, -0.0, length, -0.25 * length, 2.5 * length, 1e9, 0.05 * length, 0.95 * length, 0.5 * length};
	const double lo = inside ? 0.1 : 0.0, hi = inside ? 0.9 : 1.0;
	for (int n : {2, 3, 17})
		for (int k = 0; k < n; k++) t.push_back(length * (lo + (hi - lo) * k / (n - 1))); // exactly on keys
	t.push_back(std::nan("")), t.push_back(INFINITY), t.push_back(-INFINITY);
	return t;
}

std::vector<ClipLayer> layers_for(const Set &s, const std::vector<double> &time, int K, float weight) {
	std::vector<ClipLayer> L;
	for (size_t i = 0; i < time.size(); i++)
		for (int l = 0; l < K; l++) L.push_back(ClipLayer{time[(i + l) % time.size()], (int32_t)((i + l) % s.clip_count), weight});
	L.shrink_to_fit();
	return L;
}

} // namespace

int main() {
	int bad = 0;
	const int kinds[] = {0, 1, 2, 3, 17};
	const auto mixed = [&](int c, int j) { return kinds[(c * 7 + j * 3) % 5]; };
	for (int pass = 0; pass < 2; pass++) { // the plain path, then the layered one in both modes
		struct Case {
			const char *name;
			Set set;
			bool inside;
		};
		Case cases[] = {
				{"untracked", make_set(4, 2, false, [](int, int) { return 0; }), false},
				{"single_keys", make_set(4, 2, false, [](int, int) { return 1; }), false},
				{"times_on_keys", make_set(7, 2, false, mixed), false},
				{"wrap_branches", make_set(7, 2, true, mixed), true},
		};
		for (const Case &c : cases) {
			std::vector<double> time;
			std::vector<int32_t> clip;
			for (int k = 0; k < c.set.clip_count; k++)
				for (double t : times_for(c.set.clips[k].length, c.inside)) time.push_back(t), clip.push_back(k);
			const int count = (int)time.size();
			char name[64];
			if (pass == 0) {
				const Tally t = plain(c.set, time, clip);
				std::snprintf(name, sizeof name, "plain_%s", c.name);
				// a set without keys samples to init, NaN times included; a tracked shape never gives init's bits
				bad += report(name, c.set, t, count, 0, c.set.keys.size() > 1 ? t.init < t.floats : t.init == t.floats);
			} else {
				for (uint32_t flags = 0; flags < 2; flags++) {
					const std::vector<ClipLayer> L = layers_for(c.set, time, 2, 0.5f);
					const Tally t = layered(c.set, L, 2, flags);
					std::snprintf(name, sizeof name, "layers_%s_%s", c.name, flags ? "normalize" : "plain");
					bad += report(name, c.set, t, count, 2, c.set.keys.size() > 1 ? t.init < t.floats : t.init == t.floats);
				}
			}
		}
	}
	{ // the plain path's invalid indices: all NaN, no table read (indices far outside every table)
		const Set set = make_set(7, 3, true, mixed);
		std::vector<double> time = times_for(1.0, true);
		std::vector<int32_t> clip;
		const int32_t invalid[] = {3, INT32_MIN, -1, INT32_MAX};
		for (size_t i = 0; i < time.size(); i++) clip.push_back(invalid[i % 4]);
		const Tally t = plain(set, time, clip);
		bad += report("plain_invalid", set, t, (int)time.size(), 0, t.nan == t.floats);
	}
	const Set set = make_set(7, 3, true, mixed);
	std::vector<double> time = times_for(1.0, true);
	time.resize(time.size() - 3); // finite times only
	const int count = (int)time.size();
	for (uint32_t flags = 0; flags < 2; flags++) {
		const char *mode = flags ? "normalize" : "plain";
		char name[64];
		{ // every layer off, times and weights NaN: init
			std::vector<ClipLayer> L((size_t)count * 3, ClipLayer{std::nan(""), kClipLayerOff, std::nanf("")});
			L.shrink_to_fit();
			const Tally t = layered(set, L, 3, flags);
			std::snprintf(name, sizeof name, "off_layers_%s", mode);
			bad += report(name, set, t, count, 3, t.init == t.floats);
		}
		{ // one invalid index among valid ones: all NaN, no table read
			std::vector<ClipLayer> L = layers_for(set, time, 3, 0.5f);
			const int32_t invalid[] = {3, INT32_MIN, -2, INT32_MAX};
			for (int i = 0; i < count; i++) L[(size_t)i * 3 + i % 3].clip = invalid[i % 4];
			const Tally t = layered(set, L, 3, flags);
			std::snprintf(name, sizeof name, "invalid_layers_%s", mode);
			bad += report(name, set, t, count, 3, t.nan == t.floats);
		}
		{ // weights 0, -0, negative and below CMP_EPSILON: nothing accumulated, init
			std::vector<ClipLayer> L = layers_for(set, time, 4, 0.0f);
			const float w[] = {0.0f, -0.0f, -3.0f, 1e-6f};
			for (size_t i = 0; i < L.size(); i++) L[i].weight = w[i % 4];
			const Tally t = layered(set, L, 4, flags);
			std::snprintf(name, sizeof name, "zero_totals_%s", mode);
			bad += report(name, set, t, count, 4, t.init == t.floats);
		}
		{ // NaN weights next to plain ones: NaN where a layer tracks the shape, never a stray NaN payload
			std::vector<ClipLayer> L = layers_for(set, time, 2, 0.5f);
			for (size_t i = 0; i < L.size(); i += 2) L[i].weight = std::nanf("");
			const Tally t = layered(set, L, 2, flags);
			std::snprintf(name, sizeof name, "nan_weights_%s", mode);
			bad += report(name, set, t, count, 2, t.nan > 0 && t.nan < t.floats);
		}
		for (int K : {1, 8}) {
			std::vector<ClipLayer> L = layers_for(set, time, K, 1.0f / (float)K);
			if (K == 8)
				for (size_t i = 0; i < L.size(); i += 3) L[i].clip = kClipLayerOff;
			const Tally t = layered(set, L, K, flags);
			std::snprintf(name, sizeof name, "k%d_%s", K, mode);
			bad += report(name, set, t, count, K, t.nan == 0 && t.init < t.floats);
		}
	}
	return bad ? 1 : 0;
}
