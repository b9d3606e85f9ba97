// The samplers' CUBIC forms under ASan + UBSan: the host paths behind mbik_clip_call_cpu for all six
// kinds (clip.h, clip_layers.h, clip_shapes.h, root_motion.h; the kernels run the same per-item code)
// on built-in sets whose every track is cubic with n = 1, 2, 3 or 4 keys -- where the keys before a
// and after b alias a and b, clamp onto them or go round the clip -- with and without wrap, keys
// inside (0, length) and on its ends, at times on every key and one ulp either side, before the
// first and after the last key, 0, the length, past it, negative, and not finite.  Every table is a
// heap block of exactly its size -- headers, times and values keys + 1 (the spare entry), shape keys
// + 1, the rest pose, init, the layer records, the previous times and the outputs -- so a key index
// read out of range is a sanitizer report; every output must be written, finite for a finite time
// and the one canonical NaN otherwise.
//   clip_cubic_san   -> exit 0 and one line per case, or a sanitizer report
#include <cmath>
#include <cstdio>
#include <limits>
#include <vector>

#include "../../many_bone_ik_amd/csrc/clip_shapes.h"
#include "../../many_bone_ik_amd/csrc/root_motion.h"

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
constexpr float kUnwritten = -12345.678f;
constexpr int B = 3, P = 2, kClips = 2; // clip 0 loops (and wraps with `wrap`), clip 1 does not

struct Set {
	std::vector<ClipInfo> clips;
	std::vector<ClipHeader> headers;
	std::vector<double> times;
	std::vector<ClipValue> values;
	std::vector<float> rest;
	std::vector<ShapeHeader> shape_headers;
	std::vector<ShapeKey> keys;
	std::vector<float> init;
	ClipView view() const { return ClipView{B, kClips, clips.data(), headers.data(), times.data(), values.data(), rest.data()}; }
	ShapeView shape_view() const { return ShapeView{P, kClips, clips.data(), shape_headers.data(), keys.data(), init.data()}; }
};

double key_time(int n, int k, double length, bool inside) {
	const double lo = inside ? 0.125 : 0.0, hi = inside ? 0.875 : 1.0;
	return n == 1 ? lo * length : length * (lo + (hi - lo) * k / (n - 1));
}

// Every pose channel and every shape cubic with n keys.
Set make_set(int n, bool wrap, bool inside) {
	Set s;
	s.rest.resize((size_t)B * 10);
	for (float &r : s.rest) r = rnd(0.5f, 1.5f);
	s.init.assign(P, 0.25f);
	for (int c = 0; c < kClips; c++) {
		const double length = 1.0 + c;
		s.clips.push_back(ClipInfo{length, c == 0 ? 1 : 0, 0});
		const int flags = kClipCubic | (c == 0 && wrap ? kClipWrap : 0);
		for (int b = 0; b < B; b++)
			for (int ch = 0; ch < 3; ch++) {
				s.headers.push_back(ClipHeader{(int32_t)s.times.size(), n, flags, 0});
				for (int k = 0; k < n; k++) {
					s.times.push_back(key_time(n, k, length, inside));
					float q[4], l = 0;
					for (float &v : q) v = rnd(-1.0f, 1.0f), l += v * v;
					const float scale = b == 2 ? 1.5f : 1.0f; // bone 2: key quaternions off the unit sphere
					if (ch == 1) s.values.push_back(ClipValue{scale * q[0] / std::sqrt(l), scale * q[1] / std::sqrt(l), scale * q[2] / std::sqrt(l), scale * q[3] / std::sqrt(l)});
					else s.values.push_back(ClipValue{q[0], q[1], q[2], 0.0f});
				}
			}
		for (int j = 0; j < P; j++) {
			s.shape_headers.push_back(ShapeHeader{(int32_t)s.keys.size(), n, flags, 0});
			for (int k = 0; k < n; k++) s.keys.push_back(ShapeKey{key_time(n, k, length, inside), rnd(-0.25f, 1.25f), 0.0f});
		}
	}
	s.times.push_back(0.0);
	s.values.push_back(ClipValue{0.0f, 0.0f, 0.0f, 0.0f});
	s.keys.push_back(ShapeKey{0.0, 0.0f, 0.0f});
	s.clips.shrink_to_fit(), s.headers.shrink_to_fit(), s.times.shrink_to_fit(), s.values.shrink_to_fit(), s.rest.shrink_to_fit();
	s.shape_headers.shrink_to_fit(), s.keys.shrink_to_fit(), s.init.shrink_to_fit();
	return s;
}

// The times of interest of clip c of a set with n keys: (time, finite?) pairs.
std::vector<double> times_for(int n, int c, bool inside) {
	const double length = 1.0 + c, inf = std::numeric_limits<double>::infinity();
	std::vector<double> t{0.0, -0.0, length, std::nextafter(length, 0.0), std::nextafter(length, inf), -0.3 * length, 3.25 * length, 1e9,
			std::nan(""), inf, -inf};
	for (int k = 0; k < n; k++) {
		const double x = key_time(n, k, length, inside);
		t.insert(t.end(), {x, std::nextafter(x, -inf), std::nextafter(x, inf), x + length, 0.5 * (x + key_time(n, (k + 1) % n, length, inside))});
	}
	t.shrink_to_fit();
	return t;
}

struct Tally {
	long floats = 0, nan = 0;
	bool ok = true;
	void take(float x, bool finite_time) {
		floats++;
		if (x != x) {
			nan++;
			if (bits(x) != 0x7fc00000u || finite_time) ok = false; // not the canonical NaN, or a NaN at a finite time
		} else if (x == kUnwritten || !finite_time) {
			ok = false; // unwritten, or a number at a time that is not finite
		}
	}
};

bool run_case(const char *name, int n, bool wrap, bool inside) {
	const Set s = make_set(n, wrap, inside);
	const ClipView v = s.view();
	const ShapeView sv = s.shape_view();
	Tally plain, layered, shapes, shapes_layered, root, root_layered;
	for (int c = 0; c < kClips; c++) {
		const std::vector<double> t = times_for(n, c, inside);
		const int count = (int)t.size();
		// plain sampling and plain shapes
		std::vector<float> pose((size_t)count * B * 10, kUnwritten), w((size_t)count * P, kUnwritten);
		pose.shrink_to_fit(), w.shrink_to_fit();
		for (int i = 0; i < count; i++) {
			for (int b = 0; b < B; b++) clip_sample_bone<true>(v, c, b, t[i], 0, pose.data() + ((size_t)i * B + b) * 10);
			for (int j = 0; j < P; j++) w[(size_t)i * P + j] = shape_sample<true>(sv, c, j, t[i]);
			for (int f = 0; f < B * 10; f++) plain.take(pose[(size_t)i * B * 10 + f], std::isfinite(t[i]));
			for (int j = 0; j < P; j++) shapes.take(w[(size_t)i * P + j], std::isfinite(t[i]));
		}
		// layered: K = 1, 2 and 8 records of this clip and the other, in both modes
		for (int K : {1, 2, 8})
			for (uint32_t flags : {0u, kClipLayersNormalize}) {
				std::vector<ClipLayer> L((size_t)count * K);
				std::vector<double> prev((size_t)count * K);
				std::vector<char> finite(count, 1);
				for (int i = 0; i < count; i++)
					for (int l = 0; l < K; l++) {
						const double tl = l == 0 ? t[i] : t[(i + 3 * l) % count];
						L[(size_t)i * K + l] = ClipLayer{tl, (c + l) % kClips, l == 0 ? 1.0f : 0.5f};
						prev[(size_t)i * K + l] = tl - 0.35; // far enough back to cross the seam of the looping clip
						finite[i] = finite[i] && std::isfinite(tl);
					}
				L.shrink_to_fit(), prev.shrink_to_fit();
				std::vector<float> out((size_t)count * B * 10, kUnwritten), wl((size_t)count * P, kUnwritten), m((size_t)count * 10, kUnwritten);
				out.shrink_to_fit(), wl.shrink_to_fit(), m.shrink_to_fit();
				for (int i = 0; i < count; i++) {
					const ClipLayer *Li = L.data() + (size_t)i * K;
					for (int b = 0; b < B; b++) clip_layers_bone<true>(v, Li, K, flags, b, 0, out.data() + ((size_t)i * B + b) * 10);
					for (int j = 0; j < P; j++) wl[(size_t)i * P + j] = shape_layers<true>(sv, Li, K, flags, j);
					root_motion_skeleton<true>(v, RootLayers{Li, prev.data() + (size_t)i * K}, K, flags, 1, 0, m.data() + (size_t)i * 10, nullptr);
					for (int f = 0; f < B * 10; f++) layered.take(out[(size_t)i * B * 10 + f], finite[i]);
					for (int j = 0; j < P; j++) shapes_layered.take(wl[(size_t)i * P + j], finite[i]);
					for (int f = 0; f < 10; f++) root_layered.take(m[(size_t)i * 10 + f], finite[i]);
				}
			}
		// plain root motion
		std::vector<float> m((size_t)count * 10, kUnwritten);
		m.shrink_to_fit();
		for (int i = 0; i < count; i++) {
			root_motion_skeleton<true>(v, RootPlain{ClipLayer{t[i], c, 1.0f}, t[i] - 0.35}, 1, 0u, 1, 0, m.data() + (size_t)i * 10, nullptr);
			for (int f = 0; f < 10; f++) root.take(m[(size_t)i * 10 + f], std::isfinite(t[i]));
		}
	}
	const bool ok = plain.ok && layered.ok && shapes.ok && shapes_layered.ok && root.ok && root_layered.ok;
	std::printf("%s: %s n=%d sample=%ld/%ld layers=%ld/%ld shapes=%ld/%ld shape_layers=%ld/%ld root=%ld/%ld root_layers=%ld/%ld\n", name,
			ok ? "ok" : "FAILED", n, plain.nan, plain.floats, layered.nan, layered.floats, shapes.nan, shapes.floats, shapes_layered.nan,
			shapes_layered.floats, root.nan, root.floats, root_layered.nan, root_layered.floats);
	return ok;
}
} // namespace

int main() {
	bool ok = true;
	char name[64];
	for (int n = 1; n <= 4; n++)
		for (int wrap = 0; wrap < 2; wrap++)
			for (int inside = 0; inside < 2; inside++) {
				std::snprintf(name, sizeof name, "cubic_n%d_%s_%s", n, wrap ? "wrap" : "clamp", inside ? "inside" : "ends");
				ok = run_case(name, n, wrap != 0, inside != 0) && ok;
			}
	return ok ? 0 : 1;
}
