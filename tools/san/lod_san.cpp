// lod.h under ASan + UBSan: the host path behind mbik_cull_lod_cpu (the kernels run the same per-skeleton
// code) on built-in crowds: no skeletons, one, a wave and one more, every range count from 1 to the
// largest, both flag values, with and without the world transform, the margin and the level output,
// NaN boxes, no planes and the most planes, and the state carried through four frames.  Every buffer is
// a heap block of exactly the documented size; the lists are checked against the levels and the states.
//   lod_san   -> exit 0 and one line per case, or a sanitizer report
#include <cmath>
#include <cstdio>
#include <vector>

#include "../../many_bone_ik_amd/csrc/lod.h"

namespace {

uint32_t g_state = 20261020u;
float rnd(float lo, float hi) { // LCG, top 24 bits
	g_state = g_state * 1664525u + 1013904223u;
	return lo + (hi - lo) * (float)(g_state >> 8) * (1.0f / 16777216.0f);
}

int run(const char *name, int count, int range_count, uint32_t flags, bool with_global, float margin, bool with_level, int plane_count) {
	std::vector<float> boxes((size_t)count * 6), global(with_global ? (size_t)count * 12 : 0), planes((size_t)plane_count * 4), camera(3);
	for (int s = 0; s < count; s++)
		for (int i = 0; i < 6; i++) boxes[(size_t)s * 6 + i] = i < 3 ? rnd(-20.0f, 20.0f) : rnd(0.0f, 1.5f);
	if (count > 2) boxes[7] = NAN;
	for (size_t i = 0; i < global.size(); i++) global[i] = (i % 12 == 0 || i % 12 == 4 || i % 12 == 8 ? 1.0f : 0.0f) + rnd(-0.2f, 0.2f);
	for (int i = 0; i < plane_count; i++) {
		planes[(size_t)i * 4 + i % 3] = i % 2 ? -1.0f : 1.0f;
		planes[(size_t)i * 4 + 3] = rnd(8.0f, 16.0f);
	}
	for (float &v : camera) v = rnd(-2.0f, 2.0f);
	std::vector<mbik::LodRange> ranges((size_t)range_count);
	for (int r = 0; r < range_count; r++)
		ranges[r] = mbik::LodRange{r ? 4.0f * r : 0.0f, r == range_count - 1 ? 0.0f : 4.0f * r + 5.0f, 0.5f, 0.75f};
	std::vector<uint8_t> state((size_t)count), level(with_level ? (size_t)count : 0);
	std::vector<int32_t> indices((size_t)range_count * count), n((size_t)range_count, -1);
	long long listed = 0;
	for (int frame = 0; frame < 4; frame++) {
		camera[0] += 3.0f;
		const std::vector<uint8_t> before = state;
		mbik::cull_lod_host(count, boxes.data(), with_global ? global.data() : nullptr, margin, plane_count, planes.data(), camera.data(),
				range_count, ranges.data(), flags, state.data(), with_level ? level.data() : nullptr, indices.data(), n.data());
		std::vector<int> times((size_t)count, 0);
		for (int r = 0; r < range_count; r++) {
			if (n[r] < 0 || n[r] > count) {
				printf("%s: frame %d list %d has length %d\n", name, frame, r, n[r]);
				return 2;
			}
			for (int32_t i = 0; i < n[r]; i++) {
				const int32_t s = indices[(size_t)r * count + i];
				if (s < 0 || s >= count || (i > 0 && s <= indices[(size_t)r * count + i - 1]) || !((state[s] >> r) & 1) ||
						(with_level && (flags & mbik::kLodExclusive ? level[s] != r : level[s] > r))) {
					printf("%s: frame %d list %d entry %d\n", name, frame, r, i);
					return 2;
				}
				times[s]++;
			}
			listed += n[r];
		}
		for (int s = 0; s < count; s++)
			if ((state[s] >> range_count) != 0 || ((flags & mbik::kLodExclusive) && times[s] > 1) ||
					(with_level && (level[s] == mbik::kLodNone) != (times[s] == 0))) {
				printf("%s: frame %d skeleton %d\n", name, frame, s);
				return 2;
			}
	}
	printf("%s: ok skeletons=%d ranges=%d flags=%u planes=%d listed=%lld\n", name, count, range_count, flags, plane_count, listed);
	return 0;
}

} // namespace

int main() {
	int bad = 0;
	bad |= run("no_skeletons", 0, 3, 0, false, 0.0f, true, 6) != 0;
	bad |= run("one_skeleton", 1, 1, 0, false, 0.0f, true, 0) != 0;
	bad |= run("wave_and_one", 65, 3, 1, true, 0.25f, true, 6) != 0;
	bad |= run("no_level", 257, 3, 0, true, 0.0f, false, 6) != 0;
	bad |= run("most_planes", 300, 2, 1, false, -0.1f, true, mbik::kCullMaxPlanes) != 0;
	for (int r = 1; r <= mbik::kLodMaxRanges; r++) {
		char name[32];
		snprintf(name, sizeof name, "ranges_%d", r);
		bad |= run(name, 1000, r, r & 1, r % 3 == 0, r % 2 ? 0.0f : 0.4f, true, 6) != 0;
	}
	return bad ? 1 : 0;
}
