// fk.h under ASan + UBSan: the depth-ordered schedule builder and the host forward-kinematics
// core behind mbik_pose_globals_cpu (the kernel runs the same per-bone functions), on the edge
// rigs of tests/test_pose_globals_cpu.py, a 300-bone chain, and descriptions the builder must
// refuse.  Every buffer is a heap block of exactly the documented size.
//   fk_san   -> exit 0 and one line per rig, or a sanitizer report
#include <cstdio>
#include <vector>

#include "../../many_bone_ik_amd/csrc/fk.h"

namespace {

uint32_t g_state = 20240807u;
float rnd(float lo, float hi) { // LCG, top 24 bits
	g_state = g_state * 1664525u + 1013904223u;
	return lo + (hi - lo) * (float)(g_state >> 8) * (1.0f / 16777216.0f);
}

int run(const char *name, const std::vector<int32_t> &parents, const std::vector<int32_t> &pins, int n) {
	const int B = (int)parents.size(), P = (int)pins.size();
	std::vector<int32_t> depth(B), order(B), level_off(B + 1);
	const int levels = mbik::fk_build_schedule(B, parents.data(), depth.data(), order.data(), level_off.data());
	if (levels < 0) {
		printf("%s: refused (%d)\n", name, levels);
		return levels;
	}
	// every bone once, parents in earlier levels
	std::vector<int> seen(B, 0);
	for (int l = 0; l < levels; l++)
		for (int i = level_off[l]; i < level_off[l + 1]; i++) {
			const int b = order[i];
			if (seen[b]++ || depth[b] != l || (parents[b] >= 0 ? depth[parents[b]] != l - 1 : l != 0)) {
				printf("%s: bad schedule at bone %d\n", name, b);
				return 1;
			}
		}
	if (level_off[levels] != B) {
		printf("%s: schedule covers %d of %d bones\n", name, level_off[levels], B);
		return 1;
	}
	std::vector<float> pose((size_t)n * B * 10), inv_bind((size_t)B * 12), targets((size_t)n * P * 12);
	for (size_t i = 0; i < pose.size(); i++) {
		const int f = (int)(i % 10);
		pose[i] = f < 4 ? rnd(-1.5f, 1.5f) : (f < 7 ? rnd(-1.0f, 1.0f) : rnd(0.9f, 1.1f) * (rnd(0.0f, 1.0f) < 0.25f ? -1.0f : 1.0f));
	}
	for (float &v : inv_bind) v = rnd(-1.0f, 1.0f);
	for (float &v : targets) v = rnd(-2.0f, 2.0f);
	double chk = 0;
	for (int skin = 0; skin < 2; skin++) {
		std::vector<float> globals((size_t)n * B * 12), dist((size_t)n * P), scratch((size_t)B * 12);
		for (int s = 0; s < n; s++) {
			float *out = globals.data() + (size_t)s * B * 12;
			mbik::fk_skeleton(B, parents.data(), order.data(), P, pins.data(), pose.data() + (size_t)s * B * 10,
					skin ? inv_bind.data() : nullptr, targets.data() + (size_t)s * P * 12, skin ? scratch.data() : out, out,
					dist.data() + (size_t)s * P);
			// distances only
			mbik::fk_skeleton(B, parents.data(), order.data(), P, pins.data(), pose.data() + (size_t)s * B * 10, nullptr,
					targets.data() + (size_t)s * P * 12, scratch.data(), nullptr, dist.data() + (size_t)s * P);
		}
		for (float v : globals) chk += v;
		for (float v : dist) chk += v;
	}
	printf("%s: ok B=%d levels=%d skeletons=%d checksum=%.6g\n", name, B, levels, n, chk);
	return 0;
}

} // namespace

int main() {
	int bad = 0;
	bad |= run("unsorted_parents", {2, 2, -1, 1, 0}, {3, 4}, 3) != 0;
	bad |= run("multi_root", {-1, 0, 1, -1, 3, 4}, {2, 5}, 3) != 0;
	bad |= run("pinned_root", {-1, 0, 1, 0, 3}, {0, 2, 4}, 3) != 0;
	std::vector<int32_t> chain(300);
	for (int b = 0; b < 300; b++) chain[b] = b - 1;
	bad |= run("chain300", chain, {299}, 2) != 0;
	std::vector<int32_t> reversed(300);
	for (int b = 0; b < 300; b++) reversed[b] = b == 299 ? -1 : b + 1;
	bad |= run("chain300_reversed", reversed, {0}, 2) != 0;
	bad |= run("empty", {}, {}, 1) != 0;
	// refused descriptions: a self parent, a two-bone cycle behind a tail, parents out of range
	bad |= run("self_parent", {0, 0}, {}, 1) != -2;
	bad |= run("cycle", {-1, 2, 3, 1, 3}, {}, 1) != -2;
	bad |= run("parent_too_large", {-1, 7}, {}, 1) != -1;
	bad |= run("parent_too_small", {-1, -2}, {}, 1) != -1;
	return bad ? 1 : 0;
}
