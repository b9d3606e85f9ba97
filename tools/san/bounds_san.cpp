// bounds.h under ASan + UBSan: the bone-box builder, the packing of the used-bone table, and the three
// host paths behind mbik_bone_boxes_cpu, mbik_skin_bounds_cpu and mbik_cull_boxes_cpu (the kernels run
// the same per-box code), on built-in meshes: one vertex, every bone used, every third bone used, no
// bone used, no vertices, the largest rig, NaN and signed weights, every output combination of the
// cull.  Every buffer is a heap block of exactly the documented size.
//   bounds_san   -> exit 0 and one line per case, or a sanitizer report
#include <cmath>
#include <cstdio>
#include <vector>

#include "../../many_bone_ik_amd/csrc/bounds.h"

namespace {

uint32_t g_state = 20250601u;
float rnd(float lo, float hi) { // LCG, top 24 bits
	g_state = g_state * 1664525u + 1013904223u;
	return lo + (hi - lo) * (float)(g_state >> 8) * (1.0f / 16777216.0f);
}

// every: the mesh names bones that are multiples of `every` only; zero_weights: no bone is used
int run(const char *name, int B, int V, int K, int every, bool zero_weights, int count, int plane_count) {
	std::vector<float> pos((size_t)V * 3), w((size_t)V * K), skin((size_t)count * B * 12);
	std::vector<int32_t> idx((size_t)V * K);
	for (float &v : pos) v = rnd(-2.0f, 2.0f);
	for (size_t i = 0; i < w.size(); i++) w[i] = zero_weights ? (i % 2 ? 0.0f : -0.0f) : (i % 5 == 3 ? 0.0f : rnd(-0.5f, 1.0f));
	for (float &v : skin) v = rnd(-1.5f, 1.5f);
	for (size_t i = 0; i < idx.size(); i++) idx[i] = ((int32_t)(rnd(0.0f, 1.0f) * (float)B) % B) / every * every;
	if (V > 1 && !zero_weights) idx[idx.size() - 1] = (B - 1) / every * every, w[w.size() - 1] = 0.5f, pos[3] = NAN, w[0] = NAN;
	if (mbik::skin_check_mesh(B, V, K, pos.data(), idx.data(), w.data()) != mbik::SKIN_OK) {
		printf("%s: mesh refused\n", name);
		return 1;
	}
	std::vector<float> boxes((size_t)B * 6);
	std::vector<uint8_t> used((size_t)B);
	mbik::bone_boxes_build(B, V, K, pos.data(), idx.data(), w.data(), boxes.data(), used.data());
	// the table: the used bones, ascending, each record its bone's index and box with a zero pad
	const int32_t U = mbik::bone_table_count(B, used.data());
	std::vector<unsigned char> table((size_t)U * mbik::kBoneRecordBytes);
	if (mbik::bone_table_pack(B, boxes.data(), used.data(), table.data()) != U) {
		printf("%s: record count\n", name);
		return 2;
	}
	int32_t last = -1;
	const float zero = 0.0f;
	for (int32_t u = 0; u < U; u++) {
		const unsigned char *r = table.data() + (size_t)u * mbik::kBoneRecordBytes;
		int32_t b;
		memcpy(&b, r, 4);
		if (b <= last || b >= B || !used[b] || memcmp(r + 4, boxes.data() + (size_t)b * 6, 12) != 0 ||
				memcmp(r + 16, boxes.data() + (size_t)b * 6 + 3, 12) != 0 || memcmp(r + 28, &zero, 4) != 0) {
			printf("%s: record %d differs\n", name, u);
			return 2;
		}
		last = b;
	}
	for (int32_t b = 0; b < B; b++)
		if (!used[b])
			for (int i = 0; i < 6; i++)
				if (boxes[(size_t)b * 6 + i] != 0.0f) {
					printf("%s: unused bone %d has a box\n", name, b);
					return 2;
				}
	std::vector<float> out((size_t)count * 6), global((size_t)count * 12), planes((size_t)plane_count * 4);
	mbik::skin_bounds_host(B, boxes.data(), used.data(), count, skin.data(), out.data());
	for (float &v : global) v = rnd(-1.0f, 1.0f);
	for (float &v : planes) v = rnd(-1.0f, 1.0f);
	std::vector<uint8_t> visible((size_t)count);
	std::vector<int32_t> indices((size_t)count), n(1, -1);
	int64_t seen = 0;
	// every output combination, with and without the world transform and the margin
	mbik::cull_boxes_host(count, out.data(), nullptr, 0.0f, plane_count, planes.data(), visible.data(), nullptr, nullptr);
	for (uint8_t v : visible) seen += v;
	mbik::cull_boxes_host(count, out.data(), global.data(), 0.25f, plane_count, planes.data(), nullptr, indices.data(), n.data());
	std::vector<int32_t> exact((size_t)n[0]); // (the list written into a block of exactly its length)
	mbik::cull_boxes_host(count, out.data(), global.data(), 0.25f, plane_count, planes.data(), visible.data(), exact.data(), n.data());
	for (int32_t i = 0; i < n[0]; i++)
		if (exact[i] != indices[i] || !visible[exact[i]] || (i > 0 && exact[i] <= exact[i - 1])) {
			printf("%s: visible list\n", name);
			return 2;
		}
	double chk = 0;
	for (float v : out)
		if (v == v) chk += v;
	printf("%s: ok B=%d V=%d K=%d used=%d skeletons=%d planes=%d visible=%lld listed=%d checksum=%.6g\n", name, B, V, K, U, count,
			plane_count, (long long)seen, n[0], chk);
	return 0;
}

} // namespace

int main() {
	int bad = 0;
	bad |= run("one_vertex", 3, 1, 4, 1, false, 2, 1) != 0;
	bad |= run("every_bone", 32, 400, 8, 1, false, 5, 6) != 0;
	bad |= run("every_third_bone", 200, 300, 4, 3, false, 3, 6) != 0;
	bad |= run("no_bone_used", 7, 20, 4, 1, true, 3, 2) != 0;
	bad |= run("no_vertices", 5, 0, 8, 1, false, 2, 0) != 0;
	bad |= run("no_skeletons", 5, 9, 4, 1, false, 0, 6) != 0;
	bad |= run("no_bones", 0, 0, 4, 1, false, 2, 1) != 0;
	bad |= run("max_bones", mbik::kSkinMaxBones, 5000, 4, 1, false, 1, mbik::kCullMaxPlanes) != 0;
	return bad ? 1 : 0;
}
