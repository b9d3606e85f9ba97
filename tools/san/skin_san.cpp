// skin.h under ASan + UBSan: the mesh validation, the device mesh layout's packing and the host
// skinning path behind mbik_skin_vertices_cpu (the kernel runs the same blend and transform), on
// built-in meshes: one vertex, 4 and 8 influences, bone indices at 0 and B - 1, odd and even
// vertex counts, with and without normals, and meshes the validation must refuse.  Every buffer
// is a heap block of exactly the documented size.
//   skin_san   -> exit 0 and one line per mesh, or a sanitizer report
#include <cstdio>
#include <vector>

#include "../../many_bone_ik_amd/csrc/skin.h"

namespace {

uint32_t g_state = 20240914u;
float rnd(float lo, float hi) { // LCG, top 24 bits
	g_state = g_state * 1664525u + 1013904223u;
	return lo + (hi - lo) * (float)(g_state >> 8) * (1.0f / 16777216.0f);
}

// edge: 0 random indices, 1 all bone 0, 2 all bone B - 1
int run(const char *name, int B, int V, int K, bool normals, int count, int edge) {
	std::vector<float> pos((size_t)V * 3), nrm(normals ? (size_t)V * 3 : 0), w((size_t)V * K), skin((size_t)count * B * 12);
	std::vector<int32_t> idx((size_t)V * K);
	for (float &v : pos) v = rnd(-2.0f, 2.0f);
	for (float &v : nrm) v = rnd(-1.0f, 1.0f);
	for (float &v : w) v = rnd(-0.5f, 1.0f);
	for (float &v : skin) v = rnd(-1.5f, 1.5f);
	for (size_t i = 0; i < idx.size(); i++) idx[i] = edge == 1 ? 0 : (edge == 2 ? B - 1 : (int32_t)(rnd(0.0f, 1.0f) * (float)B) % B);
	if (V > 0 && edge == 0) idx[0] = 0, idx[idx.size() - 1] = B - 1;
	const mbik::SkinCheck c = mbik::skin_check_mesh(B, V, K, pos.data(), idx.data(), w.data());
	if (c != mbik::SKIN_OK) {
		printf("%s: refused (%s)\n", name, mbik::skin_check_text(c));
		return 1;
	}
	// the packed planes, read back against the inputs
	const mbik::SkinLayout l = mbik::skin_layout(V, K, normals);
	std::vector<unsigned char> packed((size_t)l.bytes);
	mbik::skin_pack(V, K, pos.data(), normals ? nrm.data() : nullptr, idx.data(), w.data(), packed.data());
	const int64_t n = ((int64_t)V + 1) & ~(int64_t)1;
	for (int64_t v = 0; v < V; v++) {
		bool same = memcmp(packed.data() + l.pos + v * 16, pos.data() + v * 3, 12) == 0;
		if (normals) same = same && memcmp(packed.data() + l.nrm + v * 16, nrm.data() + v * 3, 12) == 0;
		for (int k = 0; k < K; k++) {
			uint16_t b;
			float wk;
			memcpy(&b, packed.data() + l.idx + (v * K + k) * 2, 2);
			memcpy(&wk, packed.data() + l.wgt + ((k / 4) * n + v) * 16 + (k % 4) * 4, 4);
			same = same && b == idx[v * K + k] && memcmp(&wk, &w[v * K + k], 4) == 0;
		}
		if (!same) {
			printf("%s: packed vertex %lld differs\n", name, (long long)v);
			return 2;
		}
	}
	std::vector<float> out_p((size_t)count * V * 3), out_n(normals ? (size_t)count * V * 3 : 0);
	mbik::skin_vertices_host(B, V, K, pos.data(), normals ? nrm.data() : nullptr, idx.data(), w.data(), count, skin.data(),
			out_p.data(), normals ? out_n.data() : nullptr);
	double chk = 0;
	for (float v : out_p) chk += v;
	for (float v : out_n) chk += v;
	printf("%s: ok B=%d V=%d K=%d normals=%d skeletons=%d bytes=%lld checksum=%.6g\n", name, B, V, K, (int)normals, count,
			(long long)l.bytes, chk);
	return 0;
}

int refused(const char *name, int B, int V, int K, const float *pos, const int32_t *idx, const float *w, mbik::SkinCheck want) {
	const mbik::SkinCheck c = mbik::skin_check_mesh(B, V, K, pos, idx, w);
	printf("%s: %s (%s)\n", name, c != want ? "UNEXPECTED" : (want == mbik::SKIN_OK ? "accepted" : "refused"), mbik::skin_check_text(c));
	return c != want;
}

} // namespace

int main() {
	int bad = 0;
	bad |= run("one_vertex_k4", 3, 1, 4, false, 2, 0) != 0;
	bad |= run("one_vertex_k8", 3, 1, 8, true, 2, 0) != 0;
	bad |= run("one_bone", 1, 5, 4, true, 3, 0) != 0;
	bad |= run("bone0_k4", 37, 64, 4, true, 2, 1) != 0;
	bad |= run("last_bone_k8", 37, 65, 8, false, 2, 2) != 0;
	bad |= run("odd_count_k4", 200, 257, 4, false, 3, 0) != 0;
	bad |= run("even_count_k8", 200, 1000, 8, true, 3, 0) != 0;
	bad |= run("max_bones", mbik::kSkinMaxBones, 130, 4, true, 1, 0) != 0;
	bad |= run("no_vertices", 5, 0, 4, false, 2, 0) != 0;
	bad |= run("no_skeletons", 5, 9, 8, true, 0, 0) != 0;
	// refused meshes
	const float f[8] = {0, 0, 0, 1, 0, 0, 0, 0};
	const int32_t in_range[4] = {0, 1, 2, 4}, too_large[4] = {0, 1, 2, 5}, negative[4] = {0, -1, 2, 3};
	bad |= refused("influences_3", 5, 1, 3, f, in_range, f, mbik::SKIN_BAD_INFLUENCES);
	bad |= refused("index_is_bone_count", 5, 1, 4, f, too_large, f, mbik::SKIN_BAD_INDEX);
	bad |= refused("index_negative", 5, 1, 4, f, negative, f, mbik::SKIN_BAD_INDEX);
	bad |= refused("null_positions", 5, 1, 4, nullptr, in_range, f, mbik::SKIN_NULL);
	bad |= refused("negative_vertices", 5, -1, 4, f, in_range, f, mbik::SKIN_NEGATIVE);
	bad |= refused("accepted", 5, 1, 4, f, in_range, f, mbik::SKIN_OK);
	return bad ? 1 : 0;
}
