// morph.h under ASan + UBSan: the shape validation, the packing of the shape planes behind skin.h's
// mesh planes, and the host path behind mbik_skin_vertices_shaped_cpu (the kernel runs the same
// per-vertex morph), on built-in meshes: one vertex and one shape, the last vertex of the last
// plane, odd and even vertex counts, both modes, with and without normals, the LDS limit, and
// shapes the validation must refuse.  Every buffer is a heap block of exactly the documented size.
//   morph_san   -> exit 0 and one line per case, or a sanitizer report
#include <cstdio>
#include <vector>

#include "../../many_bone_ik_amd/csrc/morph.h"

namespace {

uint32_t g_state = 20250301u;
float rnd(float lo, float hi) { // LCG, top 24 bits
	g_state = g_state * 1664525u + 1013904223u;
	return lo + (hi - lo) * (float)(g_state >> 8) * (1.0f / 16777216.0f);
}

int run(const char *name, int B, int V, int K, int P, int mode, bool normals, int count) {
	std::vector<float> pos((size_t)V * 3), nrm(normals ? (size_t)V * 3 : 0), w((size_t)V * K), skin((size_t)count * B * 12);
	std::vector<float> sp((size_t)P * V * 3), sn(normals ? (size_t)P * V * 3 : 0), c((size_t)count * P);
	std::vector<int32_t> idx((size_t)V * K);
	for (float &v : pos) v = rnd(-2.0f, 2.0f);
	for (float &v : nrm) v = rnd(-1.0f, 1.0f);
	for (float &v : w) v = rnd(-0.5f, 1.0f);
	for (float &v : skin) v = rnd(-1.5f, 1.5f);
	for (float &v : sp) v = rnd(-0.5f, 0.5f);
	for (float &v : sn) v = rnd(-0.1f, 0.1f);
	for (size_t i = 0; i < c.size(); i++) c[i] = i % 3 == 1 ? 0.0f : rnd(-1.0f, 1.0f); // (every third weight is skipped)
	for (size_t i = 0; i < idx.size(); i++) idx[i] = (int32_t)(rnd(0.0f, 1.0f) * (float)B) % B;
	if (V > 0) idx[0] = 0, idx[idx.size() - 1] = B - 1;
	const float *np = normals ? nrm.data() : nullptr, *snp = normals ? sn.data() : nullptr;
	if (mbik::skin_check_mesh(B, V, K, pos.data(), idx.data(), w.data()) != mbik::SKIN_OK) {
		printf("%s: mesh refused\n", name);
		return 1;
	}
	const mbik::MorphCheck ck = mbik::morph_check(B, V, normals, P, mode, sp.data(), snp, mbik::kSkinMaxLdsBytes);
	if (ck != mbik::MORPH_OK) {
		printf("%s: refused (%s)\n", name, mbik::morph_check_text(ck));
		return 1;
	}
	// the packed planes: the mesh's are where skin_layout() puts them, the shapes' behind them
	const mbik::SkinLayout sl = mbik::skin_layout(V, K, normals);
	const mbik::MorphLayout l = mbik::morph_layout(V, K, normals, P);
	if (l.pos != sl.bytes || l.pos % 16 || (normals && l.nrm % 16) || l.bytes != sl.bytes + (normals ? 2 : 1) * (int64_t)P * l.stride * 16) {
		printf("%s: layout\n", name);
		return 2;
	}
	std::vector<unsigned char> packed((size_t)l.bytes), plain((size_t)sl.bytes);
	mbik::skin_pack(V, K, pos.data(), np, idx.data(), w.data(), packed.data());
	mbik::morph_pack(V, K, P, sp.data(), snp, packed.data());
	mbik::skin_pack(V, K, pos.data(), np, idx.data(), w.data(), plain.data());
	if (sl.bytes && memcmp(packed.data(), plain.data(), (size_t)sl.bytes) != 0) {
		printf("%s: the shape planes moved the mesh planes\n", name);
		return 2;
	}
	const float zero = 0.0f;
	for (int64_t j = 0; j < P; j++)
		for (int64_t v = 0; v < V; v++) {
			const unsigned char *rp = packed.data() + l.pos + (j * l.stride + v) * 16;
			bool same = memcmp(rp, sp.data() + (j * V + v) * 3, 12) == 0 && memcmp(rp + 12, &zero, 4) == 0;
			if (normals) {
				const unsigned char *rn = packed.data() + l.nrm + (j * l.stride + v) * 16;
				same = same && memcmp(rn, sn.data() + (j * V + v) * 3, 12) == 0 && memcmp(rn + 12, &zero, 4) == 0;
			}
			if (!same) {
				printf("%s: packed shape %lld vertex %lld differs\n", name, (long long)j, (long long)v);
				return 2;
			}
		}
	std::vector<float> out_p((size_t)count * V * 3), out_n(normals ? (size_t)count * V * 3 : 0);
	mbik::morph_skin_vertices_host(B, V, K, pos.data(), np, idx.data(), w.data(), P, mode, sp.data(), snp, count, skin.data(), c.data(),
			out_p.data(), normals ? out_n.data() : nullptr);
	double chk = 0;
	for (float v : out_p) chk += v;
	for (float v : out_n) chk += v;
	printf("%s: ok B=%d V=%d K=%d P=%d mode=%d normals=%d skeletons=%d bytes=%lld checksum=%.6g\n", name, B, V, K, P, mode, (int)normals,
			count, (long long)l.bytes, chk);
	return 0;
}

int refused(const char *name, int B, int V, bool mesh_normals, int P, int mode, const float *sp, const float *sn, int64_t limit,
		mbik::MorphCheck want) {
	const mbik::MorphCheck c = mbik::morph_check(B, V, mesh_normals, P, mode, sp, sn, limit);
	printf("%s: %s (%s)\n", name, c != want ? "UNEXPECTED" : (want == mbik::MORPH_OK ? "accepted" : "refused"), mbik::morph_check_text(c));
	return c != want;
}

} // namespace

int main() {
	int bad = 0;
	bad |= run("one_vertex_one_shape", 3, 1, 4, 1, 0, false, 2) != 0;
	bad |= run("one_vertex_one_shape_normals", 3, 1, 8, 1, 1, true, 2) != 0;
	bad |= run("last_plane_odd", 37, 65, 8, 17, 0, true, 3) != 0;   // (the last vertex of the last plane ends the block)
	bad |= run("last_plane_even", 37, 64, 4, 3, 1, true, 3) != 0;
	bad |= run("positions_only", 200, 257, 4, 17, 1, false, 2) != 0;
	bad |= run("lds_limit", mbik::kSkinMaxBones, 130, 4, 4, 0, true, 1) != 0;
	bad |= run("no_vertices", 5, 0, 4, 3, 0, false, 2) != 0;
	bad |= run("no_skeletons", 5, 9, 8, 3, 1, true, 0) != 0;
	// refused shapes
	const float f[3] = {0, 0, 0};
	const int64_t lim = mbik::kSkinMaxLdsBytes;
	bad |= refused("no_shapes", 5, 1, false, 0, 0, f, nullptr, lim, mbik::MORPH_BAD_COUNT);
	bad |= refused("mode_2", 5, 1, false, 1, 2, f, nullptr, lim, mbik::MORPH_BAD_MODE);
	bad |= refused("null_positions", 5, 1, false, 1, 0, nullptr, nullptr, lim, mbik::MORPH_NULL);
	bad |= refused("normals_on_shapes_only", 5, 1, false, 1, 0, f, f, lim, mbik::MORPH_NORMALS_MISMATCH);
	bad |= refused("normals_on_mesh_only", 5, 1, true, 1, 0, f, nullptr, lim, mbik::MORPH_NORMALS_MISMATCH);
	bad |= refused("five_shapes_at_max_bones", mbik::kSkinMaxBones, 1, false, 5, 0, f, nullptr, lim, mbik::MORPH_TOO_LARGE);
	bad |= refused("four_shapes_at_max_bones", mbik::kSkinMaxBones, 1, false, 4, 0, f, nullptr, lim, mbik::MORPH_OK);
	bad |= refused("five_shapes_no_limit", mbik::kSkinMaxBones, 1, false, 5, 0, f, nullptr, -1, mbik::MORPH_OK);
	bad |= refused("accepted", 5, 1, true, 1, 1, f, f, lim, mbik::MORPH_OK);
	return bad ? 1 : 0;
}
