// The tangent stream's host code under ASan + UBSan: skin.h's and morph.h's tangent validation,
// tangent_layout / tangent_pack and the host paths behind mbik_skin_vertices_call_cpu (the kernels run the same
// per-vertex code), in the plain, the shaped and the listed form, compact and in place.  Every buffer is a heap block
// of exactly the documented size -- tangents V x 4 floats, shape tangents P x V x 3, out_tangents rows x V x 4 with
// rows = count or max_list, the device image tangent_layout().bytes -- so a read or a write one element off is a
// sanitizer report.  The results are also compared with the normal path fed the tangents (the tangent's steps are the
// normal's on another array), the sign with the input's bits, and the packed image with the arrays.
//   skin_tangent_san   -> exit 0 and one line per case, or a sanitizer report
#include <cstdio>
#include <vector>

#include "../../many_bone_ik_amd/csrc/skin_list.h"

namespace {

uint32_t g_state = 20261020u;
float rnd(float lo, float hi) { // LCG, top 24 bits
	g_state = g_state * 1664525u + 1013904223u;
	return lo + (hi - lo) * (float)(g_state >> 8) * (1.0f / 16777216.0f);
}

constexpr float kSentinel = -12345.678f;
// signs that no arithmetic may touch: -0, a signalling NaN with a payload, -inf, a denormal, -1, +1
const uint32_t kSigns[] = {0x80000000u, 0x7FA12345u, 0xFF800000u, 0x00000001u, 0xBF800000u, 0x3F800000u};

struct Mesh {
	int B, V, K, P, mode;
	std::vector<float> pos, nrm, tan, tan3, w, sp, sn, st;
	std::vector<int32_t> idx;
};

Mesh make_mesh(int B, int V, int K, int P, int mode) {
	Mesh m{B, V, K, P, mode, {}, {}, {}, {}, {}, {}, {}, {}, {}};
	m.pos.resize((size_t)V * 3), m.nrm.resize((size_t)V * 3), m.tan.resize((size_t)V * 4), m.tan3.resize((size_t)V * 3);
	m.w.resize((size_t)V * K), m.idx.resize((size_t)V * K);
	m.sp.resize((size_t)P * V * 3), m.sn.resize((size_t)P * V * 3), m.st.resize((size_t)P * V * 3);
	for (float &v : m.pos) v = rnd(-2.0f, 2.0f);
	for (float &v : m.nrm) v = rnd(-1.0f, 1.0f);
	for (int v = 0; v < V; v++) {
		for (int a = 0; a < 3; a++) m.tan3[(size_t)v * 3 + a] = m.tan[(size_t)v * 4 + a] = rnd(-1.0f, 1.0f);
		memcpy(&m.tan[(size_t)v * 4 + 3], &kSigns[v % 6], 4);
	}
	for (float &v : m.w) v = rnd(0.0f, 0.5f);
	for (int32_t &i : m.idx) i = (int32_t)(rnd(0.0f, 1.0f) * (float)B) % B;
	for (float &v : m.sp) v = rnd(-0.5f, 0.5f);
	for (float &v : m.sn) v = rnd(-0.1f, 0.1f);
	for (float &v : m.st) v = rnd(-0.1f, 0.1f);
	return m;
}

bool differ(const float *a, const float *b, size_t n) { return n != 0 && memcmp(a, b, n * 4) != 0; }

// validation, layout and packing
int check_layout(const char *name, const Mesh &m) {
	if (mbik::skin_check_tangents(nullptr, m.tan.data()) != mbik::SKIN_TANGENTS_WITHOUT_NORMALS ||
			mbik::skin_check_tangents(m.nrm.data(), m.tan.data()) != mbik::SKIN_OK || mbik::skin_check_tangents(nullptr, nullptr) != mbik::SKIN_OK ||
			mbik::tangent_check_shapes(true, true, nullptr) == mbik::TANGENT_OK || mbik::tangent_check_shapes(true, false, m.tan.data()) == mbik::TANGENT_OK ||
			mbik::tangent_check_shapes(false, true, m.tan.data()) == mbik::TANGENT_OK || mbik::tangent_check_shapes(true, true, m.tan.data()) != mbik::TANGENT_OK ||
			mbik::tangent_check_shapes(false, true, nullptr) != mbik::TANGENT_OK) {
		printf("%s: validation\n", name);
		return 2;
	}
	const mbik::SkinLayout sl = mbik::skin_layout(m.V, m.K, true);
	const mbik::MorphLayout ml = mbik::morph_layout(m.V, m.K, true, m.P);
	const mbik::TangentLayout none = mbik::tangent_layout(m.V, m.K, true, m.P, false), tl = mbik::tangent_layout(m.V, m.K, true, m.P, true);
	const int64_t front = m.P ? ml.bytes : sl.bytes;
	if (none.bytes != front || none.tan != -1 || none.stan != -1 || tl.tan != front || tl.tan % 16 != 0 ||
			tl.stan != (m.P ? front + tl.stride * 16 : -1) || tl.bytes != front + (int64_t)(1 + m.P) * tl.stride * 16) {
		printf("%s: layout\n", name);
		return 2;
	}
	// the image of a mesh without tangents, then the same with: the front part must not move
	std::vector<unsigned char> old_image((size_t)front), image((size_t)tl.bytes);
	for (std::vector<unsigned char> *im : {&old_image, &image}) {
		mbik::skin_pack(m.V, m.K, m.pos.data(), m.nrm.data(), m.idx.data(), m.w.data(), im->data());
		if (m.P) mbik::morph_pack(m.V, m.K, m.P, m.sp.data(), m.sn.data(), im->data());
	}
	mbik::tangent_pack(m.V, m.K, m.P, m.tan.data(), m.P ? m.st.data() : nullptr, image.data());
	if (front && memcmp(old_image.data(), image.data(), (size_t)front) != 0) {
		printf("%s: the planes in front moved\n", name);
		return 2;
	}
	for (int64_t v = 0; v < m.V; v++) {
		if (memcmp(image.data() + tl.tan + v * 16, m.tan.data() + v * 4, 16) != 0) return printf("%s: base tangent %lld\n", name, (long long)v), 2;
		for (int64_t j = 0; j < m.P; j++) {
			const unsigned char *r = image.data() + tl.stan + (j * tl.stride + v) * 16;
			const float zero = 0.0f;
			if (memcmp(r, m.st.data() + (j * m.V + v) * 3, 12) != 0 || memcmp(r + 12, &zero, 4) != 0)
				return printf("%s: shape tangent %lld of shape %lld\n", name, (long long)v, (long long)j), 2;
		}
	}
	mbik::tangent_pack(0, m.K, m.P, nullptr, nullptr, nullptr); // (a mesh without vertices)
	printf("%s: layout ok V=%d K=%d P=%d front=%lld bytes=%lld\n", name, m.V, m.K, m.P, (long long)front, (long long)tl.bytes);
	return 0;
}

// one list (empty: the range call) on one mesh
int run(const char *name, const Mesh &m, int count, const std::vector<int32_t> &list, int32_t list_count) {
	const bool listed = !list.empty();
	const int32_t max_list = (int32_t)list.size();
	std::vector<float> skin((size_t)count * m.B * 12), cw((size_t)count * m.P);
	for (float &v : skin) v = rnd(-1.5f, 1.5f);
	for (size_t i = 0; i < cw.size(); i++) cw[i] = i % 3 == 0 ? 0.00005f : rnd(-0.5f, 0.5f);
	const std::vector<int32_t> indices(list), n1(1, list_count);
	int64_t written = 0;
	for (int shaped = 0; shaped < (m.P ? 2 : 1); shaped++)
		for (int compact = 0; compact < (listed ? 2 : 1); compact++) {
			const size_t rows = listed && compact ? (size_t)max_list : (size_t)count;
			const size_t n3 = rows * m.V * 3, n4 = rows * m.V * 4;
			std::vector<float> out_p(n3, kSentinel), out_n(n3, kSentinel), out_t(n4, kSentinel);
			// the same form with the tangents as normals: positions again, and what out_tangents.xyz must be
			std::vector<float> as_p(n3, kSentinel), as_n(n3, kSentinel);
			const float *c = shaped ? cw.data() : nullptr;
			if (listed) {
				mbik::skin_vertices_listed_host(m.B, m.V, m.K, m.pos.data(), m.nrm.data(), m.idx.data(), m.w.data(), m.P, m.mode, m.sp.data(),
						m.sn.data(), count, indices.data(), n1.data(), max_list, skin.data(), c, compact != 0, out_p.data(), out_n.data(),
						m.tan.data(), shaped ? m.st.data() : nullptr, out_t.data());
				mbik::skin_vertices_listed_host(m.B, m.V, m.K, m.pos.data(), m.tan3.data(), m.idx.data(), m.w.data(), m.P, m.mode, m.sp.data(),
						m.st.data(), count, indices.data(), n1.data(), max_list, skin.data(), c, compact != 0, as_p.data(), as_n.data());
			} else if (shaped) {
				mbik::morph_skin_vertices_host(m.B, m.V, m.K, m.pos.data(), m.nrm.data(), m.idx.data(), m.w.data(), m.P, m.mode, m.sp.data(),
						m.sn.data(), count, skin.data(), c, out_p.data(), out_n.data(), m.tan.data(), m.st.data(), out_t.data());
				mbik::morph_skin_vertices_host(m.B, m.V, m.K, m.pos.data(), m.tan3.data(), m.idx.data(), m.w.data(), m.P, m.mode, m.sp.data(),
						m.st.data(), count, skin.data(), c, as_p.data(), as_n.data());
			} else {
				mbik::skin_vertices_host(m.B, m.V, m.K, m.pos.data(), m.nrm.data(), m.idx.data(), m.w.data(), count, skin.data(), out_p.data(),
						out_n.data(), m.tan.data(), out_t.data());
				mbik::skin_vertices_host(m.B, m.V, m.K, m.pos.data(), m.tan3.data(), m.idx.data(), m.w.data(), count, skin.data(), as_p.data(),
						as_n.data());
			}
			if (differ(out_p.data(), as_p.data(), n3)) return printf("%s: positions differ (shaped=%d compact=%d)\n", name, shaped, compact), 2;
			for (size_t r = 0; r < rows; r++) {
				const bool touched = m.V > 0 && memcmp(&out_p[r * m.V * 3], &kSentinel, 4) != 0;
				written += touched;
				for (size_t v = 0; v < (size_t)m.V; v++) {
					const float *t = &out_t[(r * m.V + v) * 4];
					if (!touched) {
						if (memcmp(t, &kSentinel, 4) != 0 || memcmp(t + 3, &kSentinel, 4) != 0) return printf("%s: an unlisted row was written\n", name), 2;
						continue;
					}
					if (differ(t, &as_n[(r * m.V + v) * 3], 3)) return printf("%s: tangent xyz differs (shaped=%d compact=%d)\n", name, shaped, compact), 2;
					if (memcmp(t + 3, &m.tan[v * 4 + 3], 4) != 0) return printf("%s: the sign's bits changed\n", name), 2;
				}
			}
		}
	printf("%s: ok B=%d V=%d K=%d P=%d skeletons=%d max_list=%d list_count=%d rows_written=%lld\n", name, m.B, m.V, m.K, m.P, count, max_list,
			list_count, (long long)written);
	return 0;
}

} // namespace

int main() {
	int bad = 0;
	const Mesh plain = make_mesh(5, 41, 4, 0, 0), rel = make_mesh(9, 33, 8, 3, mbik::MORPH_RELATIVE),
			   nor = make_mesh(4, 17, 4, 5, mbik::MORPH_NORMALIZED), one = make_mesh(1, 1, 8, 1, mbik::MORPH_RELATIVE);
	const int count = 6;
	bad |= check_layout("plain", plain) != 0;
	bad |= check_layout("relative", rel) != 0;
	bad |= check_layout("normalized", nor) != 0;
	bad |= check_layout("one_vertex", one) != 0;
	bad |= run("range", plain, count, {}, 0) != 0;
	bad |= run("range_relative", rel, count, {}, 0) != 0;
	bad |= run("range_normalized", nor, count, {}, 0) != 0;
	bad |= run("range_one_vertex", one, count, {}, 0) != 0;
	bad |= run("count_zero", rel, count, {0, 1, 2}, 0) != 0;
	bad |= run("all", plain, count, {0, 1, 2, 3, 4, 5}, 6) != 0;
	bad |= run("out_of_range", nor, count, {2, -1, 5, count, 0}, 5) != 0;
	bad |= run("duplicates", rel, count, {0, 0, 5, 5}, 4) != 0;
	bad |= run("count_above_buffer", nor, count, {1, 3}, 1000) != 0;
	bad |= run("list_longer_than_batch", rel, count, {0, 1, 2, 3, 4, 5, 5, 4, 3}, 9) != 0;
	return bad ? 1 : 0;
}
