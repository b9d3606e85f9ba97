// skin_list.h under ASan + UBSan: the host path behind mbik_skin_vertices_listed_cpu (the kernels run the
// same per-vertex code) on built-in meshes and lists: empty, every skeleton, out-of-range entries (-1 and
// count), duplicates, a count above and below the list's buffer, compact and in place, plain and shaped.
// Every buffer is a heap block of exactly the documented size -- the compact outputs max_list rows, the
// in-place ones count rows, indices max_list entries -- so an entry that is not skipped, or a row placed
// by the wrong rule, is a sanitizer report; the rows are also compared with the whole-batch host calls.
//   skin_list_san   -> exit 0 and one line per case, or a sanitizer report
#include <cstdio>
#include <vector>

#include "../../many_bone_ik_amd/csrc/skin_list.h"

namespace {

uint32_t g_state = 20250915u;
float rnd(float lo, float hi) { // LCG, top 24 bits
	g_state = g_state * 1664525u + 1013904223u;
	return lo + (hi - lo) * (float)(g_state >> 8) * (1.0f / 16777216.0f);
}

constexpr float kSentinel = -12345.678f;

struct Mesh {
	int B, V, K, P, mode;
	std::vector<float> pos, nrm, w, sp, sn;
	std::vector<int32_t> idx;
};

Mesh make_mesh(int B, int V, int K, int P, int mode) {
	Mesh m{B, V, K, P, mode, {}, {}, {}, {}, {}, {}};
	m.pos.resize((size_t)V * 3), m.nrm.resize((size_t)V * 3), m.w.resize((size_t)V * K), m.idx.resize((size_t)V * K);
	m.sp.resize((size_t)P * V * 3), m.sn.resize((size_t)P * V * 3);
	for (float &v : m.pos) v = rnd(-2.0f, 2.0f);
	for (float &v : m.nrm) v = rnd(-1.0f, 1.0f);
	for (float &v : m.w) v = rnd(0.0f, 0.5f);
	for (int32_t &i : m.idx) i = (int32_t)(rnd(0.0f, 1.0f) * (float)B) % B;
	for (float &v : m.sp) v = rnd(-0.5f, 0.5f);
	for (float &v : m.sn) v = rnd(-0.1f, 0.1f);
	return m;
}

// one list on one mesh: compact and in place, with and without shape weights (shaped meshes), with and without normals
int run(const char *name, const Mesh &m, int count, const std::vector<int32_t> &list, int32_t list_count) {
	const int32_t max_list = (int32_t)list.size();
	std::vector<float> skin((size_t)count * m.B * 12), cw((size_t)count * m.P);
	for (float &v : skin) v = rnd(-1.5f, 1.5f);
	for (size_t i = 0; i < cw.size(); i++) cw[i] = i % 3 == 0 ? 0.00005f : rnd(-0.5f, 0.5f);
	const std::vector<int32_t> indices(list); // (exactly max_list entries)
	const std::vector<int32_t> n1(1, list_count);
	const size_t row = (size_t)m.V * 3;
	// the whole batch by the existing host paths
	std::vector<float> full_p[2], full_n[2];
	for (int shaped = 0; shaped < (m.P ? 2 : 1); shaped++) {
		full_p[shaped].resize((size_t)count * row), full_n[shaped].resize((size_t)count * row);
		if (shaped)
			mbik::morph_skin_vertices_host(m.B, m.V, m.K, m.pos.data(), m.nrm.data(), m.idx.data(), m.w.data(), m.P, m.mode, m.sp.data(),
					m.sn.data(), count, skin.data(), cw.data(), full_p[1].data(), full_n[1].data());
		else
			mbik::skin_vertices_host(m.B, m.V, m.K, m.pos.data(), m.nrm.data(), m.idx.data(), m.w.data(), count, skin.data(),
					full_p[0].data(), full_n[0].data());
	}
	const int32_t n = mbik::skin_list_length(n1.data(), max_list);
	int64_t written = 0;
	for (int shaped = 0; shaped < (m.P ? 2 : 1); shaped++)
		for (int compact = 0; compact < 2; compact++)
			for (int normals = 0; normals < 2; normals++) {
				const size_t rows = compact ? (size_t)max_list : (size_t)count;
				std::vector<float> out_p(rows * row, kSentinel), out_n(normals ? rows * row : 0, kSentinel);
				mbik::skin_vertices_listed_host(m.B, m.V, m.K, m.pos.data(), normals ? m.nrm.data() : nullptr, m.idx.data(), m.w.data(), m.P,
						m.mode, m.sp.data(), normals ? m.sn.data() : nullptr, count, indices.data(), n1.data(), max_list, skin.data(),
						shaped ? cw.data() : nullptr, compact != 0, out_p.data(), normals ? out_n.data() : nullptr);
				std::vector<float> want_p(rows * row, kSentinel), want_n(out_n.size(), kSentinel);
				for (int32_t r = 0; r < n; r++) {
					const int32_t s = indices[r];
					if (s < 0 || s >= count) continue;
					const size_t to = (compact ? (size_t)r : (size_t)s) * row;
					memcpy(want_p.data() + to, full_p[shaped].data() + (size_t)s * row, row * 4);
					// (the shaped call renormalises the normal and a call without normals has none: compare what was asked for)
					if (normals) memcpy(want_n.data() + to, full_n[shaped].data() + (size_t)s * row, row * 4);
					written++;
				}
				const auto differ = [](const std::vector<float> &a, const std::vector<float> &b) {
					return !a.empty() && memcmp(a.data(), b.data(), a.size() * 4) != 0; // (bitwise; an empty block has no address)
				};
				if (differ(out_p, want_p) || differ(out_n, want_n)) {
					printf("%s: rows differ (shaped=%d compact=%d normals=%d)\n", name, shaped, compact, normals);
					return 2;
				}
			}
	printf("%s: ok B=%d V=%d K=%d P=%d skeletons=%d max_list=%d list_count=%d n=%d rows_written=%lld\n", name, m.B, m.V, m.K, m.P, count,
			max_list, list_count, n, (long long)written);
	return 0;
}

} // namespace

int main() {
	int bad = 0;
	const Mesh plain = make_mesh(5, 40, 4, 0, 0), rel = make_mesh(9, 33, 8, 3, mbik::MORPH_RELATIVE),
			   nor = make_mesh(4, 17, 4, 5, mbik::MORPH_NORMALIZED);
	const int count = 6;
	bad |= run("empty_list", plain, count, {}, 0) != 0;
	bad |= run("count_zero", rel, count, {0, 1, 2}, 0) != 0;
	bad |= run("count_negative", nor, count, {3, 4}, -7) != 0;
	bad |= run("all", plain, count, {0, 1, 2, 3, 4, 5}, 6) != 0;
	bad |= run("all_shaped", rel, count, {0, 1, 2, 3, 4, 5}, 6) != 0;
	bad |= run("descending", nor, count, {5, 4, 3, 2, 1, 0}, 6) != 0;
	bad |= run("out_of_range", plain, count, {2, -1, 5, count, 0}, 5) != 0;
	bad |= run("out_of_range_shaped", nor, count, {-1, count, 3, -1}, 4) != 0;
	bad |= run("only_out_of_range", rel, count, {count, -1}, 2) != 0;
	bad |= run("duplicates", plain, count, {4, 4, 1, 4, 1}, 5) != 0;
	bad |= run("duplicates_shaped", rel, count, {0, 0, 5, 5}, 4) != 0;
	bad |= run("count_above_buffer", nor, count, {1, 3}, 1000) != 0;
	bad |= run("stale_tail", plain, count, {3, 0, 5, 1, 2}, 2) != 0;
	bad |= run("list_longer_than_batch", rel, count, {0, 1, 2, 3, 4, 5, 5, 4, 3}, 9) != 0;
	return bad ? 1 : 0;
}
