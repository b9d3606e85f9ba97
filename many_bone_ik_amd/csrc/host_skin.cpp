// Linear blend skinning of meshes from skin transforms (include/mbik.h, ABI 10): the mesh handle,
// mbik_skin_vertices, which launches k_skin.hip's kernel on the mesh's device, and
// mbik_skin_vertices_cpu, which runs the same per-vertex code (skin.h) on the host.  The
// semantics are those of Godot's skeleton compute shader on ArrayMesh surface arrays;
// DESIGN.md §14.  Blend shapes in front of the skinning (ABI 13, morph.h):
// mbik_mesh_create_shaped, mbik_skin_vertices_shaped and mbik_skin_vertices_shaped_cpu.  The mesh
// also carries its bone boxes (ABI 14, bounds.h); host_bounds.cpp uses them.
// List-driven skinning (ABI 15, skin_list.h): mbik_skin_vertices_listed, which launches
// k_skin_list.hip's kernels, and mbik_skin_vertices_listed_cpu.  The tangent stream and the struct-based call over
// the three forms: mbik_mesh_create_desc, mbik_skin_vertices_call and mbik_skin_vertices_call_cpu.
#include "host.h"

#include "bounds.h"
#include "morph.h"
#include "skin.h"
#include "skin_list.h"

using namespace mbik_host;

namespace mbik_host {

int check_mesh(int32_t B, int32_t V, int32_t K, const float *positions, const int32_t *bone_indices, const float *weights) {
	int64_t bad_v = 0;
	int bad_k = 0;
	const mbik::SkinCheck c = mbik::skin_check_mesh(B, V, K, positions, bone_indices, weights, &bad_v, &bad_k);
	if (c == mbik::SKIN_BAD_INDEX)
		return fail(MBIK_EINVAL, "vertex " + std::to_string(bad_v) + " influence " + std::to_string(bad_k) + ": bone index " +
				std::to_string(bone_indices[bad_v * K + bad_k]) + " outside [0, " + std::to_string(B) + ")");
	if (c != mbik::SKIN_OK) return fail(MBIK_EINVAL, mbik::skin_check_text(c));
	return MBIK_OK;
}

} // namespace mbik_host

namespace {

// LDS a block aims for: eight 256-thread blocks (all 32 wave slots) share a CU's 160 KiB.
// (-DMBIK_SKIN_LDS_TARGET_KIB=n: A/B builds of the skeletons-per-block trade-off)
#ifndef MBIK_SKIN_LDS_TARGET_KIB
#define MBIK_SKIN_LDS_TARGET_KIB 20
#endif
constexpr int64_t kSkinBlockLdsTarget = MBIK_SKIN_LDS_TARGET_KIB * 1024;
// Skeletons a block loops over with one vertex in registers; more would amortise nothing further
// (the mesh is read from L2) and leave fewer blocks to balance.
constexpr int kSkinMaxSkeletonsPerBlock = 16;
// Blocks the grid aims for before it stops splitting the vertex range: eight per CU.
constexpr int kSkinBlocksPerCu = 8;

struct SkinShape {
	int S, chunk, chunks, vshift;
};

// S: as many skeletons as the LDS target holds.  Vertex chunks: enough for kSkinBlocksPerCu blocks
// a CU, but no chunk shorter than 256 vertices or than 8 vertices per bone -- every block stages
// its S x B matrices again, 12 LDS dword writes a bone against 3 K quad reads a vertex.
// shaped: a block also stages its skeletons' shape weights (mbik_skin_vertices_shaped).
SkinShape shape_of(const mbik_mesh *m, int64_t count, bool shaped) {
	const int64_t per = std::max<int64_t>(48, (int64_t)m->B * 48) + (shaped ? (int64_t)m->P * 4 : 0);
	SkinShape sh;
	sh.S = (int)std::max<int64_t>(1, std::min<int64_t>({kSkinBlockLdsTarget / per, kSkinMaxSkeletonsPerBlock, count}));
	const int64_t tiles = std::max<int64_t>(1, (count + sh.S - 1) / sh.S);
	const int64_t chunk_min = std::max<int64_t>(256, ((int64_t)m->B * 8 + 255) / 256 * 256);
	const int64_t want = ((int64_t)m->cu_count * kSkinBlocksPerCu + tiles - 1) / tiles;
	const int64_t n = std::max<int64_t>(1, std::min<int64_t>(want, m->V / chunk_min));
	sh.chunk = (int)std::max<int64_t>(256, ((m->V + n - 1) / n + 255) / 256 * 256);
	sh.chunks = (int)std::max<int64_t>(1, ((int64_t)m->V + sh.chunk - 1) / sh.chunk);
	const int lanes = std::min<int64_t>(sh.chunk, m->V);
	sh.vshift = lanes <= 64 ? 6 : (lanes <= 128 ? 7 : 8);
	return sh;
}

// The argument checks of a skinning call past the mesh's own; 0 = launch, 1 = nothing to do.
// out_rows: the outputs' rows where they are not `count` (the listed call's compact form; 0 = nothing to do).
int check_call(int32_t B, int32_t V, bool mesh_normals, int32_t count, const float *skin, const float *out_positions,
		const float *out_normals, int64_t out_rows = -1) {
	if (count < 0) return fail(MBIK_EINVAL, "negative count");
	if (out_normals && !mesh_normals) return fail(MBIK_EINVAL, "out_normals given for a mesh without normals");
	if (count == 0 || V == 0 || out_rows == 0) return 1;
	if (!skin) return fail(MBIK_EINVAL, "null skin");
	if (!out_positions) return fail(MBIK_EINVAL, "null out_positions");
	const size_t nskin = (size_t)count * B * 12 * sizeof(float), nout = (size_t)(out_rows < 0 ? count : out_rows) * V * 3 * sizeof(float);
	if (overlap(skin, nskin, out_positions, nout)) return fail(MBIK_EINVAL, "out_positions overlaps skin");
	if (out_normals && overlap(skin, nskin, out_normals, nout)) return fail(MBIK_EINVAL, "out_normals overlaps skin");
	if (out_normals && overlap(out_positions, nout, out_normals, nout)) return fail(MBIK_EINVAL, "out_normals overlaps out_positions");
	return 0;
}

// The shape checks mbik_mesh_create_shaped and mbik_skin_vertices_shaped_cpu share; lds_limit as morph_check's.
int check_shapes(int32_t B, int32_t V, bool mesh_normals, const mbik_mesh_shapes *sh, int64_t lds_limit) {
	if (!sh) return fail(MBIK_EINVAL, "null shapes");
	if (sh->struct_size < (int32_t)sizeof(mbik_mesh_shapes)) return fail(MBIK_EINVAL, "mbik_mesh_shapes.struct_size is too small");
	const mbik::MorphCheck c = mbik::morph_check(B, V, mesh_normals, sh->shape_count, sh->mode, sh->positions, sh->normals, lds_limit);
	if (c == mbik::MORPH_TOO_LARGE)
		return fail(MBIK_EUNSUPPORTED, "rig has " + std::to_string(B) + " bones and " + std::to_string(sh->shape_count) +
				" shapes: " + mbik::morph_check_text(c) + " (MBIK_MAX_LDS_BYTES)");
	if (c != mbik::MORPH_OK) return fail(MBIK_EINVAL, mbik::morph_check_text(c));
	return MBIK_OK;
}

// The checks of a shaped call's weights, past check_call's; out_rows as there.
int check_shape_weights(int32_t V, int32_t P, int32_t count, const float *shape_weights, const float *out_positions,
		const float *out_normals, int64_t out_rows = -1) {
	if (!shape_weights) return fail(MBIK_EINVAL, "null shape_weights");
	const size_t nw = (size_t)count * P * sizeof(float), nout = (size_t)(out_rows < 0 ? count : out_rows) * V * 3 * sizeof(float);
	if (overlap(shape_weights, nw, out_positions, nout)) return fail(MBIK_EINVAL, "out_positions overlaps shape_weights");
	if (out_normals && overlap(shape_weights, nw, out_normals, nout)) return fail(MBIK_EINVAL, "out_normals overlaps shape_weights");
	return MBIK_OK;
}

// The checks of a listed call (mbik_skin_vertices_listed and its _cpu form) past the mesh's and the shapes' own: everything
// the plain or the shaped call refuses, with the outputs sized by the flag, and the list's own.  P: the mesh's shapes
// (0: none).  0 = run, 1 = nothing to do.
int check_listed(int32_t B, int32_t V, bool mesh_normals, int32_t P, int32_t count, const int32_t *indices, const int32_t *list_count,
		int32_t max_list, const float *skin, const float *shape_weights, uint32_t flags, const float *out_positions,
		const float *out_normals) {
	if (flags & ~mbik::kSkinListFlags) return fail(MBIK_EINVAL, "unknown flag bits");
	if (max_list < 0) return fail(MBIK_EINVAL, "negative max_list");
	if (shape_weights && P < 1) return fail(MBIK_EINVAL, "shape_weights given for a mesh without shapes");
	const int64_t rows = max_list == 0 ? 0 : ((flags & mbik::kSkinListCompact) ? max_list : count);
	if (int rc = check_call(B, V, mesh_normals, count, skin, out_positions, out_normals, rows)) return rc;
	if (shape_weights)
		if (int rc = check_shape_weights(V, P, count, shape_weights, out_positions, out_normals, rows)) return rc;
	if (!indices) return fail(MBIK_EINVAL, "null indices");
	if (!list_count) return fail(MBIK_EINVAL, "null list_count");
	const size_t nout = (size_t)rows * V * 3 * sizeof(float), nidx = (size_t)max_list * sizeof(int32_t);
	for (const float *out : {out_positions, out_normals}) {
		if (!out) continue;
		const char *which = out == out_positions ? "out_positions" : "out_normals";
		if (overlap(indices, nidx, out, nout)) return fail(MBIK_EINVAL, std::string(which) + " overlaps indices");
		if (overlap(list_count, sizeof(int32_t), out, nout)) return fail(MBIK_EINVAL, std::string(which) + " overlaps list_count");
	}
	return 0;
}

// What the three device entry points do behind their checks: guard the mesh's device, pick the launch shape for
// `tiled` skeletons or list entries, fill in what the mesh knows of `a` (the caller has set count, the buffers and, listed,
// the list), launch.  A call with a.shape_weights is a shaped one.  failed: the error text's head.
int launch_on_mesh(const mbik_mesh *m, void *hip_stream, int64_t tiled, mbik::SkinLaunch a, hipError_t (*launch)(const mbik::SkinLaunch &),
		const char *failed) {
	DeviceGuard guard(m->device);
	const SkinShape sh = shape_of(m, tiled, a.shape_weights != nullptr);
	a.st = reinterpret_cast<hipStream_t>(hip_stream);
	a.K = m->K, a.mode = m->mode, a.B = m->B, a.V = m->V, a.P = m->P;
	a.S = sh.S, a.chunk = sh.chunk, a.chunks = sh.chunks, a.vshift = sh.vshift;
	a.mesh = m->mesh.as<unsigned char>(), a.mesh_normals = m->normals, a.mesh_tangents = m->tangents;
	const hipError_t e = launch(a);
	if (e != hipSuccess) return fail(MBIK_EHIP, std::string(failed) + hipGetErrorString(e));
	return MBIK_OK;
}

// The tangent checks mbik_mesh_create_desc and mbik_skin_vertices_call_cpu share.
int check_tangents(const float *normals, const float *tangents, bool shaped, const float *shape_tangents) {
	const mbik::SkinCheck c = mbik::skin_check_tangents(normals, tangents);
	if (c != mbik::SKIN_OK) return fail(MBIK_EINVAL, mbik::skin_check_text(c));
	const mbik::TangentCheck t = mbik::tangent_check_shapes(shaped, tangents != nullptr, shape_tangents);
	if (t != mbik::TANGENT_OK) return fail(MBIK_EINVAL, mbik::tangent_check_text(t));
	return MBIK_OK;
}

// mbik_mesh_create (shaped == false: `shapes` is not looked at), mbik_mesh_create_shaped and, with tangents [V][4] (and
// shape_tangents [P][V][3] on a shaped mesh), mbik_mesh_create_desc.  Without tangents the device image is what it always was.
int create_mesh(int32_t bone_count, int32_t vertex_count, int32_t influences, const float *positions, const float *normals,
		const int32_t *bone_indices, const float *weights, bool shaped, const mbik_mesh_shapes *shapes, int32_t device,
		mbik_mesh **out_mesh, const float *tangents = nullptr, const float *shape_tangents = nullptr) {
	if (!out_mesh) return fail(MBIK_EINVAL, "null out_mesh");
	*out_mesh = nullptr;
	if (influences != 4 && influences != 8) return fail(MBIK_EINVAL, mbik::skin_check_text(mbik::SKIN_BAD_INFLUENCES));
	if (bone_count < 0 || vertex_count < 0) return fail(MBIK_EINVAL, mbik::skin_check_text(mbik::SKIN_NEGATIVE));
	if (vertex_count > 0 && (!positions || !bone_indices || !weights)) return fail(MBIK_EINVAL, mbik::skin_check_text(mbik::SKIN_NULL));
	if (bone_count > mbik::kSkinMaxBones)
		return fail(MBIK_EUNSUPPORTED, "rig has " + std::to_string(bone_count) + " bones; a mesh supports at most " +
				std::to_string(mbik::kSkinMaxBones) + " (MBIK_SKIN_MAX_BONES: one skeleton's matrices must fit 160 KiB of LDS)");
	if (shaped)
		if (int rc = check_shapes(bone_count, vertex_count, normals != nullptr, shapes, mbik::kSkinMaxLdsBytes)) return rc;
	if (int rc = check_tangents(normals, tangents, shaped, shape_tangents)) return rc;
	if (int rc = check_mesh(bone_count, vertex_count, influences, positions, bone_indices, weights)) return rc;
	if (int rc = check_device(device)) return rc;
	std::unique_ptr<mbik_mesh> m(new mbik_mesh());
	m->device = device, m->B = bone_count, m->V = vertex_count, m->K = influences, m->normals = normals != nullptr;
	m->tangents = tangents != nullptr;
	if (shaped) m->P = shapes->shape_count, m->mode = shapes->mode;
	DeviceGuard guard(device);
	m->cu_count = cu_count_of(device);
	if (vertex_count > 0) {
		const mbik::SkinLayout l = mbik::skin_layout(vertex_count, influences, m->normals);
		int64_t bytes = shaped ? mbik::morph_layout(vertex_count, influences, m->normals, m->P).bytes : l.bytes;
		if (tangents) bytes = mbik::tangent_layout(vertex_count, influences, true, m->P, true).bytes;
		std::vector<unsigned char> packed((size_t)bytes);
		mbik::skin_pack(vertex_count, influences, positions, normals, bone_indices, weights, packed.data());
		if (shaped) mbik::morph_pack(vertex_count, influences, m->P, shapes->positions, shapes->normals, packed.data());
		if (tangents) mbik::tangent_pack(vertex_count, influences, m->P, tangents, shape_tangents, packed.data());
		if (int rc = m->mesh.upload(packed.data(), packed.size(), "the mesh")) return rc;
	}
	// the bone boxes (bounds.h): a table of their own, the used bones only
	m->bone_boxes.resize((size_t)bone_count * 6), m->bone_used.resize((size_t)bone_count);
	mbik::bone_boxes_build(bone_count, vertex_count, influences, positions, bone_indices, weights, m->bone_boxes.data(), m->bone_used.data());
	m->used_bones = mbik::bone_table_count(bone_count, m->bone_used.data());
	if (m->used_bones > 0) {
		std::vector<unsigned char> table((size_t)m->used_bones * mbik::kBoneRecordBytes);
		mbik::bone_table_pack(bone_count, m->bone_boxes.data(), m->bone_used.data(), table.data());
		if (int rc = m->bone_table.upload(table.data(), table.size(), "the mesh's bone boxes")) return rc;
	}
	*out_mesh = m.release();
	return MBIK_OK;
}

// ---- mbik_skin_vertices_call and its _cpu form ----
struct MeshFacts {
	int32_t B, V, P;
	bool normals, tangents;
};

int check_call_struct(const mbik_skin_call *c) {
	if (!c) return fail(MBIK_EINVAL, "null call");
	if (c->struct_size < (int32_t)sizeof(mbik_skin_call)) return fail(MBIK_EINVAL, "mbik_skin_call.struct_size is too small");
	return MBIK_OK;
}

// The checks both entries run on a call past its struct's own: the form's existing checks with their texts, then the
// tangent output's.  0 = run, 1 = nothing to do.
int check_skin_call(const MeshFacts &f, const mbik_skin_call *c) {
	if ((c->indices != nullptr) != (c->list_count != nullptr)) return fail(MBIK_EINVAL, "indices and list_count must be given together");
	if (c->out_tangents && !f.tangents) return fail(MBIK_EINVAL, "out_tangents given for a mesh without tangents");
	if (c->out_tangents && !c->out_normals) return fail(MBIK_EINVAL, "out_tangents given without out_normals");
	const bool listed = c->indices != nullptr;
	int64_t rows = c->count;
	if (listed) {
		if (int rc = check_listed(f.B, f.V, f.normals, f.P, c->count, c->indices, c->list_count, c->max_list, c->skin, c->shape_weights,
					c->flags, c->out_positions, c->out_normals))
			return rc;
		rows = (c->flags & mbik::kSkinListCompact) ? c->max_list : c->count;
	} else {
		if (c->shape_weights && f.P < 1) return fail(MBIK_EINVAL, "the mesh has no shapes (mbik_mesh_create_shaped)");
		if (int rc = check_call(f.B, f.V, f.normals, c->count, c->skin, c->out_positions, c->out_normals)) return rc;
		if (c->shape_weights)
			if (int rw = check_shape_weights(f.V, f.P, c->count, c->shape_weights, c->out_positions, c->out_normals)) return rw;
	}
	if (!c->out_tangents) return 0;
	const size_t nt = (size_t)rows * f.V * 4 * sizeof(float), nout = (size_t)rows * f.V * 3 * sizeof(float);
	const auto hit = [&](const void *p, size_t n) { return p && overlap(p, n, c->out_tangents, nt); };
	if (hit(c->skin, (size_t)c->count * f.B * 12 * sizeof(float))) return fail(MBIK_EINVAL, "out_tangents overlaps skin");
	if (hit(c->shape_weights, (size_t)c->count * f.P * sizeof(float))) return fail(MBIK_EINVAL, "out_tangents overlaps shape_weights");
	if (listed && hit(c->indices, (size_t)c->max_list * sizeof(int32_t))) return fail(MBIK_EINVAL, "out_tangents overlaps indices");
	if (listed && hit(c->list_count, sizeof(int32_t))) return fail(MBIK_EINVAL, "out_tangents overlaps list_count");
	if (hit(c->out_positions, nout)) return fail(MBIK_EINVAL, "out_tangents overlaps out_positions");
	if (hit(c->out_normals, nout)) return fail(MBIK_EINVAL, "out_tangents overlaps out_normals");
	return 0;
}

int check_desc_struct(const mbik_mesh_desc *d) {
	if (!d) return fail(MBIK_EINVAL, "null desc");
	if (d->struct_size < (int32_t)sizeof(mbik_mesh_desc)) return fail(MBIK_EINVAL, "mbik_mesh_desc.struct_size is too small");
	return MBIK_OK;
}

} // namespace

extern "C" {

int32_t mbik_mesh_create_desc(const mbik_mesh_desc *d, int32_t device, mbik_mesh **out_mesh) {
	if (out_mesh) *out_mesh = nullptr;
	if (int rc = check_desc_struct(d)) return rc;
	return create_mesh(d->bone_count, d->vertex_count, d->influences, d->positions, d->normals, d->bone_indices, d->weights,
			d->shapes != nullptr, d->shapes, device, out_mesh, d->tangents, d->shape_tangents);
}

int32_t mbik_skin_vertices_call(mbik_mesh *m, const mbik_skin_call *c, void *hip_stream) {
	if (int rc = check_call_struct(c)) return rc;
	if (!m) return fail(MBIK_EINVAL, "null mesh");
	const int rc = check_skin_call(MeshFacts{m->B, m->V, m->P, m->normals, m->tangents}, c);
	if (rc) return rc < 0 ? rc : MBIK_OK;
	mbik::SkinLaunch a{};
	a.count = c->count, a.skin = c->skin, a.shape_weights = c->shape_weights;
	a.out_p = c->out_positions, a.out_n = c->out_normals, a.out_t = c->out_tangents;
	if (!c->indices)
		return launch_on_mesh(m, hip_stream, c->count, a, mbik::launch_skin,
				c->shape_weights ? "shaped skinning launch failed: " : "skinning launch failed: ");
	a.indices = c->indices, a.list_count = c->list_count, a.max_list = c->max_list, a.compact = (c->flags & mbik::kSkinListCompact) != 0;
	return launch_on_mesh(m, hip_stream, c->max_list, a, mbik::launch_skin_listed, "listed skinning launch failed: ");
}

int32_t mbik_skin_vertices_call_cpu(const mbik_mesh_desc *d, const mbik_skin_call *c) {
	if (int rc = check_desc_struct(d)) return rc;
	if (int rc = check_call_struct(c)) return rc;
	if (int rc = check_mesh(d->bone_count, d->vertex_count, d->influences, d->positions, d->bone_indices, d->weights)) return rc;
	if (d->shapes)
		if (int rc = check_shapes(d->bone_count, d->vertex_count, d->normals != nullptr, d->shapes, -1)) return rc;
	if (int rc = check_tangents(d->normals, d->tangents, d->shapes != nullptr, d->shape_tangents)) return rc;
	const int32_t P = d->shapes ? d->shapes->shape_count : 0;
	const int rc = check_skin_call(MeshFacts{d->bone_count, d->vertex_count, P, d->normals != nullptr, d->tangents != nullptr}, c);
	if (rc) return rc < 0 ? rc : MBIK_OK;
	const float *tan = c->out_tangents ? d->tangents : nullptr, *stan = c->out_tangents ? d->shape_tangents : nullptr;
	if (c->indices)
		mbik::skin_vertices_listed_host(d->bone_count, d->vertex_count, d->influences, d->positions, d->normals, d->bone_indices, d->weights,
				P, d->shapes ? d->shapes->mode : 0, d->shapes ? d->shapes->positions : nullptr, d->shapes ? d->shapes->normals : nullptr,
				c->count, c->indices, c->list_count, c->max_list, c->skin, c->shape_weights, (c->flags & mbik::kSkinListCompact) != 0,
				c->out_positions, c->out_normals, tan, stan, c->out_tangents);
	else if (c->shape_weights)
		mbik::morph_skin_vertices_host(d->bone_count, d->vertex_count, d->influences, d->positions, d->normals, d->bone_indices, d->weights,
				P, d->shapes->mode, d->shapes->positions, d->shapes->normals, c->count, c->skin, c->shape_weights, c->out_positions,
				c->out_normals, tan, stan, c->out_tangents);
	else
		mbik::skin_vertices_host(d->bone_count, d->vertex_count, d->influences, d->positions, d->normals, d->bone_indices, d->weights,
				c->count, c->skin, c->out_positions, c->out_normals, tan, c->out_tangents);
	return MBIK_OK;
}

int32_t mbik_mesh_create(int32_t bone_count, int32_t vertex_count, int32_t influences, const float *positions, const float *normals,
		const int32_t *bone_indices, const float *weights, int32_t device, mbik_mesh **out_mesh) {
	return create_mesh(bone_count, vertex_count, influences, positions, normals, bone_indices, weights, false, nullptr, device, out_mesh);
}

int32_t mbik_mesh_create_shaped(int32_t bone_count, int32_t vertex_count, int32_t influences, const float *positions,
		const float *normals, const int32_t *bone_indices, const float *weights, const mbik_mesh_shapes *shapes, int32_t device,
		mbik_mesh **out_mesh) {
	return create_mesh(bone_count, vertex_count, influences, positions, normals, bone_indices, weights, true, shapes, device, out_mesh);
}

void mbik_mesh_destroy(mbik_mesh *m) { delete m; }

int32_t mbik_mesh_launch_shape(const mbik_mesh *m, int32_t count, int32_t *skeletons_per_block, int32_t *vertex_chunks) {
	if (!m) return fail(MBIK_EINVAL, "null mesh");
	if (count < 0) return fail(MBIK_EINVAL, "negative count");
	const SkinShape sh = shape_of(m, count, m->P > 0);
	if (skeletons_per_block) *skeletons_per_block = sh.S;
	if (vertex_chunks) *vertex_chunks = sh.chunks;
	return MBIK_OK;
}

int32_t mbik_skin_vertices(mbik_mesh *m, int32_t count, const float *skin, float *out_positions, float *out_normals,
		void *hip_stream) {
	if (!m) return fail(MBIK_EINVAL, "null mesh");
	const int rc = check_call(m->B, m->V, m->normals, count, skin, out_positions, out_normals);
	if (rc) return rc < 0 ? rc : MBIK_OK;
	mbik::SkinLaunch a{};
	a.count = count, a.skin = skin, a.out_p = out_positions, a.out_n = out_normals;
	return launch_on_mesh(m, hip_stream, count, a, mbik::launch_skin, "skinning launch failed: ");
}

int32_t mbik_skin_vertices_shaped(mbik_mesh *m, int32_t count, const float *skin, const float *shape_weights, float *out_positions,
		float *out_normals, void *hip_stream) {
	if (!m) return fail(MBIK_EINVAL, "null mesh");
	if (m->P < 1) return fail(MBIK_EINVAL, "the mesh has no shapes (mbik_mesh_create_shaped)");
	const int rc = check_call(m->B, m->V, m->normals, count, skin, out_positions, out_normals);
	if (rc) return rc < 0 ? rc : MBIK_OK;
	if (int rw = check_shape_weights(m->V, m->P, count, shape_weights, out_positions, out_normals)) return rw;
	mbik::SkinLaunch a{};
	a.count = count, a.skin = skin, a.shape_weights = shape_weights, a.out_p = out_positions, a.out_n = out_normals;
	return launch_on_mesh(m, hip_stream, count, a, mbik::launch_skin, "shaped skinning launch failed: ");
}

int32_t mbik_skin_vertices_listed(mbik_mesh *m, int32_t count, const int32_t *indices, const int32_t *list_count, int32_t max_list,
		const float *skin, const float *shape_weights, uint32_t flags, float *out_positions, float *out_normals, void *hip_stream) {
	if (!m) return fail(MBIK_EINVAL, "null mesh");
	const int rc = check_listed(m->B, m->V, m->normals, m->P, count, indices, list_count, max_list, skin, shape_weights, flags,
			out_positions, out_normals);
	if (rc) return rc < 0 ? rc : MBIK_OK;
	mbik::SkinLaunch a{};
	a.count = count, a.skin = skin, a.shape_weights = shape_weights, a.out_p = out_positions, a.out_n = out_normals;
	a.indices = indices, a.list_count = list_count, a.max_list = max_list, a.compact = (flags & mbik::kSkinListCompact) != 0;
	return launch_on_mesh(m, hip_stream, max_list, a, mbik::launch_skin_listed, "listed skinning launch failed: "); // (a tile is S list entries)
}

int32_t mbik_skin_vertices_cpu(int32_t bone_count, int32_t vertex_count, int32_t influences, const float *positions,
		const float *normals, const int32_t *bone_indices, const float *weights, int32_t count, const float *skin,
		float *out_positions, float *out_normals) {
	if (int rc = check_mesh(bone_count, vertex_count, influences, positions, bone_indices, weights)) return rc;
	const int rc = check_call(bone_count, vertex_count, normals != nullptr, count, skin, out_positions, out_normals);
	if (rc) return rc < 0 ? rc : MBIK_OK;
	mbik::skin_vertices_host(bone_count, vertex_count, influences, positions, normals, bone_indices, weights, count, skin,
			out_positions, out_normals);
	return MBIK_OK;
}

int32_t mbik_skin_vertices_shaped_cpu(int32_t bone_count, int32_t vertex_count, int32_t influences, const float *positions,
		const float *normals, const int32_t *bone_indices, const float *weights, const mbik_mesh_shapes *shapes, int32_t count,
		const float *skin, const float *shape_weights, float *out_positions, float *out_normals) {
	if (int rc = check_mesh(bone_count, vertex_count, influences, positions, bone_indices, weights)) return rc;
	if (int rc = check_shapes(bone_count, vertex_count, normals != nullptr, shapes, -1)) return rc;
	const int rc = check_call(bone_count, vertex_count, normals != nullptr, count, skin, out_positions, out_normals);
	if (rc) return rc < 0 ? rc : MBIK_OK;
	if (int rw = check_shape_weights(vertex_count, shapes->shape_count, count, shape_weights, out_positions, out_normals)) return rw;
	mbik::morph_skin_vertices_host(bone_count, vertex_count, influences, positions, normals, bone_indices, weights, shapes->shape_count,
			shapes->mode, shapes->positions, shapes->normals, count, skin, shape_weights, out_positions, out_normals);
	return MBIK_OK;
}

int32_t mbik_skin_vertices_listed_cpu(int32_t bone_count, int32_t vertex_count, int32_t influences, const float *positions,
		const float *normals, const int32_t *bone_indices, const float *weights, const mbik_mesh_shapes *shapes, int32_t count,
		const int32_t *indices, const int32_t *list_count, int32_t max_list, const float *skin, const float *shape_weights,
		uint32_t flags, float *out_positions, float *out_normals) {
	if (int rc = check_mesh(bone_count, vertex_count, influences, positions, bone_indices, weights)) return rc;
	if (shapes)
		if (int rc = check_shapes(bone_count, vertex_count, normals != nullptr, shapes, -1)) return rc;
	const int32_t P = shapes ? shapes->shape_count : 0;
	const int rc = check_listed(bone_count, vertex_count, normals != nullptr, P, count, indices, list_count, max_list, skin,
			shape_weights, flags, out_positions, out_normals);
	if (rc) return rc < 0 ? rc : MBIK_OK;
	mbik::skin_vertices_listed_host(bone_count, vertex_count, influences, positions, normals, bone_indices, weights, P,
			shapes ? shapes->mode : 0, shapes ? shapes->positions : nullptr, shapes ? shapes->normals : nullptr, count, indices,
			list_count, max_list, skin, shape_weights, (flags & mbik::kSkinListCompact) != 0, out_positions, out_normals);
	return MBIK_OK;
}

} // extern "C"
