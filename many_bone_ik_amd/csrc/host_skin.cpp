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
// Every skinning entry is one call of skin_on_device or skin_on_host: the older entries build the mbik_skin_call (and the
// _cpu forms the mbik_mesh_desc) from their arguments and say which form they are.
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

// The shape checks mbik_mesh_create_shaped and mbik_skin_vertices_shaped_cpu share; lds_limit as morph_check's.
int check_shapes(int32_t B, int32_t V, bool mesh_normals, const mbik_mesh_shapes *sh, int64_t lds_limit) {
	if (int rc = check_given(sh, "shapes")) return rc;
	if (sh->struct_size < (int32_t)sizeof(mbik_mesh_shapes)) return fail(MBIK_EINVAL, "mbik_mesh_shapes.struct_size is too small");
	const mbik::MorphCheck c = mbik::morph_check(B, V, mesh_normals, sh->shape_count, sh->mode, sh->positions, sh->normals, lds_limit);
	if (c == mbik::MORPH_TOO_LARGE)
		return fail(MBIK_EUNSUPPORTED, "rig has " + std::to_string(B) + " bones and " + std::to_string(sh->shape_count) +
				" shapes: " + mbik::morph_check_text(c) + " (MBIK_MAX_LDS_BYTES)");
	if (c != mbik::MORPH_OK) return fail(MBIK_EINVAL, mbik::morph_check_text(c));
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

int check_desc_struct(const mbik_mesh_desc *d) {
	if (int rc = check_given(d, "desc")) return rc;
	if (d->struct_size < (int32_t)sizeof(mbik_mesh_desc)) return fail(MBIK_EINVAL, "mbik_mesh_desc.struct_size is too small");
	return MBIK_OK;
}

int check_call_struct(const mbik_skin_call *c) {
	if (int rc = check_given(c, "call")) return rc;
	if (c->struct_size < (int32_t)sizeof(mbik_skin_call)) return fail(MBIK_EINVAL, "mbik_skin_call.struct_size is too small");
	return MBIK_OK;
}

// The mesh arrays of the entries older than mbik_mesh_desc, as one.
mbik_mesh_desc desc_of(int32_t bone_count, int32_t vertex_count, int32_t influences, const float *positions, const float *normals,
		const int32_t *bone_indices, const float *weights, const mbik_mesh_shapes *shapes = nullptr) {
	return mbik_mesh_desc{(int32_t)sizeof(mbik_mesh_desc), bone_count, vertex_count, influences, positions, normals, nullptr, bone_indices,
			weights, shapes, nullptr};
}

// mbik_mesh_create, mbik_mesh_create_shaped (need_shapes: a mesh without is refused) and mbik_mesh_create_desc.  Without
// tangents the device image is what it always was.
int create_mesh(const mbik_mesh_desc &d, bool need_shapes, int32_t device, mbik_mesh **out_mesh) {
	if (!out_mesh) return fail(MBIK_EINVAL, "null out_mesh");
	*out_mesh = nullptr;
	const int32_t bone_count = d.bone_count, vertex_count = d.vertex_count, influences = d.influences;
	const bool shaped = need_shapes || d.shapes;
	if (influences != 4 && influences != 8) return fail(MBIK_EINVAL, mbik::skin_check_text(mbik::SKIN_BAD_INFLUENCES));
	if (bone_count < 0 || vertex_count < 0) return fail(MBIK_EINVAL, mbik::skin_check_text(mbik::SKIN_NEGATIVE));
	if (vertex_count > 0 && (!d.positions || !d.bone_indices || !d.weights)) return fail(MBIK_EINVAL, mbik::skin_check_text(mbik::SKIN_NULL));
	if (bone_count > mbik::kSkinMaxBones)
		return fail(MBIK_EUNSUPPORTED, "rig has " + std::to_string(bone_count) + " bones; a mesh supports at most " +
				std::to_string(mbik::kSkinMaxBones) + " (MBIK_SKIN_MAX_BONES: one skeleton's matrices must fit 160 KiB of LDS)");
	if (shaped)
		if (int rc = check_shapes(bone_count, vertex_count, d.normals != nullptr, d.shapes, mbik::kSkinMaxLdsBytes)) return rc;
	if (int rc = check_tangents(d.normals, d.tangents, shaped, d.shape_tangents)) return rc;
	if (int rc = check_mesh(bone_count, vertex_count, influences, d.positions, d.bone_indices, d.weights)) return rc;
	if (int rc = check_device(device)) return rc;
	std::unique_ptr<mbik_mesh> m(new mbik_mesh());
	m->device = device, m->B = bone_count, m->V = vertex_count, m->K = influences, m->normals = d.normals != nullptr;
	m->tangents = d.tangents != nullptr;
	if (shaped) m->P = d.shapes->shape_count, m->mode = d.shapes->mode;
	DeviceGuard guard(device);
	m->cu_count = cu_count_of(device);
	if (vertex_count > 0) {
		const mbik::SkinLayout l = mbik::skin_layout(vertex_count, influences, m->normals);
		int64_t bytes = shaped ? mbik::morph_layout(vertex_count, influences, m->normals, m->P).bytes : l.bytes;
		if (d.tangents) bytes = mbik::tangent_layout(vertex_count, influences, true, m->P, true).bytes;
		std::vector<unsigned char> packed((size_t)bytes);
		mbik::skin_pack(vertex_count, influences, d.positions, d.normals, d.bone_indices, d.weights, packed.data());
		if (shaped) mbik::morph_pack(vertex_count, influences, m->P, d.shapes->positions, d.shapes->normals, packed.data());
		if (d.tangents) mbik::tangent_pack(vertex_count, influences, m->P, d.tangents, d.shape_tangents, packed.data());
		if (int rc = m->mesh.upload(packed.data(), packed.size(), "the mesh")) return rc;
	}
	// the bone boxes (bounds.h): a table of their own, the used bones only
	m->bone_boxes.resize((size_t)bone_count * 6), m->bone_used.resize((size_t)bone_count);
	mbik::bone_boxes_build(bone_count, vertex_count, influences, d.positions, d.bone_indices, d.weights, m->bone_boxes.data(), m->bone_used.data());
	m->used_bones = mbik::bone_table_count(bone_count, m->bone_used.data());
	if (m->used_bones > 0) {
		std::vector<unsigned char> table((size_t)m->used_bones * mbik::kBoneRecordBytes);
		mbik::bone_table_pack(bone_count, m->bone_boxes.data(), m->bone_used.data(), table.data());
		if (int rc = m->bone_table.upload(table.data(), table.size(), "the mesh's bone boxes")) return rc;
	}
	*out_mesh = m.release();
	return MBIK_OK;
}

// ---- a skinning call ----
// What a call's checks need of the mesh: the handle's fields or the description's.
struct MeshFacts {
	int32_t B, V, P;
	bool normals, tangents;
};
// Which entry a call came through.  kByCall (mbik_skin_vertices_call): the call's pointers say whether it is listed or
// shaped.  The older entries are one form each; kShaped refuses a mesh without shapes and a missing shape_weights.
enum SkinForm { kByCall, kPlain, kShaped, kListed };

inline bool listed(SkinForm form, const mbik_skin_call &c) { return form == kListed || (form == kByCall && c.indices); }
inline bool compact(const mbik_skin_call &c) { return (c.flags & mbik::kSkinListCompact) != 0; }

// Every check of a skinning call past the mesh's and the structs' own, in the order the entries have always made them:
// 0 = run, kNothingToDo, or the refusal.
int check_skin_call(const MeshFacts &f, const mbik_skin_call &c, SkinForm form) {
	if (form == kByCall && (c.indices != nullptr) != (c.list_count != nullptr))
		return fail(MBIK_EINVAL, "indices and list_count must be given together");
	if (c.out_tangents && !f.tangents) return fail(MBIK_EINVAL, "out_tangents given for a mesh without tangents");
	if (c.out_tangents && !c.out_normals) return fail(MBIK_EINVAL, "out_tangents given without out_normals");
	const bool list = listed(form, c);
	if (list) {
		// (these two say "unknown flag bits" where check_flags says "unknown flags N", and the listed form has its own words
		// for a mesh without shapes: both texts are older than the helpers and stay)
		if (c.flags & ~mbik::kSkinListFlags) return fail(MBIK_EINVAL, "unknown flag bits");
		if (c.max_list < 0) return fail(MBIK_EINVAL, "negative max_list");
		if (c.shape_weights && f.P < 1) return fail(MBIK_EINVAL, "shape_weights given for a mesh without shapes");
	} else if ((c.shape_weights || form == kShaped) && f.P < 1) {
		return fail(MBIK_EINVAL, "the mesh has no shapes (mbik_mesh_create_shaped)");
	}
	if (int rc = check_count(c.count)) return rc;
	if (c.out_normals && !f.normals) return fail(MBIK_EINVAL, "out_normals given for a mesh without normals");
	if (c.count == 0 || f.V == 0 || (list && c.max_list == 0)) return kNothingToDo;
	if (int rc = check_given(c.skin, "skin")) return rc;
	if (int rc = check_given(c.out_positions, "out_positions")) return rc;
	// the outputs' rows: the listed call's compact form has one a list entry
	const size_t rows = list && compact(c) ? (size_t)c.max_list : (size_t)c.count, nout = rows * f.V * 3 * sizeof(float);
	const Range skin{c.skin, (size_t)c.count * f.B * 12 * sizeof(float), "skin"};
	const Range weights{c.shape_weights, (size_t)c.count * f.P * sizeof(float), "shape_weights"};
	const Range indices{list ? c.indices : nullptr, (size_t)c.max_list * sizeof(int32_t), "indices"};
	const Range list_count{list ? c.list_count : nullptr, sizeof(int32_t), "list_count"};
	const Range out_p{c.out_positions, nout, "out_positions"}, out_n{c.out_normals, nout, "out_normals"};
	if (int rc = check_disjoint({out_p, out_n}, {skin})) return rc;
	if (form == kShaped)
		if (int rc = check_given(c.shape_weights, "shape_weights")) return rc;
	if (int rc = check_disjoint({out_p, out_n}, {weights})) return rc;
	if (list) {
		if (int rc = check_given(c.indices, "indices")) return rc;
		if (int rc = check_given(c.list_count, "list_count")) return rc;
		if (int rc = check_disjoint({out_p, out_n}, {indices, list_count})) return rc;
	}
	return check_disjoint({Range{c.out_tangents, rows * f.V * 4 * sizeof(float), "out_tangents"}}, {skin, weights, indices, list_count, out_p, out_n});
}

// The device tail of every skinning entry: the checks, the launch shape for the call's tiles (skeletons, or list entries),
// what the mesh knows of the launch, the launch on the mesh's device.
int skin_on_device(const mbik_mesh *m, const mbik_skin_call &c, SkinForm form, void *hip_stream) {
	if (int rc = check_given(m, "mesh")) return rc;
	if (int rc = check_skin_call(MeshFacts{m->B, m->V, m->P, m->normals, m->tangents}, c, form)) return settled(rc);
	const bool list = listed(form, c);
	const SkinShape sh = shape_of(m, list ? c.max_list : c.count, c.shape_weights != nullptr);
	mbik::SkinLaunch a{};
	a.st = reinterpret_cast<hipStream_t>(hip_stream);
	a.K = m->K, a.mode = m->mode, a.B = m->B, a.V = m->V, a.P = m->P;
	a.S = sh.S, a.chunk = sh.chunk, a.chunks = sh.chunks, a.vshift = sh.vshift;
	a.mesh = m->mesh.as<unsigned char>(), a.mesh_normals = m->normals, a.mesh_tangents = m->tangents;
	a.count = c.count, a.skin = c.skin, a.shape_weights = c.shape_weights;
	a.out_p = c.out_positions, a.out_n = c.out_normals, a.out_t = c.out_tangents;
	if (list) a.indices = c.indices, a.list_count = c.list_count, a.max_list = c.max_list, a.compact = compact(c);
	return launched(m->device, list ? "listed skinning" : (c.shape_weights ? "shaped skinning" : "skinning"),
			[&] { return list ? mbik::launch_skin_listed(a) : mbik::launch_skin(a); });
}

// The host tail of every skinning entry: the description's checks (but the LDS limit: any bone and shape count), the
// call's, and the host loop of the call's form.
int skin_on_host(const mbik_mesh_desc &d, const mbik_skin_call &c, SkinForm form) {
	if (int rc = check_mesh(d.bone_count, d.vertex_count, d.influences, d.positions, d.bone_indices, d.weights)) return rc;
	if (d.shapes || form == kShaped)
		if (int rc = check_shapes(d.bone_count, d.vertex_count, d.normals != nullptr, d.shapes, -1)) return rc;
	if (int rc = check_tangents(d.normals, d.tangents, d.shapes != nullptr, d.shape_tangents)) return rc;
	const mbik_mesh_shapes none{};
	const mbik_mesh_shapes &sh = d.shapes ? *d.shapes : none;
	const int32_t P = sh.shape_count;
	if (int rc = check_skin_call(MeshFacts{d.bone_count, d.vertex_count, P, d.normals != nullptr, d.tangents != nullptr}, c, form))
		return settled(rc);
	const float *tan = c.out_tangents ? d.tangents : nullptr, *stan = c.out_tangents ? d.shape_tangents : nullptr;
	if (listed(form, c))
		mbik::skin_vertices_listed_host(d.bone_count, d.vertex_count, d.influences, d.positions, d.normals, d.bone_indices, d.weights, P,
				sh.mode, sh.positions, sh.normals, c.count, c.indices, c.list_count, c.max_list, c.skin, c.shape_weights, compact(c),
				c.out_positions, c.out_normals, tan, stan, c.out_tangents);
	else if (c.shape_weights)
		mbik::morph_skin_vertices_host(d.bone_count, d.vertex_count, d.influences, d.positions, d.normals, d.bone_indices, d.weights, P,
				sh.mode, sh.positions, sh.normals, c.count, c.skin, c.shape_weights, c.out_positions, c.out_normals, tan, stan, c.out_tangents);
	else
		mbik::skin_vertices_host(d.bone_count, d.vertex_count, d.influences, d.positions, d.normals, d.bone_indices, d.weights, c.count,
				c.skin, c.out_positions, c.out_normals, tan, c.out_tangents);
	return MBIK_OK;
}

// The older entries' arguments as the struct (max_list and flags: the listed form's).
mbik_skin_call call_of(int32_t count, const float *skin, const float *shape_weights, float *out_positions, float *out_normals,
		const int32_t *indices = nullptr, const int32_t *list_count = nullptr, int32_t max_list = 0, uint32_t flags = 0) {
	return mbik_skin_call{(int32_t)sizeof(mbik_skin_call), count, skin, shape_weights, indices, list_count, max_list, flags, out_positions,
			out_normals, nullptr};
}

} // namespace

extern "C" {

int32_t mbik_mesh_create_desc(const mbik_mesh_desc *d, int32_t device, mbik_mesh **out_mesh) {
	if (out_mesh) *out_mesh = nullptr;
	if (int rc = check_desc_struct(d)) return rc;
	return create_mesh(*d, false, device, out_mesh);
}

int32_t mbik_mesh_create(int32_t bone_count, int32_t vertex_count, int32_t influences, const float *positions, const float *normals,
		const int32_t *bone_indices, const float *weights, int32_t device, mbik_mesh **out_mesh) {
	return create_mesh(desc_of(bone_count, vertex_count, influences, positions, normals, bone_indices, weights), false, device, out_mesh);
}

int32_t mbik_mesh_create_shaped(int32_t bone_count, int32_t vertex_count, int32_t influences, const float *positions,
		const float *normals, const int32_t *bone_indices, const float *weights, const mbik_mesh_shapes *shapes, int32_t device,
		mbik_mesh **out_mesh) {
	return create_mesh(desc_of(bone_count, vertex_count, influences, positions, normals, bone_indices, weights, shapes), true, device, out_mesh);
}

void mbik_mesh_destroy(mbik_mesh *m) { delete m; }

int32_t mbik_mesh_launch_shape(const mbik_mesh *m, int32_t count, int32_t *skeletons_per_block, int32_t *vertex_chunks) {
	if (int rc = check_given(m, "mesh")) return rc;
	if (int rc = check_count(count)) return rc;
	const SkinShape sh = shape_of(m, count, m->P > 0);
	if (skeletons_per_block) *skeletons_per_block = sh.S;
	if (vertex_chunks) *vertex_chunks = sh.chunks;
	return MBIK_OK;
}

int32_t mbik_skin_vertices_call(mbik_mesh *m, const mbik_skin_call *c, void *hip_stream) {
	if (int rc = check_call_struct(c)) return rc;
	return skin_on_device(m, *c, kByCall, hip_stream);
}

int32_t mbik_skin_vertices_call_cpu(const mbik_mesh_desc *d, const mbik_skin_call *c) {
	if (int rc = check_desc_struct(d)) return rc;
	if (int rc = check_call_struct(c)) return rc;
	return skin_on_host(*d, *c, kByCall);
}

int32_t mbik_skin_vertices(mbik_mesh *m, int32_t count, const float *skin, float *out_positions, float *out_normals,
		void *hip_stream) {
	return skin_on_device(m, call_of(count, skin, nullptr, out_positions, out_normals), kPlain, hip_stream);
}

int32_t mbik_skin_vertices_shaped(mbik_mesh *m, int32_t count, const float *skin, const float *shape_weights, float *out_positions,
		float *out_normals, void *hip_stream) {
	return skin_on_device(m, call_of(count, skin, shape_weights, out_positions, out_normals), kShaped, hip_stream);
}

int32_t mbik_skin_vertices_listed(mbik_mesh *m, int32_t count, const int32_t *indices, const int32_t *list_count, int32_t max_list,
		const float *skin, const float *shape_weights, uint32_t flags, float *out_positions, float *out_normals, void *hip_stream) {
	return skin_on_device(m, call_of(count, skin, shape_weights, out_positions, out_normals, indices, list_count, max_list, flags), kListed,
			hip_stream);
}

int32_t mbik_skin_vertices_cpu(int32_t bone_count, int32_t vertex_count, int32_t influences, const float *positions,
		const float *normals, const int32_t *bone_indices, const float *weights, int32_t count, const float *skin,
		float *out_positions, float *out_normals) {
	return skin_on_host(desc_of(bone_count, vertex_count, influences, positions, normals, bone_indices, weights),
			call_of(count, skin, nullptr, out_positions, out_normals), kPlain);
}

int32_t mbik_skin_vertices_shaped_cpu(int32_t bone_count, int32_t vertex_count, int32_t influences, const float *positions,
		const float *normals, const int32_t *bone_indices, const float *weights, const mbik_mesh_shapes *shapes, int32_t count,
		const float *skin, const float *shape_weights, float *out_positions, float *out_normals) {
	return skin_on_host(desc_of(bone_count, vertex_count, influences, positions, normals, bone_indices, weights, shapes),
			call_of(count, skin, shape_weights, out_positions, out_normals), kShaped);
}

int32_t mbik_skin_vertices_listed_cpu(int32_t bone_count, int32_t vertex_count, int32_t influences, const float *positions,
		const float *normals, const int32_t *bone_indices, const float *weights, const mbik_mesh_shapes *shapes, int32_t count,
		const int32_t *indices, const int32_t *list_count, int32_t max_list, const float *skin, const float *shape_weights,
		uint32_t flags, float *out_positions, float *out_normals) {
	return skin_on_host(desc_of(bone_count, vertex_count, influences, positions, normals, bone_indices, weights, shapes),
			call_of(count, skin, shape_weights, out_positions, out_normals, indices, list_count, max_list, flags), kListed);
}

} // extern "C"
