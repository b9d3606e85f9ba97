// Animation clip sampling (include/mbik.h, ABI 12): the clip-set handle, mbik_clip_sample, which
// launches k_clip.hip's kernel on the set's device, and mbik_clip_sample_cpu, which runs the same
// per-bone code (clip.h) on the host.  The front stage of a frame: the poses mbik_solve reads are
// sampled on the solve's stream from a time and a clip index per skeleton.  DESIGN.md §16.
// mbik_clip_sample_layers and its _cpu form blend up to 8 (time, clip, weight) layers a skeleton
// the same way (k_clip.hip, clip_layers.h).  A set made by
// mbik_clipset_create_shaped carries blend-shape tracks as well: mbik_clip_sample_shapes and
// mbik_clip_sample_shapes_layers write the [count][P] weights the shaped skinning reads
// (k_clip_shapes.hip, clip_shapes.h).  mbik_clip_root_motion[_layers] extract the root
// bone's motion over the frame from the same tables and mbik_root_motion_apply composes it into
// skeleton_global (k_root_motion.hip, root_motion.h).
#include "host.h"

#include <cmath>
#include <cstddef>
#include <type_traits>

#include "clip_shapes.h"
#include "root_motion.h"

using namespace mbik_host;

struct mbik_clipset {
	int device = 0;
	int32_t B = 0, clip_count = 0, libm = 0;
	DevBuf blob;
	mbik::ClipView view{}; // device pointers into blob
	int32_t P = 0;         // 0: a set without shapes
	bool cubic_pose = false, cubic_shapes = false; // a pose / shape header carries kClipCubic: the kernels' CUBIC forms
	DevBuf shape_blob;
	mbik::ShapeView shapes{}; // device pointers into shape_blob
};

namespace {

// A key track's checks past the place it names (bone and channel, or shape), and its header: what the pose tracks and the
// shape tracks share.  0: `h` is filled and the caller appends the key_count keys at key_total; kNothingToDo: a track without
// keys, the same as no track; < 0: a refusal.  `values` is tested for null only; duplicate() is the text behind `tw` for a
// header that already has keys.  allow_cubic: interpolation 2 is taken (mbik_clipset_create_desc, mbik_clip_call_cpu).
template <class Header, class Duplicate>
int pack_track(bool allow_cubic, int32_t interpolation, int32_t loop_wrap, int32_t key_count, const double *times, const void *values, const mbik_clip_desc &d,
		const std::string &tw, size_t key_total, const char *too_many_keys, Header &h, Duplicate duplicate) {
	if (interpolation != 0 && interpolation != 1 && !(allow_cubic && interpolation == 2)) return fail(MBIK_EINVAL, tw + ": unknown interpolation " + std::to_string(interpolation));
	if (key_count < 0) return fail(MBIK_EINVAL, tw + ": negative key_count");
	if (key_count == 0) return kNothingToDo;
	if (!times || !values) return fail(MBIK_EINVAL, tw + ": null times or values");
	if (h.key_count) return fail(MBIK_EINVAL, tw + duplicate());
	if (key_total + (size_t)key_count > (size_t)INT32_MAX) return fail(MBIK_EUNSUPPORTED, too_many_keys);
	for (int32_t i = 0; i < key_count; i++) {
		const double x = times[i];
		if (!std::isfinite(x) || !(x >= 0) || !(x <= d.length))
			return fail(MBIK_EINVAL, tw + ": key " + std::to_string(i) + " has a time that is not finite or outside [0, length]");
		if (i > 0 && !(x > times[i - 1])) return fail(MBIK_EINVAL, tw + ": key times are not strictly increasing at key " + std::to_string(i));
	}
	h.key_off = (int32_t)key_total, h.key_count = key_count;
	h.flags = (interpolation == 1 ? mbik::kClipLinear : 0) | (interpolation == 2 ? mbik::kClipCubic : 0) | (d.loop_mode == 1 && loop_wrap ? mbik::kClipWrap : 0);
	return 0;
}

// A clip set on the host, repacked (clip.h, clip_shapes.h) and checked: everything the per-bone and per-shape code indexes
// without a test.  The _cpu entries read their views from it; create_set uploads it.
struct PackedSet {
	int32_t B = 0;
	std::vector<mbik::ClipInfo> clips;
	std::vector<mbik::ClipHeader> headers;
	std::vector<double> times;
	std::vector<mbik::ClipValue> values;
	std::vector<float> rest;
	// with shapes:
	std::vector<mbik::ShapeHeader> shape_headers;
	std::vector<mbik::ShapeKey> keys;
	std::vector<float> init;
	bool cubic_pose = false, cubic_shapes = false; // a pose / shape track with keys is cubic
	int32_t libm = 0;

	// The pose tracks, then with `shaped` the shape tracks: mbik_clipset_create[_shaped]'s refusals in their order.
	// allow_cubic: the entries that take a mbik_clipset_desc.
	int pack(int32_t bone_count, const float *rest_pose, int32_t clip_count, const mbik_clip_desc *descs, int32_t libm_variant, bool shaped,
			const mbik_clipset_shapes *sh, bool allow_cubic = false) {
		cubic = allow_cubic;
		if (int rc = pack_pose(bone_count, rest_pose, clip_count, descs, libm_variant)) return rc;
		libm = libm_variant;
		return shaped ? pack_shapes(descs, sh) : MBIK_OK;
	}
	mbik::ClipView view() const {
		return mbik::ClipView{B, (int32_t)clips.size(), clips.data(), headers.data(), times.data(), values.data(), rest.data()};
	}
	mbik::ShapeView shape_view() const {
		return mbik::ShapeView{(int32_t)init.size(), (int32_t)clips.size(), clips.data(), shape_headers.data(), keys.data(), init.data()};
	}

private:
	bool cubic = false; // pack()'s allow_cubic

	int pack_pose(int32_t bone_count, const float *rest_pose, int32_t clip_count, const mbik_clip_desc *descs, int32_t libm_variant) {
		if (bone_count < 0 || clip_count < 0) return fail(MBIK_EINVAL, "negative count");
		if (!rest_pose) return fail(MBIK_EINVAL, "null rest_pose");
		if (clip_count == 0) return fail(MBIK_EINVAL, "a clip set needs at least one clip");
		if (!descs) return fail(MBIK_EINVAL, "null clips");
		if (libm_variant != MBIK_LIBM_VARIANT_FMA && libm_variant != MBIK_LIBM_VARIANT_SSE2) return fail(MBIK_EINVAL, "unknown libm_variant");
		if ((int64_t)clip_count * bone_count * 3 > INT32_MAX) return fail(MBIK_EUNSUPPORTED, "more than 2^31 (clip, bone, channel) headers");
		B = bone_count;
		clips.resize(clip_count);
		headers.assign((size_t)clip_count * B * 3, mbik::ClipHeader{0, 0, 0, 0});
		rest.assign(rest_pose, rest_pose + (size_t)B * 10);
		for (int32_t c = 0; c < clip_count; c++) {
			const mbik_clip_desc &d = descs[c];
			const std::string where = "clip " + std::to_string(c);
			if (int rc = check_clip(d, where)) return rc;
			if (d.track_count < 0) return fail(MBIK_EINVAL, where + ": negative track_count");
			if (d.track_count > 0 && !d.tracks) return fail(MBIK_EINVAL, where + ": null tracks");
			clips[c] = mbik::ClipInfo{d.length, d.loop_mode, 0};
			for (int32_t k = 0; k < d.track_count; k++) {
				const mbik_clip_track &t = d.tracks[k];
				const std::string tw = where + " track " + std::to_string(k);
				if (t.bone < 0 || t.bone >= B) return fail(MBIK_EINVAL, tw + ": bone " + std::to_string(t.bone) + " outside [0, " + std::to_string(B) + ")");
				if (t.channel < 0 || t.channel > 2) return fail(MBIK_EINVAL, tw + ": unknown channel " + std::to_string(t.channel));
				const int rc = pack_track(cubic, t.interpolation, t.loop_wrap, t.key_count, t.times, t.values, d, tw, times.size(),
						"more than 2^31 keys in a clip set", headers[((size_t)c * B + t.bone) * 3 + t.channel], [&] {
							return ": a second track with keys for bone " + std::to_string(t.bone) + " channel " + std::to_string(t.channel);
						});
				if (rc < 0) return rc;
				if (rc == kNothingToDo) continue;
				cubic_pose = cubic_pose || t.interpolation == 2;
				const int w = t.channel == 1 ? 4 : 3;
				for (int32_t i = 0; i < t.key_count; i++) {
					const float *v = t.values + (size_t)i * w;
					times.push_back(t.times[i]);
					values.push_back(mbik::ClipValue{v[0], v[1], v[2], w == 4 ? v[3] : 0.0f});
				}
			}
		}
		// the spare entry that makes index key_off + 0 valid for every header (clip.h)
		times.push_back(0.0);
		values.push_back(mbik::ClipValue{0.0f, 0.0f, 0.0f, 0.0f});
		return MBIK_OK;
	}

	// `descs` has passed pack_pose().
	int pack_shapes(const mbik_clip_desc *descs, const mbik_clipset_shapes *sh) {
		if (!sh) return fail(MBIK_EINVAL, "null shapes");
		if (sh->struct_size < (int32_t)sizeof(mbik_clipset_shapes)) return fail(MBIK_EINVAL, "shapes->struct_size is smaller than mbik_clipset_shapes");
		const int32_t P = sh->shape_count, clip_count = (int32_t)clips.size();
		if (P < 1) return fail(MBIK_EINVAL, "shape_count must be at least 1");
		if (!sh->clips) return fail(MBIK_EINVAL, "null shapes->clips");
		if ((int64_t)clip_count * P > INT32_MAX) return fail(MBIK_EUNSUPPORTED, "more than 2^31 (clip, shape) headers");
		shape_headers.assign((size_t)clip_count * P, mbik::ShapeHeader{0, 0, 0, 0});
		if (sh->init) init.assign(sh->init, sh->init + P);
		else init.assign((size_t)P, 0.0f);
		for (int32_t c = 0; c < clip_count; c++) {
			const mbik_clip_shape_tracks &st = sh->clips[c];
			const std::string where = "clip " + std::to_string(c);
			if (st.track_count < 0) return fail(MBIK_EINVAL, where + ": negative shape track_count");
			if (st.track_count > 0 && !st.tracks) return fail(MBIK_EINVAL, where + ": null shape tracks");
			for (int32_t k = 0; k < st.track_count; k++) {
				const mbik_shape_track &t = st.tracks[k];
				const std::string tw = where + " shape track " + std::to_string(k);
				if (t.shape < 0 || t.shape >= P) return fail(MBIK_EINVAL, tw + ": shape " + std::to_string(t.shape) + " outside [0, " + std::to_string(P) + ")");
				const int rc = pack_track(cubic, t.interpolation, t.loop_wrap, t.key_count, t.times, t.values, descs[c], tw, keys.size(),
						"more than 2^31 shape keys in a clip set", shape_headers[(size_t)c * P + t.shape],
						[&] { return ": a second track with keys for shape " + std::to_string(t.shape); });
				if (rc < 0) return rc;
				if (rc == kNothingToDo) continue;
				cubic_shapes = cubic_shapes || t.interpolation == 2;
				for (int32_t i = 0; i < t.key_count; i++) keys.push_back(mbik::ShapeKey{t.times[i], t.values[i], 0.0f});
			}
		}
		// the spare record that makes index key_off + 0 valid for every header (clip_shapes.h)
		keys.push_back(mbik::ShapeKey{0.0, 0.0f, 0.0f});
		return MBIK_OK;
	}
};

int check_clip_index(const int32_t *clip_index, int32_t clip, int32_t clip_count) {
	if (!clip_index && (clip < 0 || clip >= clip_count))
		return fail(MBIK_EINVAL, "clip " + std::to_string(clip) + " outside the set's " + std::to_string(clip_count) + " clips");
	return MBIK_OK;
}

int check_root_bone(int32_t root_bone, int32_t B) {
	if (root_bone < 0 || root_bone >= B) return fail(MBIK_EINVAL, "root_bone " + std::to_string(root_bone) + " outside [0, " + std::to_string(B) + ")");
	return MBIK_OK;
}

// One launch's items (bones, weights) against the 2^31 blocks of 256 a grid can have.
int check_total(int64_t count, int64_t per, const char *items) {
	if (count * per > (int64_t)INT32_MAX * 256) return fail(MBIK_EUNSUPPORTED, std::string("more than 2^39 ") + items + " in one call");
	return MBIK_OK;
}

// The checks of mbik_clip_sample past the set's own.
int check_sample(int32_t B, int32_t clip_count, int32_t count, const double *time, const int32_t *clip_index, int32_t clip,
		const float *pose_out) {
	if (int rc = check_count(count)) return rc;
	if (count == 0 || B == 0) return kNothingToDo;
	if (int rc = check_given(time, "time")) return rc;
	if (int rc = check_given(pose_out, "pose_out")) return rc;
	// (no overlap test here: mbik.h promises none for pose_out of the plain form)
	return check_clip_index(clip_index, clip, clip_count);
}

// The checks of mbik_clip_sample_shapes.
int check_sample_shapes(int32_t P, int32_t clip_count, int32_t count, const double *time, const int32_t *clip_index, int32_t clip,
		const float *weights_out) {
	if (int rc = check_count(count)) return rc;
	// (a set with shapes has P >= 1: no second way out, as check_sample has for a set without bones)
	if (count == 0) return kNothingToDo;
	if (int rc = check_given(time, "time")) return rc;
	if (int rc = check_given(weights_out, "weights_out")) return rc;
	if (int rc = check_clip_index(clip_index, clip, clip_count)) return rc;
	const size_t bytes = (size_t)count * P * sizeof(float);
	if (int rc = check_apart(time, (size_t)count * sizeof(double), "time", weights_out, bytes, "weights_out")) return rc;
	return clip_index ? check_apart(clip_index, (size_t)count * sizeof(int32_t), "clip_index", weights_out, bytes, "weights_out") : MBIK_OK;
}

// The checks of the two layered sampling calls, which write `per` floats a skeleton to `out` (poses: B * 10, and a set
// without bones has nothing to do; weights: P >= 1); the records themselves are the kernel's (or the per-item code's) to test.
int check_sample_layers(int64_t per, int32_t count, int32_t layer_count, const mbik_clip_layer *layers, uint32_t flags, const float *out,
		const char *out_name) {
	if (int rc = check_count(count)) return rc;
	if (int rc = check_layer_count(layer_count)) return rc;
	if (int rc = check_flags(flags, MBIK_CLIP_LAYERS_NORMALIZE)) return rc;
	if (count == 0 || per == 0) return kNothingToDo;
	if (int rc = check_given(layers, "layers")) return rc;
	if (int rc = check_given(out, out_name)) return rc;
	if (int rc = check_aligned8(layers, "layers")) return rc;
	return check_apart(layers, (size_t)count * layer_count * sizeof(mbik_clip_layer), "layers", out, (size_t)count * per * sizeof(float), out_name);
}
static_assert(sizeof(mbik_clip_layer) == sizeof(mbik::ClipLayer) && offsetof(mbik_clip_layer, clip) == offsetof(mbik::ClipLayer, clip) &&
				offsetof(mbik_clip_layer, weight) == offsetof(mbik::ClipLayer, weight),
		"mbik_clip_layer is clip_layers.h's ClipLayer");

// The checks of mbik_clip_root_motion.  (Unlike the sampling calls, both root-motion forms test every scalar, the clip
// included, before count == 0 lets them return.)
int check_root_motion(int32_t B, int32_t clip_count, int32_t count, int32_t root_bone, const double *time_prev, const double *time,
		const int32_t *clip_index, int32_t clip, const float *motion_out, const float *pose) {
	if (int rc = check_count(count)) return rc;
	if (int rc = check_root_bone(root_bone, B)) return rc;
	if (int rc = check_clip_index(clip_index, clip, clip_count)) return rc;
	if (count == 0) return kNothingToDo;
	if (int rc = check_given(time, "time")) return rc;
	if (int rc = check_given(time_prev, "time_prev")) return rc;
	if (int rc = check_given(motion_out, "motion_out")) return rc;
	if (int rc = check_aligned8(time, "time")) return rc;
	if (int rc = check_aligned8(time_prev, "time_prev")) return rc;
	const size_t times = (size_t)count * sizeof(double), out = (size_t)count * 10 * sizeof(float);
	if (int rc = check_apart(time, times, "time", motion_out, out, "motion_out")) return rc;
	if (int rc = check_apart(time_prev, times, "time_prev", motion_out, out, "motion_out")) return rc;
	if (clip_index)
		if (int rc = check_apart(clip_index, (size_t)count * sizeof(int32_t), "clip_index", motion_out, out, "motion_out")) return rc;
	return pose ? check_apart(pose, (size_t)count * B * 10 * sizeof(float), "pose", motion_out, out, "motion_out") : MBIK_OK;
}

// The checks of mbik_clip_root_motion_layers.
int check_root_motion_layers(int32_t B, int32_t count, int32_t layer_count, int32_t root_bone, const mbik_clip_layer *layers,
		const double *time_prev, uint32_t flags, const float *motion_out, const float *pose) {
	if (int rc = check_count(count)) return rc;
	if (int rc = check_root_bone(root_bone, B)) return rc;
	if (int rc = check_layer_count(layer_count)) return rc;
	if (int rc = check_flags(flags, MBIK_CLIP_LAYERS_NORMALIZE)) return rc;
	if (count == 0) return kNothingToDo;
	if (int rc = check_given(layers, "layers")) return rc;
	if (int rc = check_given(time_prev, "time_prev")) return rc;
	if (int rc = check_given(motion_out, "motion_out")) return rc;
	if (int rc = check_aligned8(layers, "layers")) return rc;
	if (int rc = check_aligned8(time_prev, "time_prev")) return rc;
	const size_t per = (size_t)count * layer_count, out = (size_t)count * 10 * sizeof(float);
	if (int rc = check_apart(layers, per * sizeof(mbik_clip_layer), "layers", motion_out, out, "motion_out")) return rc;
	if (int rc = check_apart(time_prev, per * sizeof(double), "time_prev", motion_out, out, "motion_out")) return rc;
	return pose ? check_apart(pose, (size_t)count * B * 10 * sizeof(float), "pose", motion_out, out, "motion_out") : MBIK_OK;
}

int check_root_apply(int32_t count, const float *motion, uint32_t flags, const float *skeleton_global) {
	if (int rc = check_count(count)) return rc;
	if (int rc = check_flags(flags, MBIK_ROOT_MOTION_ORTHONORMALIZE)) return rc;
	if (count == 0) return kNothingToDo;
	if (int rc = check_given(motion, "motion")) return rc;
	if (int rc = check_given(skeleton_global, "skeleton_global")) return rc;
	return check_apart(motion, (size_t)count * 10 * sizeof(float), "motion", skeleton_global, (size_t)count * 12 * sizeof(float), "skeleton_global");
}
static_assert(MBIK_ROOT_MOTION_ORTHONORMALIZE == mbik::kRootMotionOrthonormalize, "the flag is root_motion.h's");

const mbik::ClipLayer *records(const mbik_clip_layer *layers) { return reinterpret_cast<const mbik::ClipLayer *>(layers); }

// The per-item code's CUBIC form for a set that has a cubic track, its plain form otherwise: f(std::bool_constant<CUBIC>).
template <class F>
void with_cubic(bool cubic, F f) {
	if (cubic) f(std::true_type{});
	else f(std::false_type{});
}

// The host forms' loops over a packed and checked set: one item after the other through the code the kernels run.
void sample_host(const PackedSet &pk, int32_t count, const double *time, const int32_t *clip_index, int32_t clip, float *pose_out) {
	const mbik::ClipView v = pk.view();
	with_cubic(pk.cubic_pose, [&](auto cubic) {
		for (int64_t s = 0; s < count; s++) {
			const int32_t c = clip_index ? clip_index[s] : clip;
			for (int32_t b = 0; b < v.B; b++) mbik::clip_sample_bone<decltype(cubic)::value>(v, c, b, time[s], pk.libm, pose_out + (s * v.B + b) * 10);
		}
	});
}

void sample_layers_host(const PackedSet &pk, int32_t count, int32_t K, const mbik_clip_layer *layers, uint32_t flags, float *pose_out) {
	const mbik::ClipView v = pk.view();
	with_cubic(pk.cubic_pose, [&](auto cubic) {
		for (int64_t s = 0; s < count; s++)
			for (int32_t b = 0; b < v.B; b++)
				mbik::clip_layers_bone<decltype(cubic)::value>(v, records(layers) + s * K, K, flags, b, pk.libm, pose_out + (s * v.B + b) * 10);
	});
}

void sample_shapes_host(const PackedSet &pk, int32_t count, const double *time, const int32_t *clip_index, int32_t clip, float *weights_out) {
	const mbik::ShapeView v = pk.shape_view();
	with_cubic(pk.cubic_shapes, [&](auto cubic) {
		for (int64_t s = 0; s < count; s++)
			for (int32_t j = 0; j < v.P; j++)
				weights_out[s * v.P + j] = mbik::shape_sample<decltype(cubic)::value>(v, clip_index ? clip_index[s] : clip, j, time[s]);
	});
}

void sample_shapes_layers_host(const PackedSet &pk, int32_t count, int32_t K, const mbik_clip_layer *layers, uint32_t flags,
		float *weights_out) {
	const mbik::ShapeView v = pk.shape_view();
	with_cubic(pk.cubic_shapes, [&](auto cubic) {
		for (int64_t s = 0; s < count; s++)
			for (int32_t j = 0; j < v.P; j++)
				weights_out[s * v.P + j] = mbik::shape_layers<decltype(cubic)::value>(v, records(layers) + s * K, K, flags, j);
	});
}

// The host form of both extraction calls: one skeleton after the other through root_motion.h.
void root_motion_host(const PackedSet &pk, int32_t count, int32_t K, int32_t root, const mbik::ClipLayer *L, const double *time_prev,
		const double *time, const int32_t *clip_index, int32_t clip, uint32_t flags, float *motion_out, float *pose) {
	const mbik::ClipView v = pk.view();
	with_cubic(pk.cubic_pose, [&](auto cubic) {
		constexpr bool CUBIC = decltype(cubic)::value;
		for (int64_t s = 0; s < count; s++) {
			float *pose_s = pose ? pose + s * v.B * 10 : nullptr;
			if (L) {
				mbik::root_motion_skeleton<CUBIC>(v, mbik::RootLayers{L + s * K, time_prev + s * K}, K, flags, root, pk.libm, motion_out + s * 10,
						pose_s);
			} else {
				const mbik::RootPlain src{mbik::ClipLayer{time[s], clip_index ? clip_index[s] : clip, 1.0f}, time_prev[s]};
				mbik::root_motion_skeleton<CUBIC>(v, src, 1, 0u, root, pk.libm, motion_out + s * 10, pose_s);
			}
		}
	});
}

// The struct checks of the entries that take a mbik_clipset_desc or a mbik_clip_call.
int check_set_desc(const mbik_clipset_desc *d) {
	if (!d) return fail(MBIK_EINVAL, "null mbik_clipset_desc");
	if (d->struct_size < (int32_t)sizeof(mbik_clipset_desc)) return fail(MBIK_EINVAL, "mbik_clipset_desc.struct_size is too small");
	if (d->flags != 0) return fail(MBIK_EINVAL, "mbik_clipset_desc.flags must be 0");
	return MBIK_OK;
}
int check_call_struct(const mbik_clip_call *c) {
	if (!c) return fail(MBIK_EINVAL, "null mbik_clip_call");
	if (c->struct_size < (int32_t)sizeof(mbik_clip_call)) return fail(MBIK_EINVAL, "mbik_clip_call.struct_size is too small");
	if (c->kind < MBIK_CLIP_CALL_SAMPLE || c->kind > MBIK_CLIP_CALL_ROOT_MOTION_LAYERS)
		return fail(MBIK_EINVAL, "unknown mbik_clip_call.kind " + std::to_string(c->kind));
	return MBIK_OK;
}

// mbik_clipset_create, with `shaped` mbik_clipset_create_shaped, and with allow_cubic mbik_clipset_create_desc.
int create_set(int32_t bone_count, const float *rest_pose, int32_t clip_count, const mbik_clip_desc *clips, bool shaped,
		const mbik_clipset_shapes *shapes, int32_t libm_variant, int32_t device, mbik_clipset **out, bool allow_cubic = false) {
	if (!out) return fail(MBIK_EINVAL, "null out");
	*out = nullptr;
	PackedSet pk;
	if (int rc = pk.pack(bone_count, rest_pose, clip_count, clips, libm_variant, shaped, shapes, allow_cubic)) return rc;
	if (int rc = check_device(device)) return rc;
	std::unique_ptr<mbik_clipset> s(new mbik_clipset());
	s->device = device, s->B = bone_count, s->clip_count = clip_count, s->libm = libm_variant;
	s->cubic_pose = pk.cubic_pose, s->cubic_shapes = pk.cubic_shapes;
	DeviceGuard guard(device);
	Blob b;
	const size_t o_info = b.add(pk.clips), o_head = b.add(pk.headers), o_time = b.add(pk.times), o_val = b.add(pk.values), o_rest = b.add(pk.rest);
	if (int rc = b.upload(s->blob, "the clip set")) return rc;
	s->view = mbik::ClipView{bone_count, clip_count, b.at<mbik::ClipInfo>(o_info), b.at<mbik::ClipHeader>(o_head), b.at<double>(o_time),
			b.at<mbik::ClipValue>(o_val), b.at<float>(o_rest)};
	if (shaped) {
		// a blob of its own, with its own copy of the clip infos
		Blob sb;
		const size_t p_info = sb.add(pk.clips), p_head = sb.add(pk.shape_headers), p_key = sb.add(pk.keys), p_init = sb.add(pk.init);
		if (int rc = sb.upload(s->shape_blob, "the clip set's shape tracks")) return rc;
		s->P = (int32_t)pk.init.size();
		s->shapes = mbik::ShapeView{s->P, clip_count, sb.at<mbik::ClipInfo>(p_info), sb.at<mbik::ShapeHeader>(p_head), sb.at<mbik::ShapeKey>(p_key),
				sb.at<float>(p_init)};
	}
	*out = s.release();
	return MBIK_OK;
}

// A device entry's set: the handle given and, for the shape calls, made with shapes.
int check_set(const mbik_clipset *s, bool shapes = false) {
	if (!s) return fail(MBIK_EINVAL, "null clip set");
	if (shapes && !s->P) return fail(MBIK_EINVAL, "the clip set has no shapes (mbik_clipset_create_shaped)");
	return MBIK_OK;
}

hipStream_t stream_of(void *hip_stream) { return reinterpret_cast<hipStream_t>(hip_stream); }

} // namespace

int mbik_host::check_layer_count(int32_t layer_count) {
	if (layer_count < 1 || layer_count > MBIK_CLIP_MAX_LAYERS)
		return fail(MBIK_EINVAL, "layer_count " + std::to_string(layer_count) + " outside [1, " + std::to_string(MBIK_CLIP_MAX_LAYERS) + "]");
	return MBIK_OK;
}

int mbik_host::check_clip(const mbik_clip_desc &d, const std::string &where) {
	if (!(d.length > 0) || !std::isfinite(d.length)) return fail(MBIK_EINVAL, where + ": length must be positive and finite");
	if (d.loop_mode != 0 && d.loop_mode != 1) return fail(MBIK_EINVAL, where + ": unknown loop_mode " + std::to_string(d.loop_mode));
	return MBIK_OK;
}

int mbik_host::clipset_clips(const mbik_clipset *set, int &device, std::vector<mbik::ClipInfo> &clips) {
	device = set->device;
	clips.resize((size_t)set->clip_count);
	DeviceGuard guard(set->device);
	if (hipMemcpy(clips.data(), set->view.clips, clips.size() * sizeof(mbik::ClipInfo), hipMemcpyDeviceToHost) != hipSuccess)
		return fail(MBIK_EHIP, "hipMemcpy failed for the clip set's clip table");
	return MBIK_OK;
}

extern "C" {

int32_t mbik_clipset_create(int32_t bone_count, const float *rest_pose, int32_t clip_count, const mbik_clip_desc *clips,
		int32_t libm_variant, int32_t device, mbik_clipset **out) {
	return create_set(bone_count, rest_pose, clip_count, clips, false, nullptr, libm_variant, device, out);
}

int32_t mbik_clipset_create_shaped(int32_t bone_count, const float *rest_pose, int32_t clip_count, const mbik_clip_desc *clips,
		const mbik_clipset_shapes *shapes, int32_t libm_variant, int32_t device, mbik_clipset **out) {
	return create_set(bone_count, rest_pose, clip_count, clips, true, shapes, libm_variant, device, out);
}

int32_t mbik_clipset_create_desc(const mbik_clipset_desc *d, int32_t device, mbik_clipset **out) {
	if (out) *out = nullptr;
	if (int rc = check_set_desc(d)) return rc;
	return create_set(d->bone_count, d->rest_pose, d->clip_count, d->clips, d->shapes != nullptr, d->shapes, d->libm_variant, device, out, true);
}

void mbik_clipset_destroy(mbik_clipset *s) { delete s; }

int32_t mbik_clip_sample(mbik_clipset *s, int32_t count, const double *time, const int32_t *clip_index, int32_t clip, float *pose_out,
		void *hip_stream) {
	if (int rc = check_set(s)) return rc;
	if (int rc = check_sample(s->B, s->clip_count, count, time, clip_index, clip, pose_out)) return settled(rc);
	if (int rc = check_total(count, s->B, "bones")) return rc;
	return launched(s->device, "clip sample",
			[&] { return mbik::launch_clip(stream_of(hip_stream), s->view, s->libm, s->cubic_pose, (int64_t)count * s->B, time, clip_index, clip, pose_out); });
}

int32_t mbik_clip_sample_cpu(int32_t bone_count, const float *rest_pose, int32_t clip_count, const mbik_clip_desc *clips,
		int32_t libm_variant, int32_t count, const double *time, const int32_t *clip_index, int32_t clip, float *pose_out) {
	PackedSet pk;
	if (int rc = pk.pack(bone_count, rest_pose, clip_count, clips, libm_variant, false, nullptr)) return rc;
	if (int rc = check_sample(bone_count, clip_count, count, time, clip_index, clip, pose_out)) return settled(rc);
	sample_host(pk, count, time, clip_index, clip, pose_out);
	return MBIK_OK;
}

int32_t mbik_clip_sample_layers(mbik_clipset *s, int32_t count, int32_t layer_count, const mbik_clip_layer *layers, uint32_t flags,
		float *pose_out, void *hip_stream) {
	if (int rc = check_set(s)) return rc;
	if (int rc = check_sample_layers((int64_t)s->B * 10, count, layer_count, layers, flags, pose_out, "pose_out")) return settled(rc);
	if (int rc = check_total(count, s->B, "bones")) return rc;
	return launched(s->device, "layered clip sample", [&] {
		return mbik::launch_clip_layers(stream_of(hip_stream), s->view, s->libm, s->cubic_pose, (int64_t)count * s->B, records(layers), layer_count, flags, pose_out);
	});
}

int32_t mbik_clip_sample_layers_cpu(int32_t bone_count, const float *rest_pose, int32_t clip_count, const mbik_clip_desc *clips,
		int32_t libm_variant, int32_t count, int32_t layer_count, const mbik_clip_layer *layers, uint32_t flags, float *pose_out) {
	PackedSet pk;
	if (int rc = pk.pack(bone_count, rest_pose, clip_count, clips, libm_variant, false, nullptr)) return rc;
	if (int rc = check_sample_layers((int64_t)bone_count * 10, count, layer_count, layers, flags, pose_out, "pose_out")) return settled(rc);
	sample_layers_host(pk, count, layer_count, layers, flags, pose_out);
	return MBIK_OK;
}

int32_t mbik_clip_sample_shapes(mbik_clipset *s, int32_t count, const double *time, const int32_t *clip_index, int32_t clip,
		float *weights_out, void *hip_stream) {
	if (int rc = check_set(s, true)) return rc;
	if (int rc = check_sample_shapes(s->P, s->clip_count, count, time, clip_index, clip, weights_out)) return settled(rc);
	if (int rc = check_total(count, s->P, "weights")) return rc;
	return launched(s->device, "shape sample", [&] {
		return mbik::launch_clip_shapes(stream_of(hip_stream), s->shapes, s->cubic_shapes, (int64_t)count * s->P, time, clip_index, clip, weights_out);
	});
}

int32_t mbik_clip_sample_shapes_layers(mbik_clipset *s, int32_t count, int32_t layer_count, const mbik_clip_layer *layers, uint32_t flags,
		float *weights_out, void *hip_stream) {
	if (int rc = check_set(s, true)) return rc;
	if (int rc = check_sample_layers(s->P, count, layer_count, layers, flags, weights_out, "weights_out")) return settled(rc);
	if (int rc = check_total(count, s->P, "weights")) return rc;
	return launched(s->device, "layered shape sample", [&] {
		return mbik::launch_clip_shapes_layers(stream_of(hip_stream), s->shapes, s->cubic_shapes, (int64_t)count * s->P, records(layers), layer_count, flags,
				weights_out);
	});
}

int32_t mbik_clip_sample_shapes_cpu(int32_t bone_count, const float *rest_pose, int32_t clip_count, const mbik_clip_desc *clips,
		const mbik_clipset_shapes *shapes, int32_t libm_variant, int32_t count, const double *time, const int32_t *clip_index, int32_t clip,
		float *weights_out) {
	PackedSet pk;
	if (int rc = pk.pack(bone_count, rest_pose, clip_count, clips, libm_variant, true, shapes)) return rc;
	if (int rc = check_sample_shapes((int32_t)pk.init.size(), clip_count, count, time, clip_index, clip, weights_out)) return settled(rc);
	sample_shapes_host(pk, count, time, clip_index, clip, weights_out);
	return MBIK_OK;
}

int32_t mbik_clip_sample_shapes_layers_cpu(int32_t bone_count, const float *rest_pose, int32_t clip_count, const mbik_clip_desc *clips,
		const mbik_clipset_shapes *shapes, int32_t libm_variant, int32_t count, int32_t layer_count, const mbik_clip_layer *layers,
		uint32_t flags, float *weights_out) {
	PackedSet pk;
	if (int rc = pk.pack(bone_count, rest_pose, clip_count, clips, libm_variant, true, shapes)) return rc;
	if (int rc = check_sample_layers((int64_t)pk.init.size(), count, layer_count, layers, flags, weights_out, "weights_out")) return settled(rc);
	sample_shapes_layers_host(pk, count, layer_count, layers, flags, weights_out);
	return MBIK_OK;
}

int32_t mbik_clip_root_motion(mbik_clipset *s, int32_t count, int32_t root_bone, const double *time_prev, const double *time,
		const int32_t *clip_index, int32_t clip, float *motion_out, float *pose, void *hip_stream) {
	if (int rc = check_set(s)) return rc;
	if (int rc = check_root_motion(s->B, s->clip_count, count, root_bone, time_prev, time, clip_index, clip, motion_out, pose)) return settled(rc);
	return launched(s->device, "root motion", [&] {
		return mbik::launch_root_motion(stream_of(hip_stream), s->view, s->libm, s->cubic_pose, count, 1, root_bone, nullptr, time_prev, time, clip_index, clip, 0u,
				motion_out, pose);
	});
}

int32_t mbik_clip_root_motion_layers(mbik_clipset *s, int32_t count, int32_t layer_count, int32_t root_bone, const mbik_clip_layer *layers,
		const double *time_prev, uint32_t flags, float *motion_out, float *pose, void *hip_stream) {
	if (int rc = check_set(s)) return rc;
	if (int rc = check_root_motion_layers(s->B, count, layer_count, root_bone, layers, time_prev, flags, motion_out, pose)) return settled(rc);
	return launched(s->device, "layered root motion", [&] {
		return mbik::launch_root_motion(stream_of(hip_stream), s->view, s->libm, s->cubic_pose, count, layer_count, root_bone, records(layers), time_prev, nullptr,
				nullptr, 0, flags, motion_out, pose);
	});
}

int32_t mbik_root_motion_apply(mbik_clipset *s, int32_t count, const float *motion, uint32_t flags, float *skeleton_global, void *hip_stream) {
	if (int rc = check_set(s)) return rc;
	if (int rc = check_root_apply(count, motion, flags, skeleton_global)) return settled(rc);
	return launched(s->device, "root motion apply",
			[&] { return mbik::launch_root_apply(stream_of(hip_stream), count, motion, flags, skeleton_global); });
}

int32_t mbik_clip_root_motion_cpu(int32_t bone_count, const float *rest_pose, int32_t clip_count, const mbik_clip_desc *clips,
		int32_t libm_variant, int32_t count, int32_t root_bone, const double *time_prev, const double *time, const int32_t *clip_index,
		int32_t clip, float *motion_out, float *pose) {
	PackedSet pk;
	if (int rc = pk.pack(bone_count, rest_pose, clip_count, clips, libm_variant, false, nullptr)) return rc;
	if (int rc = check_root_motion(bone_count, clip_count, count, root_bone, time_prev, time, clip_index, clip, motion_out, pose)) return settled(rc);
	root_motion_host(pk, count, 1, root_bone, nullptr, time_prev, time, clip_index, clip, 0u, motion_out, pose);
	return MBIK_OK;
}

int32_t mbik_clip_root_motion_layers_cpu(int32_t bone_count, const float *rest_pose, int32_t clip_count, const mbik_clip_desc *clips,
		int32_t libm_variant, int32_t count, int32_t layer_count, int32_t root_bone, const mbik_clip_layer *layers, const double *time_prev,
		uint32_t flags, float *motion_out, float *pose) {
	PackedSet pk;
	if (int rc = pk.pack(bone_count, rest_pose, clip_count, clips, libm_variant, false, nullptr)) return rc;
	if (int rc = check_root_motion_layers(bone_count, count, layer_count, root_bone, layers, time_prev, flags, motion_out, pose)) return settled(rc);
	root_motion_host(pk, count, layer_count, root_bone, records(layers), time_prev, nullptr, nullptr, 0, flags, motion_out, pose);
	return MBIK_OK;
}

int32_t mbik_clip_call_cpu(const mbik_clipset_desc *d, const mbik_clip_call *c) {
	if (int rc = check_set_desc(d)) return rc;
	if (int rc = check_call_struct(c)) return rc;
	const bool shape_kind = c->kind == MBIK_CLIP_CALL_SHAPES || c->kind == MBIK_CLIP_CALL_SHAPES_LAYERS;
	PackedSet pk;
	if (int rc = pk.pack(d->bone_count, d->rest_pose, d->clip_count, d->clips, d->libm_variant, shape_kind || d->shapes != nullptr, d->shapes, true))
		return rc;
	const int32_t B = d->bone_count, P = (int32_t)pk.init.size();
	switch (c->kind) {
	case MBIK_CLIP_CALL_SAMPLE:
		if (int rc = check_sample(B, d->clip_count, c->count, c->time, c->clip_index, c->clip, c->out)) return settled(rc);
		sample_host(pk, c->count, c->time, c->clip_index, c->clip, c->out);
		return MBIK_OK;
	case MBIK_CLIP_CALL_SAMPLE_LAYERS:
		if (int rc = check_sample_layers((int64_t)B * 10, c->count, c->layer_count, c->layers, c->flags, c->out, "pose_out")) return settled(rc);
		sample_layers_host(pk, c->count, c->layer_count, c->layers, c->flags, c->out);
		return MBIK_OK;
	case MBIK_CLIP_CALL_SHAPES:
		if (int rc = check_sample_shapes(P, d->clip_count, c->count, c->time, c->clip_index, c->clip, c->out)) return settled(rc);
		sample_shapes_host(pk, c->count, c->time, c->clip_index, c->clip, c->out);
		return MBIK_OK;
	case MBIK_CLIP_CALL_SHAPES_LAYERS:
		if (int rc = check_sample_layers(P, c->count, c->layer_count, c->layers, c->flags, c->out, "weights_out")) return settled(rc);
		sample_shapes_layers_host(pk, c->count, c->layer_count, c->layers, c->flags, c->out);
		return MBIK_OK;
	case MBIK_CLIP_CALL_ROOT_MOTION:
		if (int rc = check_root_motion(B, d->clip_count, c->count, c->root_bone, c->time_prev, c->time, c->clip_index, c->clip, c->out, c->pose))
			return settled(rc);
		root_motion_host(pk, c->count, 1, c->root_bone, nullptr, c->time_prev, c->time, c->clip_index, c->clip, 0u, c->out, c->pose);
		return MBIK_OK;
	default: // MBIK_CLIP_CALL_ROOT_MOTION_LAYERS
		if (int rc = check_root_motion_layers(B, c->count, c->layer_count, c->root_bone, c->layers, c->time_prev, c->flags, c->out, c->pose))
			return settled(rc);
		root_motion_host(pk, c->count, c->layer_count, c->root_bone, records(c->layers), c->time_prev, nullptr, nullptr, 0, c->flags, c->out, c->pose);
		return MBIK_OK;
	}
}

int32_t mbik_root_motion_apply_cpu(int32_t count, const float *motion, uint32_t flags, float *skeleton_global) {
	if (int rc = check_root_apply(count, motion, flags, skeleton_global)) return settled(rc);
	for (int64_t s = 0; s < count; s++) mbik::root_motion_apply(motion + s * 10, flags, skeleton_global + s * 12);
	return MBIK_OK;
}

} // extern "C"
