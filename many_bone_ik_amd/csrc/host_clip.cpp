// Animation clip sampling (include/mbik.h, ABI 12): the clip-set handle, mbik_clip_sample, which
// launches k_clip.hip's kernel on the set's device, and mbik_clip_sample_cpu, which runs the same
// per-bone code (clip.h) on the host.  The front stage of a frame: the poses mbik_solve reads are
// sampled on the solve's stream from a time and a clip index per skeleton.  DESIGN.md §16.
// mbik_clip_sample_layers and its _cpu form blend up to 8 (time, clip, weight) layers a skeleton
// the same way (k_clip_layers.hip, clip_layers.h).  A set made by
// mbik_clipset_create_shaped carries blend-shape tracks as well: mbik_clip_sample_shapes and
// mbik_clip_sample_shapes_layers write the [count][P] weights the shaped skinning reads
// (k_clip_shapes.hip, clip_shapes.h).  mbik_clip_root_motion[_layers] extract the root
// bone's motion over the frame from the same tables and mbik_root_motion_apply composes it into
// skeleton_global (k_root_motion.hip, root_motion.h).
#include "host.h"

#include <cmath>
#include <cstddef>

#include "clip_shapes.h"
#include "root_motion.h"

using namespace mbik_host;

struct mbik_clipset {
	int device = 0;
	int32_t B = 0, clip_count = 0, libm = 0;
	DevBuf blob;
	mbik::ClipView view{}; // device pointers into blob
	int32_t P = 0;         // 0: a set without shapes
	DevBuf shape_blob;
	mbik::ShapeView shapes{}; // device pointers into shape_blob
};

namespace {

// The repacked tables (clip.h), checked: everything the per-bone code indexes without a test.
struct Packed {
	std::vector<mbik::ClipInfo> clips;
	std::vector<mbik::ClipHeader> headers;
	std::vector<double> times;
	std::vector<mbik::ClipValue> values;
	std::vector<float> rest;
	mbik::ClipView view(int32_t B) const {
		return mbik::ClipView{B, (int32_t)clips.size(), clips.data(), headers.data(), times.data(), values.data(), rest.data()};
	}
};

int pack(int32_t B, const float *rest_pose, int32_t clip_count, const mbik_clip_desc *clips, int32_t libm_variant, Packed &out) {
	if (B < 0 || clip_count < 0) return fail(MBIK_EINVAL, "negative count");
	if (!rest_pose) return fail(MBIK_EINVAL, "null rest_pose");
	if (clip_count == 0) return fail(MBIK_EINVAL, "a clip set needs at least one clip");
	if (!clips) return fail(MBIK_EINVAL, "null clips");
	if (libm_variant != MBIK_LIBM_VARIANT_FMA && libm_variant != MBIK_LIBM_VARIANT_SSE2) return fail(MBIK_EINVAL, "unknown libm_variant");
	if ((int64_t)clip_count * B * 3 > INT32_MAX) return fail(MBIK_EUNSUPPORTED, "more than 2^31 (clip, bone, channel) headers");
	out.clips.resize(clip_count);
	out.headers.assign((size_t)clip_count * B * 3, mbik::ClipHeader{0, 0, 0, 0});
	out.rest.assign(rest_pose, rest_pose + (size_t)B * 10);
	for (int32_t c = 0; c < clip_count; c++) {
		const mbik_clip_desc &d = clips[c];
		const std::string where = "clip " + std::to_string(c);
		if (!(d.length > 0) || !std::isfinite(d.length)) return fail(MBIK_EINVAL, where + ": length must be positive and finite");
		if (d.loop_mode != 0 && d.loop_mode != 1) return fail(MBIK_EINVAL, where + ": unknown loop_mode " + std::to_string(d.loop_mode));
		if (d.track_count < 0) return fail(MBIK_EINVAL, where + ": negative track_count");
		if (d.track_count > 0 && !d.tracks) return fail(MBIK_EINVAL, where + ": null tracks");
		out.clips[c] = mbik::ClipInfo{d.length, d.loop_mode, 0};
		for (int32_t k = 0; k < d.track_count; k++) {
			const mbik_clip_track &t = d.tracks[k];
			const std::string tw = where + " track " + std::to_string(k);
			if (t.bone < 0 || t.bone >= B) return fail(MBIK_EINVAL, tw + ": bone " + std::to_string(t.bone) + " outside [0, " + std::to_string(B) + ")");
			if (t.channel < 0 || t.channel > 2) return fail(MBIK_EINVAL, tw + ": unknown channel " + std::to_string(t.channel));
			if (t.interpolation != 0 && t.interpolation != 1) return fail(MBIK_EINVAL, tw + ": unknown interpolation " + std::to_string(t.interpolation));
			if (t.key_count < 0) return fail(MBIK_EINVAL, tw + ": negative key_count");
			if (t.key_count == 0) continue; // the same as no track
			if (!t.times || !t.values) return fail(MBIK_EINVAL, tw + ": null times or values");
			mbik::ClipHeader &h = out.headers[((size_t)c * B + t.bone) * 3 + t.channel];
			if (h.key_count) return fail(MBIK_EINVAL, tw + ": a second track with keys for bone " + std::to_string(t.bone) + " channel " + std::to_string(t.channel));
			if (out.times.size() + (size_t)t.key_count > (size_t)INT32_MAX) return fail(MBIK_EUNSUPPORTED, "more than 2^31 keys in a clip set");
			for (int32_t i = 0; i < t.key_count; i++) {
				const double x = t.times[i];
				if (!std::isfinite(x) || !(x >= 0) || !(x <= d.length))
					return fail(MBIK_EINVAL, tw + ": key " + std::to_string(i) + " has a time that is not finite or outside [0, length]");
				if (i > 0 && !(x > t.times[i - 1])) return fail(MBIK_EINVAL, tw + ": key times are not strictly increasing at key " + std::to_string(i));
			}
			h.key_off = (int32_t)out.times.size(), h.key_count = t.key_count;
			h.flags = (t.interpolation == 1 ? mbik::kClipLinear : 0) | (d.loop_mode == 1 && t.loop_wrap ? mbik::kClipWrap : 0);
			const int w = t.channel == 1 ? 4 : 3;
			for (int32_t i = 0; i < t.key_count; i++) {
				const float *v = t.values + (size_t)i * w;
				out.times.push_back(t.times[i]);
				out.values.push_back(mbik::ClipValue{v[0], v[1], v[2], w == 4 ? v[3] : 0.0f});
			}
		}
	}
	// the spare entry that makes index key_off + 0 valid for every header (clip.h)
	out.times.push_back(0.0);
	out.values.push_back(mbik::ClipValue{0.0f, 0.0f, 0.0f, 0.0f});
	return MBIK_OK;
}

// The checks of a sampling call past the set's own; 0 = go on, 1 = nothing to do.
int check_call(int32_t B, int32_t clip_count, int32_t count, const double *time, const int32_t *clip_index, int32_t clip,
		const float *pose_out) {
	if (count < 0) return fail(MBIK_EINVAL, "negative count");
	if (count == 0 || B == 0) return 1;
	if (!time) return fail(MBIK_EINVAL, "null time");
	if (!pose_out) return fail(MBIK_EINVAL, "null pose_out");
	if (!clip_index && (clip < 0 || clip >= clip_count))
		return fail(MBIK_EINVAL, "clip " + std::to_string(clip) + " outside the set's " + std::to_string(clip_count) + " clips");
	return 0;
}

// The same for a layered call; the records themselves are the kernel's (or the per-bone code's) to test.
int check_layers_call(int32_t B, int32_t count, int32_t layer_count, const mbik_clip_layer *layers, uint32_t flags, const float *pose_out) {
	if (count < 0) return fail(MBIK_EINVAL, "negative count");
	if (layer_count < 1 || layer_count > MBIK_CLIP_MAX_LAYERS)
		return fail(MBIK_EINVAL, "layer_count " + std::to_string(layer_count) + " outside [1, " + std::to_string(MBIK_CLIP_MAX_LAYERS) + "]");
	if (flags & ~MBIK_CLIP_LAYERS_NORMALIZE) return fail(MBIK_EINVAL, "unknown flags " + std::to_string(flags));
	if (count == 0 || B == 0) return 1;
	if (!layers) return fail(MBIK_EINVAL, "null layers");
	if (!pose_out) return fail(MBIK_EINVAL, "null pose_out");
	if (reinterpret_cast<uintptr_t>(layers) % 8) return fail(MBIK_EINVAL, "layers is not 8-byte aligned");
	if (overlap(layers, (size_t)count * layer_count * sizeof(mbik_clip_layer), pose_out, (size_t)count * B * 10 * sizeof(float)))
		return fail(MBIK_EINVAL, "pose_out overlaps layers");
	return 0;
}
static_assert(sizeof(mbik_clip_layer) == sizeof(mbik::ClipLayer) && offsetof(mbik_clip_layer, clip) == offsetof(mbik::ClipLayer, clip) &&
				offsetof(mbik_clip_layer, weight) == offsetof(mbik::ClipLayer, weight),
		"mbik_clip_layer is clip_layers.h's ClipLayer");

// The checks of the two root-motion extraction calls; 0 = go on, 1 = nothing to do.  `layers` null: the plain form, whose
// `time` takes the records' place.
int check_root_call(int32_t B, int32_t clip_count, int32_t count, int32_t layer_count, int32_t root_bone, bool plain,
		const mbik_clip_layer *layers, const double *time_prev, const double *time, const int32_t *clip_index, int32_t clip, uint32_t flags,
		const float *motion_out, const float *pose) {
	if (count < 0) return fail(MBIK_EINVAL, "negative count");
	if (root_bone < 0 || root_bone >= B)
		return fail(MBIK_EINVAL, "root_bone " + std::to_string(root_bone) + " outside [0, " + std::to_string(B) + ")");
	if (layer_count < 1 || layer_count > MBIK_CLIP_MAX_LAYERS)
		return fail(MBIK_EINVAL, "layer_count " + std::to_string(layer_count) + " outside [1, " + std::to_string(MBIK_CLIP_MAX_LAYERS) + "]");
	if (flags & ~MBIK_CLIP_LAYERS_NORMALIZE) return fail(MBIK_EINVAL, "unknown flags " + std::to_string(flags));
	if (plain && !clip_index && (clip < 0 || clip >= clip_count))
		return fail(MBIK_EINVAL, "clip " + std::to_string(clip) + " outside the set's " + std::to_string(clip_count) + " clips");
	if (count == 0) return 1;
	if (!plain && !layers) return fail(MBIK_EINVAL, "null layers");
	if (plain && !time) return fail(MBIK_EINVAL, "null time");
	if (!time_prev) return fail(MBIK_EINVAL, "null time_prev");
	if (!motion_out) return fail(MBIK_EINVAL, "null motion_out");
	if (!plain && reinterpret_cast<uintptr_t>(layers) % 8) return fail(MBIK_EINVAL, "layers is not 8-byte aligned");
	if (plain && reinterpret_cast<uintptr_t>(time) % 8) return fail(MBIK_EINVAL, "time is not 8-byte aligned");
	if (reinterpret_cast<uintptr_t>(time_prev) % 8) return fail(MBIK_EINVAL, "time_prev is not 8-byte aligned");
	const size_t per = (size_t)count * layer_count, out_bytes = (size_t)count * 10 * sizeof(float);
	if (!plain && overlap(layers, per * sizeof(mbik_clip_layer), motion_out, out_bytes)) return fail(MBIK_EINVAL, "motion_out overlaps layers");
	if (plain && overlap(time, per * sizeof(double), motion_out, out_bytes)) return fail(MBIK_EINVAL, "motion_out overlaps time");
	if (overlap(time_prev, per * sizeof(double), motion_out, out_bytes)) return fail(MBIK_EINVAL, "motion_out overlaps time_prev");
	if (plain && clip_index && overlap(clip_index, (size_t)count * sizeof(int32_t), motion_out, out_bytes))
		return fail(MBIK_EINVAL, "motion_out overlaps clip_index");
	if (pose && overlap(pose, (size_t)count * B * 10 * sizeof(float), motion_out, out_bytes)) return fail(MBIK_EINVAL, "motion_out overlaps pose");
	return 0;
}

int check_root_apply(int32_t count, const float *motion, uint32_t flags, const float *skeleton_global) {
	if (count < 0) return fail(MBIK_EINVAL, "negative count");
	if (flags & ~MBIK_ROOT_MOTION_ORTHONORMALIZE) return fail(MBIK_EINVAL, "unknown flags " + std::to_string(flags));
	if (count == 0) return 1;
	if (!motion) return fail(MBIK_EINVAL, "null motion");
	if (!skeleton_global) return fail(MBIK_EINVAL, "null skeleton_global");
	if (overlap(motion, (size_t)count * 10 * sizeof(float), skeleton_global, (size_t)count * 12 * sizeof(float)))
		return fail(MBIK_EINVAL, "skeleton_global overlaps motion");
	return 0;
}
static_assert(MBIK_ROOT_MOTION_ORTHONORMALIZE == mbik::kRootMotionOrthonormalize, "the flag is root_motion.h's");

// The host form of both extraction calls: one skeleton after the other through root_motion.h.
void root_motion_host(const mbik::ClipView &v, int32_t libm, int32_t count, int32_t K, int32_t root, const mbik::ClipLayer *L,
		const double *time_prev, const double *time, const int32_t *clip_index, int32_t clip, uint32_t flags, float *motion_out, float *pose) {
	for (int64_t s = 0; s < count; s++) {
		float *pose_s = pose ? pose + s * v.B * 10 : nullptr;
		if (L) {
			mbik::root_motion_skeleton(v, mbik::RootLayers{L + s * K, time_prev + s * K}, K, flags, root, libm, motion_out + s * 10, pose_s);
		} else {
			const mbik::RootPlain src{mbik::ClipLayer{time[s], clip_index ? clip_index[s] : clip, 1.0f}, time_prev[s]};
			mbik::root_motion_skeleton(v, src, 1, 0u, root, libm, motion_out + s * 10, pose_s);
		}
	}
}

size_t up16(size_t n) { return (n + 15) & ~(size_t)15; }

// The repacked shape tracks (clip_shapes.h), checked.  `clips` has passed pack().
struct PackedShapes {
	std::vector<mbik::ClipInfo> clips;
	std::vector<mbik::ShapeHeader> headers;
	std::vector<mbik::ShapeKey> keys;
	std::vector<float> init;
	mbik::ShapeView view() const {
		return mbik::ShapeView{(int32_t)init.size(), (int32_t)clips.size(), clips.data(), headers.data(), keys.data(), init.data()};
	}
};

int pack_shapes(int32_t clip_count, const mbik_clip_desc *clips, const mbik_clipset_shapes *sh, PackedShapes &out) {
	if (!sh) return fail(MBIK_EINVAL, "null shapes");
	if (sh->struct_size < (int32_t)sizeof(mbik_clipset_shapes)) return fail(MBIK_EINVAL, "shapes->struct_size is smaller than mbik_clipset_shapes");
	const int32_t P = sh->shape_count;
	if (P < 1) return fail(MBIK_EINVAL, "shape_count must be at least 1");
	if (!sh->clips) return fail(MBIK_EINVAL, "null shapes->clips");
	if ((int64_t)clip_count * P > INT32_MAX) return fail(MBIK_EUNSUPPORTED, "more than 2^31 (clip, shape) headers");
	out.clips.resize(clip_count);
	out.headers.assign((size_t)clip_count * P, mbik::ShapeHeader{0, 0, 0, 0});
	if (sh->init) out.init.assign(sh->init, sh->init + P);
	else out.init.assign((size_t)P, 0.0f);
	for (int32_t c = 0; c < clip_count; c++) {
		const mbik_clip_desc &d = clips[c];
		const mbik_clip_shape_tracks &st = sh->clips[c];
		const std::string where = "clip " + std::to_string(c);
		out.clips[c] = mbik::ClipInfo{d.length, d.loop_mode, 0};
		if (st.track_count < 0) return fail(MBIK_EINVAL, where + ": negative shape track_count");
		if (st.track_count > 0 && !st.tracks) return fail(MBIK_EINVAL, where + ": null shape tracks");
		for (int32_t k = 0; k < st.track_count; k++) {
			const mbik_shape_track &t = st.tracks[k];
			const std::string tw = where + " shape track " + std::to_string(k);
			if (t.shape < 0 || t.shape >= P) return fail(MBIK_EINVAL, tw + ": shape " + std::to_string(t.shape) + " outside [0, " + std::to_string(P) + ")");
			if (t.interpolation != 0 && t.interpolation != 1) return fail(MBIK_EINVAL, tw + ": unknown interpolation " + std::to_string(t.interpolation));
			if (t.key_count < 0) return fail(MBIK_EINVAL, tw + ": negative key_count");
			if (t.key_count == 0) continue; // the same as no track
			if (!t.times || !t.values) return fail(MBIK_EINVAL, tw + ": null times or values");
			mbik::ShapeHeader &h = out.headers[(size_t)c * P + t.shape];
			if (h.key_count) return fail(MBIK_EINVAL, tw + ": a second track with keys for shape " + std::to_string(t.shape));
			if (out.keys.size() + (size_t)t.key_count > (size_t)INT32_MAX) return fail(MBIK_EUNSUPPORTED, "more than 2^31 shape keys in a clip set");
			for (int32_t i = 0; i < t.key_count; i++) {
				const double x = t.times[i];
				if (!std::isfinite(x) || !(x >= 0) || !(x <= d.length))
					return fail(MBIK_EINVAL, tw + ": key " + std::to_string(i) + " has a time that is not finite or outside [0, length]");
				if (i > 0 && !(x > t.times[i - 1])) return fail(MBIK_EINVAL, tw + ": key times are not strictly increasing at key " + std::to_string(i));
			}
			h.key_off = (int32_t)out.keys.size(), h.key_count = t.key_count;
			h.flags = (t.interpolation == 1 ? mbik::kClipLinear : 0) | (d.loop_mode == 1 && t.loop_wrap ? mbik::kClipWrap : 0);
			for (int32_t i = 0; i < t.key_count; i++) out.keys.push_back(mbik::ShapeKey{t.times[i], t.values[i], 0.0f});
		}
	}
	// the spare record that makes index key_off + 0 valid for every header (clip_shapes.h)
	out.keys.push_back(mbik::ShapeKey{0.0, 0.0f, 0.0f});
	return MBIK_OK;
}

// The checks of the two shape sampling calls; 0 = go on, 1 = nothing to do.
int check_shapes_call(int32_t P, int32_t clip_count, int32_t count, const double *time, const int32_t *clip_index, int32_t clip,
		const float *weights_out) {
	if (count < 0) return fail(MBIK_EINVAL, "negative count");
	if (count == 0) return 1;
	if (!time) return fail(MBIK_EINVAL, "null time");
	if (!weights_out) return fail(MBIK_EINVAL, "null weights_out");
	if (!clip_index && (clip < 0 || clip >= clip_count))
		return fail(MBIK_EINVAL, "clip " + std::to_string(clip) + " outside the set's " + std::to_string(clip_count) + " clips");
	const size_t bytes = (size_t)count * P * sizeof(float);
	if (overlap(time, (size_t)count * sizeof(double), weights_out, bytes)) return fail(MBIK_EINVAL, "weights_out overlaps time");
	if (clip_index && overlap(clip_index, (size_t)count * sizeof(int32_t), weights_out, bytes))
		return fail(MBIK_EINVAL, "weights_out overlaps clip_index");
	return 0;
}

int check_shapes_layers_call(int32_t P, int32_t count, int32_t layer_count, const mbik_clip_layer *layers, uint32_t flags,
		const float *weights_out) {
	if (count < 0) return fail(MBIK_EINVAL, "negative count");
	if (layer_count < 1 || layer_count > MBIK_CLIP_MAX_LAYERS)
		return fail(MBIK_EINVAL, "layer_count " + std::to_string(layer_count) + " outside [1, " + std::to_string(MBIK_CLIP_MAX_LAYERS) + "]");
	if (flags & ~MBIK_CLIP_LAYERS_NORMALIZE) return fail(MBIK_EINVAL, "unknown flags " + std::to_string(flags));
	if (count == 0) return 1;
	if (!layers) return fail(MBIK_EINVAL, "null layers");
	if (!weights_out) return fail(MBIK_EINVAL, "null weights_out");
	if (reinterpret_cast<uintptr_t>(layers) % 8) return fail(MBIK_EINVAL, "layers is not 8-byte aligned");
	if (overlap(layers, (size_t)count * layer_count * sizeof(mbik_clip_layer), weights_out, (size_t)count * P * sizeof(float)))
		return fail(MBIK_EINVAL, "weights_out overlaps layers");
	return 0;
}

// mbik_clipset_create, and with `shapes` mbik_clipset_create_shaped.
int create_set(int32_t bone_count, const float *rest_pose, int32_t clip_count, const mbik_clip_desc *clips, bool shaped,
		const mbik_clipset_shapes *shapes, int32_t libm_variant, int32_t device, mbik_clipset **out) {
	if (!out) return fail(MBIK_EINVAL, "null out");
	*out = nullptr;
	Packed pk;
	if (int rc = pack(bone_count, rest_pose, clip_count, clips, libm_variant, pk)) return rc;
	PackedShapes ps;
	if (shaped)
		if (int rc = pack_shapes(clip_count, clips, shapes, ps)) return rc;
	if (int rc = check_device(device)) return rc;
	std::unique_ptr<mbik_clipset> s(new mbik_clipset());
	s->device = device, s->B = bone_count, s->clip_count = clip_count, s->libm = libm_variant;
	// one blob: clip infos, headers, times, values, rest pose, each from a 16-byte boundary
	const size_t n_info = pk.clips.size() * sizeof(mbik::ClipInfo), n_head = pk.headers.size() * sizeof(mbik::ClipHeader),
				 n_time = pk.times.size() * sizeof(double), n_val = pk.values.size() * sizeof(mbik::ClipValue),
				 n_rest = pk.rest.size() * sizeof(float);
	const size_t o_info = 0, o_head = up16(o_info + n_info), o_time = up16(o_head + n_head), o_val = up16(o_time + n_time),
				 o_rest = up16(o_val + n_val), bytes = up16(o_rest + n_rest) + 16;
	std::vector<unsigned char> blob(bytes, 0);
	std::memcpy(blob.data() + o_info, pk.clips.data(), n_info);
	if (n_head) std::memcpy(blob.data() + o_head, pk.headers.data(), n_head);
	if (n_time) std::memcpy(blob.data() + o_time, pk.times.data(), n_time);
	if (n_val) std::memcpy(blob.data() + o_val, pk.values.data(), n_val);
	if (n_rest) std::memcpy(blob.data() + o_rest, pk.rest.data(), n_rest);
	DeviceGuard guard(device);
	if (int rc = s->blob.reserve(bytes, "hipMalloc failed for the clip set")) return rc;
	unsigned char *b = s->blob.as<unsigned char>();
	if (hipMemcpy(b, blob.data(), bytes, hipMemcpyHostToDevice) != hipSuccess) return fail(MBIK_EHIP, "hipMemcpy failed for the clip set");
	s->view = mbik::ClipView{bone_count, clip_count, reinterpret_cast<const mbik::ClipInfo *>(b + o_info),
			reinterpret_cast<const mbik::ClipHeader *>(b + o_head), reinterpret_cast<const double *>(b + o_time),
			reinterpret_cast<const mbik::ClipValue *>(b + o_val), reinterpret_cast<const float *>(b + o_rest)};
	if (shaped) {
		// a blob of its own: clip infos, headers, key records, init, each from a 16-byte boundary
		const size_t m_info = ps.clips.size() * sizeof(mbik::ClipInfo), m_head = ps.headers.size() * sizeof(mbik::ShapeHeader),
					 m_key = ps.keys.size() * sizeof(mbik::ShapeKey), m_init = ps.init.size() * sizeof(float);
		const size_t p_info = 0, p_head = up16(p_info + m_info), p_key = up16(p_head + m_head), p_init = up16(p_key + m_key),
					 total = up16(p_init + m_init) + 16;
		std::vector<unsigned char> sb(total, 0);
		std::memcpy(sb.data() + p_info, ps.clips.data(), m_info);
		std::memcpy(sb.data() + p_head, ps.headers.data(), m_head);
		std::memcpy(sb.data() + p_key, ps.keys.data(), m_key);
		std::memcpy(sb.data() + p_init, ps.init.data(), m_init);
		if (int rc = s->shape_blob.reserve(total, "hipMalloc failed for the clip set's shape tracks")) return rc;
		unsigned char *d = s->shape_blob.as<unsigned char>();
		if (hipMemcpy(d, sb.data(), total, hipMemcpyHostToDevice) != hipSuccess)
			return fail(MBIK_EHIP, "hipMemcpy failed for the clip set's shape tracks");
		s->P = (int32_t)ps.init.size();
		s->shapes = mbik::ShapeView{s->P, clip_count, reinterpret_cast<const mbik::ClipInfo *>(d + p_info),
				reinterpret_cast<const mbik::ShapeHeader *>(d + p_head), reinterpret_cast<const mbik::ShapeKey *>(d + p_key),
				reinterpret_cast<const float *>(d + p_init)};
	}
	*out = s.release();
	return MBIK_OK;
}

} // namespace

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

void mbik_clipset_destroy(mbik_clipset *s) { delete s; }

int32_t mbik_clip_sample(mbik_clipset *s, int32_t count, const double *time, const int32_t *clip_index, int32_t clip, float *pose_out,
		void *hip_stream) {
	if (!s) return fail(MBIK_EINVAL, "null clip set");
	const int rc = check_call(s->B, s->clip_count, count, time, clip_index, clip, pose_out);
	if (rc) return rc < 0 ? rc : MBIK_OK;
	if ((int64_t)count * s->B > (int64_t)INT32_MAX * 256) return fail(MBIK_EUNSUPPORTED, "more than 2^39 bones in one call");
	DeviceGuard guard(s->device);
	hipError_t e = mbik::launch_clip(reinterpret_cast<hipStream_t>(hip_stream), s->view, s->libm, (int64_t)count * s->B, time, clip_index,
			clip, pose_out);
	if (e != hipSuccess) return fail(MBIK_EHIP, std::string("clip sample launch failed: ") + hipGetErrorString(e));
	return MBIK_OK;
}

int32_t mbik_clip_sample_cpu(int32_t bone_count, const float *rest_pose, int32_t clip_count, const mbik_clip_desc *clips,
		int32_t libm_variant, int32_t count, const double *time, const int32_t *clip_index, int32_t clip, float *pose_out) {
	Packed pk;
	if (int rc = pack(bone_count, rest_pose, clip_count, clips, libm_variant, pk)) return rc;
	const int rc = check_call(bone_count, clip_count, count, time, clip_index, clip, pose_out);
	if (rc) return rc < 0 ? rc : MBIK_OK;
	const mbik::ClipView v = pk.view(bone_count);
	for (int64_t s = 0; s < count; s++) {
		const int32_t c = clip_index ? clip_index[s] : clip;
		for (int32_t b = 0; b < bone_count; b++) mbik::clip_sample_bone(v, c, b, time[s], libm_variant, pose_out + (s * bone_count + b) * 10);
	}
	return MBIK_OK;
}

int32_t mbik_clip_sample_layers(mbik_clipset *s, int32_t count, int32_t layer_count, const mbik_clip_layer *layers, uint32_t flags,
		float *pose_out, void *hip_stream) {
	if (!s) return fail(MBIK_EINVAL, "null clip set");
	const int rc = check_layers_call(s->B, count, layer_count, layers, flags, pose_out);
	if (rc) return rc < 0 ? rc : MBIK_OK;
	if ((int64_t)count * s->B > (int64_t)INT32_MAX * 256) return fail(MBIK_EUNSUPPORTED, "more than 2^39 bones in one call");
	DeviceGuard guard(s->device);
	hipError_t e = mbik::launch_clip_layers(reinterpret_cast<hipStream_t>(hip_stream), s->view, s->libm, (int64_t)count * s->B,
			reinterpret_cast<const mbik::ClipLayer *>(layers), layer_count, flags, pose_out);
	if (e != hipSuccess) return fail(MBIK_EHIP, std::string("layered clip sample launch failed: ") + hipGetErrorString(e));
	return MBIK_OK;
}

int32_t mbik_clip_sample_layers_cpu(int32_t bone_count, const float *rest_pose, int32_t clip_count, const mbik_clip_desc *clips,
		int32_t libm_variant, int32_t count, int32_t layer_count, const mbik_clip_layer *layers, uint32_t flags, float *pose_out) {
	Packed pk;
	if (int rc = pack(bone_count, rest_pose, clip_count, clips, libm_variant, pk)) return rc;
	const int rc = check_layers_call(bone_count, count, layer_count, layers, flags, pose_out);
	if (rc) return rc < 0 ? rc : MBIK_OK;
	const mbik::ClipView v = pk.view(bone_count);
	const mbik::ClipLayer *L = reinterpret_cast<const mbik::ClipLayer *>(layers);
	for (int64_t s = 0; s < count; s++)
		for (int32_t b = 0; b < bone_count; b++)
			mbik::clip_layers_bone(v, L + s * layer_count, layer_count, flags, b, libm_variant, pose_out + (s * bone_count + b) * 10);
	return MBIK_OK;
}

int32_t mbik_clip_sample_shapes(mbik_clipset *s, int32_t count, const double *time, const int32_t *clip_index, int32_t clip,
		float *weights_out, void *hip_stream) {
	if (!s) return fail(MBIK_EINVAL, "null clip set");
	if (!s->P) return fail(MBIK_EINVAL, "the clip set has no shapes (mbik_clipset_create_shaped)");
	const int rc = check_shapes_call(s->P, s->clip_count, count, time, clip_index, clip, weights_out);
	if (rc) return rc < 0 ? rc : MBIK_OK;
	if ((int64_t)count * s->P > (int64_t)INT32_MAX * 256) return fail(MBIK_EUNSUPPORTED, "more than 2^39 weights in one call");
	DeviceGuard guard(s->device);
	hipError_t e = mbik::launch_clip_shapes(reinterpret_cast<hipStream_t>(hip_stream), s->shapes, (int64_t)count * s->P, time, clip_index,
			clip, weights_out);
	if (e != hipSuccess) return fail(MBIK_EHIP, std::string("shape sample launch failed: ") + hipGetErrorString(e));
	return MBIK_OK;
}

int32_t mbik_clip_sample_shapes_layers(mbik_clipset *s, int32_t count, int32_t layer_count, const mbik_clip_layer *layers, uint32_t flags,
		float *weights_out, void *hip_stream) {
	if (!s) return fail(MBIK_EINVAL, "null clip set");
	if (!s->P) return fail(MBIK_EINVAL, "the clip set has no shapes (mbik_clipset_create_shaped)");
	const int rc = check_shapes_layers_call(s->P, count, layer_count, layers, flags, weights_out);
	if (rc) return rc < 0 ? rc : MBIK_OK;
	if ((int64_t)count * s->P > (int64_t)INT32_MAX * 256) return fail(MBIK_EUNSUPPORTED, "more than 2^39 weights in one call");
	DeviceGuard guard(s->device);
	hipError_t e = mbik::launch_clip_shapes_layers(reinterpret_cast<hipStream_t>(hip_stream), s->shapes, (int64_t)count * s->P,
			reinterpret_cast<const mbik::ClipLayer *>(layers), layer_count, flags, weights_out);
	if (e != hipSuccess) return fail(MBIK_EHIP, std::string("layered shape sample launch failed: ") + hipGetErrorString(e));
	return MBIK_OK;
}

int32_t mbik_clip_sample_shapes_cpu(int32_t bone_count, const float *rest_pose, int32_t clip_count, const mbik_clip_desc *clips,
		const mbik_clipset_shapes *shapes, int32_t libm_variant, int32_t count, const double *time, const int32_t *clip_index, int32_t clip,
		float *weights_out) {
	Packed pk;
	if (int rc = pack(bone_count, rest_pose, clip_count, clips, libm_variant, pk)) return rc;
	PackedShapes ps;
	if (int rc = pack_shapes(clip_count, clips, shapes, ps)) return rc;
	const mbik::ShapeView v = ps.view();
	const int rc = check_shapes_call(v.P, clip_count, count, time, clip_index, clip, weights_out);
	if (rc) return rc < 0 ? rc : MBIK_OK;
	for (int64_t s = 0; s < count; s++)
		for (int32_t j = 0; j < v.P; j++) weights_out[s * v.P + j] = mbik::shape_sample(v, clip_index ? clip_index[s] : clip, j, time[s]);
	return MBIK_OK;
}

int32_t mbik_clip_sample_shapes_layers_cpu(int32_t bone_count, const float *rest_pose, int32_t clip_count, const mbik_clip_desc *clips,
		const mbik_clipset_shapes *shapes, int32_t libm_variant, int32_t count, int32_t layer_count, const mbik_clip_layer *layers,
		uint32_t flags, float *weights_out) {
	Packed pk;
	if (int rc = pack(bone_count, rest_pose, clip_count, clips, libm_variant, pk)) return rc;
	PackedShapes ps;
	if (int rc = pack_shapes(clip_count, clips, shapes, ps)) return rc;
	const mbik::ShapeView v = ps.view();
	const int rc = check_shapes_layers_call(v.P, count, layer_count, layers, flags, weights_out);
	if (rc) return rc < 0 ? rc : MBIK_OK;
	const mbik::ClipLayer *L = reinterpret_cast<const mbik::ClipLayer *>(layers);
	for (int64_t s = 0; s < count; s++)
		for (int32_t j = 0; j < v.P; j++) weights_out[s * v.P + j] = mbik::shape_layers(v, L + s * layer_count, layer_count, flags, j);
	return MBIK_OK;
}

int32_t mbik_clip_root_motion(mbik_clipset *s, int32_t count, int32_t root_bone, const double *time_prev, const double *time,
		const int32_t *clip_index, int32_t clip, float *motion_out, float *pose, void *hip_stream) {
	if (!s) return fail(MBIK_EINVAL, "null clip set");
	const int rc = check_root_call(s->B, s->clip_count, count, 1, root_bone, true, nullptr, time_prev, time, clip_index, clip, 0u, motion_out, pose);
	if (rc) return rc < 0 ? rc : MBIK_OK;
	DeviceGuard guard(s->device);
	hipError_t e = mbik::launch_root_motion(reinterpret_cast<hipStream_t>(hip_stream), s->view, s->libm, count, 1, root_bone, nullptr, time_prev,
			time, clip_index, clip, 0u, motion_out, pose);
	if (e != hipSuccess) return fail(MBIK_EHIP, std::string("root motion launch failed: ") + hipGetErrorString(e));
	return MBIK_OK;
}

int32_t mbik_clip_root_motion_layers(mbik_clipset *s, int32_t count, int32_t layer_count, int32_t root_bone, const mbik_clip_layer *layers,
		const double *time_prev, uint32_t flags, float *motion_out, float *pose, void *hip_stream) {
	if (!s) return fail(MBIK_EINVAL, "null clip set");
	const int rc = check_root_call(s->B, s->clip_count, count, layer_count, root_bone, false, layers, time_prev, nullptr, nullptr, 0, flags,
			motion_out, pose);
	if (rc) return rc < 0 ? rc : MBIK_OK;
	DeviceGuard guard(s->device);
	hipError_t e = mbik::launch_root_motion(reinterpret_cast<hipStream_t>(hip_stream), s->view, s->libm, count, layer_count, root_bone,
			reinterpret_cast<const mbik::ClipLayer *>(layers), time_prev, nullptr, nullptr, 0, flags, motion_out, pose);
	if (e != hipSuccess) return fail(MBIK_EHIP, std::string("layered root motion launch failed: ") + hipGetErrorString(e));
	return MBIK_OK;
}

int32_t mbik_root_motion_apply(mbik_clipset *s, int32_t count, const float *motion, uint32_t flags, float *skeleton_global, void *hip_stream) {
	if (!s) return fail(MBIK_EINVAL, "null clip set");
	const int rc = check_root_apply(count, motion, flags, skeleton_global);
	if (rc) return rc < 0 ? rc : MBIK_OK;
	DeviceGuard guard(s->device);
	hipError_t e = mbik::launch_root_apply(reinterpret_cast<hipStream_t>(hip_stream), count, motion, flags, skeleton_global);
	if (e != hipSuccess) return fail(MBIK_EHIP, std::string("root motion apply launch failed: ") + hipGetErrorString(e));
	return MBIK_OK;
}

int32_t mbik_clip_root_motion_cpu(int32_t bone_count, const float *rest_pose, int32_t clip_count, const mbik_clip_desc *clips,
		int32_t libm_variant, int32_t count, int32_t root_bone, const double *time_prev, const double *time, const int32_t *clip_index,
		int32_t clip, float *motion_out, float *pose) {
	Packed pk;
	if (int rc = pack(bone_count, rest_pose, clip_count, clips, libm_variant, pk)) return rc;
	const int rc = check_root_call(bone_count, clip_count, count, 1, root_bone, true, nullptr, time_prev, time, clip_index, clip, 0u, motion_out, pose);
	if (rc) return rc < 0 ? rc : MBIK_OK;
	root_motion_host(pk.view(bone_count), libm_variant, count, 1, root_bone, nullptr, time_prev, time, clip_index, clip, 0u, motion_out, pose);
	return MBIK_OK;
}

int32_t mbik_clip_root_motion_layers_cpu(int32_t bone_count, const float *rest_pose, int32_t clip_count, const mbik_clip_desc *clips,
		int32_t libm_variant, int32_t count, int32_t layer_count, int32_t root_bone, const mbik_clip_layer *layers, const double *time_prev,
		uint32_t flags, float *motion_out, float *pose) {
	Packed pk;
	if (int rc = pack(bone_count, rest_pose, clip_count, clips, libm_variant, pk)) return rc;
	const int rc = check_root_call(bone_count, clip_count, count, layer_count, root_bone, false, layers, time_prev, nullptr, nullptr, 0, flags,
			motion_out, pose);
	if (rc) return rc < 0 ? rc : MBIK_OK;
	root_motion_host(pk.view(bone_count), libm_variant, count, layer_count, root_bone, reinterpret_cast<const mbik::ClipLayer *>(layers),
			time_prev, nullptr, nullptr, 0, flags, motion_out, pose);
	return MBIK_OK;
}

int32_t mbik_root_motion_apply_cpu(int32_t count, const float *motion, uint32_t flags, float *skeleton_global) {
	const int rc = check_root_apply(count, motion, flags, skeleton_global);
	if (rc) return rc < 0 ? rc : MBIK_OK;
	for (int64_t s = 0; s < count; s++) mbik::root_motion_apply(motion + s * 10, flags, skeleton_global + s * 12);
	return MBIK_OK;
}

} // extern "C"
