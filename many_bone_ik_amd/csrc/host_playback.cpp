// Device-side playback (include/mbik.h): the playback object, which owns the
// per-skeleton playback state of a crowd on a clip set's device, mbik_playback_advance, which
// launches k_playback.hip's kernel, mbik_playback_write / mbik_playback_read, which convert
// between the public records and the object's structure of arrays, and
// mbik_playback_advance_cpu, which runs the same per-skeleton code (playback.h) on the host.
#include "host.h"

#include <cmath>

#include "playback.h"

using namespace mbik_host;

struct mbik_playback {
	int device = 0;
	int32_t capacity = 0, K = 0;
	std::vector<mbik::ClipInfo> clips; // the set's lengths and loop modes: write's checks
	DevBuf tables;                     // clip infos, next, blend_times
	DevBuf state;                      // playback.h's PlaybackState planes
	mbik::PlaybackTables tab{};        // device pointers into tables
	mbik::PlaybackState st{};          // device pointers into state
};

static_assert(sizeof(mbik_playback_slot) == sizeof(mbik::PlaybackSlot) && offsetof(mbik_playback_slot, clip) == offsetof(mbik::PlaybackSlot, clip) &&
				offsetof(mbik_playback_slot, speed) == offsetof(mbik::PlaybackSlot, speed) &&
				offsetof(mbik_playback_slot, blend_left) == offsetof(mbik::PlaybackSlot, blend_left) &&
				offsetof(mbik_playback_slot, blend_time) == offsetof(mbik::PlaybackSlot, blend_time),
		"mbik_playback_slot is playback.h's PlaybackSlot");
static_assert(sizeof(mbik_playback_cmd) == sizeof(mbik::PlaybackCmd) && offsetof(mbik_playback_cmd, skeleton) == offsetof(mbik::PlaybackCmd, skeleton) &&
				offsetof(mbik_playback_cmd, clip) == offsetof(mbik::PlaybackCmd, clip) &&
				offsetof(mbik_playback_cmd, blend_time) == offsetof(mbik::PlaybackCmd, blend_time) &&
				offsetof(mbik_playback_cmd, speed) == offsetof(mbik::PlaybackCmd, speed),
		"mbik_playback_cmd is playback.h's PlaybackCmd");
static_assert(MBIK_PLAYBACK_STARTED == mbik::kPlaybackStarted && MBIK_PLAYBACK_ENDED == mbik::kPlaybackEnded &&
				MBIK_PLAYBACK_LOOPED == mbik::kPlaybackLooped && MBIK_PLAYBACK_TRANSITIONED == mbik::kPlaybackTransitioned &&
				MBIK_PLAYBACK_BAD_COMMAND == mbik::kPlaybackBadCommand && MBIK_PLAYBACK_FADE_DROPPED == mbik::kPlaybackFadeDropped,
		"the flag and event bits are playback.h's");

namespace {

// The desc against the clip count: what the per-skeleton code indexes without a test.
int check_desc(int32_t clip_count, const mbik_playback_desc *desc) {
	if (!desc) return MBIK_OK;
	if (desc->struct_size < (int32_t)sizeof(mbik_playback_desc)) return fail(MBIK_EINVAL, "mbik_playback_desc.struct_size is too small");
	if (!std::isfinite(desc->default_blend_time) || desc->default_blend_time < 0)
		return fail(MBIK_EINVAL, "default_blend_time must be finite and not negative");
	if (desc->next)
		for (int32_t c = 0; c < clip_count; c++)
			if (desc->next[c] < -1 || desc->next[c] >= clip_count)
				return fail(MBIK_EINVAL, "next[" + std::to_string(c) + "] = " + std::to_string(desc->next[c]) + " outside [-1, " + std::to_string(clip_count) + ")");
	if (desc->blend_times)
		for (int64_t i = 0; i < (int64_t)clip_count * clip_count; i++)
			if (!std::isfinite(desc->blend_times[i]) || desc->blend_times[i] < 0)
				return fail(MBIK_EINVAL, "blend_times[" + std::to_string(i / clip_count) + "][" + std::to_string(i % clip_count) + "] must be finite and not negative");
	return MBIK_OK;
}

// mbik_playback_write's checks of [n][K] records and [n] flag words: what the per-skeleton code trusts.
int check_state(const std::vector<mbik::ClipInfo> &clips, int64_t n, int32_t K, const mbik_playback_slot *slots, const uint32_t *flags) {
	const int32_t clip_count = (int32_t)clips.size();
	for (int64_t s = 0; s < n; s++) {
		const std::string where = "skeleton " + std::to_string(s);
		if (flags[s] & ~(MBIK_PLAYBACK_STARTED | MBIK_PLAYBACK_ENDED)) return fail(MBIK_EINVAL, where + ": unknown flag bits " + std::to_string(flags[s]));
		bool off_seen = false;
		for (int32_t j = 0; j < K; j++) {
			const mbik_playback_slot &r = slots[s * K + j];
			const std::string sw = where + " slot " + std::to_string(j);
			if (r.clip < -1 || r.clip >= clip_count) return fail(MBIK_EINVAL, sw + ": clip " + std::to_string(r.clip) + " outside [-1, " + std::to_string(clip_count) + ")");
			if (r.clip == -1) {
				off_seen = true;
				continue;
			}
			if (off_seen) return fail(MBIK_EINVAL, sw + ": an on slot behind an off slot");
			if (!std::isfinite(r.pos) || !(r.pos >= 0) || !(r.pos <= clips[r.clip].length)) return fail(MBIK_EINVAL, sw + ": pos is not finite or outside [0, length]");
			if (!std::isfinite(r.speed)) return fail(MBIK_EINVAL, sw + ": speed is not finite");
			if (j > 0 && (!std::isfinite(r.blend_time) || !(r.blend_time > 0) || !std::isfinite(r.blend_left)))
				return fail(MBIK_EINVAL, sw + ": a fade needs a finite blend_time > 0 and a finite blend_left");
		}
	}
	return MBIK_OK;
}

// The records as the state stores them: an off slot is all +0 with clip -1, slot 0 has no fade fields.
mbik::PlaybackSlot stored(const mbik_playback_slot &r, int j) {
	if (r.clip == -1) return mbik::playback_off();
	return mbik::PlaybackSlot{r.pos, r.clip, r.speed, j ? r.blend_left : 0.0f, j ? r.blend_time : 0.0f};
}

// The checks of an advance past the object's own.
int check_advance(int32_t count, int32_t K, double delta, float speed_scale, const mbik_playback_cmd *cmds, int32_t cmd_count,
		const mbik_clip_layer *layers_out, const double *time_prev_out, const uint8_t *events_out) {
	if (!std::isfinite(delta)) return fail(MBIK_EINVAL, "delta is not finite");
	if (!std::isfinite(speed_scale)) return fail(MBIK_EINVAL, "speed_scale is not finite");
	if (cmd_count < 0) return fail(MBIK_EINVAL, "negative cmd_count");
	if (count == 0) return kNothingToDo;
	if (int rc = check_given(layers_out, "layers_out")) return rc;
	if (int rc = check_given(time_prev_out, "time_prev_out")) return rc;
	const bool with_cmds = cmd_count > 0; // cmds is not looked at without
	if (int rc = with_cmds ? check_given(cmds, "cmds") : MBIK_OK) return rc;
	if (int rc = check_aligned8(layers_out, "layers_out")) return rc;
	if (int rc = check_aligned8(time_prev_out, "time_prev_out")) return rc;
	if (int rc = with_cmds ? check_aligned8(cmds, "cmds") : MBIK_OK) return rc;
	const size_t per = (size_t)count * K, nl = per * sizeof(mbik_clip_layer), np = per * sizeof(double), ne = (size_t)count,
				 nc = (size_t)cmd_count * sizeof(mbik_playback_cmd);
	if (int rc = check_apart(layers_out, nl, "layers_out", time_prev_out, np, "time_prev_out")) return rc;
	if (int rc = events_out ? check_apart(layers_out, nl, "layers_out", events_out, ne, "events_out") : MBIK_OK) return rc;
	if (int rc = events_out ? check_apart(time_prev_out, np, "time_prev_out", events_out, ne, "events_out") : MBIK_OK) return rc;
	if (int rc = with_cmds ? check_apart(cmds, nc, "cmds", layers_out, nl, "layers_out") : MBIK_OK) return rc;
	if (int rc = with_cmds ? check_apart(cmds, nc, "cmds", time_prev_out, np, "time_prev_out") : MBIK_OK) return rc;
	if (int rc = with_cmds && events_out ? check_apart(cmds, nc, "cmds", events_out, ne, "events_out") : MBIK_OK) return rc;
	return 0;
}

int check_range(const mbik_playback *pb, int32_t first, int32_t n, const void *slots, const void *flags) {
	if (!pb) return fail(MBIK_EINVAL, "null playback object");
	if (first < 0 || n < 0 || (int64_t)first + n > pb->capacity)
		return fail(MBIK_EINVAL, "skeletons [" + std::to_string(first) + ", " + std::to_string((int64_t)first + n) + ") outside the capacity " + std::to_string(pb->capacity));
	if (n > 0 && (!slots || !flags)) return fail(MBIK_EINVAL, "null slots or flags");
	return MBIK_OK;
}

// One field of the state, slot j, skeletons [first, first + n): a contiguous run of the structure of arrays, from `dev`.
template <class T>
int copy_run(T *dev, int32_t n, T *host, bool to_device) {
	const hipError_t e = to_device ? hipMemcpy(dev, host, (size_t)n * sizeof(T), hipMemcpyHostToDevice)
									 : hipMemcpy(host, dev, (size_t)n * sizeof(T), hipMemcpyDeviceToHost);
	if (e != hipSuccess) return fail(MBIK_EHIP, std::string("hipMemcpy failed for the playback state: ") + hipGetErrorString(e));
	return MBIK_OK;
}

// The whole range, either way, through host copies of each run.
int copy_state(const mbik_playback *pb, int32_t first, int32_t n, mbik_playback_slot *slots, uint32_t *flags, bool to_device) {
	DeviceGuard guard(pb->device);
	const int32_t K = pb->K;
	std::vector<double> pos((size_t)n);
	std::vector<int32_t> clip((size_t)n);
	std::vector<float> speed((size_t)n), left((size_t)n), time((size_t)n);
	for (int32_t j = 0; j < K; j++) {
		if (to_device)
			for (int64_t s = 0; s < n; s++) {
				const mbik::PlaybackSlot r = stored(slots[s * K + j], j);
				pos[s] = r.pos, clip[s] = r.clip, speed[s] = r.speed, left[s] = r.blend_left, time[s] = r.blend_time;
			}
		if (int rc = copy_run(pb->st.pos(j, first), n, pos.data(), to_device)) return rc;
		if (int rc = copy_run(pb->st.clip(j, first), n, clip.data(), to_device)) return rc;
		if (int rc = copy_run(pb->st.speed(j, first), n, speed.data(), to_device)) return rc;
		if (int rc = copy_run(pb->st.blend_left(j, first), n, left.data(), to_device)) return rc;
		if (int rc = copy_run(pb->st.blend_time(j, first), n, time.data(), to_device)) return rc;
		if (!to_device)
			for (int64_t s = 0; s < n; s++) slots[s * K + j] = mbik_playback_slot{pos[s], clip[s], speed[s], left[s], time[s]};
	}
	return copy_run(pb->st.flags(first), n, flags, to_device);
}

} // namespace

extern "C" {

int32_t mbik_playback_create(mbik_clipset *set, int32_t capacity, int32_t layer_count, const mbik_playback_desc *desc, mbik_playback **out) {
	if (!out) return fail(MBIK_EINVAL, "null out");
	*out = nullptr;
	if (!set) return fail(MBIK_EINVAL, "null clip set");
	if (capacity < 0) return fail(MBIK_EINVAL, "negative capacity");
	if (int rc = check_layer_count(layer_count)) return rc;
	std::unique_ptr<mbik_playback> pb(new mbik_playback());
	if (int rc = clipset_clips(set, pb->device, pb->clips)) return rc;
	const int32_t cc = (int32_t)pb->clips.size();
	if (int rc = check_desc(cc, desc)) return rc;
	pb->capacity = capacity, pb->K = layer_count;
	DeviceGuard guard(pb->device);
	// the tables: clip infos, next, blend_times; a table the desc leaves out is an empty section and a null pointer
	const int32_t *next = desc ? desc->next : nullptr;
	const float *blend_times = desc ? desc->blend_times : nullptr;
	Blob t;
	const size_t o_info = t.add(pb->clips), o_next = t.add(next, next ? (size_t)cc * sizeof(int32_t) : 0),
				 o_bt = t.add(blend_times, blend_times ? (size_t)cc * cc * sizeof(float) : 0);
	if (int rc = t.upload(pb->tables, "the playback tables")) return rc;
	pb->tab = mbik::PlaybackTables{cc, desc ? desc->default_blend_time : 0.0f, t.at<mbik::ClipInfo>(o_info),
			next ? t.at<int32_t>(o_next) : nullptr, blend_times ? t.at<float>(o_bt) : nullptr};
	// the state: every slot off
	mbik::PlaybackState st{nullptr, ((int64_t)capacity + 3) & ~(int64_t)3, layer_count};
	const size_t s_bytes = st.bytes() + 16;
	std::vector<unsigned char> sb(s_bytes, 0);
	st.base = sb.data();
	for (int32_t j = 0; j < layer_count; j++)
		for (int64_t s = 0; s < st.stride; s++) *st.clip(j, s) = mbik::kClipLayerOff;
	if (int rc = pb->state.reserve(s_bytes, "hipMalloc failed for the playback state")) return rc;
	st.base = pb->state.as<unsigned char>();
	if (hipMemcpy(st.base, sb.data(), s_bytes, hipMemcpyHostToDevice) != hipSuccess) return fail(MBIK_EHIP, "hipMemcpy failed for the playback state");
	pb->st = st;
	*out = pb.release();
	return MBIK_OK;
}

void mbik_playback_destroy(mbik_playback *pb) { delete pb; }

int32_t mbik_playback_write(mbik_playback *pb, int32_t first, int32_t n, const mbik_playback_slot *slots, const uint32_t *flags) {
	if (int rc = check_range(pb, first, n, slots, flags)) return rc;
	if (n == 0) return MBIK_OK;
	if (int rc = check_state(pb->clips, n, pb->K, slots, flags)) return rc;
	return copy_state(pb, first, n, const_cast<mbik_playback_slot *>(slots), const_cast<uint32_t *>(flags), true);
}

int32_t mbik_playback_read(mbik_playback *pb, int32_t first, int32_t n, mbik_playback_slot *slots, uint32_t *flags) {
	if (int rc = check_range(pb, first, n, slots, flags)) return rc;
	if (n == 0) return MBIK_OK;
	return copy_state(pb, first, n, slots, flags, false);
}

int32_t mbik_playback_advance(mbik_playback *pb, int32_t count, double delta, float speed_scale, const mbik_playback_cmd *cmds, int32_t cmd_count,
		mbik_clip_layer *layers_out, double *time_prev_out, uint8_t *events_out, void *hip_stream) {
	if (!pb) return fail(MBIK_EINVAL, "null playback object");
	if (count < 0 || count > pb->capacity) return fail(MBIK_EINVAL, "count " + std::to_string(count) + " outside [0, " + std::to_string(pb->capacity) + "]");
	if (int rc = check_advance(count, pb->K, delta, speed_scale, cmds, cmd_count, layers_out, time_prev_out, events_out)) return settled(rc);
	return launched(pb->device, "playback advance", [&] {
		return mbik::launch_playback(reinterpret_cast<hipStream_t>(hip_stream), pb->tab, pb->st, count, pb->K, delta, speed_scale,
				reinterpret_cast<const mbik::PlaybackCmd *>(cmds), cmd_count, reinterpret_cast<mbik::ClipLayer *>(layers_out), time_prev_out, events_out);
	});
}

int32_t mbik_playback_advance_cpu(int32_t clip_count, const mbik_clip_desc *clips, const mbik_playback_desc *desc, int32_t count,
		int32_t layer_count, mbik_playback_slot *slots, uint32_t *flags, double delta, float speed_scale, const mbik_playback_cmd *cmds,
		int32_t cmd_count, mbik_clip_layer *layers_out, double *time_prev_out, uint8_t *events_out) {
	if (clip_count <= 0) return fail(MBIK_EINVAL, "a clip set needs at least one clip");
	if (!clips) return fail(MBIK_EINVAL, "null clips");
	std::vector<mbik::ClipInfo> info((size_t)clip_count);
	for (int32_t c = 0; c < clip_count; c++) {
		if (int rc = check_clip(clips[c], "clip " + std::to_string(c))) return rc;
		info[c] = mbik::ClipInfo{clips[c].length, clips[c].loop_mode, 0};
	}
	if (int rc = check_desc(clip_count, desc)) return rc;
	if (int rc = check_count(count)) return rc;
	if (int rc = check_layer_count(layer_count)) return rc;
	if (count > 0 && (!slots || !flags)) return fail(MBIK_EINVAL, "null slots or flags");
	if (int rc = check_state(info, count, layer_count, slots, flags)) return rc;
	if (int rc = check_advance(count, layer_count, delta, speed_scale, cmds, cmd_count, layers_out, time_prev_out, events_out)) return settled(rc);
	const mbik::PlaybackTables T{clip_count, desc ? desc->default_blend_time : 0.0f, info.data(), desc ? desc->next : nullptr,
			desc ? desc->blend_times : nullptr};
	mbik::PlaybackSlot *S = reinterpret_cast<mbik::PlaybackSlot *>(slots);
	mbik::ClipLayer *L = reinterpret_cast<mbik::ClipLayer *>(layers_out);
	for (int64_t s = 0; s < count; s++) {
		for (int32_t j = 0; j < layer_count; j++) {
			const mbik_playback_slot r = slots[s * layer_count + j];
			S[s * layer_count + j] = stored(r, j);
		}
		const uint32_t ev = mbik::playback_skeleton(T, mbik::PlaybackRecords{S + s * layer_count, flags + s}, layer_count, (int)s, delta, speed_scale,
				reinterpret_cast<const mbik::PlaybackCmd *>(cmds), cmd_count, mbik::PlaybackDirect{L + s * layer_count, time_prev_out + s * layer_count});
		if (events_out) events_out[s] = (uint8_t)ev;
	}
	return MBIK_OK;
}

} // extern "C"
