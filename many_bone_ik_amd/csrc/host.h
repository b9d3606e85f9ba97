// The host side of the C ABI (host_*.cpp): the plan and group objects behind mbik.h's opaque
// handles, and the internal functions the host translation units share (schedule, launch, errors).
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstddef>
#include <cstdint>
#include <cstring>
#include <initializer_list>
#include <memory>
#include <mutex>
#include <string>
#include <vector>

#include "kernels.h"

using mbik::CmodeState;
using mbik::DevPlan;
using mbik::GroupEntry;
using mbik::kCmodeMaxWaves;
using mbik::kHelpF4;
using mbik::kHelpRingBytes;
using mbik::kLocTile;
using mbik::kPrioDefault;
using mbik::kRowTile;
using mbik::node_area_floats;
using mbik::node_at;
using mbik::TopoSlice;
namespace mbik {
struct ClipInfo; // clip.h
}

namespace mbik_host {

// The calling thread's last error message (mbik_last_error) and the error-return helper.
extern thread_local std::string g_err;
int fail(int code, const std::string &msg);
// Puts the last error message back at the end of its scope, for a caller that asks a function
// which reports through fail() a question whose "no" is not the caller's failure.
struct KeepError {
	std::string saved = g_err;
	~KeepError() { g_err = saved; }
};

struct DeviceGuard {
	int prev = -1;
	explicit DeviceGuard(int dev) {
		if (hipGetDevice(&prev) != hipSuccess) prev = -1;
		if (prev != dev) (void)hipSetDevice(dev);
	}
	~DeviceGuard() {
		int cur = -1;
		if (prev >= 0 && hipGetDevice(&cur) == hipSuccess && cur != prev) (void)hipSetDevice(prev);
	}
};

// One hipMalloc allocation and its size, owned: freed with the object that holds it, on the device
// it was taken on.  The handles and every local scratch buffer of the host side own their device
// memory through it; the device-side views (DevPlan, CmodeState, SetupView, ClipView) hold raw
// pointers into these.
class DevBuf {
public:
	DevBuf() = default;
	DevBuf(DevBuf &&o) noexcept : p_(o.p_), bytes_(o.bytes_), device_(o.device_) { o.p_ = nullptr, o.bytes_ = 0; }
	DevBuf &operator=(DevBuf &&o) noexcept {
		std::swap(p_, o.p_), std::swap(bytes_, o.bytes_), std::swap(device_, o.device_);
		return *this;
	}
	~DevBuf() { reset(); }
	// Grow-only: leaves a buffer of at least `bytes` on the current device.  A larger one is
	// allocated before the old one is freed, and its contents are undefined.  Fails with
	// MBIK_ENOMEM and the text `what`, which names what was being allocated; the old buffer stays.
	int reserve(size_t bytes, const char *what);
	// reserve(), then a copy of `bytes` host bytes into the buffer (synchronous): MBIK_ENOMEM "hipMalloc failed for <what>" or
	// MBIK_EHIP "hipMemcpy failed for <what>".
	int upload(const void *src, size_t bytes, const std::string &what) {
		if (int rc = reserve(bytes, ("hipMalloc failed for " + what).c_str())) return rc;
		if (hipMemcpy(p_, src, bytes, hipMemcpyHostToDevice) != hipSuccess) return fail(MBIK_EHIP, "hipMemcpy failed for " + what);
		return MBIK_OK;
	}
	void reset();
	size_t bytes() const { return bytes_; }
	explicit operator bool() const { return p_ != nullptr; }
	template <class T>
	T *as() const { return static_cast<T *>(p_); }

private:
	void *p_ = nullptr;
	size_t bytes_ = 0;
	int device_ = 0;
};

// A table image for the device in the one format the clip set and the playback object use: sections, each from a 16-byte
// boundary, the gaps zero, 16 spare bytes behind the last.  An empty section takes no room: it shares its offset with the
// next one.
class Blob {
public:
	// Appends a section; its offset.
	size_t add(const void *src, size_t bytes) {
		const size_t off = up16(image_.size());
		image_.resize(off + bytes, 0);
		if (bytes) std::memcpy(image_.data() + off, src, bytes);
		return off;
	}
	template <class T>
	size_t add(const std::vector<T> &v) { return add(v.data(), v.size() * sizeof(T)); }
	// The image into `buf` on the current device (DevBuf::upload); at() then gives device pointers.
	int upload(DevBuf &buf, const std::string &what) {
		image_.resize(up16(image_.size()) + 16, 0);
		if (int rc = buf.upload(image_.data(), image_.size(), what)) return rc;
		base_ = buf.as<unsigned char>();
		return MBIK_OK;
	}
	template <class T>
	const T *at(size_t off) const { return reinterpret_cast<const T *>(base_ + off); }

private:
	static size_t up16(size_t n) { return (n + 15) & ~(size_t)15; }
	std::vector<unsigned char> image_;
	const unsigned char *base_ = nullptr;
};

// The layout settings a caller may pin (mbik_plan_set_*), saved with the plan, and what an
// autotune may change: an autotune that fails, or that times nothing, copies the caller's back.
struct LayoutPins {
	int lanes = 0, spw = 0, interval = 0; // mbik_plan_set_launch / mbik_plan_set_layout; 0 = automatic
	int staging = -1;                     // mbik_plan_set_heading_staging; -1 = automatic
	int locals = -1;                      // mbik_plan_set_locals_placement; -1 = automatic
	int waves = -1;                       // mbik_plan_set_waves_per_simd; -1 = automatic
	int helper = -1;                      // mbik_plan_set_helper_wave; -1 = automatic
	int roles = -1;                       // mbik_plan_set_wave_roles; -1 = automatic (off until autotuned)
	int cm_lanes = 0;                     // constraint_mode: lanes per skeleton (0 = auto)
	int cm_spw_div = 0;                   // constraint_mode: skeletons per wave = (64 / K) >> cm_spw_div
	bool operator==(const LayoutPins &o) const {
		return lanes == o.lanes && spw == o.spw && interval == o.interval && staging == o.staging && locals == o.locals &&
				waves == o.waves && helper == o.helper && roles == o.roles && cm_lanes == o.cm_lanes && cm_spw_div == o.cm_spw_div;
	}
};

// What the uploaded topology blob (mbik_plan::topo, with the lane schedule) was packed for.
struct BlobKey {
	int K = -1, interval = -1, staging = -1, placement = -1, roles = -1;
	bool operator==(const BlobKey &o) const {
		return K == o.K && interval == o.interval && staging == o.staging && placement == o.placement && roles == o.roles;
	}
};

} // namespace mbik_host

struct mbik_group {
	std::vector<mbik_plan *> plans; // not owned
	int device = 0;
	mbik_host::DevBuf d_plans, d_entries;
};

struct mbik_plan {
	mbik_plan() = default;
	mbik_plan(const mbik_plan &) = delete;
	mbik_plan &operator=(const mbik_plan &) = delete;
	~mbik_plan(); // the event and the host-mapped flag word; every buffer frees itself

	mbik::HostPlan host;
	int device = 0;
	mbik_host::LayoutPins pins;
	int cu_count = 256;
	DevPlan dev{};
	// device memory counted: the table uploads, locals, state, checkpoint globals, the tiled
	// tables, constraint_mode's node caches and dirty words, the fk schedule; not the topology
	// blob, the mbik_solve_host scratch or the flag word
	int64_t device_bytes = 0;
	double alg_bytes = 0;
	double alg_flops = 0;
	mbik_host::BlobKey blob_key;                         // layout of the uploaded topology blob (invalidate_layout)
	int tab64 = 0;                                       // mbik_plan_set_table_addressing
	// tables uploaded once and never resized: D / CF / CD, constraint_mode's pre-order tables, the
	// setup view's (mbik_plan_rebuild_setup); dev, cm and dsetup point into them
	std::vector<mbik_host::DevBuf> uploads;
	mbik_host::DevBuf locals;                            // [N][B][12] for state_hbm 1
	mbik_host::DevBuf state;                             // [N][state stride] for state_hbm 2
	mbik_host::DevBuf gtile;                             // state_hbm 2: checkpoint globals, skeleton-tiled
	mbik_host::DevBuf topo; // topology blob (includes the lane schedule)
	// scratch for mbik_solve_host
	mbik_host::DevBuf h_in, h_tg, h_out;
	size_t scratch_skel = 0;
	// device copies of the setup tables (mbik_plan_rebuild_setup)
	mbik::SetupView dsetup{};
	bool dsetup_ready = false;
	// constraint_mode: the persistent IKNode3D caches (cmode.h)
	CmodeState cm{};
	mbik_host::DevBuf cm_node, cm_dirty;
	// the creation inputs, for mbik_plan_save (the topology is rebuilt from them on load)
	std::vector<int32_t> src_parents;
	std::vector<mbik_pin> src_pins;
	std::vector<mbik_constraint> src_cons;
	std::vector<float> src_bone_damp;
	int32_t src_max_cones = 1;
	mbik_config src_cfg{};
	bool setup_on_device = false; // mbik_plan_create_device: the setup pose given to finish_plan is a device buffer
	// skeleton-tiled copies of D / CF / CD for launches with the whole state in device memory
	// (DevPlan::row_at); rebuilt when the tables changed since (tables_version)
	mbik_host::DevBuf Dt, CFt, CDt;
	int tables_version = 1, tiled_version = 0;
	// the tiling's completion, for launches on another stream than the one that tiled
	hipEvent_t tile_ev = nullptr;
	hipStream_t tile_stream = nullptr;
	bool tile_pending = false;
	// helper-wave timeouts (DevPlan::help_flag): the plan's own host-mapped flag word, which a
	// launch's kernel sets and the plan's next call reports (take_helper_timeout); the deadline
	// override of mbik_plan_debug_helper (0: kHelpTimeoutMs)
	unsigned int *help_flag = nullptr;
	int help_timeout_us = 0;
	// mbik_pose_globals: the device copy of the depth-ordered bone schedule (kernels.h launch_fk), built
	// from src_parents / src_pins on the first call
	mbik_host::DevBuf fk_sched;
	int fk_levels = 0;
#ifdef MBIK_REPLAY
	mbik_host::DevBuf rec_dump; // mbik_debug_replay's records (DevPlan::rec_dump)
#endif
};

// One mesh surface on one device (host_skin.cpp creates it; host_bounds.cpp reads its bone boxes).
struct mbik_mesh {
	int device = 0, cu_count = 256;
	int32_t B = 0, V = 0, K = 4;
	bool normals = false;
	bool tangents = false;           // (mbik_mesh_create_desc)
	int32_t P = 0, mode = 0;         // shapes (P == 0: a mesh without)
	mbik_host::DevBuf mesh;          // skin_layout()'s planes, then morph_layout()'s, then tangent_layout()'s
	// the bone boxes (bounds.h): host copies for mbik_mesh_bone_boxes, and the used bones' records on the device
	std::vector<float> bone_boxes;   // [B][6]
	std::vector<uint8_t> bone_used;  // [B]
	int32_t used_bones = 0;
	mbik_host::DevBuf bone_table;    // [used_bones] 32-byte records (bone_table_pack)
	mbik_host::DevBuf cull_totals;   // mbik_cull_boxes' block counts (mbik_cull_lod's, a row a range); grows with the largest count seen
	mbik_host::DevBuf lod_member;    // mbik_cull_lod's member bytes, one a skeleton; grows likewise
};

namespace mbik_host {

// MBIK_OK, or MBIK_ENODEV "no HIP device visible" / MBIK_EINVAL with `out_of_range`.
int check_device(int device, const char *out_of_range = "device index out of range");
// The device's compute units (256 where the query fails).
int cu_count_of(int device);
// Whether the byte ranges [a, a + na) and [b, b + nb) share a byte.
inline bool overlap(const void *a, size_t na, const void *b, size_t nb) {
	const uintptr_t x = reinterpret_cast<uintptr_t>(a), y = reinterpret_cast<uintptr_t>(b);
	return x < y + nb && y < x + na;
}

// The mesh checks mbik_mesh_create and the _cpu entries share (skin.h's skin_check_mesh with its error text; host_skin.cpp).
int check_mesh(int32_t B, int32_t V, int32_t K, const float *positions, const int32_t *bone_indices, const float *weights);

// device-memory areas addressed through buffer resources (32-bit byte offsets): the state of
// placements 1 and 2, and the setup tables of every layout that can (kTab32 / kTabTiled)
constexpr size_t kMaxBufBytes = 0xFFFFFFF0u;
bool tables_fit_32(const mbik_plan *p);
int take_helper_timeout(mbik_plan *p);
// Resident one-wave blocks per CU at a block LDS size (ctx: the plan), for build_schedule.
int blocks_per_cu(void *ctx, int64_t lds_bytes);
// A setter changed a pin: the next ensure_schedule packs and uploads the topology blob again.
inline void invalidate_layout(mbik_plan *p) { p->blob_key = BlobKey{}; }
// pins -> LayoutRequest -> build_schedule -> (buffers, topology blob) for a launch of nlaunch skeletons.
int ensure_schedule(mbik_plan *p, int64_t nlaunch);

// One solve launch of the plan's current layout (ensure_schedule), resolved: the only place that
// picks the kernel, the grid and the LDS.  launch(), mbik_plan_get_info, mbik_group_solve and the
// autotune read it.
struct SolveLaunch {
	bool cmode = false;                // which handle the launch takes: cm (constraint_mode) or solve
	mbik::SolveKernel solve = nullptr;
	mbik::CmodeKernel cm = nullptr;
	unsigned blocks = 0, threads = 64;
	size_t lds_bytes = 0;              // the launch's dynamic LDS
	// What mbik_plan_get_info reports as lds_bytes_per_block.  constraint_mode: lds_bytes.  Else
	// build_schedule's figure for its last launch size (HostPlan::lds_block_bytes): the classic
	// block before the blob was packed, without the helper ring.  Kept as reported so far.
	int64_t schedule_lds_bytes = 0;
	int skeletons_per_block = 0;
	int cm_spw = 0, cm_wpb = 0;        // constraint_mode: skeletons per wave, waves per block (CmodeState)
	bool wave_roles = false;           // a wave per role (either kernel family)
	bool helper = false;               // the helper-wave kernel (128 threads, or 64 when replaying)
	bool needs_flag = false;           // the kernel reports a handshake timeout: the plan's flag word (ensure_help_flag)
	bool tiled_rows = false;           // the kernel reads the skeleton-tiled D / CF / CD (ensure_tiled_rows)
};
// MBIK_OK, or the refusal of a block that exceeds the LDS (MBIK_EUNSUPPORTED) or of an impossible
// role count (MBIK_EINVAL).  No allocation, no HIP call.  replay: MBIK_REPLAY's DevPlan::replay.
int resolve_launch(const mbik_plan *p, int64_t count, SolveLaunch &out, int replay = 0);

// One solve of skeletons [first, first + count); nonfinite and replay reach the kernel through a
// copy of the plan's DevPlan / CmodeState: a launch leaves the plan's own as they were.
struct LaunchArgs {
	int first, count;
	const float *pose_in, *targets;
	float *pose_out;
	hipStream_t stream;
	int iterations, seg_lo, seg_hi;
	unsigned char *nonfinite = nullptr;
	int replay = 0;
};
// The whole-skeleton solve of mbik_solve (every iteration, every segment).
LaunchArgs full_solve(const mbik_plan *p, int first, int count, const float *pose_in, const float *targets, float *pose_out, hipStream_t stream);
int launch(mbik_plan *p, const LaunchArgs &a);

// constraint_mode state in device memory and in a plan file: node caches, then dirty words
size_t cmode_node_bytes(const mbik::HostPlan &h);
size_t cmode_dirty_bytes(const mbik::HostPlan &h);
size_t cmode_file_node_bytes(const mbik::HostPlan &h);
std::vector<float> cmode_nodes_tiled(const mbik::HostPlan &h, const float *plain);
void cmode_nodes_plain(const mbik::HostPlan &h, const float *tiled, float *plain);

// ---- the pieces the animation and mesh entries (host_clip.cpp, host_playback.cpp, host_skin.cpp, host_bounds.cpp) compose their call
// checks from ----
// A call check returns 0 to go on, kNothingToDo for a call that is valid and empty, or a refusal (< 0); settled() is what
// the entry returns for the last two.  Each piece is MBIK_OK or its refusal, and builds its text only when it refuses.
constexpr int kNothingToDo = 1;
inline int settled(int rc) { return rc < 0 ? rc : MBIK_OK; }
inline int check_count(int32_t count) { return count < 0 ? fail(MBIK_EINVAL, "negative count") : MBIK_OK; }
int check_layer_count(int32_t layer_count); // [1, MBIK_CLIP_MAX_LAYERS]
inline int check_flags(uint32_t flags, uint32_t known) {
	return flags & ~known ? fail(MBIK_EINVAL, "unknown flags " + std::to_string(flags)) : MBIK_OK;
}
inline int check_given(const void *p, const char *name) { return p ? MBIK_OK : fail(MBIK_EINVAL, std::string("null ") + name); }
inline int check_aligned8(const void *p, const char *name) {
	return reinterpret_cast<uintptr_t>(p) % 8 ? fail(MBIK_EINVAL, std::string(name) + " is not 8-byte aligned") : MBIK_OK;
}
inline int check_apart(const void *in, size_t n_in, const char *in_name, const void *out, size_t n_out, const char *out_name) {
	return overlap(in, n_in, out, n_out) ? fail(MBIK_EINVAL, std::string(out_name) + " overlaps " + in_name) : MBIK_OK;
}
// A buffer of a call by its name in the entry's signature; a null one is in nobody's way.
struct Range {
	const void *p;
	size_t n;
	const char *name;
};
// Every output apart from every input and from the outputs in front of it, an output at a time: "<output> overlaps <other>".
inline int check_disjoint(std::initializer_list<Range> outputs, std::initializer_list<Range> inputs) {
	for (const Range *o = outputs.begin(); o != outputs.end(); o++) {
		if (!o->p) continue;
		for (const Range &i : inputs)
			if (i.p)
				if (int rc = check_apart(i.p, i.n, i.name, o->p, o->n, o->name)) return rc;
		for (const Range *q = outputs.begin(); q != o; q++)
			if (q->p)
				if (int rc = check_apart(q->p, q->n, q->name, o->p, o->n, o->name)) return rc;
	}
	return MBIK_OK;
}
// What a launch's error becomes: MBIK_EHIP "<what> launch failed: <HIP's text>".
inline int launch_result(hipError_t e, const char *what) {
	return e == hipSuccess ? MBIK_OK : fail(MBIK_EHIP, std::string(what) + " launch failed: " + hipGetErrorString(e));
}
// The tail of a device entry: launch() with `device` current.
template <class Launch>
int launched(int device, const char *what, Launch launch) {
	DeviceGuard guard(device);
	return launch_result(launch(), what);
}
// A clip's length and loop mode (mbik_clipset_create's test; `where`: "clip <c>").
int check_clip(const mbik_clip_desc &d, const std::string &where);

// What a playback object takes from a clip set at its creation (host_clip.cpp): the set's device and each clip's
// length and loop mode, read back from the set's tables.
int clipset_clips(const mbik_clipset *set, int &device, std::vector<mbik::ClipInfo> &clips);

// plan creation (host_plan.cpp)
int read_options(const mbik_plan_options *opts, int &libm);
void keep_inputs(mbik_plan *p, const mbik_skeleton_desc &desc, const mbik_config &cfg);
int finish_plan(mbik_plan *p, const float *setup_pose, const void *cm_state);

} // namespace mbik_host
