// The C ABI's core (include/mbik.h): plan creation and upload, the launch layout
// (ensure_schedule), kernel selection and launch, the solve entry points, groups, target capture
// and the layout setters.  Replaces the reference's ManyBoneIK3D::_bone_list_changed
// (many_bone_ik_3d.cpp:1011-1068) and the per-frame _process_modification (:645-694) with its
// pose capture / write-back (:91-116); DESIGN.md §2.
#include "host.h"

#include "gd_math.h"

using namespace gd;
using namespace mbik_host;

namespace mbik_host {
thread_local std::string g_err;
int fail(int code, const std::string &msg) {
	g_err = msg;
	return code;
}

int DevBuf::reserve(size_t bytes, const char *what) {
	if (p_ && bytes <= bytes_) return MBIK_OK;
	void *a = nullptr;
	if (hipMalloc(&a, bytes) != hipSuccess) return fail(MBIK_ENOMEM, what);
	reset();
	p_ = a;
	bytes_ = bytes;
	if (hipGetDevice(&device_) != hipSuccess) device_ = 0;
	return MBIK_OK;
}
void DevBuf::reset() {
	if (p_) {
		DeviceGuard guard(device_);
		(void)hipFree(p_);
	}
	p_ = nullptr;
	bytes_ = 0;
}

int check_device(int device, const char *out_of_range) {
	int ndev = 0;
	if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) return fail(MBIK_ENODEV, "no HIP device visible");
	if (device < 0 || device >= ndev) return fail(MBIK_EINVAL, out_of_range);
	return MBIK_OK;
}
int cu_count_of(int device) {
	int cus = 0;
	return hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, device) == hipSuccess && cus > 0 ? cus : 256;
}

// Grows one of the plan's counted buffers (mbik_plan::device_bytes follows its size).
static int reserve_counted(mbik_plan *p, DevBuf &b, size_t bytes, const char *what) {
	const size_t old = b.bytes();
	if (int rc = b.reserve(bytes, what)) return rc;
	p->device_bytes += (int64_t)b.bytes() - (int64_t)old;
	return MBIK_OK;
}

template <typename T>
int upload(mbik_plan *p, const std::vector<T> &v, const T *&dst) {
	DevBuf b;
	if (int rc = reserve_counted(p, b, std::max<size_t>(1, v.size()) * sizeof(T), "hipMalloc failed for plan table")) return rc;
	if (!v.empty() && hipMemcpy(b.as<void>(), v.data(), v.size() * sizeof(T), hipMemcpyHostToDevice) != hipSuccess)
		return fail(MBIK_EHIP, "hipMemcpy failed for plan table");
	dst = b.as<const T>();
	p->uploads.push_back(std::move(b));
	return MBIK_OK;
}

// Packs the topology tables (and the schedule for the current lane count) into one blob.
int upload_topology(mbik_plan *p) {
	const mbik::HostPlan &h = p->host;
	DevPlan &d = p->dev;
	std::vector<uint32_t> blob;
	auto add = [&](const void *data, size_t bytes, size_t align_words, int &off) {
		while (blob.size() % align_words) blob.push_back(0);
		off = (int)blob.size();
		size_t w = (bytes + 3) / 4;
		blob.resize(blob.size() + std::max<size_t>(w, 1), 0);
		if (bytes) std::memcpy(blob.data() + off, data, bytes);
	};
	std::vector<int4> rows(h.sched.size());
	for (size_t i = 0; i < rows.size(); i++) {
		// .w: the SCHED_* bits, and above bit 8 the row's longest segment in bone-steps (row_steps)
		const int nq = mbik::row_max_steps(h, (int)(i / (size_t)h.K));
		// (and SCHED_ROOT4, which only this copy carries)
		const int root4 = mbik::row_is_root4(h, (int)(i / (size_t)h.K)) ? mbik::SCHED_ROOT4 : 0;
		rows[i] = make_int4(h.sched[i].seg, h.sched[i].j, h.sched[i].m, h.sched[i].flags | root4 | (nq << 8));
	}
	// the rows' step classes follow the schedule (HostPlan::step_class; solve_block.h row_classes):
	// no table pointer of their own, so DevPlan -- every solve kernel's argument -- keeps its size
	for (size_t i = 0; i < h.step_class.size(); i += 4) {
		auto w = [&](size_t j) { return j < h.step_class.size() ? h.step_class[j] : 0; };
		rows.push_back(make_int4(w(i), w(i + 1), w(i + 2), w(i + 3)));
	}
	add(rows.data(), rows.size() * sizeof(int4), 4, d.o_sched);
#define MBIK_ADD(T, name) \
	if (std::string(#name) != "sched") add(h.name.data(), h.name.size() * sizeof(h.name[0]), sizeof(T) >= 16 ? 4 : (sizeof(T) >= 8 ? 2 : 1), d.o_##name);
	MBIK_TOPO_TABLES(MBIK_ADD)
#undef MBIK_ADD
	while (blob.size() % 4) blob.push_back(0);
	p->topo.reset(); // (exactly the blob's size: a smaller one may follow a larger)
	if (int rc = p->topo.reserve(blob.size() * 4, "hipMalloc topology blob")) return rc;
	if (hipMemcpy(p->topo.as<void>(), blob.data(), blob.size() * 4, hipMemcpyHostToDevice) != hipSuccess)
		return fail(MBIK_EHIP, "hipMemcpy topology blob");
	d.topo_blob = p->topo.as<const uint4>();
	d.topo_words = (int)blob.size();
	// diagnostics (tools/topo_const.py): the blob's table offsets, for a timing-only build that
	// compiles one plan's offsets in (solve_block.h MBIK_TOPO_CONST)
	if (getenv("MBIK_DEBUG_TOPO_OFFSETS")) {
#define MBIK_PRINT(T, name) fprintf(stderr, "MBIK_TC %s %d\n", #name, d.o_##name);
		MBIK_TOPO_TABLES(MBIK_PRINT)
#undef MBIK_PRINT
		fprintf(stderr, "MBIK_TC_K %d\n", h.K);
	}
	return MBIK_OK;
}

// Every setup table (D, CF, CD, and their skeleton-tiled copies, sized for the padded N) below
// 4 GiB: the solve can address them with 32-bit offsets.  Placement-0 plans beyond that run
// the 64-bit-index instantiation; placements 1 and 2 require it.
bool tables_fit_32(const mbik_plan *p) {
	const mbik::HostPlan &h = p->host;
	if (p->tab64) return false;
	const size_t n = h.padded_n();
	return h.d_floats(n) * sizeof(float) <= kMaxBufBytes && h.cf_floats(n) * sizeof(float) <= kMaxBufBytes &&
			h.cd_doubles(n) * sizeof(double) <= kMaxBufBytes;
}
// The solve kernel instantiation of a plan's current layout (stabilization x locals placement
// x waves per SIMD, and for placement 0 the table addressing): k_solve_w1.hip, k_solve_w2.hip,
// k_solve_rw.hip.  Never the helper-wave kernel: resolve_launch swaps that in.
static mbik::SolveKernel solve_kernel_for(const mbik_plan *p) {
	const mbik::HostPlan &h = p->host;
	if (h.wave_roles) return mbik::solve_kernel_rw(h.K, h.waves_per_simd, p->dev.prio_mask);
	const int pl = std::min(2, std::max(0, (int)h.state_hbm));
	const bool two = h.waves_per_simd == 2 && h.stabilization_passes == 0;
	// placement 0 with tables of 4 GiB or more: 64-bit element indices
	const bool t32 = !(pl == 0 && !tables_fit_32(p));
	if (two) return mbik::solve_kernel_w2(pl, t32, h.has_xs, p->dev.prio_mask);
	return mbik::solve_kernel_w1(h.stabilization_passes > 0, pl, t32, p->dev.prio_mask);
}

// A classic block's LDS: its spw skeletons' state and one copy of the topology blob.
static size_t block_lds_bytes(const mbik_plan *p) {
	return ((size_t)p->host.spw * p->dev.lds_stride + p->dev.topo_words) * sizeof(float);
}

// Whether a launch of the plan's current layout runs with the helper wave
// (mbik_solve_kernel_help): asked for, and a layout it serves -- state in LDS, no
// stabilization, one wave per SIMD, 32-bit tables -- whose block LDS still fits with the ring.
static bool helper_on(const mbik_plan *p) {
	const mbik::HostPlan &h = p->host;
	if (p->pins.helper != 1) return false;
	// (packed levels run row by row there: both waves walk the same rows)
	if (h.state_hbm != 0 || h.stabilization_passes != 0 || h.waves_per_simd != 1 || h.constraint_mode || !tables_fit_32(p)) return false;
	return block_lds_bytes(p) + kHelpRingBytes <= (size_t)mbik::kLdsBytes;
}

// The helper wave's handshake deadline: a wait gives up when the awaited counter has not moved
// for this long.  A real wait lasts at most one iteration of the partner wave (under a
// millisecond at the BASELINE sizes, tens of milliseconds for a 4,096-bone chain).
constexpr int kHelpTimeoutMs = 2000;
// A helper-wave launch needs the plan's timeout flag and the deadline in wall-clock ticks.
int ensure_help_flag(mbik_plan *p) {
	if (!p->help_flag) {
		void *h = nullptr;
		if (hipHostMalloc(&h, sizeof(unsigned int), hipHostMallocMapped | hipHostMallocCoherent) != hipSuccess)
			return fail(MBIK_ENOMEM, "hipHostMalloc helper timeout flag");
		p->help_flag = static_cast<unsigned int *>(h);
		*p->help_flag = 0u;
		void *d = nullptr;
		if (hipHostGetDevicePointer(&d, h, 0) != hipSuccess) return fail(MBIK_EHIP, "hipHostGetDevicePointer");
		p->dev.help_flag = static_cast<unsigned int *>(d);
	}
	int khz = 0;
	if (hipDeviceGetAttribute(&khz, hipDeviceAttributeWallClockRate, p->device) != hipSuccess || khz <= 0) khz = 100000;
	const uint64_t us = p->help_timeout_us > 0 ? (uint64_t)p->help_timeout_us : (uint64_t)kHelpTimeoutMs * 1000u;
	p->dev.help_timeout = (uint64_t)khz * us / 1000u;
	return MBIK_OK;
}
// Reports (once) a helper-wave timeout of an earlier launch of this plan: its skeletons were
// written as failures (write_help_timeout) and flagged non-finite.  The asynchronous calls report
// it on the plan's next call; the synchronous ones right after their own launch.
int take_helper_timeout(mbik_plan *p) {
	// one exchange: a still-running launch that sets the flag between a load and a clear would
	// otherwise have its timeout cleared unreported
	if (!p->help_flag || __atomic_exchange_n(p->help_flag, 0u, __ATOMIC_ACQ_REL) == 0u) return MBIK_OK;
	return fail(MBIK_EHIP, "helper wave: a launch of this plan timed out in the two-wave handshake; its skeletons "
						   "were written as failures (identity rotation, NaN position) and flagged non-finite");
}

// Resident one-wave blocks per CU for a block's LDS size, from the runtime's occupancy
// query on the kernel instantiation the plan launches (LDS granularity and registers).
// Deliberately the classic or wave-roles kernel of the layout at 64 threads, also where the
// launch runs the helper-wave kernel or K waves per block: build_schedule's choice of skeletons
// per block and checkpoint interval depends on this answer, so changing the query changes layouts.
int blocks_per_cu(void *ctx, int64_t lds_bytes) {
	const mbik_plan *p = static_cast<const mbik_plan *>(ctx);
	int n = 0;
	const void *k = (const void *)solve_kernel_for(p);
	if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&n, k, 64, (size_t)lds_bytes) != hipSuccess || n <= 0)
		return (int)(mbik::kLdsBytes / std::max<int64_t>(1, lds_bytes));
	return n;
}

// constraint_mode lanes per skeleton without a measurement: at most 4.  Its bone-steps are
// cheap and its state lives in HBM, so the chip's VALU issue (many narrow waves), not one
// skeleton's chain, bounds it beyond that (C2 / C3 / C5: DESIGN.md §1, profiles/r01_cmode_lanes_sweep.jsonl).
constexpr int kCmodeLanes = 4;
// The constraint_mode wave-roles block's LDS: the topology (topo_bytes), the pre-order tables, the
// dirty words of its spw skeletons, then per wave the chain stacks and pending cleanings, and the
// flags.  ensure_schedule bounds it from the host plan alone (topology_bytes: the blob's upper
// bound); a launch has the uploaded blob's size (cmode_lds_bytes).
static int64_t cmode_rw_lds(const mbik::HostPlan &h, int64_t topo_bytes, int64_t spw) {
	return topo_bytes + (2 * (int64_t)h.B + spw * 4 * h.cm_dirty_words() + (int64_t)h.K * 64 * h.cm_maxd + (int64_t)h.K * 4 * 64 + 64) * 4;
}

// constraint_mode block LDS (cmode.h): the topology blob and pre-order tables once per block;
// per wave the dirty words of its spw skeletons, and per lane the chain stack and, with
// stabilization, the target-heading origins.
static size_t cmode_wave_words(const mbik_plan *p, int spw) {
	const mbik::HostPlan &h = p->host;
	return (size_t)spw * 4 * p->cm.W + 64 * ((size_t)p->cm.maxd + (h.stabilization_passes > 0 ? 3 * (size_t)h.P : 0));
}
// constraint_mode launch shape: spw skeletons per wave (cm_spw_div halves 64 / K that many
// times), and as many waves per block (<= kCmodeMaxWaves) as share the block's LDS within
// kLdsBytes and leave the launch with at least one block per CU.
struct CmShape {
	int spw, wpb;
};
static CmShape cmode_shape_of(const mbik_plan *p, int64_t count) {
	const mbik::HostPlan &h = p->host;
	if (h.cm_roles) // wave roles: a block is K waves x spw skeletons (64, halved cm_spw_div times)
		return CmShape{p->pins.spw > 0 ? std::min(64, p->pins.spw) : std::max(1, 64 >> std::max(0, p->pins.cm_spw_div)), 1};
	const int full = 64 >> h.log2K;
	const int spw = p->pins.spw > 0 ? std::min(full, p->pins.spw) : std::max(1, full >> std::max(0, p->pins.cm_spw_div));
	int wpb = kCmodeMaxWaves;
	const size_t fixed = (size_t)p->dev.topo_words + 2 * (size_t)h.B;
	while (wpb > 1 && ((fixed + (size_t)wpb * cmode_wave_words(p, spw)) * sizeof(float) > (size_t)mbik::kLdsBytes ||
							  (size_t)(count + (int64_t)wpb * spw - 1) / ((size_t)wpb * spw) < (size_t)p->cu_count))
		wpb >>= 1;
	return CmShape{spw, wpb};
}
static size_t cmode_lds_bytes(const mbik_plan *p, CmShape sh) {
	const mbik::HostPlan &h = p->host;
	if (h.cm_roles) return (size_t)cmode_rw_lds(h, (int64_t)p->dev.topo_words * 4, sh.spw);
	return ((size_t)p->dev.topo_words + 2 * (size_t)h.B + (size_t)sh.wpb * cmode_wave_words(p, sh.spw)) * sizeof(float);
}

// The pins resolved to what build_schedule is asked for: decisions only, no device allocation and
// no HIP call.  It does write p->host: the role-count probe is a whole build_schedule (without the
// occupancy query) of which only K is read, and the build that follows in ensure_schedule_as
// overwrites the rest.  A refusal returns before that build, so the plan keeps the launch shape
// of its last successful ensure_schedule (or the probe's), not the refused one.
// roles_ok false: the classic layout even where wave roles are asked for (ensure_schedule_as).
static int request_for(mbik_plan *p, int64_t nlaunch, bool roles_ok, mbik::LayoutRequest &rq) {
	mbik::HostPlan &h = p->host;
	rq = mbik::LayoutRequest{};
	rq.lanes = p->pins.lanes;
	rq.spw = p->pins.spw;
	rq.interval = p->pins.interval;
	if (rq.lanes == 0 && h.constraint_mode && p->pins.cm_lanes > 0) rq.lanes = p->pins.cm_lanes;
	rq.staging = p->pins.staging < 0 ? 1 : p->pins.staging;
	rq.state_hbm = h.constraint_mode ? 0 : std::max(0, p->pins.locals);
	rq.waves_per_simd = (p->pins.waves == 2 && !h.constraint_mode && h.stabilization_passes == 0) ? 2 : 1;
	// Wave roles (mbik_plan_set_wave_roles): the whole state in device memory, one wave per role
	// (K = 2, 4 or 8 waves per block; 8 only at two waves per SIMD), no stabilization, 32-bit tables.
	if (roles_ok && p->pins.roles == 1 && !h.constraint_mode && h.stabilization_passes == 0 && tables_fit_32(p)) {
		const int cap = 4 * rq.waves_per_simd;
		int roles = std::min(rq.lanes, cap);
		if (roles == 0) {
			mbik::LayoutRequest widest;
			widest.interval = p->pins.interval;
			mbik::build_schedule(h, widest, nlaunch, nullptr, nullptr, p->cu_count);
			roles = std::min(h.K, cap);
		}
		// one role is the classic layout with 64 skeletons per wave: no wave roles then
		if (roles >= 2) {
			rq.lanes = roles;
			rq.state_hbm = 2;
			rq.staging = 0;
			rq.wave_roles = 1;
		}
	}
	// constraint_mode with wave roles (cmode.h mbik_cmode_kernel_rw): K = 2, 4 or 8 waves per block
	if (roles_ok && h.constraint_mode && p->pins.roles == 1 && h.stabilization_passes == 0 && tables_fit_32(p) &&
			cmode_node_bytes(h) < (size_t(1) << 32)) {
		int roles = 1;
		while (roles < (rq.lanes > 0 ? rq.lanes : kCmodeLanes)) roles <<= 1;
		roles = std::min(8, roles);
		if (roles >= 2) {
			rq.lanes = roles;
			rq.cm_roles = 1;
		}
	}
	if (rq.state_hbm >= 1 && !tables_fit_32(p))
		return fail(MBIK_EUNSUPPORTED, "state placements 1 and 2 need every setup table < 4 GiB (fewer skeletons per plan)");
	// split-exchange (staging 4 / 5) runs in the 32-bit-table two-wave builds; the 64-bit-index
	// two-wave build solves those segments alone (4 -> 0) or staged (5 -> 2)
	if (rq.waves_per_simd == 2 && !tables_fit_32(p) && rq.staging >= 4) rq.staging = rq.staging == 4 ? 0 : 2;
	return MBIK_OK;
}

// The placement buffers grow with the layouts a plan has run.  Placements 1 and 2: the bone locals
// (reserved before the schedule is built, as ever: a wave-roles request that falls back to the
// classic layout has them counted in device_bytes all the same).
static int reserve_locals(mbik_plan *p, int state_hbm) {
	const mbik::HostPlan &h = p->host;
	if (state_hbm >= 1 && !p->locals) {
		// LocTiled: whole tiles of kLocTile skeletons
		const size_t bytes = (size_t)((h.N + kLocTile - 1) / kLocTile) * kLocTile * h.B * 12 * sizeof(float);
		if (int rc = reserve_counted(p, p->locals, bytes, "hipMalloc locals")) return rc;
		p->dev.Lg = p->locals.as<float>();
		p->dev.lg_bytes = (uint32_t)std::min<size_t>(bytes, 0xFFFFFFFFu); // (placement 2 refuses > kMaxBufBytes)
	}
	return MBIK_OK;
}
// Placement 2, once the schedule says how many checkpoints a skeleton keeps.
static int reserve_state(mbik_plan *p) {
	const mbik::HostPlan &h = p->host;
	if (h.state_hbm == 2) {
		// the whole state in device memory: one skeleton's LDS layout per skeleton (the locals
		// and the checkpoint globals live in skeleton-tiled areas, d_locals and d_gtile)
		const int stride = (mbik::state_floats_per_skeleton(h) - 12 * h.B - 12 * h.n_gck + 3) & ~3;
		const size_t need = (size_t)h.N * stride;
		const size_t gneed = (size_t)((h.N + kLocTile - 1) / kLocTile) * kLocTile * (size_t)std::max(1, h.n_gck) * 12;
		if (need * sizeof(float) > kMaxBufBytes || p->dev.lg_bytes > kMaxBufBytes || gneed * sizeof(float) > kMaxBufBytes)
			return fail(MBIK_EUNSUPPORTED, "solve state in device memory needs < 4 GiB per area (fewer skeletons per plan)");
		if (int rc = reserve_counted(p, p->gtile, gneed * sizeof(float), "hipMalloc checkpoint globals")) return rc;
		p->dev.Gg = p->gtile.as<float>();
		p->dev.gg_bytes = (uint32_t)p->gtile.bytes();
		if (int rc = reserve_counted(p, p->state, need * sizeof(float), "hipMalloc state")) return rc;
		p->dev.Sg = p->state.as<float>();
		p->dev.sg_bytes = (uint32_t)p->state.bytes();
		p->dev.state_stride = stride;
	}
	return MBIK_OK;
}

// Packs and uploads the topology blob unless the one on the device was packed for this layout.
static int upload_blob(mbik_plan *p) {
	const mbik::HostPlan &h = p->host;
	const BlobKey key{h.K, h.g_interval, h.staging, h.state_hbm, h.wave_roles | h.cm_roles << 1};
	if (p->blob_key == key && p->topo) {
		p->dev.spw = h.spw;
		return MBIK_OK;
	}
	if (int rc = upload_topology(p)) return rc;
	p->blob_key = key;
	p->dev.nrows = h.nrows;
	p->dev.K = h.K;
	p->dev.log2K = h.log2K;
	p->dev.spw = h.spw;
	p->dev.hs_floats = h.hs_floats;
	p->dev.rw_xslots = h.rw_xslots;
	p->dev.n_gck = h.n_gck;
	p->dev.lds_stride = (mbik::lds_floats_per_skeleton(h) + 3) & ~3;
	return MBIK_OK;
}

static int ensure_schedule_as(mbik_plan *p, int64_t nlaunch, bool roles_ok) {
	mbik::HostPlan &h = p->host;
	mbik::LayoutRequest rq;
	if (int rc = request_for(p, nlaunch, roles_ok, rq)) return rc;
	if (int rc = reserve_locals(p, rq.state_hbm)) return rc;
	mbik::build_schedule(h, rq, nlaunch, blocks_per_cu, p, p->cu_count);
	if (rq.lanes == 0 && h.constraint_mode && h.K > kCmodeLanes && !h.cm_roles) {
		rq.lanes = kCmodeLanes;
		mbik::build_schedule(h, rq, nlaunch, blocks_per_cu, p, p->cu_count);
	}
	// A wave-roles block holds the topology, the non-finite flags and, with cooperative rows, the
	// block's targets and the effector-global exchange (the root segment's row alone takes a slot
	// per pin); constraint_mode's holds per-wave chain stacks of the deepest pose chain.  Where that
	// exceeds the LDS the plan falls back to the classic layout, as it does for stabilization or
	// 64-bit tables: a pinned mbik_plan_set_wave_roles(1) still solves, and the autotune times the
	// classic layout for such a candidate instead of failing on it.
	if (roles_ok && ((h.wave_roles && h.lds_block_bytes > mbik::kLdsBytes) ||
							(h.cm_roles && cmode_rw_lds(h, mbik::topology_bytes(h), cmode_shape_of(p, nlaunch).spw) > mbik::kLdsBytes)))
		return ensure_schedule_as(p, nlaunch, false);
	if (int rc = reserve_state(p)) return rc;
	return upload_blob(p);
}

int ensure_schedule(mbik_plan *p, int64_t nlaunch) { return ensure_schedule_as(p, nlaunch, true); }

// Resets the constraint_mode node caches of skeletons [first, first+count) to a fresh tree
// built on `setup_pose` (device pointer, indexed from `first`).
int cmode_reset(mbik_plan *p, int first, int count, const float *setup_pose, hipStream_t stream) {
	if (count <= 0) return MBIK_OK;
	hipError_t e = mbik::launch_cmode_reset(stream, p->dev, p->cm, first, count, setup_pose);
	if (e != hipSuccess) return fail(MBIK_EHIP, std::string("constraint_mode reset launch: ") + hipGetErrorString(e));
	return MBIK_OK;
}

// Plan files keep constraint_mode's node caches in the plain [slot][12][N] order (format 1's);
// the device holds them skeleton-tiled (node_at).
size_t cmode_file_node_bytes(const mbik::HostPlan &h) { return (size_t)h.cm_slots() * 12 * (size_t)h.N * sizeof(float); }
size_t cmode_node_bytes(const mbik::HostPlan &h) { return node_area_floats(h.cm_slots(), (size_t)h.N) * sizeof(float); }
size_t cmode_dirty_bytes(const mbik::HostPlan &h) { return 4 * (size_t)h.cm_dirty_words() * (size_t)h.N * sizeof(uint32_t); }
std::vector<float> cmode_nodes_tiled(const mbik::HostPlan &h, const float *plain) {
	const int slots = h.cm_slots();
	const size_t N = (size_t)h.N;
	std::vector<float> t(node_area_floats(slots, N), 0.0f);
	for (int k = 0; k < slots; k++)
		for (int f = 0; f < 12; f++)
			for (size_t s = 0; s < N; s++) t[node_at(slots, s, k, f)] = plain[((size_t)k * 12 + f) * N + s];
	return t;
}
void cmode_nodes_plain(const mbik::HostPlan &h, const float *tiled, float *plain) {
	const int slots = h.cm_slots();
	const size_t N = (size_t)h.N;
	for (int k = 0; k < slots; k++)
		for (int f = 0; f < 12; f++)
			for (size_t s = 0; s < N; s++) plain[((size_t)k * 12 + f) * N + s] = tiled[node_at(slots, s, k, f)];
}

// constraint_mode: allocates the persistent node caches and builds the fresh tree from the
// host setup poses of mbik_plan_create.
int cmode_create(mbik_plan *p, const float *setup_pose, const void *saved) {
	const mbik::HostPlan &h = p->host;
	CmodeState &c = p->cm;
	c.W = h.cm_dirty_words();
	c.maxd = h.cm_maxd;
	int rc = upload(p, h.cm_pre, c.pre);
	rc = rc ? rc : upload(p, h.cm_sub, c.sub);
	if (rc) return rc;
	const size_t N = (size_t)h.N;
	const size_t node_bytes = cmode_node_bytes(h), dirty_bytes = cmode_dirty_bytes(h);
	if ((rc = p->cm_node.reserve(std::max<size_t>(node_bytes, 4), "hipMalloc constraint_mode node caches")) != MBIK_OK) return rc;
	if ((rc = p->cm_dirty.reserve(std::max<size_t>(dirty_bytes, 4), "hipMalloc constraint_mode dirty bits")) != MBIK_OK) return rc;
	p->device_bytes += (int64_t)(node_bytes + dirty_bytes);
	c.node = p->cm_node.as<float>();
	c.dirty = p->cm_dirty.as<uint32_t>();
	if (N == 0) return MBIK_OK;
	if (saved) { // mbik_plan_load: the saved frame-to-frame node caches ([slot][12][N] in the file)
		const char *sv = static_cast<const char *>(saved);
		const std::vector<float> tiled = cmode_nodes_tiled(h, reinterpret_cast<const float *>(sv));
		if (hipMemcpy(c.node, tiled.data(), node_bytes, hipMemcpyHostToDevice) != hipSuccess ||
				hipMemcpy(c.dirty, sv + cmode_file_node_bytes(h), dirty_bytes, hipMemcpyHostToDevice) != hipSuccess)
			return fail(MBIK_EHIP, "hipMemcpy constraint_mode state");
		return MBIK_OK;
	}
	if (p->setup_on_device) { // mbik_plan_create_device: the setup pose already lives on the device
		rc = cmode_reset(p, 0, (int)N, setup_pose, nullptr);
		if (rc == 0 && hipDeviceSynchronize() != hipSuccess) rc = fail(MBIK_EHIP, "constraint_mode reset");
		return rc;
	}
	const size_t pose_bytes = N * h.B * 10 * sizeof(float);
	DevBuf sp;
	if ((rc = sp.reserve(pose_bytes, "hipMalloc setup pose")) != MBIK_OK) return rc;
	rc = hipMemcpy(sp.as<void>(), setup_pose, pose_bytes, hipMemcpyHostToDevice) == hipSuccess ? MBIK_OK : fail(MBIK_EHIP, "hipMemcpy setup pose");
	if (rc == 0) rc = cmode_reset(p, 0, (int)N, sp.as<const float>(), nullptr);
	if (rc == 0 && hipDeviceSynchronize() != hipSuccess) rc = fail(MBIK_EHIP, "constraint_mode reset");
	return rc;
}

// The skeleton-tiled copies of the plan's D / CF / CD (DevPlan::row_at) for launches with the
// whole state in device memory, (re)built on the launch stream when the tables changed.
int ensure_tiled_rows(mbik_plan *p, hipStream_t stream) {
	if (p->tiled_version == p->tables_version && p->Dt) return MBIK_OK;
	const mbik::HostPlan &h = p->host;
	const int Npad = (int)h.padded_n();
	const size_t nD = h.d_floats(Npad), nCF = h.cf_floats(Npad), nCD = h.cd_doubles(Npad);
	if (!p->Dt) {
		DevBuf a, b, c;
		const size_t bD = std::max<size_t>(nD, 1) * sizeof(float), bCF = std::max<size_t>(nCF, 1) * sizeof(float),
					 bCD = std::max<size_t>(nCD, 1) * sizeof(double);
		if (a.reserve(bD, "hipMalloc tiled setup tables") || b.reserve(bCF, "hipMalloc tiled setup tables") ||
				c.reserve(bCD, "hipMalloc tiled setup tables"))
			return MBIK_ENOMEM;
		// padding skeletons read zeros
		if (hipMemsetAsync(a.as<void>(), 0, bD, stream) != hipSuccess || hipMemsetAsync(b.as<void>(), 0, bCF, stream) != hipSuccess ||
				hipMemsetAsync(c.as<void>(), 0, bCD, stream) != hipSuccess) {
			(void)hipStreamSynchronize(stream); // (the buffers are freed on return)
			return fail(MBIK_EHIP, "hipMemsetAsync tiled setup tables");
		}
		p->Dt = std::move(a);
		p->CFt = std::move(b);
		p->CDt = std::move(c);
		p->device_bytes += (int64_t)((nD + nCF) * sizeof(float) + nCD * sizeof(double));
	}
	hipError_t e = hipSuccess;
	if (nD && e == hipSuccess) e = mbik::launch_tile_rows(stream, p->dev.D, p->Dt.as<float>(), h.B, 9, h.N, Npad);
	if (nCF && e == hipSuccess) e = mbik::launch_tile_rows(stream, p->dev.CF, p->CFt.as<float>(), h.NC, h.cf_stride(), h.N, Npad);
	if (nCD && e == hipSuccess) e = mbik::launch_tile_rows(stream, p->dev.CD, p->CDt.as<double>(), h.NC, h.cd_stride(), h.N, Npad);
	if (e != hipSuccess) return fail(MBIK_EHIP, std::string("tile launch failed: ") + hipGetErrorString(e));
	// A launch on another stream must not read the copy before the tiling has run: record its
	// completion; launch() makes other streams wait on it until it has completed.
	if (!p->tile_ev && hipEventCreateWithFlags(&p->tile_ev, hipEventDisableTiming) != hipSuccess) {
		p->tile_ev = nullptr;
		return fail(MBIK_EHIP, "hipEventCreate");
	}
	if (hipEventRecord(p->tile_ev, stream) != hipSuccess) return fail(MBIK_EHIP, "hipEventRecord");
	p->tile_stream = stream;
	p->tile_pending = true;
	p->tiled_version = p->tables_version;
	return MBIK_OK;
}
// Orders a launch on `stream` after the last tiling of the plan's tables (ensure_tiled_rows).
int wait_tiled_rows(mbik_plan *p, hipStream_t stream) {
	if (!p->tile_pending) return MBIK_OK;
	if (hipEventQuery(p->tile_ev) == hipSuccess) {
		p->tile_pending = false;
		return MBIK_OK;
	}
	if (stream != p->tile_stream && hipStreamWaitEvent(stream, p->tile_ev, 0) != hipSuccess)
		return fail(MBIK_EHIP, "hipStreamWaitEvent");
	return MBIK_OK;
}

int resolve_launch(const mbik_plan *p, int64_t count, SolveLaunch &o, int replay) {
	const mbik::HostPlan &h = p->host;
	o = SolveLaunch{};
	o.wave_roles = h.wave_roles || h.cm_roles;
	if (h.constraint_mode) {
		const CmShape sh = cmode_shape_of(p, count);
		o.cmode = true;
		o.cm_spw = sh.spw;
		o.cm_wpb = sh.wpb;
		// (reported so: a classic constraint_mode block holds wpb waves of at most this many)
		o.skeletons_per_block = h.cm_roles ? sh.spw : 64 >> h.log2K;
		o.lds_bytes = cmode_lds_bytes(p, sh);
		o.schedule_lds_bytes = (int64_t)o.lds_bytes;
		if (o.lds_bytes > (size_t)mbik::kLdsBytes) return fail(MBIK_EUNSUPPORTED, "skeleton too large for the constraint_mode LDS layout");
		// node caches below 4 GiB: buffer-resource addressing (cmode.h, NB32)
		const bool nb32 = cmode_node_bytes(h) < (size_t(1) << 32) && tables_fit_32(p);
		o.cm = mbik::cmode_kernel(h.stabilization_passes > 0, nb32, h.has_chain);
		o.threads = 64u * (unsigned)sh.wpb;
		if (h.cm_roles) {
			// wave roles: K waves x spw skeletons per block (request_for: K in {2, 4, 8}, 32-bit addressing)
			if (h.K != 2 && h.K != 4 && h.K != 8) return fail(MBIK_EINVAL, "constraint_mode wave roles: 2, 4 or 8 roles");
			o.cm = mbik::cmode_kernel_rw(h.has_chain, h.K);
			o.threads = 64u * (unsigned)h.K;
		}
		const int64_t per_block = (int64_t)sh.spw * sh.wpb;
		o.blocks = (unsigned)((count + per_block - 1) / per_block);
		return MBIK_OK;
	}
	o.skeletons_per_block = h.spw;
	o.schedule_lds_bytes = h.lds_block_bytes;
	o.tiled_rows = h.state_hbm == 2;
	o.lds_bytes = block_lds_bytes(p);
	if constexpr (kAblate & ABL_SOALDS) o.lds_bytes += ((size_t)p->dev.B * 9 + p->dev.NC * p->dev.cf_stride + 2 * p->dev.NC * p->dev.cd_stride + 2) * sizeof(float);
	if (o.lds_bytes > (size_t)mbik::kLdsBytes) return fail(MBIK_EUNSUPPORTED, "skeleton too large for LDS at this lane count");
	o.blocks = (unsigned)((count + h.spw - 1) / h.spw);
	o.solve = solve_kernel_for(p);
	if (h.wave_roles) {
		o.threads = 64u * (unsigned)h.K; // a wave per role
		// non-finite flags; with cooperative rows the targets, the effector-global exchange and the
		// groups' parent-side records
		o.lds_bytes += (size_t)mbik::rw_extra_lds_bytes(h);
		if (o.lds_bytes > (size_t)mbik::kLdsBytes) return fail(MBIK_EUNSUPPORTED, "wave roles: a row's effector-global exchange exceeds the LDS");
		// the cooperative groups' record handshake has a deadline and reports through the plan's
		// timeout flag, as the helper wave's does (rw_wait)
		o.needs_flag = h.rw_xslots != 0;
	} else if (helper_on(p)) {
		o.helper = o.needs_flag = true;
		o.lds_bytes += kHelpRingBytes;
		o.threads = replay == 2 ? 64 : 128; // (replay mode 2: the solving wave alone)
		o.solve = mbik::solve_kernel_help(p->dev.prio_mask, replay == 2);
	}
	return MBIK_OK;
}

// Whether mbik_group_solve's fused kernel (one wave per block, state in LDS, 32-bit tables) serves
// the plan's current layout.  constraint_mode plans have their own kernel, so do plans laid out
// with state in device memory (wave roles among them), plans whose setup tables need 64-bit
// indices and plans with split-exchange segments (the two-wave build); pinless plans only copy.
static bool group_fusable(const mbik_plan *p) {
	const mbik::HostPlan &h = p->host;
	return !h.constraint_mode && h.P > 0 && h.state_hbm == 0 && tables_fit_32(p) && !h.has_xs;
}

LaunchArgs full_solve(const mbik_plan *p, int first, int count, const float *pose_in, const float *targets, float *pose_out, hipStream_t stream) {
	return LaunchArgs{first, count, pose_in, targets, pose_out, stream, p->host.iterations, 0, p->host.NS - 1};
}

int launch(mbik_plan *p, const LaunchArgs &a) {
	if (a.first < 0 || a.count < 0 || (int64_t)a.first + a.count > p->host.N) return fail(MBIK_EINVAL, "skeleton range out of plan");
	if (a.count == 0) return MBIK_OK;
	if (!a.pose_in || !a.pose_out || (p->host.P > 0 && !a.targets)) return fail(MBIK_EINVAL, "null buffer");
	const mbik::HostPlan &h = p->host;
	if (h.P == 0) {
		// get_effector_count() == 0: _process_modification returns before solving
		// (many_bone_ik_3d.cpp:649-651) and the skeleton keeps its pose.
		if (a.pose_out != a.pose_in &&
				hipMemcpyAsync(a.pose_out, a.pose_in, (size_t)a.count * h.B * 10 * sizeof(float), hipMemcpyDeviceToDevice, a.stream) != hipSuccess)
			return fail(MBIK_EHIP, "hipMemcpyAsync");
		return MBIK_OK;
	}
	int rc = ensure_schedule(p, a.count);
	if (rc) return rc;
	SolveLaunch sl;
	if ((rc = resolve_launch(p, a.count, sl, a.replay)) != MBIK_OK) return rc;
	if (sl.needs_flag && (rc = ensure_help_flag(p)) != MBIK_OK) return rc;
	// the kernels take copies: what belongs to this call alone never reaches the plan's own
	DevPlan d = p->dev;
	d.nonfinite = a.nonfinite;
#ifdef MBIK_REPLAY
	d.replay = a.replay;
#endif
	if (sl.tiled_rows) {
		if ((rc = ensure_tiled_rows(p, a.stream)) != MBIK_OK) return rc;
		if ((rc = wait_tiled_rows(p, a.stream)) != MBIK_OK) return rc;
		d.D = p->Dt.as<float>();
		d.CF = p->CFt.as<float>();
		d.CD = p->CDt.as<double>();
		d.row_n = (int)h.padded_n();
	}
	if (sl.cmode) {
		CmodeState c = p->cm;
		c.spw = sl.cm_spw;
		c.wpb = sl.cm_wpb;
		hipLaunchKernelGGL(sl.cm, dim3(sl.blocks), dim3(sl.threads), sl.lds_bytes, a.stream, d, c, a.first, a.count, a.pose_in, a.targets,
				a.pose_out, a.iterations, a.seg_lo, a.seg_hi);
	} else {
		hipLaunchKernelGGL(sl.solve, dim3(sl.blocks), dim3(sl.threads), sl.lds_bytes, a.stream, d, a.first, a.count, a.pose_in, a.targets,
				a.pose_out, a.iterations, a.seg_lo, a.seg_hi);
	}
	hipError_t e = hipGetLastError();
	if (e != hipSuccess) return fail(MBIK_EHIP, std::string("kernel launch failed: ") + hipGetErrorString(e));
	return MBIK_OK;
}

} // namespace

namespace mbik_host {
// mbik_plan_options: NULL = the defaults; fields past struct_size keep theirs.
int read_options(const mbik_plan_options *opts, int &libm) {
	libm = MBIK_LIBM_VARIANT_FMA;
	if (!opts) return MBIK_OK;
	if (opts->struct_size < (int32_t)sizeof(int32_t)) return fail(MBIK_EINVAL, "mbik_plan_options.struct_size too small");
	if (opts->struct_size >= (int32_t)(offsetof(mbik_plan_options, libm_variant) + sizeof(int32_t))) libm = opts->libm_variant;
	if (libm != MBIK_LIBM_VARIANT_FMA && libm != MBIK_LIBM_VARIANT_SSE2) return fail(MBIK_EINVAL, "unknown libm_variant");
	return MBIK_OK;
}

} // namespace mbik_host

mbik_plan::~mbik_plan() {
	DeviceGuard guard(device);
	if (tile_ev) (void)hipEventDestroy(tile_ev);
	if (help_flag) (void)hipHostFree(help_flag);
}

extern "C" {

const char *mbik_last_error(void) { return g_err.c_str(); }

int32_t mbik_describe_topology(const mbik_skeleton_desc *desc, const mbik_config *config, int32_t *bone_list,
		int32_t *bone_list_count, int32_t *seg_root, int32_t *seg_tip, int32_t *seg_parent, int32_t *seg_headings) {
	if (!desc || !config) return fail(MBIK_EINVAL, "null argument");
	mbik::HostPlan h;
	std::string err = mbik::build_topology(*desc, *config, h);
	if (!err.empty()) return fail(MBIK_EINVAL, err);
	if (bone_list) std::copy(h.bone_list.begin(), h.bone_list.end(), bone_list);
	if (bone_list_count) *bone_list_count = (int32_t)h.bone_list.size();
	for (int i = 0; i < h.NS; i++) {
		if (seg_root) seg_root[i] = h.seg_root[i];
		if (seg_tip) seg_tip[i] = h.seg_tip[i];
		if (seg_parent) seg_parent[i] = h.seg_parent[i];
		if (seg_headings) seg_headings[i] = h.seg_nh[i];
	}
	return h.NS;
}

int32_t mbik_plan_create(const mbik_skeleton_desc *desc, const mbik_config *config, int32_t n_skeletons, const float *setup_pose,
		const float *cones, const float *twist, int32_t device, mbik_plan **out_plan) {
	return mbik_plan_create_opts(desc, config, nullptr, n_skeletons, setup_pose, cones, twist, device, out_plan);
}

int32_t mbik_plan_create_opts(const mbik_skeleton_desc *desc, const mbik_config *config, const mbik_plan_options *opts,
		int32_t n_skeletons, const float *setup_pose, const float *cones, const float *twist, int32_t device,
		mbik_plan **out_plan) {
	if (!desc || !config || !out_plan) return fail(MBIK_EINVAL, "null argument");
	int libm = 0;
	if (read_options(opts, libm)) return MBIK_EINVAL;
	*out_plan = nullptr;
	if (int rc = check_device(device)) return rc;
	std::unique_ptr<mbik_plan> p(new mbik_plan());
	p->device = device;
	if (desc->bone_count < 0 || desc->pin_count < 0 || desc->constraint_count < 0 || config->bone_damp_count < 0)
		return fail(MBIK_EINVAL, "negative count");
	keep_inputs(p.get(), *desc, *config);
	std::string err = mbik::build_topology(*desc, *config, p->host);
	if (!err.empty()) return fail(MBIK_EINVAL, err);
	p->host.libm_variant = libm;
	err = mbik::build_skeletons(p->host, n_skeletons, setup_pose, cones, twist, std::max(1, desc->max_cones));
	if (!err.empty()) return fail(MBIK_EINVAL, err);
	const int rc = finish_plan(p.get(), setup_pose, nullptr);
	if (rc) return rc;
	*out_plan = p.release();
	return MBIK_OK;
}

} // extern "C"
namespace mbik_host {
void keep_inputs(mbik_plan *p, const mbik_skeleton_desc &desc, const mbik_config &cfg) {
	p->src_parents.assign(desc.parents, desc.parents + (desc.parents ? desc.bone_count : 0));
	p->src_pins.assign(desc.pins, desc.pins + (desc.pins ? desc.pin_count : 0));
	p->src_cons.assign(desc.constraints, desc.constraints + (desc.constraints ? desc.constraint_count : 0));
	p->src_bone_damp.assign(cfg.bone_damp, cfg.bone_damp + (cfg.bone_damp ? std::max(0, cfg.bone_damp_count) : 0));
	p->src_max_cones = desc.max_cones;
	p->src_cfg = cfg;
	p->src_cfg.bone_damp = nullptr;
}

// The device side of a plan whose HostPlan holds the topology and the per-skeleton tables
// (D / CF / CD): uploads them, builds the launch schedule, and the constraint_mode node caches
// -- from the setup pose (a new plan), or copied from a saved plan's bytes (cm_state: node
// caches then dirty words, as mbik_plan_save wrote them).
int finish_plan(mbik_plan *p, const float *setup_pose, const void *cm_state) {
	const int device = p->device;
	const int n_skeletons = p->host.N;
	for (int b = 0; b < p->host.B; b++)
		if ((p->host.bone_flags[b] & mbik::BF_PINNED) && p->host.bone_pin[b] >= 0) {
			int e = p->host.bone_pin[b];
			if (p->host.eff_path_off[e + 1] - p->host.eff_path_off[e] > 4096) return fail(MBIK_EUNSUPPORTED, "skeleton too deep");
		}
	DeviceGuard guard(device);
	p->cu_count = cu_count_of(device);
	mbik::HostPlan &h = p->host;
	DevPlan &d = p->dev;
	d.B = h.B; d.P = h.P; d.NS = h.NS; d.NC = h.NC; d.max_cones = h.max_cones; d.N = h.N;
	d.cf_stride = h.cf_stride(); d.cd_stride = h.cd_stride();
	d.stab = h.stabilization_passes; d.constraint_mode = h.constraint_mode; d.hs_floats = h.hs_floats;
	d.libm = h.libm_variant;
	d.n_gck = h.n_gck;
	// One heading slot mask shared by every effector -- the reference's default priorities, the
	// usual case -- runs bone-steps specialised for it (kPrioDefault).
	{
		int pm = -1;
		for (int e = 0; e < h.P && pm != 0; e++) {
			int m = 1;
			for (int a = 0; a < 3; a++)
				if (h.eff_prio[3 * e + a] > 0.0f) m |= 6 << (2 * a);
			pm = pm < 0 || pm == m ? m : 0;
		}
		d.prio_mask = pm == kPrioDefault ? pm : 0;
	}
	d.lds_stride = (mbik::lds_floats_per_skeleton(h) + 3) & ~3;
	int rc = 0;
	rc = rc ? rc : upload(p, h.D, d.D);
	rc = rc ? rc : upload(p, h.CF, d.CF);
	rc = rc ? rc : upload(p, h.CD, d.CD);
	rc = rc ? rc : ensure_schedule(p, n_skeletons);
	if (rc == 0 && h.constraint_mode) rc = cmode_create(p, setup_pose, cm_state);
	if (rc) return rc; // (the caller deletes the plan, which frees what it took)
	// Algorithmic flops: per bone-step 50 H + 14 H [translate] + 72 E_seg
	// + 465, plus 770 + 140 C - 60 for a constrained bone with C cones; x iterations.
	double f = 0;
	for (int sg = 0; sg < h.NS; sg++) {
		const int H = h.seg_nh[sg], E = h.seg_eff_off[sg + 1] - h.seg_eff_off[sg];
		const bool tr = (h.seg_flags[sg] & mbik::SF_TRANSLATE) != 0;
		for (int k = h.seg_bone_off[sg]; k < h.seg_bone_off[sg + 1]; k++) {
			const int b = h.seg_bones[k];
			if (!h.constraint_mode) f += 50.0 * H + (tr ? 14.0 * H : 0.0) + 72.0 * E + 465.0; // no fit in constraint_mode
			if (h.bone_flags[b] & (mbik::BF_ORIENT | mbik::BF_AXIAL)) {
				const int C = (h.bone_flags[b] & mbik::BF_ORIENT) ? h.cons_ncones[h.bone_cons[b]] : 0;
				f += 770.0 + 140.0 * C - 60.0;
			}
		}
	}
	p->alg_flops = f * h.iterations;
	// Algorithmic HBM bytes per skeleton, SURVEY.md §8(d)'s definition (the one bench.py's
	// roofline and BASELINE.md divide by): each input the solve needs read once, each output
	// written once -- per bone the input pose (quaternion, position, scale: 40 B), its
	// bone-direction quaternion (16 B) and damp (4 B), and the output pose (40 B); per
	// effector the target transform (48 B) and its weight and priorities (16 B); per
	// constrained bone the orientation and twist quaternions, the twist centre (16 B each),
	// the twist half-cosine (4 B) and 52 B per cone.  C2 8,292 B, C3 3,456, C4 6,912,
	// C5 52,068.
	double cons = 0;
	for (int c = 0; c < h.NC; c++) cons += 16.0 * 3 + 4.0 + 52.0 * h.cons_ncones[c];
	p->alg_bytes = (double)h.B * (40 + 16 + 4 + 40) + (double)h.P * (48 + 16) + cons;
	if (h.constraint_mode) // the persistent node caches, read and written once per frame
		p->alg_bytes += 2.0 * ((double)h.cm_slots() * 12 * 4 + 4.0 * p->cm.W * 4);
	h.D.clear(); h.D.shrink_to_fit();
	h.CF.clear(); h.CF.shrink_to_fit();
	h.CD.clear(); h.CD.shrink_to_fit();
	return MBIK_OK;
}
} // namespace

extern "C" {

void mbik_plan_destroy(mbik_plan *p) { delete p; }

int32_t mbik_plan_get_info(const mbik_plan *p, mbik_plan_info *o) {
	if (!p || !o) return fail(MBIK_EINVAL, "null argument");
	const mbik::HostPlan &h = p->host;
	int maxh = 0;
	for (int i = 0; i < h.NS; i++) maxh = std::max(maxh, h.seg_height[i]);
	// the launch of the whole plan, independent of earlier launches' counts (a block that exceeds
	// the LDS is still reported: the refusal belongs to the solve)
	SolveLaunch sl;
	const KeepError keep; // (a report is no failure: mbik_last_error stays as it was)
	(void)resolve_launch(p, h.N, sl);
	o->abi_version = MBIK_ABI_VERSION;
	o->skeleton_count = h.N;
	o->bone_count = h.B;
	o->pin_count = h.P;
	o->segment_count = h.NS;
	o->level_count = maxh + 1;
	o->lanes_per_skeleton = h.K;
	o->skeletons_per_block = sl.skeletons_per_block;
	o->max_headings = h.max_headings;
	o->device = p->device;
	o->device_bytes = p->device_bytes;
	o->algorithmic_bytes_per_skeleton = p->alg_bytes;
	o->algorithmic_flops_per_skeleton = p->alg_flops;
	o->lds_bytes_per_block = sl.schedule_lds_bytes; // (not the launch's: SolveLaunch)
	o->checkpoint_interval = h.g_interval;
	o->heading_staging = h.staging;
	o->state_placement = h.state_hbm;
	o->waves_per_simd = h.waves_per_simd;
	o->constraint_slots = h.NC;
	o->cf_stride = h.cf_stride();
	o->cd_stride = h.cd_stride();
	o->libm_variant = h.libm_variant;
	o->helper_wave = sl.helper ? 1 : 0;
	o->heading_slots = p->dev.prio_mask;
	o->wave_roles = sl.wave_roles ? 1 : 0;
	return MBIK_OK;
}

int32_t mbik_plan_set_launch(mbik_plan *p, int32_t lanes) {
	if (!p) return fail(MBIK_EINVAL, "null plan");
	if (lanes < 0 || lanes > 64 || (lanes & (lanes - 1))) return fail(MBIK_EINVAL, "lanes_per_skeleton must be 0 or a power of two <= 64");
	p->pins.lanes = lanes;
	invalidate_layout(p);
	return MBIK_OK;
}

int32_t mbik_plan_set_layout(mbik_plan *p, int32_t lanes, int32_t skeletons_per_block, int32_t global_checkpoint_interval) {
	if (!p) return fail(MBIK_EINVAL, "null plan");
	if (lanes < 0 || lanes > 64 || (lanes & (lanes - 1))) return fail(MBIK_EINVAL, "lanes_per_skeleton must be 0 or a power of two <= 64");
	if (skeletons_per_block < 0 || skeletons_per_block > 64) return fail(MBIK_EINVAL, "skeletons_per_block must be in [0, 64]");
	if (global_checkpoint_interval < 0) return fail(MBIK_EINVAL, "global_checkpoint_interval must be >= 0");
	p->pins.lanes = lanes;
	p->pins.spw = skeletons_per_block;
	p->pins.interval = global_checkpoint_interval;
	invalidate_layout(p);
	return MBIK_OK;
}

int32_t mbik_plan_set_waves_per_simd(mbik_plan *p, int32_t waves) {
	if (!p) return fail(MBIK_EINVAL, "null plan");
	if (waves != -1 && waves != 1 && waves != 2) return fail(MBIK_EINVAL, "waves_per_simd must be -1 (automatic), 1 or 2");
	p->pins.waves = waves;
	invalidate_layout(p);
	return MBIK_OK;
}

int32_t mbik_plan_set_helper_wave(mbik_plan *p, int32_t helper) {
	if (!p) return fail(MBIK_EINVAL, "null plan");
	if (helper < -1 || helper > 1) return fail(MBIK_EINVAL, "helper wave must be -1 (automatic), 0 (off) or 1 (on)");
	// no invalidate_layout: the helper wave changes neither the schedule nor the topology blob,
	// only the kernel and the LDS resolve_launch picks
	p->pins.helper = helper;
	return MBIK_OK;
}

int32_t mbik_plan_set_wave_roles(mbik_plan *p, int32_t roles) {
	if (!p) return fail(MBIK_EINVAL, "null plan");
	if (roles < -1 || roles > 1) return fail(MBIK_EINVAL, "wave roles must be -1 (automatic), 0 (off) or 1 (on)");
	p->pins.roles = roles;
	invalidate_layout(p);
	return MBIK_OK;
}

int32_t mbik_plan_set_table_addressing(mbik_plan *p, int32_t wide) {
	if (!p) return fail(MBIK_EINVAL, "null plan");
	if (wide != 0 && wide != 1) return fail(MBIK_EINVAL, "table addressing must be 0 (automatic) or 1 (64-bit indices)");
	p->tab64 = wide;
	invalidate_layout(p);
	return MBIK_OK;
}

int32_t mbik_plan_set_locals_placement(mbik_plan *p, int32_t placement) {
	if (!p) return fail(MBIK_EINVAL, "null plan");
	if (placement < -1 || placement > 2)
		return fail(MBIK_EINVAL, "placement must be -1 (automatic), 0 (LDS), 1 (locals in device memory) or 2 (all state)");
	p->pins.locals = placement;
	invalidate_layout(p);
	return MBIK_OK;
}

int32_t mbik_plan_set_heading_staging(mbik_plan *p, int32_t staging) {
	if (!p) return fail(MBIK_EINVAL, "null plan");
	if (staging < -1 || staging > 5) return fail(MBIK_EINVAL, "staging must be -1 (automatic), 0, 1, 2, 3, 4 or 5");
	p->pins.staging = staging;
	invalidate_layout(p);
	return MBIK_OK;
}

int32_t mbik_plan_rebuild_setup(mbik_plan *p, int32_t first, int32_t count, const float *setup_pose, const float *cones,
		const float *twist, void *hip_stream) {
	if (!p) return fail(MBIK_EINVAL, "null plan");
	mbik::HostPlan &h = p->host;
	if (first < 0 || count < 0 || (int64_t)first + count > h.N) return fail(MBIK_EINVAL, "skeleton range out of plan");
	if (count == 0) return MBIK_OK;
	if (!setup_pose || (h.NC > 0 && (!cones || !twist))) return fail(MBIK_EINVAL, "null buffer");
	DeviceGuard guard(p->device);
	if (!p->dsetup_ready) {
		mbik::SetupView v = mbik::setup_view(h, h.N, h.setup_max_cones);
		int rc = 0;
		auto up = [&](const std::vector<int32_t> &vec, const int *&dst) {
			if (rc == 0) rc = upload(p, vec, dst);
		};
		up(h.setup_topo, v.topo);
		up(h.bone_list, v.bone_list);
		up(h.bone_flags, v.bone_flags);
		up(h.bone_pose_parent, v.bone_pose_parent);
		up(h.bone_ik_parent, v.bone_ik_parent);
		up(h.ik_child_off, v.ik_child_off);
		up(h.ik_children, v.ik_children);
		up(h.cons_order, v.cons_order);
		up(h.cons_order_slot, v.cons_order_slot);
		up(h.cons_order_ncones, v.cons_order_ncones);
		up(h.cons_bone, v.cons_bone);
		if (rc) return rc;
		p->dsetup = v;
		p->dsetup_ready = true;
	}
	const mbik::SetupView &v = p->dsetup;
	const size_t stride = (mbik::setup_scratch_bytes(v.B, v.NC, v.max_cones_in) + 255) & ~size_t(255);
	const int threads = std::min(count, 8192);
	DevBuf scratch;
	if (int rc = scratch.reserve(stride * (size_t)threads, "hipMalloc setup scratch")) return rc;
	hipStream_t st = reinterpret_cast<hipStream_t>(hip_stream);
	const DevPlan &d = p->dev;
	hipError_t e = mbik::launch_setup(st, threads, v, first, count, setup_pose, cones, twist, scratch.as<char>(), stride,
			const_cast<float *>(d.D), const_cast<float *>(d.CF), const_cast<double *>(d.CD));
	// the scratch is freed after the kernel; a fault while it runs surfaces at this sync and
	// must not be reported as success (the D/CF/CD tables may be partly written)
	hipError_t es = hipStreamSynchronize(st);
	scratch.reset();
	if (e != hipSuccess) return fail(MBIK_EHIP, std::string("setup launch: ") + hipGetErrorString(e));
	if (es != hipSuccess) return fail(MBIK_EHIP, std::string("setup kernel: ") + hipGetErrorString(es));
	p->tables_version++;
	// a rebuilt tree starts with fresh node caches (_bone_list_changed)
	if (h.constraint_mode) return cmode_reset(p, first, count, setup_pose, st);
	return MBIK_OK;
}

int32_t mbik_plan_setup_tables(const mbik_plan *p, float *D, float *CF, double *CD) {
	if (!p) return fail(MBIK_EINVAL, "null plan");
	const mbik::HostPlan &h = p->host;
	DeviceGuard guard(p->device);
	const size_t N = (size_t)h.N;
	if (D && hipMemcpy(D, p->dev.D, h.d_floats(N) * sizeof(float), hipMemcpyDeviceToHost) != hipSuccess)
		return fail(MBIK_EHIP, "hipMemcpy D");
	if (CF && h.NC && hipMemcpy(CF, p->dev.CF, h.cf_floats(N) * sizeof(float), hipMemcpyDeviceToHost) != hipSuccess)
		return fail(MBIK_EHIP, "hipMemcpy CF");
	if (CD && h.NC && hipMemcpy(CD, p->dev.CD, h.cd_doubles(N) * sizeof(double), hipMemcpyDeviceToHost) != hipSuccess)
		return fail(MBIK_EHIP, "hipMemcpy CD");
	return MBIK_OK;
}

int32_t mbik_plan_resident_blocks(const mbik_plan *p, int64_t lds_bytes_per_block) {
	if (!p) return fail(MBIK_EINVAL, "null plan");
	DeviceGuard guard(p->device);
	return blocks_per_cu(const_cast<mbik_plan *>(p), lds_bytes_per_block);
}

int32_t mbik_solve(mbik_plan *p, int32_t first, int32_t count, const float *pose_in, const float *targets, float *pose_out,
		void *stream) {
	if (!p) return fail(MBIK_EINVAL, "null plan");
	if (int rc = take_helper_timeout(p)) return rc;
	DeviceGuard guard(p->device);
	return launch(p, full_solve(p, first, count, pose_in, targets, pose_out, (hipStream_t)stream));
}

int32_t mbik_plan_status(const mbik_plan *p, uint32_t *status) {
	if (!p || !status) return fail(MBIK_EINVAL, "null argument");
	*status = (p->help_flag && __atomic_load_n(p->help_flag, __ATOMIC_ACQUIRE)) ? MBIK_STATUS_HELPER_TIMEOUT : 0u;
	return MBIK_OK;
}

int32_t mbik_plan_debug_helper(mbik_plan *p, int32_t drop_record, int32_t timeout_us) {
	if (!p) return fail(MBIK_EINVAL, "null plan");
	if (drop_record < -1 || timeout_us < 0) return fail(MBIK_EINVAL, "drop_record must be >= -1 and timeout_us >= 0");
	p->dev.help_drop = drop_record;
	p->help_timeout_us = timeout_us;
	return MBIK_OK;
}

int32_t mbik_solve_checked(mbik_plan *p, int32_t first, int32_t count, const float *pose_in, const float *targets,
		float *pose_out, uint8_t *nonfinite, void *stream) {
	if (!p) return fail(MBIK_EINVAL, "null plan");
	if (!nonfinite) return fail(MBIK_EINVAL, "null nonfinite buffer");
	if (int rc = take_helper_timeout(p)) return rc;
	DeviceGuard guard(p->device);
	if (p->host.P == 0 && count > 0 && first >= 0 && (int64_t)first + count <= p->host.N &&
			hipMemsetAsync(nonfinite, 0, (size_t)count, (hipStream_t)stream) != hipSuccess)
		return fail(MBIK_EHIP, "hipMemsetAsync");
	LaunchArgs a = full_solve(p, first, count, pose_in, targets, pose_out, (hipStream_t)stream);
	a.nonfinite = nonfinite;
	return launch(p, a);
}

int32_t mbik_segment_solve(mbik_plan *p, int32_t seg, int32_t first, int32_t count, float *pose_inout, const float *targets,
		void *stream) {
	if (!p) return fail(MBIK_EINVAL, "null plan");
	if (seg < 0 || seg >= p->host.NS) return fail(MBIK_EINVAL, "segment out of range");
	if (int rc = take_helper_timeout(p)) return rc;
	DeviceGuard guard(p->device);
	return launch(p, LaunchArgs{first, count, pose_inout, targets, pose_inout, (hipStream_t)stream, 1, p->host.seg_tin[seg], seg});
}

int32_t mbik_group_create(mbik_plan *const *plans, int32_t n_plans, mbik_group **out_group) {
	if (!plans || n_plans <= 0 || !out_group) return fail(MBIK_EINVAL, "null argument or empty group");
	*out_group = nullptr;
	for (int i = 0; i < n_plans; i++) {
		if (!plans[i]) return fail(MBIK_EINVAL, "null plan in group");
		if (plans[i]->device != plans[0]->device) return fail(MBIK_EINVAL, "group plans must share one device");
	}
	std::unique_ptr<mbik_group> g(new mbik_group());
	g->plans.assign(plans, plans + n_plans);
	g->device = plans[0]->device;
	DeviceGuard guard(g->device);
	if (g->d_plans.reserve(sizeof(DevPlan) * n_plans, "hipMalloc group tables") ||
			g->d_entries.reserve(sizeof(GroupEntry) * n_plans, "hipMalloc group tables"))
		return MBIK_ENOMEM;
	*out_group = g.release();
	return MBIK_OK;
}

void mbik_group_destroy(mbik_group *g) { delete g; }

int32_t mbik_group_solve(mbik_group *g, const int32_t *first, const int32_t *count, const float *const *pose_in,
		const float *const *targets, float *const *pose_out, void *hip_stream) {
	if (!g) return fail(MBIK_EINVAL, "null group");
	if (!pose_in || !targets || !pose_out) return fail(MBIK_EINVAL, "null buffer array");
	for (mbik_plan *p : g->plans)
		if (int rc = take_helper_timeout(p)) return rc;
	DeviceGuard guard(g->device);
	hipStream_t stream = reinterpret_cast<hipStream_t>(hip_stream);
	const int n = (int)g->plans.size();
	std::vector<DevPlan> dp;
	std::vector<GroupEntry> ent;
	size_t lds = 0;
	int blocks = 0;
	bool stab = false;
	// Longest chain first (iterations x critical-path bone-steps of the plan's schedule).
	std::vector<std::pair<double, int>> order;
	for (int i = 0; i < n; i++) {
		const mbik::HostPlan &h = g->plans[i]->host;
		double steps = 0;
		for (int r = 0; r < h.nrows; r++) steps += mbik::row_max_steps(h, r);
		order.push_back({-(double)h.iterations * steps, i});
	}
	std::stable_sort(order.begin(), order.end());
	for (auto [key, i] : order) {
		(void)key;
		mbik_plan *p = g->plans[i];
		const int f = first ? first[i] : 0;
		const int c = count ? count[i] : p->host.N - f;
		if (f < 0 || c < 0 || (int64_t)f + c > p->host.N) return fail(MBIK_EINVAL, "skeleton range out of plan");
		if (c == 0) continue;
		if (!pose_in[i] || !pose_out[i] || (p->host.P > 0 && !targets[i])) return fail(MBIK_EINVAL, "null buffer");
		int rc = p->host.P > 0 ? ensure_schedule(p, c) : MBIK_OK;
		if (rc) return rc;
		if (!group_fusable(p)) {
			rc = launch(p, full_solve(p, f, c, pose_in[i], targets[i], pose_out[i], stream));
			if (rc) return rc;
			continue;
		}
		const mbik::HostPlan &h = p->host;
		SolveLaunch sl;
		if ((rc = resolve_launch(p, c, sl)) != MBIK_OK) return rc;
		// (the fused kernel runs the classic block also for a plan with the helper wave on)
		lds = std::max(lds, sl.lds_bytes - (sl.helper ? kHelpRingBytes : 0));
		stab = stab || h.stabilization_passes > 0;
		dp.push_back(p->dev);
		ent.push_back(GroupEntry{blocks, f, c, h.iterations, pose_in[i], targets[i], pose_out[i]});
		blocks += (int)sl.blocks;
	}
	if (ent.empty()) return MBIK_OK;
	if (hipMemcpyAsync(g->d_plans.as<void>(), dp.data(), sizeof(DevPlan) * dp.size(), hipMemcpyHostToDevice, stream) != hipSuccess ||
			hipMemcpyAsync(g->d_entries.as<void>(), ent.data(), sizeof(GroupEntry) * ent.size(), hipMemcpyHostToDevice, stream) != hipSuccess)
		return fail(MBIK_EHIP, "hipMemcpyAsync group tables");
	const mbik::GroupKernel kern = mbik::group_kernel(stab);
	hipLaunchKernelGGL(kern, dim3((unsigned)blocks), dim3(64), lds, stream, g->d_plans.as<const DevPlan>(),
			g->d_entries.as<const GroupEntry>(), (int)ent.size());
	hipError_t e = hipGetLastError();
	if (e != hipSuccess) return fail(MBIK_EHIP, std::string("group launch failed: ") + hipGetErrorString(e));
	// the staged tables above are pageable: hipMemcpyAsync has consumed them on return
	return MBIK_OK;
}
int32_t mbik_capture_targets(mbik_plan *p, int32_t first, int32_t count, const float *skeleton_global,
		const float *target_global, const uint8_t *visible, float *targets, void *hip_stream) {
	if (!p) return fail(MBIK_EINVAL, "null plan");
	if (first < 0 || count < 0 || (int64_t)first + count > p->host.N) return fail(MBIK_EINVAL, "skeleton range out of plan");
	const int P = p->host.P;
	if (count == 0 || P == 0) return MBIK_OK;
	if (!skeleton_global || !target_global || !targets) return fail(MBIK_EINVAL, "null buffer");
	DeviceGuard guard(p->device);
	hipError_t e = mbik::launch_capture_targets(reinterpret_cast<hipStream_t>(hip_stream), count, P, skeleton_global, target_global,
			visible, targets);
	if (e != hipSuccess) return fail(MBIK_EHIP, std::string("capture launch failed: ") + hipGetErrorString(e));
	return MBIK_OK;
}

int32_t mbik_plan_segment_table(const mbik_plan *p, int32_t *root, int32_t *tip, int32_t *parent, int32_t cap) {
	if (!p) return fail(MBIK_EINVAL, "null plan");
	const mbik::HostPlan &h = p->host;
	for (int i = 0; i < h.NS && i < cap; i++) {
		if (root) root[i] = h.seg_root[i];
		if (tip) tip[i] = h.seg_tip[i];
		if (parent) parent[i] = h.seg_parent[i];
	}
	return h.NS;
}

static int32_t step_classes_of(const mbik::HostPlan &h, int32_t *row_steps, int32_t row_cap, int32_t *classes, int32_t class_cap) {
	int n = 0;
	for (int r = 0; r < h.nrows; r++) {
		const int nq = mbik::row_max_steps(h, r);
		if (row_steps && r < row_cap) row_steps[r] = nq;
		for (int q = 0; q < nq; q++, n++)
			if (classes && n < class_cap) classes[n] = mbik::step_class_at(h, r, q);
	}
	return h.nrows;
}
int32_t mbik_plan_step_classes(const mbik_plan *p, int32_t *row_steps, int32_t row_cap, int32_t *classes, int32_t class_cap) {
	if (!p) return fail(MBIK_EINVAL, "null plan");
	return step_classes_of(p->host, row_steps, row_cap, classes, class_cap);
}
int32_t mbik_describe_step_classes(const mbik_skeleton_desc *desc, const mbik_config *config, int32_t lanes_per_skeleton,
		int32_t *row_steps, int32_t row_cap, int32_t *classes, int32_t class_cap) {
	if (!desc || !config) return fail(MBIK_EINVAL, "null argument");
	mbik::HostPlan h;
	std::string err = mbik::build_topology(*desc, *config, h);
	if (!err.empty()) return fail(MBIK_EINVAL, err);
	h.N = 1;
	mbik::LayoutRequest rq;
	rq.lanes = std::max(0, lanes_per_skeleton);
	mbik::build_schedule(h, rq, 1);
	return step_classes_of(h, row_steps, row_cap, classes, class_cap);
}

int32_t mbik_solve_host(mbik_plan *p, int32_t first, int32_t count, const float *pose_in, const float *targets, float *pose_out) {
	if (!p) return fail(MBIK_EINVAL, "null plan");
	if (count <= 0) return count == 0 ? MBIK_OK : fail(MBIK_EINVAL, "negative count");
	DeviceGuard guard(p->device);
	const mbik::HostPlan &h = p->host;
	size_t need = (size_t)count;
	if (p->h_in.reserve(need * h.B * 10 * sizeof(float), "hipMalloc scratch") ||
			p->h_tg.reserve(std::max<size_t>(1, need * h.P * 12) * sizeof(float), "hipMalloc scratch") ||
			p->h_out.reserve(need * h.B * 10 * sizeof(float), "hipMalloc scratch"))
		return MBIK_ENOMEM;
	float *d_in = p->h_in.as<float>(), *d_tg = p->h_tg.as<float>(), *d_out = p->h_out.as<float>();
	if (hipMemcpy(d_in, pose_in, need * h.B * 10 * sizeof(float), hipMemcpyHostToDevice) != hipSuccess ||
			(h.P > 0 && hipMemcpy(d_tg, targets, need * h.P * 12 * sizeof(float), hipMemcpyHostToDevice) != hipSuccess))
		return fail(MBIK_EHIP, "hipMemcpy H2D");
	if (int rc = take_helper_timeout(p)) return rc;
	int rc = launch(p, full_solve(p, first, count, d_in, d_tg, d_out, nullptr));
	if (rc) return rc;
	if (hipMemcpy(pose_out, d_out, need * h.B * 10 * sizeof(float), hipMemcpyDeviceToHost) != hipSuccess)
		return fail(MBIK_EHIP, std::string("hipMemcpy D2H / kernel: ") + hipGetErrorString(hipGetLastError()));
	return take_helper_timeout(p); // this launch's own (the copy waited for it)
}

} // extern "C"

#ifdef MBIK_REPLAY
// Diagnostic: mode 1 runs a helper-wave solve that saves every helper record, mode 2 the solving
// wave alone replaying them (same inputs, same skeletons), mode 0 frees the buffer.
extern "C" int mbik_debug_replay(mbik_plan *p, int32_t mode, int32_t first, int32_t count, const float *pose_in,
		const float *targets, float *pose_out, void *stream) {
	DeviceGuard guard(p->device);
	if (mode == 0) {
		p->rec_dump.reset();
		p->dev.rec_dump = nullptr;
		return MBIK_OK;
	}
	int rc = ensure_schedule(p, count);
	if (rc) return rc;
	SolveLaunch sl;
	if (resolve_launch(p, count, sl, mode) != MBIK_OK || !sl.helper) return fail(MBIK_EINVAL, "replay needs a helper-wave layout");
	const mbik::HostPlan &h = p->host;
	int per_iter = 0;
	for (int r = 0; r < h.nrows; r++) per_iter += mbik::row_max_steps(h, r);
	const size_t blocks = sl.blocks;
	if (mode == 1) {
		p->rec_dump.reset();
		p->dev.rec_dump = nullptr;
		p->dev.rec_per_block = per_iter * h.iterations;
		if ((rc = p->rec_dump.reserve(blocks * p->dev.rec_per_block * kHelpF4 * 64 * sizeof(float4), "replay buffer")) != MBIK_OK) return rc;
		p->dev.rec_dump = p->rec_dump.as<float4>();
	}
	LaunchArgs a = full_solve(p, first, count, pose_in, targets, pose_out, (hipStream_t)stream);
	a.replay = mode;
	return launch(p, a);
}
#endif

#ifdef MBIK_PROF
// Diagnostic cycle accounting: the sum of every kernel TU's counters, cleared.
extern "C" int mbik_debug_prof(unsigned long long *out) {
	for (int i = 0; i < 24; i++) out[i] = 0;
	return mbik::prof_take_w1(out) | mbik::prof_take_w2(out) | mbik::prof_take_rw(out) | mbik::prof_take_cmode(out);
}
#endif
