// mbik_plan_autotune: times the launch layouts a plan can run (lanes, skeletons per block,
// checkpoint interval, heading staging, state placement, waves per SIMD, wave roles, the helper
// wave; constraint_mode's lane counts) on the caller's batch and keeps the fastest.  Every
// layout computes the same bits (tests/test_gpu_layouts.py); only the time differs.
// A candidate is a LayoutPins: the caller's pins with the fields under test set.
#include <functional>

#include "host.h"

using namespace mbik_host;

namespace {
constexpr int kNothingTimed = 1; // (internal: no candidate was eligible)

// The start and stop events of one timing, destroyed with the scope.
struct EventPair {
	hipEvent_t e0 = nullptr, e1 = nullptr;
	~EventPair() {
		if (e0) (void)hipEventDestroy(e0);
		if (e1) (void)hipEventDestroy(e1);
	}
	int create() {
		if (hipEventCreate(&e0) != hipSuccess || hipEventCreate(&e1) != hipSuccess) return fail(MBIK_EHIP, "hipEventCreate");
		return MBIK_OK;
	}
};

// ms: the device time of `reps` launches after `warm` untimed ones, back to back.  With
// before_each (constraint_mode: the node caches put back) that runs before every launch and is
// not timed: each launch is then timed on its own and waited for, and ms is the sum.
int time_launches(mbik_plan *p, const LaunchArgs &a, int warm, int reps, float &ms, const std::function<int()> &before_each = nullptr) {
	EventPair ev;
	int rc = ev.create();
	ms = 0.0f;
	for (int r = 0; r < warm + reps && rc == MBIK_OK; r++) {
		if (before_each && (rc = before_each()) != MBIK_OK) break;
		if (before_each || r == warm) (void)hipEventRecord(ev.e0, a.stream);
		if ((rc = launch(p, a)) != MBIK_OK) break;
		if (before_each || r == warm + reps - 1) {
			(void)hipEventRecord(ev.e1, a.stream);
			if (hipEventSynchronize(ev.e1) != hipSuccess) rc = fail(MBIK_EHIP, "hipEventSynchronize");
			float t = 0.0f;
			(void)hipEventElapsedTime(&t, ev.e0, ev.e1);
			if (r >= warm) ms += t;
		}
	}
	return rc;
}

// constraint_mode: every solve advances the persistent node caches (a frame), so the caches
// are saved first, each candidate lane count is timed from that saved state, and the state is
// put back: the caller's next frame sees the caches as they were.
int cmode_autotune(mbik_plan *p, const LaunchArgs &a) {
	if (p->pins.lanes) return MBIK_OK; // pinned by mbik_plan_set_launch / set_layout
	mbik::HostPlan &h = p->host;
	// candidates: 1, 2, 4, ... up to the widest sibling level's power of two (the default K)
	mbik::build_schedule(h, mbik::LayoutRequest{}, a.count, nullptr, nullptr, p->cu_count);
	const int max_lanes = h.K;
	const size_t node_bytes = cmode_node_bytes(h), dirty_bytes = cmode_dirty_bytes(h);
	DevBuf save;
	if (int rc = save.reserve(node_bytes + dirty_bytes, "hipMalloc autotune state copy")) return rc;
	char *sv = save.as<char>();
	auto copy = [&](bool to_save) {
		hipError_t x = to_save ? hipMemcpyAsync(sv, p->cm.node, node_bytes, hipMemcpyDeviceToDevice, a.stream)
							   : hipMemcpyAsync(p->cm.node, sv, node_bytes, hipMemcpyDeviceToDevice, a.stream);
		hipError_t y = to_save ? hipMemcpyAsync(sv + node_bytes, p->cm.dirty, dirty_bytes, hipMemcpyDeviceToDevice, a.stream)
							   : hipMemcpyAsync(p->cm.dirty, sv + node_bytes, dirty_bytes, hipMemcpyDeviceToDevice, a.stream);
		return x == hipSuccess && y == hipSuccess ? MBIK_OK : fail(MBIK_EHIP, "hipMemcpyAsync autotune state");
	};
	int rc = copy(true);
	// classic: lanes per skeleton x skeletons per wave (full waves, or half: twice the waves per
	// SIMD for the node-cache misses to overlap); wave roles (cmode.h mbik_cmode_kernel_rw, plans
	// without stabilization, unless pinned off): 2, 4 or 8 roles x 64, 32 or 16 skeletons per block
	const int roles0 = p->pins.roles;
	std::vector<LayoutPins> cands;
	auto add = [&](int lanes, int div, int roles) {
		LayoutPins c = p->pins;
		c.cm_lanes = lanes;
		c.cm_spw_div = div;
		c.roles = roles;
		cands.push_back(c);
	};
	if (roles0 != 1)
		for (int lanes = 1; lanes <= max_lanes && lanes <= 64; lanes <<= 1)
			for (int div = 0; div < 2; div++) add(lanes, div, 0);
	if (roles0 != 0 && h.stabilization_passes == 0)
		for (int lanes = 2; lanes <= std::min(8, std::max(2, max_lanes)); lanes <<= 1)
			for (int div = 0; div < 3; div++) add(lanes, div, 1);
	float best_ms = 0.0f;
	const LayoutPins *best = nullptr;
	for (size_t ci = 0; ci < cands.size() && rc == MBIK_OK; ci++) {
		p->pins = cands[ci];
		if ((rc = ensure_schedule(p, a.count)) != MBIK_OK) break;
		if (cands[ci].roles && !h.cm_roles) continue; // (not eligible: 64-bit addressing)
		float ms = 0.0f;
		rc = time_launches(p, a, 1, 2, ms, [&] { return copy(false); });
		if (rc == MBIK_OK && (!best || ms < best_ms)) {
			best_ms = ms;
			best = &cands[ci];
		}
	}
	if (rc == MBIK_OK) rc = copy(false);
	if (rc == MBIK_OK && hipStreamSynchronize(a.stream) != hipSuccess) rc = fail(MBIK_EHIP, "hipStreamSynchronize");
	if (rc != MBIK_OK) return rc;
	if (!best) return kNothingTimed;
	p->pins = *best;
	return ensure_schedule(p, a.count);
}

// A fully resident launch (the layout is fixed): with the helper wave left automatic, time the
// launch without and with it and keep the helper only if it is faster beyond the near-tie margin.
// The helper's second wave needs a free SIMD: at most two blocks of it per CU.
int autotune_helper(mbik_plan *p, const LaunchArgs &a) {
	if (p->pins.helper != -1) return MBIK_OK;
	p->pins.helper = 1;
	SolveLaunch sl;
	bool refused;
	{
		const KeepError keep; // (a layout without the helper is no failure)
		refused = resolve_launch(p, a.count, sl) != MBIK_OK;
	}
	if (refused || !sl.helper || (int64_t)sl.blocks > 2 * (int64_t)p->cu_count) {
		p->pins.helper = 0;
		return MBIK_OK;
	}
	float ms[2] = {0.0f, 0.0f};
	int rc = MBIK_OK;
	for (int h = 0; h < 2 && rc == MBIK_OK; h++) {
		p->pins.helper = h;
		rc = time_launches(p, a, 1, 3, ms[h]);
	}
	if (rc == MBIK_OK) rc = take_helper_timeout(p);
	p->pins.helper = rc == MBIK_OK && ms[1] * 1.015f < ms[0] ? 1 : 0;
	return rc;
}

// The layout search of mbik_plan_autotune (plans without constraint_mode).
int autotune_layouts(mbik_plan *p, const LaunchArgs &a) {
	mbik::HostPlan &h = p->host;
	const int64_t count = a.count;
	const LayoutPins pins0 = p->pins;
	if (pins0.roles != 1) {
		// A launch whose skeletons are all resident at the default layout is bound by one
		// skeleton's dependency chain; no layout shortens that, so there is nothing to time.
		p->pins.spw = 0;
		p->pins.interval = 0;
		p->pins.staging = pins0.staging < 0 ? 1 : pins0.staging;
		p->pins.locals = pins0.locals < 0 ? 0 : pins0.locals;
		p->pins.waves = pins0.waves < 0 ? 1 : pins0.waves;
		p->pins.roles = 0;
		int rc0 = ensure_schedule(p, count);
		if (rc0 != MBIK_OK) return rc0;
		if ((int64_t)blocks_per_cu(p, h.lds_block_bytes) * h.spw * p->cu_count >= count && h.g_interval == 1) {
			p->pins.roles = pins0.roles < 0 ? 0 : pins0.roles;
			return autotune_helper(p, a);
		}
	}
	// Candidate layouts: for each heading-staging mode and checkpoint interval, the largest
	// skeletons-per-block at each distinct residency (blocks per CU).  Every layout computes
	// the same bits; only the time differs.
	// Lane counts: the pinned one, or the widest sibling level and half of it (two sibling
	// segments per lane: a longer chain, twice the skeletons per wave).
	// staging 2 (only translating root segments staged) differs from 0 only with such a
	// segment of several headings
	// (3: only segments of two or more effectors)
	bool has_staged_root = false, has_multi_eff = false;
	for (int sg = 0; sg < h.NS; sg++) {
		has_staged_root |= (h.seg_flags[sg] & mbik::SF_TRANSLATE) && h.seg_nh[sg] >= 2;
		has_multi_eff |= h.seg_eff_off[sg + 1] - h.seg_eff_off[sg] >= 2;
	}
	std::vector<int> lane_cands = {pins0.lanes};
	if (pins0.lanes == 0 && h.K >= 2) lane_cands.push_back(h.K / 2);
	std::vector<LayoutPins> cands, rw_cands;
	// Wave roles (one wave per role, a lane per skeleton, 64 per block): the widest sibling level
	// and its halves as the number of waves, within what a CU holds at the register budget.
	// (after the classic candidates, so that a near-tie keeps the classic layout)
	if (pins0.roles != 0 && h.stabilization_passes == 0 && !h.constraint_mode) {
		mbik::build_schedule(h, mbik::LayoutRequest{}, count, nullptr, nullptr, p->cu_count);
		const int widest = h.K;
		for (int wv : {1, 2}) {
			if (pins0.waves > 0 && wv != pins0.waves) continue;
			for (int k : pins0.lanes > 0 ? std::vector<int>{pins0.lanes} : std::vector<int>{widest, widest / 2, widest / 4}) {
				if (k < 2 || k > 4 * wv) continue;
				for (int c : {1, 2}) {
					LayoutPins cand = p->pins;
					cand.spw = 0, cand.interval = c, cand.staging = 0, cand.locals = 2, cand.lanes = k, cand.waves = wv, cand.roles = 1;
					rw_cands.push_back(cand);
				}
			}
		}
	}
	if (pins0.roles != 1)
	for (int wv : {1, 2}) {
	if (pins0.waves > 0 && wv != pins0.waves) continue;
	if (wv == 2 && h.stabilization_passes > 0) continue;
	for (int ln : lane_cands) {
		for (int lh : {0, 1, 2}) {
			if (pins0.locals >= 0 && lh != pins0.locals) continue;
			// a second wave per SIMD only pays where LDS no longer bounds the blocks per CU
			if (wv == 2 && lh == 0 && pins0.locals < 0) continue;
			bool nothing_staged = false;
			for (int stg : {1, 3, 2, 0, 4, 5}) {
				if (pins0.staging >= 0 && stg != pins0.staging) continue;
				if (stg <= 3 && nothing_staged) continue;   // (the same layouts as the first)
				if (stg == 2 && !has_staged_root) continue; // (the same layouts as 0)
				if (stg == 3 && !has_multi_eff) continue;   // (the same layouts as 0)
				if (stg == 4 && !has_multi_eff) continue;   // (the same layouts as 0)
				if (stg == 5 && !(has_multi_eff && has_staged_root)) continue; // (as 4, or as 0)
				// with the whole state in device memory the interval does not change residency, only
				// the checkpoint writes against the rebuild products (C5: 2 is 0.7 % faster than 1)
				const std::vector<int> intervals = lh == 2 ? std::vector<int>{1, 2} : std::vector<int>{1, 2, 4, 1 << 20};
				for (int c : intervals) {
					int last_blocks = -1;
					bool split = true;
					for (int spw = 64; spw >= 1 && split; spw--) {
						mbik::LayoutRequest rq;
						rq.lanes = ln, rq.spw = spw, rq.interval = c;
						rq.staging = stg, rq.state_hbm = lh, rq.waves_per_simd = wv;
						mbik::build_schedule(h, rq, count, blocks_per_cu, p, p->cu_count);
						// 4 / 5 with no segment split over lanes (one lane per skeleton) are 0 / 2
						if (stg >= 4 && !h.has_xs) {
							split = false;
							break;
						}
						if (h.spw != spw) continue; // capped by 64 / K or by LDS
						const int blocks = blocks_per_cu(p, h.lds_block_bytes);
						if (blocks != last_blocks) {
							LayoutPins cand = p->pins;
							cand.spw = spw, cand.interval = c, cand.staging = stg, cand.locals = lh, cand.lanes = ln, cand.waves = wv, cand.roles = 0;
							cands.push_back(cand);
							last_blocks = blocks;
						}
					}
				}
				if (stg <= 3 && h.hs_floats == 0) nothing_staged = true; // nothing is staged: 3, 2, 0 are the same
			}
		}
	}
	}
	cands.insert(cands.end(), rw_cands.begin(), rw_cands.end());
	struct Timed {
		LayoutPins pins; // the candidate, with the skeletons per block and the interval it resolved to
		float ms;
	};
	std::vector<Timed> timed;
	std::vector<LayoutPins> seen; // the candidates' resolved layouts: one timing each
	float best_ms = 0.0f;
	int rc = MBIK_OK;
	for (const LayoutPins &cand : cands) {
		p->pins = cand;
		if ((rc = ensure_schedule(p, count)) != MBIK_OK) {
			// a placement this batch cannot have (device memory, or the 4 GiB buffer limit) is skipped
			if (rc == MBIK_ENOMEM || rc == MBIK_EUNSUPPORTED) {
				rc = MBIK_OK;
				continue;
			}
			break;
		}
		LayoutPins resolved = cand;
		resolved.spw = h.spw;
		resolved.interval = h.g_interval;
		LayoutPins key = resolved;
		key.lanes = h.K;
		key.roles = h.wave_roles;
		if (std::find(seen.begin(), seen.end(), key) != seen.end()) continue;
		seen.push_back(key);
		float ms = 0.0f;
		if ((rc = time_launches(p, a, 1, 2, ms)) != MBIK_OK) break;
		if (timed.empty() || ms < best_ms) best_ms = ms;
		timed.push_back({resolved, ms});
	}
	if (rc != MBIK_OK) return rc;
	if (timed.empty()) return kNothingTimed;
	// Near-ties go to the earliest candidate (a fixed order), not to run-to-run timing noise
	// (~1 %), so that boxes agree on the layout and per-layout evidence stays comparable.
	for (const Timed &c : timed)
		if (c.ms <= best_ms * 1.015f) {
			p->pins = c.pins;
			break;
		}
	return ensure_schedule(p, count);
}
} // namespace

extern "C" int32_t mbik_plan_autotune(mbik_plan *p, int32_t first, int32_t count, const float *pose_in, const float *targets,
		float *pose_out, void *hip_stream) {
	if (!p) return fail(MBIK_EINVAL, "null plan");
	if (count <= 0) return MBIK_OK;
	{
		// every candidate is timed on the same input: an in-place call would advance the
		// caller's pose by one frame per timed run
		const size_t bytes = (size_t)count * p->host.B * 10 * sizeof(float);
		const char *a = reinterpret_cast<const char *>(pose_in), *b = reinterpret_cast<const char *>(pose_out);
		if (a && b && a < b + bytes && b < a + bytes) return fail(MBIK_EINVAL, "autotune needs pose_in and pose_out not to overlap");
	}
	DeviceGuard guard(p->device);
	const LaunchArgs a = full_solve(p, first, count, pose_in, targets, pose_out, reinterpret_cast<hipStream_t>(hip_stream));
	const LayoutPins pins0 = p->pins; // an autotune that fails, or that times nothing, leaves them as the caller set them
	int rc = p->host.constraint_mode ? cmode_autotune(p, a) : autotune_layouts(p, a);
	if (rc != MBIK_OK) {
		// nothing eligible was timed (e.g. wave roles pinned on a plan that cannot have them): the
		// caller's settings stand.  A candidate failed: back to the caller's settings too, and the
		// error stands.
		const std::string err = g_err;
		p->pins = pins0;
		invalidate_layout(p);
		const int rc2 = ensure_schedule(p, count);
		if (rc == kNothingTimed) return rc2;
		g_err = err;
	}
	return rc;
}
