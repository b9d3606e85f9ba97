"""Harness shared by the sub-range / in-place / guard-band tests (tests/test_gpu_solve_ranges.py,
tests/test_gpu_group.py): the half of include/mbik.h's contract that a whole-plan launch into an
exactly sized buffer never exercises.

mbik_solve, mbik_solve_checked, mbik_segment_solve and mbik_group_solve take `first, count`, their
buffers are "indexed from skeleton `first`", and pose_out may equal pose_in.  A launch here runs
on device buffers of G + N + G skeletons:

  * G = 64 guard skeletons on each side.  64 is the largest number of skeletons one block owns in
    any layout, so a write that is off by a whole block lands inside the allocation and is seen,
    not faulted on.  The non-finite flags get `count` bytes between 64 guard bytes, preset to 7.
  * every float of the output is preset to one non-NaN sentinel bit pattern; after the launch
    every float outside rows [a, a + c) must still hold exactly those bits;
  * out of place, pose_in and targets hold the workload's rows in [a, a + c) and NaN everywhere
    else, so a read from a wrong row cannot produce the right bits, and both must come back
    unchanged bit for bit; in place there is one pose buffer, sentinels outside the range;
  * every pointer handed to the library is the buffer's row G + a;
  * the expectation is always the oracle's result for the whole workload, sliced -- never another
    call into the library.  W.generate(cfg, n, first=F) is a window of one seeded sequence, so
    ref[a:a + c] is the oracle's answer for the sub-range.
"""
import numpy as np

from many_bone_ik_amd import workloads as W
from many_bone_ik_amd.solver import Plan

from .test_gpu_degenerate import assert_equal_nan_aware
from .test_gpu_edge_cases import CASES
from .test_gpu_parity import assert_parity

G = 64
SENTINEL = np.float32(-12345.678)
SENTINEL_BITS = int(SENTINEL.view(np.uint32))
FLAG_PRESET = 7
FIRST = 70000           # where the rigs' windows of the seeded sequence start

# rig -> (skeletons, the ranges (a, c) that reach every edge at that size)
RIGS = {
    # constraints and twist; 83 is no multiple of 16 or 64
    "C2": (83, [(0, 83),     # control
                (1, 1),      # smallest launch at a non-zero first
                (15, 18),    # starts one before a 16-tile boundary, ends one past the next
                (17, 66),    # ends at N; 8 per block: 8 permuted blocks, an unpermuted tail with 2 of 8 valid
                (82, 1)]),   # the last skeleton
    # 200 bones, packed sibling levels, K = 8 roles
    "C5": (21, [(0, 21), (15, 6), (20, 1)]),
    # the one rig with bones outside the IK bone list (3 and 4): the pass-through copy
    "dropped_branch": (21, [(0, 21), (15, 6), (20, 1)]),
}


def workload(rig, first=FIRST, n=None):
    n = RIGS[rig][0] if n is None else n
    if rig == "dropped_branch":
        parents, pins, cons, ncones, twist = CASES[rig]
        return W.generate(11, n, first=first, topo=W.custom_topology(parents, pins, cons, cones_per_bone=ncones, twist=twist))
    return W.generate(int(rig[1:]), n, first=first)


# Kernel families, each selected with the public setters.  layout: mbik_plan_set_layout's
# arguments; info: the mbik_plan_get_info fields that show the intended kernel ran.  (Classic
# layouts report min(pinned skeletons per block, 64 / lanes); check_family works that out.)
FAMILIES = {
    "classic_pl0": dict(layout=(0, 3, 0), info=dict(wave_roles=0, helper_wave=0, state_placement=0, waves_per_simd=1)),
    "classic_pl1_w2": dict(layout=(0, 8, 0), placement=1, waves=2,
                           info=dict(wave_roles=0, helper_wave=0, state_placement=1, waves_per_simd=2)),
    "classic_pl2_w1": dict(layout=(0, 8, 0), placement=2, waves=1,
                           info=dict(wave_roles=0, helper_wave=0, state_placement=2, waves_per_simd=1)),
    "classic_pl2_w2": dict(layout=(0, 8, 0), placement=2, waves=2,
                           info=dict(wave_roles=0, helper_wave=0, state_placement=2, waves_per_simd=2)),
    "split_exchange": dict(layout=(0, 8, 0), staging=4, waves=2,
                           info=dict(wave_roles=0, heading_staging=4, state_placement=0, waves_per_simd=2)),
    "helper_wave": dict(layout=(0, 2, 0), helper=1, info=dict(wave_roles=0, helper_wave=1, state_placement=0, waves_per_simd=1)),
    "roles_k2": dict(layout=(2, 8, 0), waves=1, roles=1,
                     info=dict(wave_roles=1, lanes_per_skeleton=2, skeletons_per_block=8, state_placement=2, waves_per_simd=1)),
    "roles_k4": dict(layout=(4, 8, 0), waves=2, roles=1,
                     info=dict(wave_roles=1, lanes_per_skeleton=4, skeletons_per_block=8, state_placement=2, waves_per_simd=2)),
    "roles_k8": dict(layout=(8, 8, 0), waves=2, roles=1,
                     info=dict(wave_roles=1, lanes_per_skeleton=8, skeletons_per_block=8, state_placement=2, waves_per_simd=2)),
    "stabilization": dict(plan=dict(stabilization_passes=2), layout=(0, 5, 0), ref="stab2",
                          info=dict(wave_roles=0, helper_wave=0, state_placement=0, waves_per_simd=1)),
    # (mbik_plan_get_info has no field for the table addressing: check_family shows the 64-bit
    # instantiation is selected by the refusal of placement 1, which needs 32-bit tables)
    "table64": dict(layout=(0, 8, 0), tab64=1, info=dict(wave_roles=0, helper_wave=0, state_placement=0, waves_per_simd=1)),
    # constraint_mode: a plan created with it launches cmode.h's kernels and nothing else; the
    # classic one reports 64 / lanes skeletons per block whatever the launch's real block shape
    "cmode_classic": dict(plan=dict(constraint_mode=True), layout=(4, 3, 0), ref="cmode",
                          info=dict(wave_roles=0, lanes_per_skeleton=4, skeletons_per_block=16, state_placement=0)),
    "cmode_roles": dict(plan=dict(constraint_mode=True), layout=(4, 8, 0), roles=1, ref="cmode",
                        info=dict(wave_roles=1, lanes_per_skeleton=4, skeletons_per_block=8, state_placement=0)),
}


def ref_kwargs(family):
    """The oracle's configuration of a family's plans."""
    return {"plain": {}, "stab2": dict(stabilization_passes=2), "cmode": dict(constraint_mode=True)}[FAMILIES[family].get("ref", "plain")]


def make_plan(wl, family):
    f = FAMILIES[family]
    plan = Plan.from_workload(wl, **f.get("plan", {}))
    plan.set_layout(*f["layout"])
    if "placement" in f:
        plan.set_locals_placement(f["placement"])
    if "waves" in f:
        plan.set_waves_per_simd(f["waves"])
    if "staging" in f:
        plan.set_heading_staging(f["staging"])
    if "helper" in f:
        plan.set_helper_wave(f["helper"])
    if "roles" in f:
        plan.set_wave_roles(f["roles"])
    if "tab64" in f:
        plan.set_table_addressing(f["tab64"])
    return plan


def check_family(plan, family):
    """After a launch: mbik_plan_get_info shows the family's layout was in effect."""
    from many_bone_ik_amd import _lib
    f = FAMILIES[family]
    info = plan.info()
    for k, v in f["info"].items():
        assert info[k] == v, f"{family}: {k} is {info[k]}, not {v}: {info}"
    if "skeletons_per_block" not in f["info"]:
        want = min(f["layout"][1], 64 // info["lanes_per_skeleton"])
        assert info["skeletons_per_block"] == want, f"{family}: {info}"
    if f.get("tab64"):
        # a combination the library refuses: placements 1 and 2 need 32-bit tables
        import torch
        pose = torch.zeros((1, info["bone_count"], 10), dtype=torch.float32, device="cuda:0")
        tg = torch.zeros((1, info["pin_count"], 12), dtype=torch.float32, device="cuda:0")
        plan.set_locals_placement(1)
        try:
            plan.solve(pose.data_ptr(), tg.data_ptr(), pose.data_ptr(), 0, 1)
            refused = None
        except _lib.MbikError as e:
            refused = e.code
        plan.set_locals_placement(0)
        torch.cuda.synchronize()
        assert refused == _lib.MBIK_EUNSUPPORTED, f"64-bit table indices with placement 1: {refused}"


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


class RangeBuffers:
    """The device buffers of one rig shape, allocated once and refilled for every launch."""

    def __init__(self, torch, dev, n, bones, pins):
        self.torch, self.dev, self.n, self.bones, self.pins = torch, dev, n, bones, pins
        rows = G + n + G
        self.pose_in = torch.empty((rows, bones, 10), dtype=torch.float32, device=dev)
        self.pose_out = torch.empty((rows, bones, 10), dtype=torch.float32, device=dev)
        self.targets = torch.empty((rows, pins, 12), dtype=torch.float32, device=dev)
        self.flags = torch.empty(G + n + G, dtype=torch.uint8, device=dev)

    @classmethod
    def of(cls, torch, dev, wl):
        return cls(torch, dev, wl.n, wl.pose.shape[1], wl.targets.shape[1])


class RangeCase:
    """One launch on range [a, a + c): fills the buffers, hands out the pointers of row G + a,
    and checks everything the launch may and may not have touched."""

    def __init__(self, bufs, pose, targets, a, c, in_place):
        assert pose.shape[0] == bufs.n and targets.shape[0] == bufs.n and 0 <= a and a + c <= bufs.n
        self.b, self.a, self.c, self.in_place = bufs, a, c, in_place
        torch = bufs.torch
        lo, hi = G + a, G + a + c
        self.h_in = np.full(tuple(bufs.pose_in.shape), np.nan, np.float32)
        self.h_in[lo:hi] = pose[a:a + c]
        self.h_tg = np.full(tuple(bufs.targets.shape), np.nan, np.float32)
        self.h_tg[lo:hi] = targets[a:a + c]
        h_out = np.full(tuple(bufs.pose_out.shape), SENTINEL, np.float32)
        if in_place:
            h_out[lo:hi] = pose[a:a + c]
        bufs.pose_in.copy_(torch.from_numpy(self.h_in))
        bufs.targets.copy_(torch.from_numpy(self.h_tg))
        bufs.pose_out.copy_(torch.from_numpy(h_out))
        bufs.flags.fill_(FLAG_PRESET)
        torch.cuda.synchronize()
        self.pose_out_ptr = bufs.pose_out.data_ptr() + lo * bufs.bones * 40
        self.pose_in_ptr = self.pose_out_ptr if in_place else bufs.pose_in.data_ptr() + lo * bufs.bones * 40
        self.targets_ptr = bufs.targets.data_ptr() + lo * bufs.pins * 48
        self.flags_ptr = bufs.flags.data_ptr() + G

    def check(self, ref, what, flags_want=None, nan_aware=False):
        """ref: the expectation for the whole workload [N][bones][10] (rows [a, a + c) are read).
        flags_want: the c flag bytes of a checked launch; None: no flag byte may have changed."""
        b, a, c = self.b, self.a, self.c
        b.torch.cuda.synchronize()
        lo, hi = G + a, G + a + c
        out = b.pose_out.cpu().numpy()
        errors = []
        ob = bits(out)
        outside = np.ones(ob.shape[0], bool)
        outside[lo:hi] = False
        touched = np.argwhere(ob[outside] != SENTINEL_BITS)
        if touched.size:
            rows = np.flatnonzero(outside)[touched[:, 0]] - G
            errors.append(f"{len(touched)} floats outside [{a}, {a + c}) lost the sentinel; skeleton rows "
                          f"{sorted(set(rows.tolist()))[:8]} (relative to the buffer's skeleton 0)")
        if not self.in_place and not np.array_equal(bits(b.pose_in.cpu().numpy()), bits(self.h_in)):
            errors.append("pose_in was written")
        if not np.array_equal(bits(b.targets.cpu().numpy()), bits(self.h_tg)):
            errors.append("targets were written")
        fl = b.flags.cpu().numpy()
        guard = np.concatenate([fl[:G], fl[G + (c if flags_want is not None else 0):]])
        if not (guard == FLAG_PRESET).all():
            errors.append(f"{int((guard != FLAG_PRESET).sum())} flag guard bytes changed")
        if flags_want is not None and not np.array_equal(fl[G:G + c], np.asarray(flags_want, np.uint8)):
            errors.append(f"flags {fl[G:G + c].tolist()}, expected {np.asarray(flags_want).tolist()}")
        try:
            if c:       # (an empty range: nothing but the sentinels to check)
                (assert_equal_nan_aware if nan_aware else assert_parity)(out[lo:hi], np.ascontiguousarray(ref[a:a + c]), "poses")
        except AssertionError as e:
            errors.append(str(e))
        assert not errors, f"{what}: " + "; ".join(errors)


def run_range(plan, wl, ref, a, c, in_place, checked=False, stream=0, *, bufs=None, pose=None, targets=None,
              flags_want=None, nan_aware=False, segment=None, what=""):
    """Solves skeletons [a, a + c) of `plan` on guarded, poisoned buffers and checks the launch
    against ref[a:a + c] (the oracle's result for the whole workload).  pose / targets: this
    frame's inputs for the whole workload (default: the workload's); segment: mbik_segment_solve
    of that segment (always in place) instead of mbik_solve; checked: mbik_solve_checked, with
    flags_want (default all zero) the expected flag bytes."""
    import torch
    if bufs is None:
        bufs = RangeBuffers.of(torch, torch.device("cuda", 0), wl)
    case = RangeCase(bufs, wl.pose if pose is None else pose, wl.targets if targets is None else targets, a, c,
                     in_place or segment is not None)
    if segment is not None:
        plan.segment_solve(segment, case.pose_out_ptr, case.targets_ptr, a, c, stream)
    elif checked:
        flags_want = np.zeros(c, np.uint8) if flags_want is None else flags_want
        plan.solve_checked(case.pose_in_ptr, case.targets_ptr, case.pose_out_ptr, case.flags_ptr, a, c, stream)
    else:
        plan.solve(case.pose_in_ptr, case.targets_ptr, case.pose_out_ptr, a, c, stream)
    case.check(ref, f"{what} [{a}, {a + c}) {'in place' if case.in_place else 'out of place'}", flags_want, nan_aware)
    return bufs


def frame_runs(n, frames):
    """Contiguous runs [lo, hi) of skeletons that take part in the same set of frames."""
    member = np.zeros((len(frames), n), bool)
    for f, (a, c) in enumerate(frames):
        member[f, a:a + c] = True
    cuts = [0] + [s for s in range(1, n) if (member[:, s] != member[:, s - 1]).any()] + [n]
    return list(zip(cuts[:-1], cuts[1:]))


def run_cmode_frames(oracle, plan, rig, frames, in_place, seed, family, stream=0):
    """constraint_mode's node caches are per skeleton and outlive a frame, so a sub-range frame
    must advance exactly the caches of its skeletons.  Runs `frames` (ranges) on one plan and one
    set of buffers.  The reference is one oracle object graph per run of skeletons that share the
    same frames, stepped only on the frames that include it; a frame's input is the previous
    output, animated (test_gpu_constraint_mode.animate), and a skeleton left out of a frame keeps
    its pose as its input for the next frame it is in."""
    from .test_gpu_constraint_mode import animate
    wl = workload(rig)
    rng = np.random.default_rng(seed)
    runs = frame_runs(wl.n, frames)
    graphs = [oracle.Oracle(workload(rig, first=FIRST + lo, n=hi - lo), constraint_mode=True) for lo, hi in runs]
    cur = wl.pose.copy()
    bufs = None
    for f, (a, c) in enumerate(frames):
        ref = np.full_like(cur, np.nan)
        for (lo, hi), o in zip(runs, graphs):
            if a <= lo and hi <= a + c:
                ref[lo:hi] = o.solve(np.ascontiguousarray(cur[lo:hi]), np.ascontiguousarray(wl.targets[lo:hi]), threads=4)
            else:
                assert hi <= a or lo >= a + c, "a run is wholly inside or outside a frame"
        bufs = run_range(plan, wl, ref, a, c, in_place, stream=stream, bufs=bufs, pose=cur, what=f"{family} frame {f}")
        check_family(plan, family)
        cur[a:a + c] = animate(ref[a:a + c], rng)
    for o in graphs:
        o.close()
