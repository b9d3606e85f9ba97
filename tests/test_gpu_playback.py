"""mbik_playback_advance on the GPU against mbik_playback_advance_cpu, bitwise: the state (through
mbik_playback_read), the layer records, the previous times and the events after every frame of
scripted runs -- skeleton counts around the 64-skeleton block, 1, 2, 3 and 8 slots, commands on the
first and last skeleton of a block and of the crowd and 20 on one skeleton, guard bands around every
output, outputs 8 bytes off a 16-byte boundary, the commands verified unwritten, events given and
not, a crowd smaller than the capacity, write and read of a sub-range, a set destroyed before the
advance, and a small crowd's frame loop on one stream down to skeleton_global."""
import numpy as np
import pytest

from many_bone_ik_amd import _lib
from many_bone_ik_amd import animation as A
from many_bone_ik_amd import workloads as W

from . import playback_recipe as R
from .test_gpu_clip_sample import _rig_clips
from .test_gpu_parity import torch_dev  # noqa: F401 (fixture)

pytestmark = pytest.mark.gpu

GUARD = 256                      # sentinel bytes on each side of every output
SENTINEL = 0xA5
COUNTS = (1, 63, 64, 65, 257)    # 64 skeletons a block (k_playback.hip)
LAYER_COUNTS = (1, 2, 3, 8)
FRAMES = 24
SPARE = 9                        # skeletons of the capacity beyond the crowd
DESC = dict(next=R.NEXT, blend_times=R.blend_table(len(R.CLIPS)), default_blend_time=0.25)


@pytest.fixture(scope="module")
def clipset(mbik):
    with A.ClipSet(1, np.zeros((1, 10), np.float32), R.CLIPS) as cs:
        yield cs


class Guarded:
    """`nbytes` of device memory `off` bytes past an allocation, between guard bands of SENTINEL."""

    def __init__(self, torch, dev, nbytes, off=0):
        self.lo, self.hi = off + GUARD, off + GUARD + nbytes
        self.host = np.full(self.hi + GUARD, SENTINEL, np.uint8)
        self.dev = torch.from_numpy(self.host).to(dev)
        self.ptr = self.dev.data_ptr() + self.lo

    def body(self, dtype, shape):
        got = self.dev.cpu().numpy()
        assert np.array_equal(got[:self.lo], self.host[:self.lo]) and np.array_equal(got[self.hi:], self.host[self.hi:]), "guard band written"
        return got[self.lo:self.hi].view(dtype).reshape(shape)


def device_frame(torch, dev, pb, n, K, delta, speed_scale, cmds, off, events=True, stream=0):
    """One advance into guarded outputs: (layers, time_prev, events or None)."""
    lay, prev, ev = Guarded(torch, dev, n * K * 16, off), Guarded(torch, dev, n * K * 8, off), Guarded(torch, dev, n, off % 3)
    d_c = h_c = None
    if cmds is not None and len(cmds):
        h_c = np.ascontiguousarray(cmds).view(np.uint8).reshape(-1)
        d_c = torch.from_numpy(h_c.copy()).to(dev)
    torch.cuda.synchronize()
    pb.advance(delta, lay.ptr, prev.ptr, n, speed_scale=speed_scale, cmds_ptr=0 if d_c is None else d_c.data_ptr(),
               cmd_count=0 if cmds is None else len(cmds), events_ptr=ev.ptr if events else 0, stream=stream)
    torch.cuda.synchronize()
    if d_c is not None:
        assert np.array_equal(d_c.cpu().numpy(), h_c), "cmds written"
    got_ev = ev.body(np.uint8, (n,))
    if not events:
        assert (got_ev == SENTINEL).all(), "events written without a buffer"
    return lay.body(A.LAYER_DTYPE, (n, K)), prev.body(np.float64, (n, K)), got_ev if events else None


def assert_frame(where, got, want):
    for name, g, w in zip(("state", "flags", "layers", "time_prev", "events"), got, want):
        if g is None:
            continue
        bad = [s for s in range(len(w)) if not R.same_bytes(g[s], w[s])]
        assert not bad, f"{where}: {name} of {len(bad)} skeletons differ; first {bad[0]}: got {g[bad[0]]}, want {w[bad[0]]}"


@pytest.mark.parametrize("n", COUNTS)
def test_device_matches_cpu_entry(clipset, torch_dev, n):
    torch, dev = torch_dev
    seen = 0
    for K in LAYER_COUNTS:
        cap = n + SPARE
        st_all, fl_all = R.initial_state(300 + n + K, cap, K)
        delta, scale = ((1.0 / 60.0, 1.0), (0.25, 1.0), (1.0 / 30.0, -1.5), (0.25, 1.0))[LAYER_COUNTS.index(K)]
        with A.Playback(clipset, cap, K, **DESC) as pb:
            first, _ = pb.read()
            assert R.same_bytes(first, A.empty_state(cap, K)[0]) and not pb.read()[1].any(), "a new object has every slot off"
            pb.write(st_all, fl_all)
            st, fl = st_all[:n].copy(), fl_all[:n].copy()
            for frame, cmds in enumerate(R.script(n + K, n, FRAMES, marks=(0, 63, 64, n - 1))):
                events = frame % 2 == 0
                lay, prev, ev = device_frame(torch, dev, pb, n, K, delta, scale, cmds, off=8 * (frame % 4), events=events)
                st, fl, w_lay, w_prev, w_ev = A.playback_advance_cpu(R.CLIPS, st, fl, delta, scale, cmds=cmds, **DESC)
                g_st, g_fl = pb.read(0, n)
                assert_frame(f"n={n} K={K} frame={frame}", (g_st, g_fl, lay, prev, ev), (st, fl, w_lay, w_prev, w_ev))
                seen |= int(np.bitwise_or.reduce(w_ev))
            # the crowd was smaller than the capacity: the state beyond it is as written
            rest_st, rest_fl = pb.read(n, SPARE)
            assert R.same_bytes(rest_st, st_all[n:]) and np.array_equal(rest_fl, fl_all[n:])
    if n >= 63:
        assert seen == 63, f"events seen {seen:#x}"


@pytest.mark.parametrize("tables", (("next",), ("blend_times",), ()), ids=("next only", "blend_times only", "neither"))
def test_tables_a_desc_leaves_out(clipset, torch_dev, tables):
    """The tables' edge layouts: a desc with `next` only, with `blend_times` only, and none at all (an absent table is a null
    pointer to the per-skeleton code), 5 skeletons through commands and clip ends."""
    torch, dev = torch_dev
    n, K = 5, 2
    desc = {k: DESC[k] for k in tables}
    st, fl = R.initial_state(40 + len(tables), n, K)
    with A.Playback(clipset, n, K, **desc) as pb:
        pb.write(st, fl)
        for frame, cmds in enumerate(R.script(7, n, 8)):
            lay, prev, ev = device_frame(torch, dev, pb, n, K, 0.25, 1.0, cmds, off=0)
            st, fl, w_lay, w_prev, w_ev = A.playback_advance_cpu(R.CLIPS, st, fl, 0.25, 1.0, cmds=cmds, **desc)
            assert_frame(f"{tables} frame={frame}", (*pb.read(), lay, prev, ev), (st, fl, w_lay, w_prev, w_ev))


def test_write_and_read_a_sub_range(clipset, torch_dev):
    K, cap = 3, 200
    st, fl = R.initial_state(5, cap, K)
    with A.Playback(clipset, cap, K) as pb:
        pb.write(st[60:131], fl[60:131], first=60)
        got_st, got_fl = pb.read()
        want_st, want_fl = A.empty_state(cap, K)
        want_st[60:131], want_fl[60:131] = st[60:131], fl[60:131]
        assert R.same_bytes(got_st, want_st) and np.array_equal(got_fl, want_fl)
        sub_st, sub_fl = pb.read(129, 3)
        assert R.same_bytes(sub_st, want_st[129:132]) and np.array_equal(sub_fl, want_fl[129:132])
        # slot 0's fade fields and an off slot's fields are stored as +0
        odd = st[:1].copy()
        odd[0, 0]["blend_left"], odd[0, 0]["blend_time"] = 0.5, 0.5
        odd[0, 2] = (np.nan, -1, 3.0, 3.0, 3.0)
        pb.write(odd, fl[:1])
        back = pb.read(0, 1)[0]
        assert back[0, 0]["blend_left"] == 0 and back[0, 0]["blend_time"] == 0 and R.same_bytes(back[0, 2], A.empty_state(1, 1)[0][0, 0])
        pb.read(cap, 0), pb.write(st[:0], fl[:0], first=cap)


def test_the_set_may_be_destroyed_first(mbik, torch_dev):
    torch, dev = torch_dev
    n, K = 65, 2
    cs = A.ClipSet(1, np.zeros((1, 10), np.float32), R.CLIPS)
    pb = A.Playback(cs, n, K, **DESC)
    cs.close()
    st, fl = R.initial_state(8, n, K)
    pb.write(st, fl)
    for frame, cmds in enumerate(R.script(3, n, 6)):
        lay, prev, ev = device_frame(torch, dev, pb, n, K, 0.25, 1.0, cmds, off=0)
        st, fl, w_lay, w_prev, w_ev = A.playback_advance_cpu(R.CLIPS, st, fl, 0.25, 1.0, cmds=cmds, **DESC)
        assert_frame(f"frame={frame}", (*pb.read(), lay, prev, ev), (st, fl, w_lay, w_prev, w_ev))
    pb.close()


def test_nothing_to_do_and_argument_errors(clipset, torch_dev):
    torch, dev = torch_dev
    n, K = 10, 2
    E = _lib.MBIK_EINVAL

    def code(fn, *args, **k):
        with pytest.raises(_lib.MbikError) as e:
            fn(*args, **k)
        assert str(e.value)
        return e.value.code

    for bad in (dict(capacity=-1, layer_count=2), dict(capacity=4, layer_count=0), dict(capacity=4, layer_count=9),
                dict(capacity=4, layer_count=2, next=[0, 0, 0, 0, 0, 6]), dict(capacity=4, layer_count=2, default_blend_time=-1.0),
                dict(capacity=4, layer_count=2, blend_times=np.full((6, 6), np.nan))):
        assert code(A.Playback, clipset, **bad) == E
    with A.Playback(clipset, 0, 1) as empty:
        empty.advance(0.1, 0, 0, 0)
        assert empty.read()[0].shape == (0, 1)
    with A.Playback(clipset, n, K) as pb:
        st, fl = R.initial_state(1, n, K)
        pb.write(st, fl)
        lay, prev, ev = Guarded(torch, dev, n * K * 16), Guarded(torch, dev, n * K * 8), Guarded(torch, dev, n)
        cm = A.pack_commands([0, 1], [0, 1])
        d_c = torch.from_numpy(cm.view(np.uint8).copy()).to(dev)
        L, P, V, Cm = lay.ptr, prev.ptr, ev.ptr, d_c.data_ptr()
        torch.cuda.synchronize()
        pb.advance(0.1, L, P, 0)                              # count == 0: OK, no launch
        pb.advance(0.1, 0, 0, 0, cmds_ptr=0, cmd_count=3)
        torch.cuda.synchronize()
        assert (lay.body(np.uint8, -1) == SENTINEL).all() and (prev.body(np.uint8, -1) == SENTINEL).all()
        assert R.same_bytes(pb.read()[0], st)
        adv = pb.advance
        assert code(adv, 0.1, 0, P, n) == E and code(adv, 0.1, L, 0, n) == E and code(adv, 0.1, L, P, -1) == E and code(adv, 0.1, L, P, n + 1) == E
        assert code(adv, np.nan, L, P, n) == E and code(adv, np.inf, L, P, n) == E and code(adv, 0.1, L, P, n, speed_scale=np.nan) == E
        assert code(adv, 0.1, L, P, n, cmd_count=-1) == E and code(adv, 0.1, L, P, n, cmd_count=1) == E
        assert code(adv, 0.1, L + 4, P, n - 1) == E and code(adv, 0.1, L, P + 4, n - 1) == E and code(adv, 0.1, L, P, n, cmds_ptr=Cm + 4, cmd_count=1) == E
        assert code(adv, 0.1, L, L + 16, 1) == E and code(adv, 0.1, L, P, n, events_ptr=L + 5) == E and code(adv, 0.1, L, P, n, events_ptr=P + 79) == E
        assert code(adv, 0.1, L, P, n, cmds_ptr=L, cmd_count=1) == E and code(adv, 0.1, L, P, n, cmds_ptr=P, cmd_count=1) == E
        assert code(adv, 0.1, L, P, n, cmds_ptr=Cm, cmd_count=2, events_ptr=Cm + 47) == E
        assert code(pb.read, -1, 2) == E and code(pb.read, n - 1, 2) == E and code(pb.read, 0, -1) == E
        assert code(pb.write, st[:2], fl[:2], first=n - 1) == E
        bad = st.copy()
        bad[3, 0]["pos"] = 99.0
        assert code(pb.write, bad, fl) == E
        bad = st.copy()
        bad[4, 1] = (0.1, 2, 1.0, 0.5, 0.0)
        assert code(pb.write, bad, fl) == E
        assert code(pb.write, st, np.full(n, 8, np.uint32)) == E
        assert R.same_bytes(pb.read()[0], st), "a refused write changed the state"
        adv(0.1, L, P, n, cmds_ptr=Cm, cmd_count=2, events_ptr=V)
        torch.cuda.synchronize()
        want = A.playback_advance_cpu(R.CLIPS, st, fl, 0.1, cmds=cm)
        assert_frame("after the refusals", (*pb.read(), lay.body(A.LAYER_DTYPE, (n, K)), prev.body(np.float64, (n, K)), ev.body(np.uint8, (n,))), want)


def test_a_small_crowd_plays_through_the_frame_loop(mbik, torch_dev):
    """A C2 rig, 130 skeletons, 12 frames on one side stream, two slots: advance -> sample_layers
    (NORMALIZE) -> root_motion_layers (+pose) -> apply_root_motion, the layer records never leaving
    the device.  A third of the crowd switches clips with a blend in frame 3 and the crowd crosses its
    clips' seams inside the run; the poses and skeleton_global must equal the same chain of CPU twins
    bit for bit."""
    torch, dev = torch_dev
    wl = W.generate(2, 130)
    parents = wl.topo.parents.tolist()
    n, B, K = wl.n, len(parents), 2
    root = parents.index(-1)
    rest = np.ascontiguousarray(wl.pose[0])
    clips = _rig_clips(rest, 4)
    for c, clip in enumerate(clips):       # a walk and a turn on the root, at another pace in each clip
        L = clip["length"]
        clip["tracks"] = [t for t in clip["tracks"] if t["bone"] != root]
        yaw = np.radians(40.0 + 30.0 * c) * np.array([0.0, 0.5, 1.0])
        clip["tracks"] += [
            dict(bone=root, channel=A.POSITION, interpolation=A.LINEAR, loop_wrap=1, times=np.array([0.0, 0.4 * L, L]),
                 values=np.array([[0, 0, 0], [0.1, 0, 0.5 + c], [0, 0, 1.5 + 2 * c]], np.float32)),
            dict(bone=root, channel=A.ROTATION, interpolation=A.LINEAR, loop_wrap=1, times=np.array([0.0, 0.5 * L, L]),
                 values=np.stack([0 * yaw, np.sin(yaw / 2), 0 * yaw, np.cos(yaw / 2)], axis=1).astype(np.float32))]
    rng = np.random.default_rng(23)
    st, fl = A.empty_state(n, K)
    st["pos"][:, 0], st["clip"][:, 0], st["speed"][:, 0] = rng.uniform(0.0, clips[0]["length"], n), 0, rng.choice([1.0, 0.5, 2.0], n)
    switch = A.pack_commands(np.arange(0, n, 3), 1, blend_time=0.3)
    delta, flags = 0.1, A.LAYERS_NORMALIZE
    sg = np.tile(np.array([1, 0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0], np.float32), (n, 1))
    sg[:, 9:12] = rng.uniform(-10.0, 10.0, (n, 3)).astype(np.float32)
    with A.ClipSet(B, rest, clips) as cs, A.Playback(cs, n, K) as pb:
        pb.write(st, fl)
        d_sg = torch.from_numpy(sg.copy()).to(dev)
        d_cmd = torch.from_numpy(switch.view(np.uint8).copy()).to(dev)
        d_l = torch.empty(n * K * 16, dtype=torch.uint8, device=dev)
        d_t0 = torch.empty((n, K), dtype=torch.float64, device=dev)
        d_pose = torch.empty((n, B, 10), dtype=torch.float32, device=dev)
        d_m = torch.empty((n, 10), dtype=torch.float32, device=dev)
        stream = torch.cuda.Stream(device=dev)
        torch.cuda.synchronize()
        looped = fading = 0
        for frame in range(12):
            cmds = switch if frame == 3 else None
            s = stream.cuda_stream
            pb.advance(delta, d_l.data_ptr(), d_t0.data_ptr(), n, cmds_ptr=d_cmd.data_ptr() if frame == 3 else 0,
                       cmd_count=len(switch) if frame == 3 else 0, stream=s)
            cs.sample_layers(d_l.data_ptr(), d_pose.data_ptr(), n, K, flags=flags, stream=s)
            cs.root_motion_layers(d_l.data_ptr(), d_t0.data_ptr(), d_m.data_ptr(), n, K, root, flags=flags, pose_ptr=d_pose.data_ptr(), stream=s)
            cs.apply_root_motion(d_m.data_ptr(), d_sg.data_ptr(), n, flags=A.ROOT_MOTION_ORTHONORMALIZE, stream=s)
            stream.synchronize()
            # the CPU twins' frame
            st, fl, layers, t0, ev = A.playback_advance_cpu(clips, st, fl, delta, cmds=cmds)
            pose = A.clip_sample_layers_cpu(B, rest, clips, layers, flags)
            motion = A.clip_root_motion_layers_cpu(B, rest, clips, layers, t0, root, flags, pose=pose)
            sg = A.root_motion_apply_cpu(motion, sg, A.ROOT_MOTION_ORTHONORMALIZE)
            looped += int((ev & R.LOOPED != 0).sum())
            fading += int((layers["clip"][:, 1] != -1).sum())
            assert R.same_bytes(d_l.cpu().numpy().view(A.LAYER_DTYPE).reshape(n, K), layers), f"frame {frame}: layers"
            assert R.same_bytes(d_t0.cpu().numpy(), t0), f"frame {frame}: time_prev"
            assert R.same_bytes(d_pose.cpu().numpy(), pose), f"frame {frame}: poses"
            assert R.same_bytes(d_sg.cpu().numpy(), sg), f"frame {frame}: skeleton_global"
        assert_frame("the state at the end", pb.read(), (st, fl))
        assert looped >= 10 and fading >= 2 * len(switch) and np.isfinite(sg).all()
