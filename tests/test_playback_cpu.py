"""mbik_playback_advance_cpu against tests/playback_recipe.py's restatement of rules A to D, bitwise:
state, flags, layer records, previous times and events after every frame of scripted runs -- 1, 2, 3
and 8 slots, looping and non-looping clips of three lengths, short, long and empty frames, backward
playback, every kind of command, clip-to-clip transitions -- and the refusals, symbols and constants."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from many_bone_ik_amd import _lib
from many_bone_ik_amd import animation as A

from . import playback_recipe as R

HEADER = os.path.join(os.path.dirname(os.path.dirname(__file__)), "include", "mbik.h")
COUNT, FRAMES = 37, 48
# (delta, speed_scale): a 60 Hz frame, frames longer than a clip, an empty frame, backward
PACES = ((1.0 / 60.0, 1.0), (0.25, 1.0), (0.0, 1.0), (1.0 / 60.0, -1.5), (0.25, -1.0))


def run_both(K, delta, speed_scale, frames=FRAMES, count=COUNT, seed=0, desc=True):
    """Runs the script through the entry and the recipe, comparing everything after every frame;
    returns the OR of all events and the entry's last outputs."""
    kw = dict(next=R.NEXT, blend_times=R.blend_table(len(R.CLIPS)), default_blend_time=0.25) if desc else {}
    st, fl = R.initial_state(100 + K + seed, count, K)
    model = R.Model(R.CLIPS, count, K, **kw)
    model.load(st, fl)
    seen, every = 0, []
    with np.errstate(all="ignore"):
        for frame, cmds in enumerate(R.script(7 * K + seed, count, frames)):
            st, fl, layers, prev, ev = A.playback_advance_cpu(R.CLIPS, st, fl, delta, speed_scale, cmds=cmds, **kw)
            want_layers, want_prev, want_ev = model.advance(delta, speed_scale, cmds)
            want_st, want_fl = model.state()
            where = f"K={K} delta={delta} scale={speed_scale} frame={frame}"
            bad = [s for s in range(count) if not R.same_bytes(st[s], want_st[s])]
            assert not bad, f"{where}: state of skeleton {bad[0]}: got {st[bad[0]]}, want {want_st[bad[0]]}"
            assert np.array_equal(fl, want_fl), where
            bad = [s for s in range(count) if not R.same_bytes(layers[s], want_layers[s])]
            assert not bad, f"{where}: layers of skeleton {bad[0]}: got {layers[bad[0]]}, want {want_layers[bad[0]]}"
            assert R.same_bytes(prev, want_prev), where
            assert np.array_equal(ev, want_ev), f"{where}: events {ev} != {want_ev}"
            seen |= int(np.bitwise_or.reduce(ev))
            every.append((st, fl, layers, prev, ev))
    return seen, every


@pytest.mark.parametrize("K", (1, 2, 3, 8))
@pytest.mark.parametrize("pace", PACES, ids=lambda p: f"dt{p[0]:.3f}x{p[1]}")
def test_entry_matches_recipe(mbik, K, pace):
    seen, every = run_both(K, *pace)
    want = R.STARTED | R.BAD_COMMAND | R.FADE_DROPPED
    if pace[0] > 0:
        want |= R.LOOPED | R.ENDED | R.TRANSITIONED
    assert seen & want == want, f"events seen {seen:#x}"
    # the state stays what mbik_playback_write accepts: compact, slot 0 without fade fields, off slots all +0
    for st, fl, layers, prev, ev in every:
        on = st["clip"] != -1
        assert not (on[:, 1:] & ~on[:, :-1]).any()
        assert not st["blend_left"][:, 0].any() and not st["blend_time"][:, 0].any()
        off = st[~on]
        assert R.same_bytes(off, np.array([(0.0, -1, 0.0, 0.0, 0.0)] * len(off), A.SLOT_DTYPE))
        assert ((layers["clip"] == st["clip"]) | (ev[:, None] & (R.TRANSITIONED) != 0)).all()


def test_without_a_desc(mbik):
    seen, _ = run_both(3, 0.25, 1.0, frames=16, desc=False)
    assert seen & R.ENDED and not seen & R.TRANSITIONED


def frames_of(clips, st, fl, n, delta, **kw):
    out = []
    for _ in range(n):
        st, fl, layers, prev, ev = A.playback_advance_cpu(clips, st, fl, delta, **kw)
        out.append((st, fl, layers, prev, ev))
    return out


def test_ended_is_raised_exactly_once(mbik):
    clips = [dict(length=0.7, loop_mode=0, tracks=[])]
    st, fl = A.empty_state(2, 2)
    st[0, 0] = (0.0, 0, 1.0, 0, 0)
    st[1, 0] = (0.7, 0, -1.0, 0, 0)
    run = frames_of(clips, st, fl, 10, 0.25)
    for s, end in ((0, 0.7), (1, 0.0)):
        ended = [bool(f[4][s] & R.ENDED) for f in run]
        assert ended == [False, False, True] + [False] * 7
        assert all(f[1][s] == R.ENDED for f in run[2:]) and all(f[0][s, 0]["pos"] == end for f in run[2:])
        assert all(f[2][s, 0]["time"] == end and f[3][s, 0] == end for f in run[3:])


def test_next_chains(mbik):
    """a -> b -> a, a clip that follows itself, and a looping clip whose successor is never taken."""
    clips = R.CLIPS
    st, fl = A.empty_state(3, 2)
    st[0, 0], st[1, 0], st[2, 0] = (0.0, 1, 1.0, 0, 0), (0.0, 5, 2.0, 0, 0), (0.0, 0, 1.0, 0, 0)
    run = frames_of(clips, st, fl, 40, 0.25, next=R.NEXT, default_blend_time=0.3)
    order = [int(f[0][0, 0]["clip"]) for f in run]
    assert [c for i, c in enumerate(order) if i == 0 or order[i - 1] != c][:4] == [1, 3, 1, 3]
    assert {int(f[0][1, 0]["clip"]) for f in run} == {5} and sum(bool(f[4][1] & R.TRANSITIONED) for f in run) >= 4
    assert {int(f[0][2, 0]["clip"]) for f in run} == {0} and not any(f[4][2] & (R.TRANSITIONED | R.ENDED) for f in run)
    assert any(f[4][2] & R.LOOPED for f in run)
    # the frame after a transition shows the successor's start, with the clip that ended fading out from its end
    k = next(i for i, f in enumerate(run) if f[4][0] & R.TRANSITIONED)
    assert run[k][2][0, 0]["time"] == 1.0 and run[k][2][0, 0]["clip"] == 1
    after = run[k + 1]
    assert after[4][0] & R.STARTED and after[2][0, 0]["clip"] == 3 and after[2][0, 0]["time"] == 0.0 and after[3][0, 0] == 0.0
    assert after[2][0, 1]["clip"] == 1 and after[2][0, 1]["time"] == 1.0 and 0 < after[2][0, 1]["weight"] < 1


def test_one_layer_with_a_blend_time_drops_the_fade(mbik):
    st, fl = A.empty_state(1, 1)
    st[0, 0] = (0.2, 0, 1.0, 0, 0)
    st, fl, layers, prev, ev = A.playback_advance_cpu(R.CLIPS, st, fl, 0.01, cmds=A.pack_commands([0], [2], blend_time=0.5))
    assert ev[0] == R.FADE_DROPPED | R.STARTED and layers[0, 0].tolist() == (0.0, 2, 1.0)


def code(fn, *args, **kw):
    with pytest.raises(_lib.MbikError) as e:
        fn(*args, **kw)
    assert str(e.value)
    return e.value.code


def test_refusals(mbik):
    E = _lib.MBIK_EINVAL
    clips = R.CLIPS
    adv = A.playback_advance_cpu

    def state(K=3):
        st, fl = A.empty_state(4, K)
        st[1, 0] = (0.5, 0, 1.0, 0, 0)
        st[1, 1] = (0.5, 1, 1.0, 0.5, 0.2)
        return st, fl

    st, fl = state()
    adv(clips, st, fl, 0.1)
    for field, slot, value in (("clip", 0, len(clips)), ("clip", 0, -2), ("pos", 0, -0.1), ("pos", 0, 0.7000001), ("pos", 0, np.nan),
                               ("pos", 1, np.inf), ("speed", 0, np.inf), ("speed", 1, np.nan), ("blend_time", 1, 0.0), ("blend_time", 1, -1.0),
                               ("blend_time", 1, np.inf), ("blend_time", 1, np.nan), ("blend_left", 1, np.inf), ("blend_left", 1, np.nan)):
        st, fl = state()
        st[1, slot][field] = value
        assert code(adv, clips, st, fl, 0.1) == E, (field, slot, value)
    st, fl = state()
    st[1, 0]["clip"] = -1                                    # an on fade behind an off slot 0
    assert code(adv, clips, st, fl, 0.1) == E
    st, fl = state()
    st[2, 2] = (0.1, 0, 1.0, 0.5, 0.2)                       # not compact
    assert code(adv, clips, st, fl, 0.1) == E
    st, fl = state()
    fl[3] = 4                                                # unknown flag bits
    assert code(adv, clips, st, fl, 0.1) == E
    st, fl = state()
    st[0, 1] = (np.nan, -1, np.nan, np.nan, np.nan)          # an off slot's other fields are not looked at, and stored as +0
    got = adv(clips, st, fl, 0.1)[0]
    assert R.same_bytes(got[0], A.empty_state(1, 3)[0][0])
    for bad in (np.nan, np.inf, -np.inf):
        assert code(adv, clips, st, fl, bad) == E and code(adv, clips, st, fl, 0.1, speed_scale=bad) == E
    assert code(adv, clips, st, fl, 0.1, next=[0, 0, 0, 0, 0, len(clips)]) == E and code(adv, clips, st, fl, 0.1, next=[-2, 0, 0, 0, 0, 0]) == E
    for bad in (-0.5, np.nan, np.inf):
        t = R.blend_table(len(clips))
        t[2, 3] = bad
        assert code(adv, clips, st, fl, 0.1, blend_times=t) == E and code(adv, clips, st, fl, 0.1, default_blend_time=bad) == E
    assert code(adv, [dict(length=0.0, loop_mode=0)], *A.empty_state(1, 1), 0.1) == E
    assert code(adv, [dict(length=1.0, loop_mode=2)], *A.empty_state(1, 1), 0.1) == E
    # the raw entry: counts, null buffers, alignment, overlap, the desc's size
    L = mbik
    descs, keep = A._descs(clips)
    st, fl = state(2)
    lay, prev, ev = np.empty((4, 2), A.LAYER_DTYPE), np.empty((4, 2), np.float64), np.empty(4, np.uint8)
    cm = A.pack_commands([0, 1], [0, 1])
    P = lambda a: None if a is None else a.ctypes.data
    def raw(count=4, K=2, slots=st, flags=fl, cmds=None, n_cmds=0, layers=P(lay), time_prev=P(prev), events=P(ev), desc=None, clip_count=len(clips), cl=descs):
        return L.mbik_playback_advance_cpu(clip_count, cl, desc, count, K, P(slots) if isinstance(slots, np.ndarray) else slots,
                                           P(flags) if isinstance(flags, np.ndarray) else flags, 0.1, 1.0, cmds, n_cmds, layers, time_prev, events)
    assert raw() == 0 and raw(events=None) == 0 and raw(cmds=P(cm), n_cmds=2) == 0
    assert raw(count=0, slots=None, flags=None, layers=None, time_prev=None) == 0
    assert raw(count=-1) == E and raw(K=0) == E and raw(K=9) == E and raw(clip_count=0) == E and raw(cl=None) == E
    assert raw(slots=None) == E and raw(flags=None) == E and raw(layers=None) == E and raw(time_prev=None) == E
    assert raw(cmds=None, n_cmds=1) == E and raw(cmds=P(cm), n_cmds=-1) == E
    assert raw(layers=P(lay) + 4, count=3) == E and raw(time_prev=P(prev) + 4, count=3) == E and raw(cmds=P(cm) + 4, n_cmds=1) == E
    assert raw(time_prev=P(lay) + 16) == E and raw(events=P(lay) + 3) == E and raw(events=P(prev) + 8 * 7) == E
    assert raw(cmds=P(lay), n_cmds=1) == E and raw(cmds=P(prev), n_cmds=1) == E and raw(cmds=P(cm), n_cmds=2, events=P(cm) + 47) == E
    assert L.mbik_last_error()
    d = _lib.MbikPlaybackDesc()
    d.struct_size = C.sizeof(_lib.MbikPlaybackDesc) - 1
    assert raw(desc=C.byref(d)) == E
    d.struct_size = C.sizeof(_lib.MbikPlaybackDesc) + 8      # a newer caller's larger struct
    assert raw(desc=C.byref(d)) == 0
    # the device entries refuse a null handle before they touch a device
    out = C.c_void_p()
    assert L.mbik_playback_create(None, 4, 2, None, C.byref(out)) == E and L.mbik_playback_create(None, 4, 2, None, None) == E
    assert L.mbik_playback_advance(None, 0, 0.1, 1.0, None, 0, None, None, None, None) == E
    assert L.mbik_playback_write(None, 0, 0, None, None) == E and L.mbik_playback_read(None, 0, 0, None, None) == E
    L.mbik_playback_destroy(None)
    del keep


def test_commands_are_packed_sorted_and_stable():
    cm = A.pack_commands([5, 1, 5, 0, 1], [0, 1, 2, 3, 4], start=[0.1, 0.2, 0.3, 0.4, 0.5], speed=2.0)
    assert cm.dtype == A.CMD_DTYPE and cm.itemsize == 24
    assert cm["skeleton"].tolist() == [0, 1, 1, 5, 5] and cm["clip"].tolist() == [3, 1, 4, 0, 2]
    assert cm["start"].tolist() == [0.4, 0.2, 0.5, 0.1, 0.3] and (cm["speed"] == 2.0).all() and (cm["blend_time"] == -1.0).all()
    one = A.pack_commands([3], [A.PLAYBACK_STOP])
    assert np.isnan(one["start"][0]) and one["clip"][0] == -1


def test_symbols_constants_and_abi(mbik):
    header = open(HEADER).read()
    for name in ("mbik_playback_create", "mbik_playback_destroy", "mbik_playback_write", "mbik_playback_read", "mbik_playback_advance",
                 "mbik_playback_advance_cpu"):
        assert name in _lib.EXPORTED_SYMBOLS and getattr(mbik, name) and name + "(" in header
    assert re.search(r"#define MBIK_ABI_VERSION 15\b", header)
    for name, value in (("STARTED", 1), ("ENDED", 2), ("LOOPED", 4), ("TRANSITIONED", 8), ("BAD_COMMAND", 16), ("FADE_DROPPED", 32)):
        assert re.search(rf"#define MBIK_PLAYBACK_{name} {value}u\b", header)
        assert getattr(A, "PLAYBACK_" + name) == getattr(_lib, "PLAYBACK_" + name) == getattr(R, name) == value
    assert C.sizeof(_lib.MbikPlaybackSlot) == A.SLOT_DTYPE.itemsize == 24 and C.sizeof(_lib.MbikPlaybackCmd) == A.CMD_DTYPE.itemsize == 24
    for struct, dtype in ((_lib.MbikPlaybackSlot, A.SLOT_DTYPE), (_lib.MbikPlaybackCmd, A.CMD_DTYPE)):
        for name, _ in struct._fields_:
            assert getattr(struct, name).offset == dtype.fields[name][1], name
    assert C.sizeof(_lib.MbikPlaybackDesc) == 24
