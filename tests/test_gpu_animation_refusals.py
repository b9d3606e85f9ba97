"""The device entries of the animation front end against the refusal ledger (tests/test_animation_refusals_cpu.py).

One tiny shaped clip set (B = 2, 2 clips, P = 1), one set without shapes and one playback object
(capacity 4, K = 2).  Every fault of a call's arguments that a device entry shares with its _cpu form
is refused with the code and text the golden file holds for the _cpu form; the refusals only a live
handle can give are pinned to their texts here; no refused call writes a byte of device memory.  One
valid call of each device entry at count = 4 then equals its _cpu form bit for bit.
"""
import ctypes as C

import numpy as np
import pytest

from many_bone_ik_amd import _lib
from many_bone_ik_amd import animation as A

from . import test_animation_refusals_cpu as T
from .test_animation_refusals_cpu import golden  # noqa: F401 (fixture)
from .test_gpu_parity import torch_dev  # noqa: F401 (fixture)

pytestmark = pytest.mark.gpu

DEVICE_FORM = {"sample_cpu": "sample", "sample_layers_cpu": "sample_layers", "sample_shapes_cpu": "sample_shapes",
               "sample_shapes_layers_cpu": "sample_shapes_layers", "root_motion_cpu": "root_motion",
               "root_motion_layers_cpu": "root_motion_layers", "root_apply_cpu": "root_apply", "advance_cpu": "advance"}
# what each valid call writes
OUTPUTS = {"sample": ("pose_out",), "sample_layers": ("pose_out",), "sample_shapes": ("weights_out",), "sample_shapes_layers": ("weights_out",),
           "root_motion": ("motion_out", "pose"), "root_motion_layers": ("motion_out", "pose"), "root_apply": ("skeleton_global",),
           "advance": ("layers_out", "time_prev_out", "events_out")}
PLAYING = {"state": {(0, 0): dict(clip=0, pos=0.2, speed=1.0), (1, 0): dict(clip=1, pos=0.9, speed=2.0),
                     (1, 1): dict(clip=0, pos=0.1, speed=1.0, blend_left=0.2, blend_time=0.5)}}


class Arena:
    """The buffers of one call in one device allocation, with a host image to compare it against."""

    def __init__(self, torch, dev, nbytes=32 * 1024):
        self.torch, self.host, self.used = torch, np.zeros(nbytes, np.uint8), 0
        self.dev = torch.zeros(nbytes, dtype=torch.uint8, device=dev)

    def alloc(self, content):
        off, self.used = self.used, self.used + ((content.size + 255) & ~255)
        self.host[off:off + content.size] = content
        return None, self.dev.data_ptr() + off

    def call(self, changes):
        self.used = 0
        call = T.Call(changes, self.alloc)
        self.dev.copy_(self.torch.from_numpy(self.host))
        self.torch.cuda.synchronize()
        return call

    def now(self):
        self.torch.cuda.synchronize()
        return self.dev.cpu().numpy()

    def read(self, call, name):
        off = call.addr[name] - self.dev.data_ptr()
        return self.now()[off:off + T.BUF_BYTES]


@pytest.fixture(scope="module")
def handles(mbik, torch_dev):
    a = T.default_args()
    rest = np.tile(T.REST_BONE, (T.B, 1))
    with A.ClipSet(T.B, rest, a["clips"], shape_count=T.P) as shaped, A.ClipSet(T.B, rest, a["clips"]) as plain, \
            A.Playback(shaped, T.COUNT, T.K) as pb:
        yield dict(shaped=shaped.h, plain=plain.h, playback=pb.h)


def handle_of(handles, entry):
    return handles["playback"] if entry.startswith(("advance", "playback_")) else handles["shaped"]


def refused(mbik, arena, entry, changes, handle):
    """(code, text) of a device entry's call, which must not have written anything."""
    call = arena.call({**changes, "handle": handle})
    rc = T.ENTRIES[entry](mbik, call)
    out = [rc, _lib.last_error() if rc < 0 else ""]
    assert np.array_equal(arena.now(), arena.host), f"{entry} {changes}: device memory written"
    return out


def test_shared_faults_are_refused_as_the_cpu_forms_refuse_them(mbik, torch_dev, golden, handles):
    arena = Arena(*torch_dev)
    ran = 0
    for case in T.CALL_CASES:
        cpu_entry, _, changes = case
        want = golden[T.case_id(case)]
        if want[0] == _lib.MBIK_OK and changes.get("count", T.COUNT) != 0:
            continue   # a valid call: the last test's business
        entry = DEVICE_FORM[cpu_entry]
        assert refused(mbik, arena, entry, changes, handle_of(handles, entry)) == want, T.case_id(case)
        ran += 1
    assert ran >= 100


def test_refusals_only_a_live_handle_gives(mbik, torch_dev, handles):
    arena = Arena(*torch_dev)
    E = _lib.MBIK_EINVAL
    no_shapes = [E, "the clip set has no shapes (mbik_clipset_create_shaped)"]
    for entry in ("sample_shapes", "sample_shapes_layers"):
        assert refused(mbik, arena, entry, {}, handles["plain"]) == no_shapes
        assert refused(mbik, arena, entry, {"count": -1, "weights_out": None}, handles["plain"]) == no_shapes   # before the call's own
    pb = handles["playback"]
    assert refused(mbik, arena, "advance", {"count": T.COUNT + 1}, pb) == [E, "count 5 outside [0, 4]"]
    assert refused(mbik, arena, "advance", {"count": -1, "delta": T.NAN}, pb) == [E, "count -1 outside [0, 4]"]
    # write and read take host arrays
    host = lambda entry, **changes: T.run_case(mbik, entry, {**changes, "handle": pb})   # noqa: E731
    for entry in ("playback_write", "playback_read"):
        assert host(entry, first=3, n=2) == [E, "skeletons [3, 5) outside the capacity 4"]
        assert host(entry, first=-1, n=2) == [E, "skeletons [-1, 1) outside the capacity 4"]
        assert host(entry, first=0, n=-1, slots=None) == [E, "skeletons [0, -1) outside the capacity 4"]
        assert host(entry, slots=None) == [E, "null slots or flags"] and host(entry, pflags=None) == [E, "null slots or flags"]
        assert host(entry, first=T.COUNT, n=0, slots=None, pflags=None) == [_lib.MBIK_OK, ""]
    assert host("playback_write", pflag={1: 4}) == [E, "skeleton 1: unknown flag bits 4"]
    assert host("playback_write", state={(0, 0): dict(clip=0, pos=1.5)}) == [E, "skeleton 0 slot 0: pos is not finite or outside [0, length]"]
    create = lambda **changes: T.run_case(mbik, "playback_create", {**changes, "handle": handles["shaped"]})   # noqa: E731
    assert create(capacity=-1, layer_count=0) == [E, "negative capacity"]
    assert create(layer_count=9, desc=dict(struct_size=8)) == [E, "layer_count 9 outside [1, 8]"]
    assert create(desc=dict(struct_size=8)) == [E, "mbik_playback_desc.struct_size is too small"]
    assert create(desc=dict(next=[0, 2])) == [E, "next[1] = 2 outside [-1, 2)"]
    slots, flags = np.empty((T.COUNT, T.K), A.SLOT_DTYPE), np.empty(T.COUNT, np.uint32)
    assert mbik.mbik_playback_read(pb, 0, T.COUNT, slots.ctypes.data, flags.ctypes.data) == _lib.MBIK_OK
    assert (slots["clip"] == A.LAYER_OFF).all() and not flags.any(), "a refused write changed the state"


@pytest.mark.parametrize("entry", sorted(OUTPUTS))
def test_a_valid_call_equals_its_cpu_form(mbik, torch_dev, handles, entry):
    """count = 4 through the shared launch tail: the right device, the right stream, the right arguments."""
    arena = Arena(*torch_dev)
    cpu_entry = {v: k for k, v in DEVICE_FORM.items()}[entry]
    changes = dict(PLAYING) if entry == "advance" else {"clip_index": "clip_index"}
    if entry.startswith("root_motion"):
        changes["pose"] = "pose"
    if entry == "advance":
        assert T.run_case(mbik, "playback_write", {**changes, "handle": handles["playback"]})[0] == _lib.MBIK_OK
    call = arena.call({**changes, "handle": handle_of(handles, entry)})
    assert T.ENTRIES[entry](mbik, call) == _lib.MBIK_OK, _lib.last_error()
    ref = T.Call(changes)
    assert T.ENTRIES[cpu_entry](mbik, ref) == _lib.MBIK_OK, _lib.last_error()
    for name in OUTPUTS[entry]:
        want = np.frombuffer((C.c_uint8 * T.BUF_BYTES).from_address(ref.addr[name]), np.uint8)
        assert (want[:16] != T.UNWRITTEN).any(), f"{name}: the host form wrote nothing"
        assert np.array_equal(arena.read(call, name), want), f"{entry}: {name} differs from the host form's"
