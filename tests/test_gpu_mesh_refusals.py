"""The device entries of the mesh front end against the refusal ledger (tests/test_mesh_refusals_cpu.py).

A handful of 3-vertex meshes (B = 2; with and without normals, tangents and shapes, made through the three
create entries).  Every case of a call's arguments that a device entry shares with its _cpu form gives the
code and the text the golden file holds for the _cpu form and writes the buffers it names there: a refused
call writes no byte of device memory, an empty one at most its counts.  The refusals only a live handle can
give are pinned to their texts here.  One valid call of each device entry at the ledger's shape then equals
its _cpu form bit for bit.  Everything goes through the raw ctypes entries, the older ones included: Python's
Mesh no longer calls those.
"""
import ctypes as C

import numpy as np
import pytest

from many_bone_ik_amd import _lib

from . import test_mesh_refusals_cpu as T
from .test_gpu_animation_refusals import Arena as _Arena
from .test_gpu_parity import torch_dev  # noqa: F401 (fixture)
from .test_mesh_refusals_cpu import golden  # noqa: F401 (fixture)

pytestmark = pytest.mark.gpu

DEVICE_FORM = {"skin_cpu": "skin", "shaped_cpu": "shaped", "listed_cpu": "listed", "call_plain_cpu": "call_plain", "call_shaped_cpu": "call_shaped",
               "call_listed_cpu": "call_listed", "bounds_cpu": "bounds", "cull_cpu": "cull", "lod_cpu": "lod"}
# what a case may change about the mesh and still have a device twin: the handle is made to match
MESH_KEYS = ("normals", "tangents", "shape_tangents", "shapes", "shapes.normals")
HOST_ONLY_KEYS = ("vertex_count", "bone_count", "bone_boxes", "used", "influences", "bad_index", "desc", "desc.struct_size")


class Arena(_Arena):
    def call(self, entry, changes):
        self.used = 0
        call = T.make_call(entry, changes, self.alloc)
        self.dev.copy_(self.torch.from_numpy(self.host))
        self.torch.cuda.synchronize()
        return call

    def written(self, call):
        now, base = self.now(), self.dev.data_ptr()
        return T.written(call, lambda addr: now[addr - base:addr - base + T.BUF_BYTES])


class Meshes:
    """Device meshes by what a case changes about the mesh, made on first use through `create` (desc, shaped or plain)."""

    def __init__(self, L):
        self.L, self.made = L, {}

    def get(self, changes, create="desc"):
        mesh = {k: v for k, v in changes.items() if k in MESH_KEYS}
        key = (create, tuple(sorted(mesh.items())))
        if key not in self.made:
            c, h = T.Call(mesh), C.c_void_p()
            if create == "desc":
                rc = self.L.mbik_mesh_create_desc(c.desc(), 0, C.byref(h))
            elif create == "shaped":
                rc = self.L.mbik_mesh_create_shaped(*c.mesh_args(), c.shapes(), 0, C.byref(h))
            else:
                rc = self.L.mbik_mesh_create(*c.mesh_args(), 0, C.byref(h))
            assert rc == _lib.MBIK_OK and h.value, _lib.last_error()
            self.made[key] = h
        return self.made[key]

    def close(self):
        for h in self.made.values():
            self.L.mbik_mesh_destroy(h)


@pytest.fixture(scope="module")
def meshes(mbik, torch_dev):
    m = Meshes(mbik)
    yield m
    m.close()


def outcome(mbik, arena, entry, changes, handle):
    """(code, text, written buffers) of a device entry's call."""
    call = arena.call(entry, {**changes, "handle": handle})
    rc = T.ENTRIES[entry][0](mbik, call)
    wrote = arena.written(call)
    if rc < 0:
        assert np.array_equal(arena.now(), arena.host), f"{entry} {changes}: a refused call wrote device memory"
    return [rc, _lib.last_error() if rc < 0 else "", wrote]


def test_shared_cases_end_as_the_cpu_forms_end_them(mbik, torch_dev, golden, meshes):
    arena = Arena(*torch_dev)
    ran = refused = 0
    for case in T.CALL_CASES:
        cpu_entry, _, changes = case
        if cpu_entry not in DEVICE_FORM or any(k in changes for k in HOST_ONLY_KEYS):
            continue
        if cpu_entry == "shaped_cpu" and "shapes" in changes:
            continue   # the _cpu form misses its shapes argument, the device form its mesh's shapes: the next test
        entry = DEVICE_FORM[cpu_entry]
        want = golden[T.case_id(case)]
        assert outcome(mbik, arena, entry, changes, meshes.get(changes)) == want, T.case_id(case)
        ran, refused = ran + 1, refused + (want[0] < 0)
    assert ran >= 400 and refused >= 250, (ran, refused)


def test_refusals_only_a_live_handle_gives(mbik, torch_dev, golden, meshes):
    arena = Arena(*torch_dev)
    E = _lib.MBIK_EINVAL
    for case in T.NULL_MESH_CASES:
        assert outcome(mbik, arena, case[0], case[2], None) == golden[T.case_id(case)], T.case_id(case)
    unshaped = meshes.get(T.NO_SHAPES)
    no_shapes = [E, "the mesh has no shapes (mbik_mesh_create_shaped)", []]
    assert outcome(mbik, arena, "shaped", {}, unshaped) == no_shapes
    assert outcome(mbik, arena, "shaped", {"shape_weights": None, "count": -1}, unshaped) == no_shapes   # before the call's own
    assert outcome(mbik, arena, "shaped", {"count": 0}, unshaped) == no_shapes                           # and before the empty call
    assert outcome(mbik, arena, "call_shaped", {"out_tangents": None, "count": -1}, unshaped) == no_shapes
    assert outcome(mbik, arena, "call_shaped", {"shape_weights": None}, unshaped)[0] == _lib.MBIK_OK     # the plain form
    listed = [E, "shape_weights given for a mesh without shapes", []]
    assert outcome(mbik, arena, "listed", {}, unshaped) == listed
    assert outcome(mbik, arena, "call_listed", {"count": -1}, unshaped) == listed
    assert outcome(mbik, arena, "listed", {"max_list": -1}, unshaped) == [E, "negative max_list", []]
    full = meshes.get({})
    assert outcome(mbik, arena, "mesh_bone_boxes", {"boxes_out": None}, full) == [E, "null boxes or used", []]
    assert outcome(mbik, arena, "mesh_bone_boxes", {"used_out": None}, full) == [E, "null boxes or used", []]
    assert outcome(mbik, arena, "launch_shape", {"count": -1}, full) == [E, "negative count", []]
    assert outcome(mbik, arena, "launch_shape", {}, full) == [_lib.MBIK_OK, "", []]


PLAIN_MESH = {**T.NO_SHAPES, **T.NO_TANGENTS}
NO_OUT_T = {"out_tangents": None}
VALID = {
    # the three create forms
    "mbik_mesh_create": ("skin", PLAIN_MESH, "plain"),
    "mbik_mesh_create_shaped": ("shaped", dict(T.NO_TANGENTS), "shaped"),
    "mbik_mesh_create_desc": ("call_listed", {}, "desc"),
    "skin": ("skin", {}, "desc"), "shaped": ("shaped", {}, "desc"), "listed in place": ("listed", {}, "desc"),
    "listed compact": ("listed", dict(T.COMPACT), "desc"), "listed unshaped": ("listed", {"shape_weights": None}, "desc"),
    "call plain": ("call_plain", NO_OUT_T, "desc"), "call plain with tangents": ("call_plain", {}, "desc"),
    "call shaped": ("call_shaped", NO_OUT_T, "desc"), "call shaped with tangents": ("call_shaped", {}, "desc"),
    "call listed": ("call_listed", NO_OUT_T, "desc"), "call listed with tangents": ("call_listed", {}, "desc"),
    "call listed compact with tangents": ("call_listed", dict(T.COMPACT), "desc"),
    "bounds": ("bounds", {}, "desc"), "cull": ("cull", {}, "desc"), "cull verdicts only": ("cull", {"cull_indices": None, "visible_count": None}, "desc"),
    "cull list only": ("cull", {"visible": None}, "desc"), "lod": ("lod", {}, "desc"), "lod exclusive": ("lod", {"lod_flags": 1}, "desc"),
}


@pytest.mark.parametrize("name", sorted(VALID))
def test_a_valid_call_equals_its_cpu_form(mbik, torch_dev, meshes, name):
    """The ledger's shape through the shared tails: the right device, the right stream, the right arguments."""
    entry, changes, create = VALID[name]
    arena = Arena(*torch_dev)
    cpu_entry = {v: k for k, v in DEVICE_FORM.items()}[entry]
    call = arena.call(entry, {**changes, "handle": meshes.get(changes, create)})
    assert T.ENTRIES[entry][0](mbik, call) == _lib.MBIK_OK, _lib.last_error()
    ref = T.make_call(cpu_entry, changes)
    compare = {buf: buf for buf in T.INPUTS + T.OUTPUTS}
    if entry == "bounds":   # the host form takes the bone boxes the mesh was made with, and writes beside them
        assert T.ENTRIES["bone_boxes_cpu"][0](mbik, ref) == _lib.MBIK_OK, _lib.last_error()
        ref.a.update(bone_boxes="boxes_out", used="used_out", boxes_out="out_positions")
        compare = {"boxes_out": "out_positions", "skin": "skin"}
    assert T.ENTRIES[cpu_entry][0](mbik, ref) == _lib.MBIK_OK, _lib.last_error()
    assert T.written(ref), "the host form wrote nothing"
    now, base = arena.now(), arena.dev.data_ptr()
    for buf, ref_buf in compare.items():
        want = np.frombuffer((C.c_uint8 * T.BUF_BYTES).from_address(ref.addr[ref_buf]), np.uint8)
        off = call.addr[buf] - base
        assert np.array_equal(now[off:off + T.BUF_BYTES], want), f"{name}: {buf} differs from the host form's"
