"""ctypes bindings of the C ABI (include/mbik.h) exported by libmbik.so.

The product path always goes through this library: there is no CPU fallback.  If the
in-tree libmbik.so is missing the import of any solver entry point fails loudly.
"""
from __future__ import annotations

import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("MBIK_LIB_OVERRIDE") or os.path.join(_HERE, "libmbik.so")  # override: ablation timing only

MBIK_OK = 0
MBIK_EINVAL = -1
MBIK_ENOMEM = -2
MBIK_EHIP = -3
MBIK_EUNSUPPORTED = -4
MBIK_ENODEV = -5
MBIK_MULTI_STAGE_ALL = 1

# mbik_selftest_libm function codes (include/mbik.h)
LIBM_SINF, LIBM_COSF, LIBM_ACOSF, LIBM_SLERP_SCALE0, LIBM_COS_F64_OF_F32, LIBM_COS_F64, LIBM_SINF_SSE2, LIBM_COSF_SSE2, \
    LIBM_SLERP_SCALE0_SSE2, LIBM_ACOSF_UNIT = range(10)
# mbik_plan_options.libm_variant: the reference host's glibc sinf/cosf build
LIBM_VARIANT_FMA, LIBM_VARIANT_SSE2 = 0, 1
# a process's environment that makes ITS glibc pick the SSE2 build (the reference host of LIBM_VARIANT_SSE2)
GLIBC_SSE2_TUNABLES = "glibc.cpu.hwcaps=-FMA,-AVX2_Usable"

EXPORTED_SYMBOLS = (
    "mbik_plan_create", "mbik_plan_create_opts", "mbik_plan_create_device_opts", "mbik_plan_destroy", "mbik_plan_save", "mbik_plan_load", "mbik_plan_get_info", "mbik_plan_set_launch", "mbik_plan_set_layout",
    "mbik_plan_autotune", "mbik_plan_resident_blocks", "mbik_plan_set_heading_staging",
    "mbik_plan_set_locals_placement", "mbik_plan_set_waves_per_simd", "mbik_plan_set_helper_wave", "mbik_plan_set_wave_roles", "mbik_plan_set_table_addressing", "mbik_plan_rebuild_setup", "mbik_plan_setup_tables",
    "mbik_plan_status", "mbik_plan_debug_helper",
    "mbik_solve", "mbik_solve_checked", "mbik_solve_host", "mbik_segment_solve", "mbik_plan_segment_table", "mbik_describe_topology",
    "mbik_plan_step_classes", "mbik_describe_step_classes",
    "mbik_group_create", "mbik_group_solve", "mbik_group_destroy", "mbik_multi_create", "mbik_multi_solve",
    "mbik_multi_skeletons", "mbik_multi_destroy", "mbik_capture_targets", "mbik_pose_globals", "mbik_pose_globals_cpu", "mbik_pose_blend", "mbik_pose_blend_cpu", "mbik_clipset_create", "mbik_clipset_destroy", "mbik_clip_sample", "mbik_clip_sample_cpu", "mbik_clip_sample_layers", "mbik_clip_sample_layers_cpu",
    "mbik_clipset_create_shaped", "mbik_clip_sample_shapes", "mbik_clip_sample_shapes_layers", "mbik_clip_sample_shapes_cpu",
    "mbik_clip_sample_shapes_layers_cpu", "mbik_clip_root_motion", "mbik_clip_root_motion_layers", "mbik_root_motion_apply",
    "mbik_clip_root_motion_cpu", "mbik_clip_root_motion_layers_cpu", "mbik_root_motion_apply_cpu", "mbik_playback_create",
    "mbik_playback_destroy", "mbik_playback_write", "mbik_playback_read", "mbik_playback_advance", "mbik_playback_advance_cpu", "mbik_mesh_create", "mbik_mesh_destroy",
    "mbik_skin_vertices", "mbik_skin_vertices_cpu", "mbik_mesh_launch_shape", "mbik_mesh_create_shaped", "mbik_skin_vertices_shaped",
    "mbik_skin_vertices_shaped_cpu", "mbik_mesh_bone_boxes", "mbik_bone_boxes_cpu", "mbik_skin_bounds", "mbik_skin_bounds_cpu",
    "mbik_cull_boxes", "mbik_cull_boxes_cpu", "mbik_cull_lod", "mbik_cull_lod_cpu", "mbik_skin_vertices_listed", "mbik_skin_vertices_listed_cpu",
    "mbik_mesh_create_desc", "mbik_skin_vertices_call", "mbik_skin_vertices_call_cpu", "mbik_clipset_create_desc", "mbik_clip_call_cpu",
    "mbik_selftest_math",
    "mbik_selftest_libm", "mbik_selftest_div", "mbik_selftest_qcp", "mbik_selftest_point_in_limits", "mbik_selftest_xform", "mbik_selftest_topology", "mbik_plan_create_device", "mbik_last_error",
)


class MbikPin(C.Structure):
    _fields_ = [("bone", C.c_int32), ("weight", C.c_float), ("direction_priorities", C.c_float * 3),
                ("motion_propagation_factor", C.c_float)]


class MbikConstraint(C.Structure):
    _fields_ = [("bone", C.c_int32), ("cone_count", C.c_int32)]


class MbikSkeletonDesc(C.Structure):
    _fields_ = [("bone_count", C.c_int32), ("parents", C.POINTER(C.c_int32)),
                ("pin_count", C.c_int32), ("pins", C.POINTER(MbikPin)),
                ("constraint_count", C.c_int32), ("constraints", C.POINTER(MbikConstraint)),
                ("max_cones", C.c_int32)]


class MbikConfig(C.Structure):
    _fields_ = [("iterations_per_frame", C.c_int32), ("default_damp", C.c_float),
                ("constraint_mode", C.c_int32), ("stabilization_passes", C.c_int32),
                ("bone_damp_count", C.c_int32), ("bone_damp", C.POINTER(C.c_float))]


class MbikPlanInfo(C.Structure):
    _fields_ = [("abi_version", C.c_int32), ("skeleton_count", C.c_int32), ("bone_count", C.c_int32),
                ("pin_count", C.c_int32), ("segment_count", C.c_int32), ("level_count", C.c_int32),
                ("lanes_per_skeleton", C.c_int32), ("skeletons_per_block", C.c_int32),
                ("max_headings", C.c_int32), ("device", C.c_int32), ("device_bytes", C.c_int64),
                ("algorithmic_bytes_per_skeleton", C.c_double),
                ("algorithmic_flops_per_skeleton", C.c_double), ("lds_bytes_per_block", C.c_int64),
                ("checkpoint_interval", C.c_int32), ("heading_staging", C.c_int32), ("state_placement", C.c_int32),
                ("waves_per_simd", C.c_int32), ("constraint_slots", C.c_int32), ("cf_stride", C.c_int32),
                ("cd_stride", C.c_int32), ("libm_variant", C.c_int32),
                ("helper_wave", C.c_int32), ("heading_slots", C.c_int32), ("wave_roles", C.c_int32)]


class MbikPlanOptions(C.Structure):
    _fields_ = [("struct_size", C.c_int32), ("libm_variant", C.c_int32)]


class MbikClipTrack(C.Structure):
    _fields_ = [("bone", C.c_int32), ("channel", C.c_int32), ("interpolation", C.c_int32), ("loop_wrap", C.c_int32),
                ("key_count", C.c_int32), ("times", C.c_void_p), ("values", C.c_void_p)]


class MbikClipDesc(C.Structure):
    _fields_ = [("length", C.c_double), ("loop_mode", C.c_int32), ("track_count", C.c_int32),
                ("tracks", C.POINTER(MbikClipTrack))]


class MbikClipLayer(C.Structure):
    _fields_ = [("time", C.c_double), ("clip", C.c_int32), ("weight", C.c_float)]


# mbik_clip_sample_layers: the most layers a skeleton can have, and its flag
CLIP_MAX_LAYERS = 8
CLIP_LAYERS_NORMALIZE = 1
ROOT_MOTION_ORTHONORMALIZE = 1  # MBIK_ROOT_MOTION_ORTHONORMALIZE


class MbikPlaybackSlot(C.Structure):
    _fields_ = [("pos", C.c_double), ("clip", C.c_int32), ("speed", C.c_float), ("blend_left", C.c_float), ("blend_time", C.c_float)]


class MbikPlaybackCmd(C.Structure):
    _fields_ = [("start", C.c_double), ("skeleton", C.c_int32), ("clip", C.c_int32), ("blend_time", C.c_float), ("speed", C.c_float)]


class MbikPlaybackDesc(C.Structure):
    _fields_ = [("struct_size", C.c_int32), ("default_blend_time", C.c_float), ("next", C.c_void_p), ("blend_times", C.c_void_p)]


# mbik_playback: a skeleton's flag bits (the first two) and the event bits of an advance
PLAYBACK_STARTED, PLAYBACK_ENDED, PLAYBACK_LOOPED, PLAYBACK_TRANSITIONED, PLAYBACK_BAD_COMMAND, PLAYBACK_FADE_DROPPED = 1, 2, 4, 8, 16, 32


class MbikShapeTrack(C.Structure):
    _fields_ = [("shape", C.c_int32), ("interpolation", C.c_int32), ("loop_wrap", C.c_int32), ("key_count", C.c_int32),
                ("times", C.c_void_p), ("values", C.c_void_p)]


class MbikClipShapeTracks(C.Structure):
    _fields_ = [("track_count", C.c_int32), ("tracks", C.POINTER(MbikShapeTrack))]


class MbikClipsetShapes(C.Structure):
    _fields_ = [("struct_size", C.c_int32), ("shape_count", C.c_int32), ("init", C.c_void_p),
                ("clips", C.POINTER(MbikClipShapeTracks))]


class MbikClipsetDesc(C.Structure):  # mbik_clipset_desc
    _fields_ = [("struct_size", C.c_int32), ("bone_count", C.c_int32), ("rest_pose", C.c_void_p), ("clip_count", C.c_int32),
                ("clips", C.POINTER(MbikClipDesc)), ("shapes", C.POINTER(MbikClipsetShapes)), ("libm_variant", C.c_int32),
                ("flags", C.c_uint32)]


class MbikClipCall(C.Structure):  # mbik_clip_call
    _fields_ = [("struct_size", C.c_int32), ("kind", C.c_int32), ("count", C.c_int32), ("layer_count", C.c_int32),
                ("root_bone", C.c_int32), ("clip", C.c_int32), ("flags", C.c_uint32), ("time", C.c_void_p), ("time_prev", C.c_void_p),
                ("clip_index", C.c_void_p), ("layers", C.c_void_p), ("out", C.c_void_p), ("pose", C.c_void_p)]


# mbik_clip_call.kind
CLIP_CALL_SAMPLE, CLIP_CALL_SAMPLE_LAYERS, CLIP_CALL_SHAPES, CLIP_CALL_SHAPES_LAYERS, CLIP_CALL_ROOT_MOTION, \
    CLIP_CALL_ROOT_MOTION_LAYERS = range(6)


class MbikMeshShapes(C.Structure):
    _fields_ = [("struct_size", C.c_int32), ("shape_count", C.c_int32), ("mode", C.c_int32), ("positions", C.c_void_p),
                ("normals", C.c_void_p)]


class MbikMeshDesc(C.Structure):  # mbik_mesh_desc
    _fields_ = [("struct_size", C.c_int32), ("bone_count", C.c_int32), ("vertex_count", C.c_int32), ("influences", C.c_int32),
                ("positions", C.c_void_p), ("normals", C.c_void_p), ("tangents", C.c_void_p), ("bone_indices", C.c_void_p),
                ("weights", C.c_void_p), ("shapes", C.POINTER(MbikMeshShapes)), ("shape_tangents", C.c_void_p)]


class MbikSkinCall(C.Structure):  # mbik_skin_call
    _fields_ = [("struct_size", C.c_int32), ("count", C.c_int32), ("skin", C.c_void_p), ("shape_weights", C.c_void_p),
                ("indices", C.c_void_p), ("list_count", C.c_void_p), ("max_list", C.c_int32), ("flags", C.c_uint32),
                ("out_positions", C.c_void_p), ("out_normals", C.c_void_p), ("out_tangents", C.c_void_p)]


MESH_DESC, SKIN_CALL = MbikMeshDesc, MbikSkinCall
SHAPE_MODES = {"relative": 0, "normalized": 1}  # MBIK_SHAPE_MODE_*
CULL_MAX_PLANES = 16  # MBIK_CULL_MAX_PLANES
SKIN_LIST_COMPACT = 1  # MBIK_SKIN_LIST_COMPACT


class MbikLodRange(C.Structure):
    _fields_ = [("begin", C.c_float), ("end", C.c_float), ("begin_margin", C.c_float), ("end_margin", C.c_float)]


# mbik_cull_lod: the most ranges a call takes, its flag, and the level of a skeleton in no list
LOD_MAX_RANGES = 8
LOD_EXCLUSIVE = 1
LOD_NONE = 255


class MbikError(RuntimeError):
    def __init__(self, code: int, msg: str):
        super().__init__(f"mbik error {code}: {msg}")
        self.code = code


_lib = None


def load():
    """Load the in-tree libmbik.so (raises if it has not been built)."""
    global _lib
    if _lib is not None:
        return _lib
    try:
        # torch's ROCm wheel bundles its own libamdhip64.so.7 (same SONAME as /opt/rocm's).
        # Whichever is loaded first is shared by the process; torch only works on its own,
        # and libmbik's gfx950 code object runs on either, so let torch's load first.
        import torch  # noqa: F401
    except ImportError:
        pass
    if not os.path.exists(LIB_PATH):
        raise ImportError(f"{LIB_PATH} is missing: build it with `python -m many_bone_ik_amd.build` "
                          "(the HIP path has no CPU fallback)")
    L = C.CDLL(LIB_PATH)
    vp = C.c_void_p
    L.mbik_plan_create.argtypes = [C.POINTER(MbikSkeletonDesc), C.POINTER(MbikConfig), C.c_int32, vp, vp, vp, C.c_int32,
                                   C.POINTER(vp)]
    L.mbik_plan_create.restype = C.c_int32
    L.mbik_plan_create_opts.argtypes = [C.POINTER(MbikSkeletonDesc), C.POINTER(MbikConfig), C.POINTER(MbikPlanOptions), C.c_int32,
                                        vp, vp, vp, C.c_int32, C.POINTER(vp)]
    L.mbik_plan_create_opts.restype = C.c_int32
    L.mbik_plan_create_device_opts.argtypes = [C.c_int32, vp, vp, C.POINTER(MbikPlanOptions), C.POINTER(C.c_int32),
                                               C.POINTER(vp), C.POINTER(vp), C.POINTER(vp), C.c_int32, C.POINTER(vp)]
    L.mbik_plan_create_device_opts.restype = C.c_int32
    L.mbik_plan_destroy.argtypes = [vp]
    L.mbik_plan_destroy.restype = None
    L.mbik_plan_save.argtypes = [vp, vp, C.c_uint64, C.POINTER(C.c_uint64)]
    L.mbik_plan_save.restype = C.c_int32
    L.mbik_plan_load.argtypes = [vp, C.c_uint64, C.c_int32, C.POINTER(vp)]
    L.mbik_plan_load.restype = C.c_int32
    L.mbik_plan_get_info.argtypes = [vp, C.POINTER(MbikPlanInfo)]
    L.mbik_plan_get_info.restype = C.c_int32
    L.mbik_plan_set_launch.argtypes = [vp, C.c_int32]
    L.mbik_plan_set_launch.restype = C.c_int32
    L.mbik_plan_set_layout.argtypes = [vp, C.c_int32, C.c_int32, C.c_int32]
    L.mbik_plan_set_layout.restype = C.c_int32
    L.mbik_plan_set_heading_staging.argtypes = [vp, C.c_int32]
    L.mbik_plan_set_heading_staging.restype = C.c_int32
    L.mbik_plan_set_locals_placement.argtypes = [vp, C.c_int32]
    L.mbik_plan_set_locals_placement.restype = C.c_int32
    L.mbik_plan_set_waves_per_simd.argtypes = [vp, C.c_int32]
    L.mbik_plan_set_waves_per_simd.restype = C.c_int32
    if hasattr(L, "mbik_plan_set_helper_wave"):  # (absent from older A/B builds)
        L.mbik_plan_set_helper_wave.argtypes = [vp, C.c_int32]
        L.mbik_plan_set_helper_wave.restype = C.c_int32
    if hasattr(L, "mbik_plan_set_wave_roles"):  # (ABI 8; absent from older A/B builds)
        L.mbik_plan_set_wave_roles.argtypes = [vp, C.c_int32]
        L.mbik_plan_set_wave_roles.restype = C.c_int32
    if hasattr(L, "mbik_plan_status"):  # (ABI 6; absent from older A/B builds)
        L.mbik_plan_status.argtypes = [vp, C.POINTER(C.c_uint32)]
        L.mbik_plan_status.restype = C.c_int32
        L.mbik_plan_debug_helper.argtypes = [vp, C.c_int32, C.c_int32]
        L.mbik_plan_debug_helper.restype = C.c_int32
    if hasattr(L, "mbik_plan_set_table_addressing"):  # (absent from older A/B builds, tools/variant_check.py)
        L.mbik_plan_set_table_addressing.argtypes = [vp, C.c_int32]
        L.mbik_plan_set_table_addressing.restype = C.c_int32
    L.mbik_plan_autotune.argtypes = [vp, C.c_int32, C.c_int32, vp, vp, vp, vp]
    L.mbik_plan_autotune.restype = C.c_int32
    L.mbik_plan_resident_blocks.argtypes = [vp, C.c_int64]
    L.mbik_plan_resident_blocks.restype = C.c_int32
    L.mbik_plan_rebuild_setup.argtypes = [vp, C.c_int32, C.c_int32, vp, vp, vp, vp]
    L.mbik_plan_rebuild_setup.restype = C.c_int32
    L.mbik_plan_setup_tables.argtypes = [vp, vp, vp, vp]
    L.mbik_plan_setup_tables.restype = C.c_int32
    L.mbik_solve.argtypes = [vp, C.c_int32, C.c_int32, vp, vp, vp, vp]
    L.mbik_solve.restype = C.c_int32
    L.mbik_solve_checked.argtypes = [vp, C.c_int32, C.c_int32, vp, vp, vp, vp, vp]
    L.mbik_solve_checked.restype = C.c_int32
    L.mbik_selftest_math.argtypes = [C.c_int32, C.POINTER(C.c_uint64)]
    L.mbik_selftest_math.restype = C.c_int32
    L.mbik_selftest_topology.argtypes = [C.c_int32, vp, vp, C.c_int32, C.POINTER(C.c_int32)]
    L.mbik_selftest_topology.restype = C.c_int32
    L.mbik_plan_create_device.argtypes = [C.c_int32, vp, vp, C.POINTER(C.c_int32), C.POINTER(vp), C.POINTER(vp),
                                          C.POINTER(vp), C.c_int32, C.POINTER(vp)]
    L.mbik_plan_create_device.restype = C.c_int32
    L.mbik_selftest_div.argtypes = [C.c_int32, C.c_uint64, C.POINTER(C.c_uint64)]
    L.mbik_selftest_div.restype = C.c_int32
    if hasattr(L, "mbik_selftest_qcp"):  # (ABI 8; absent from older A/B builds)
        fp = C.POINTER(C.c_float)
        L.mbik_selftest_qcp.argtypes = [C.c_int32, fp, fp, C.POINTER(C.c_double), C.c_int32, C.c_double, C.c_int32, fp]
        L.mbik_selftest_qcp.restype = C.c_int32
        L.mbik_selftest_point_in_limits.argtypes = [vp, C.c_int32, C.c_int32, fp, fp, C.POINTER(C.c_double)]
        L.mbik_selftest_point_in_limits.restype = C.c_int32
        L.mbik_selftest_xform.argtypes = [C.c_int32, fp, fp, C.c_int32, fp]
        L.mbik_selftest_xform.restype = C.c_int32
    L.mbik_selftest_libm.argtypes = [C.c_int32, C.c_uint64, C.c_uint64, vp, vp, C.POINTER(C.c_uint64), vp]
    L.mbik_selftest_libm.restype = C.c_int32
    L.mbik_solve_host.argtypes = [vp, C.c_int32, C.c_int32, vp, vp, vp]
    L.mbik_solve_host.restype = C.c_int32
    L.mbik_segment_solve.argtypes = [vp, C.c_int32, C.c_int32, C.c_int32, vp, vp, vp]
    L.mbik_segment_solve.restype = C.c_int32
    L.mbik_plan_segment_table.argtypes = [vp, vp, vp, vp, C.c_int32]
    L.mbik_plan_segment_table.restype = C.c_int32
    L.mbik_describe_topology.argtypes = [C.POINTER(MbikSkeletonDesc), C.POINTER(MbikConfig), vp, vp, vp, vp, vp, vp]
    L.mbik_describe_topology.restype = C.c_int32
    if hasattr(L, "mbik_plan_step_classes"):  # (absent from older A/B builds)
        L.mbik_plan_step_classes.argtypes = [vp, vp, C.c_int32, vp, C.c_int32]
        L.mbik_plan_step_classes.restype = C.c_int32
        L.mbik_describe_step_classes.argtypes = [C.POINTER(MbikSkeletonDesc), C.POINTER(MbikConfig), C.c_int32, vp, C.c_int32, vp, C.c_int32]
        L.mbik_describe_step_classes.restype = C.c_int32
    L.mbik_group_create.argtypes = [C.POINTER(vp), C.c_int32, C.POINTER(vp)]
    L.mbik_group_create.restype = C.c_int32
    L.mbik_group_solve.argtypes = [vp, vp, vp, C.POINTER(vp), C.POINTER(vp), C.POINTER(vp), vp]
    L.mbik_group_solve.restype = C.c_int32
    L.mbik_group_destroy.argtypes = [vp]
    L.mbik_group_destroy.restype = None
    if hasattr(L, "mbik_multi_create"):  # (ABI 8; absent from older A/B builds)
        L.mbik_multi_create.argtypes = [C.POINTER(vp), C.c_int32, C.c_int32, C.c_uint32, C.POINTER(vp)]
        L.mbik_multi_create.restype = C.c_int32
        L.mbik_multi_solve.argtypes = [vp, vp, vp, vp, vp]
        L.mbik_multi_solve.restype = C.c_int32
        L.mbik_multi_skeletons.argtypes = [vp, C.POINTER(C.c_int64)]
        L.mbik_multi_skeletons.restype = C.c_int64
        L.mbik_multi_destroy.argtypes = [vp]
        L.mbik_multi_destroy.restype = None
    L.mbik_capture_targets.argtypes = [vp, C.c_int32, C.c_int32, vp, vp, vp, vp, vp]
    L.mbik_capture_targets.restype = C.c_int32
    L.mbik_pose_globals.argtypes = [vp, C.c_int32, vp, vp, vp, vp, vp, vp]
    L.mbik_pose_globals.restype = C.c_int32
    L.mbik_pose_globals_cpu.argtypes = [C.POINTER(MbikSkeletonDesc), C.c_int32, vp, vp, vp, vp, vp]
    L.mbik_pose_globals_cpu.restype = C.c_int32
    L.mbik_pose_blend.argtypes = [vp, C.c_int32, vp, vp, C.c_float, vp, vp, vp]
    L.mbik_pose_blend.restype = C.c_int32
    L.mbik_pose_blend_cpu.argtypes = [C.c_int32, C.c_int32, C.c_int32, vp, vp, C.c_float, vp, vp]
    L.mbik_pose_blend_cpu.restype = C.c_int32
    L.mbik_clipset_create.argtypes = [C.c_int32, vp, C.c_int32, C.POINTER(MbikClipDesc), C.c_int32, C.c_int32, C.POINTER(vp)]
    L.mbik_clipset_create.restype = C.c_int32
    L.mbik_clipset_destroy.argtypes = [vp]
    L.mbik_clipset_destroy.restype = None
    L.mbik_clip_sample.argtypes = [vp, C.c_int32, vp, vp, C.c_int32, vp, vp]
    L.mbik_clip_sample.restype = C.c_int32
    L.mbik_clip_sample_cpu.argtypes = [C.c_int32, vp, C.c_int32, C.POINTER(MbikClipDesc), C.c_int32, C.c_int32, vp, vp, C.c_int32, vp]
    L.mbik_clip_sample_cpu.restype = C.c_int32
    L.mbik_clip_sample_layers.argtypes = [vp, C.c_int32, C.c_int32, vp, C.c_uint32, vp, vp]
    L.mbik_clip_sample_layers.restype = C.c_int32
    L.mbik_clip_sample_layers_cpu.argtypes = [C.c_int32, vp, C.c_int32, C.POINTER(MbikClipDesc), C.c_int32, C.c_int32, C.c_int32, vp,
                                              C.c_uint32, vp]
    L.mbik_clip_sample_layers_cpu.restype = C.c_int32
    L.mbik_clipset_create_shaped.argtypes = [C.c_int32, vp, C.c_int32, C.POINTER(MbikClipDesc), C.POINTER(MbikClipsetShapes), C.c_int32,
                                             C.c_int32, C.POINTER(vp)]
    L.mbik_clipset_create_shaped.restype = C.c_int32
    L.mbik_clip_sample_shapes.argtypes = [vp, C.c_int32, vp, vp, C.c_int32, vp, vp]
    L.mbik_clip_sample_shapes.restype = C.c_int32
    L.mbik_clip_sample_shapes_layers.argtypes = [vp, C.c_int32, C.c_int32, vp, C.c_uint32, vp, vp]
    L.mbik_clip_sample_shapes_layers.restype = C.c_int32
    L.mbik_clip_sample_shapes_cpu.argtypes = [C.c_int32, vp, C.c_int32, C.POINTER(MbikClipDesc), C.POINTER(MbikClipsetShapes), C.c_int32,
                                              C.c_int32, vp, vp, C.c_int32, vp]
    L.mbik_clip_sample_shapes_cpu.restype = C.c_int32
    L.mbik_clip_sample_shapes_layers_cpu.argtypes = [C.c_int32, vp, C.c_int32, C.POINTER(MbikClipDesc), C.POINTER(MbikClipsetShapes),
                                                     C.c_int32, C.c_int32, C.c_int32, vp, C.c_uint32, vp]
    L.mbik_clip_sample_shapes_layers_cpu.restype = C.c_int32
    L.mbik_clip_root_motion.argtypes = [vp, C.c_int32, C.c_int32, vp, vp, vp, C.c_int32, vp, vp, vp]
    L.mbik_clip_root_motion.restype = C.c_int32
    L.mbik_clip_root_motion_layers.argtypes = [vp, C.c_int32, C.c_int32, C.c_int32, vp, vp, C.c_uint32, vp, vp, vp]
    L.mbik_clip_root_motion_layers.restype = C.c_int32
    L.mbik_root_motion_apply.argtypes = [vp, C.c_int32, vp, C.c_uint32, vp, vp]
    L.mbik_root_motion_apply.restype = C.c_int32
    L.mbik_clip_root_motion_cpu.argtypes = [C.c_int32, vp, C.c_int32, C.POINTER(MbikClipDesc), C.c_int32, C.c_int32, C.c_int32, vp, vp, vp,
                                            C.c_int32, vp, vp]
    L.mbik_clip_root_motion_cpu.restype = C.c_int32
    L.mbik_clip_root_motion_layers_cpu.argtypes = [C.c_int32, vp, C.c_int32, C.POINTER(MbikClipDesc), C.c_int32, C.c_int32, C.c_int32,
                                                   C.c_int32, vp, vp, C.c_uint32, vp, vp]
    L.mbik_clip_root_motion_layers_cpu.restype = C.c_int32
    L.mbik_root_motion_apply_cpu.argtypes = [C.c_int32, vp, C.c_uint32, vp]
    L.mbik_root_motion_apply_cpu.restype = C.c_int32
    L.mbik_playback_create.argtypes = [vp, C.c_int32, C.c_int32, C.POINTER(MbikPlaybackDesc), C.POINTER(vp)]
    L.mbik_playback_create.restype = C.c_int32
    L.mbik_playback_destroy.argtypes = [vp]
    L.mbik_playback_destroy.restype = None
    L.mbik_playback_write.argtypes = [vp, C.c_int32, C.c_int32, vp, vp]
    L.mbik_playback_write.restype = C.c_int32
    L.mbik_playback_read.argtypes = [vp, C.c_int32, C.c_int32, vp, vp]
    L.mbik_playback_read.restype = C.c_int32
    L.mbik_playback_advance.argtypes = [vp, C.c_int32, C.c_double, C.c_float, vp, C.c_int32, vp, vp, vp, vp]
    L.mbik_playback_advance.restype = C.c_int32
    L.mbik_playback_advance_cpu.argtypes = [C.c_int32, C.POINTER(MbikClipDesc), C.POINTER(MbikPlaybackDesc), C.c_int32, C.c_int32, vp, vp,
                                            C.c_double, C.c_float, vp, C.c_int32, vp, vp, vp]
    L.mbik_playback_advance_cpu.restype = C.c_int32
    L.mbik_mesh_create.argtypes = [C.c_int32, C.c_int32, C.c_int32, vp, vp, vp, vp, C.c_int32, C.POINTER(vp)]
    L.mbik_mesh_create.restype = C.c_int32
    L.mbik_mesh_destroy.argtypes = [vp]
    L.mbik_mesh_destroy.restype = None
    L.mbik_skin_vertices.argtypes = [vp, C.c_int32, vp, vp, vp, vp]
    L.mbik_skin_vertices.restype = C.c_int32
    L.mbik_skin_vertices_cpu.argtypes = [C.c_int32, C.c_int32, C.c_int32, vp, vp, vp, vp, C.c_int32, vp, vp, vp]
    L.mbik_skin_vertices_cpu.restype = C.c_int32
    L.mbik_mesh_launch_shape.argtypes = [vp, C.c_int32, C.POINTER(C.c_int32), C.POINTER(C.c_int32)]
    L.mbik_mesh_launch_shape.restype = C.c_int32
    L.mbik_mesh_create_shaped.argtypes = [C.c_int32, C.c_int32, C.c_int32, vp, vp, vp, vp, C.POINTER(MbikMeshShapes), C.c_int32,
                                          C.POINTER(vp)]
    L.mbik_mesh_create_shaped.restype = C.c_int32
    L.mbik_skin_vertices_shaped.argtypes = [vp, C.c_int32, vp, vp, vp, vp, vp]
    L.mbik_skin_vertices_shaped.restype = C.c_int32
    L.mbik_skin_vertices_shaped_cpu.argtypes = [C.c_int32, C.c_int32, C.c_int32, vp, vp, vp, vp, C.POINTER(MbikMeshShapes), C.c_int32,
                                                vp, vp, vp, vp]
    L.mbik_skin_vertices_shaped_cpu.restype = C.c_int32
    L.mbik_mesh_bone_boxes.argtypes = [vp, vp, vp]
    L.mbik_mesh_bone_boxes.restype = C.c_int32
    L.mbik_bone_boxes_cpu.argtypes = [C.c_int32, C.c_int32, C.c_int32, vp, vp, vp, vp, vp]
    L.mbik_bone_boxes_cpu.restype = C.c_int32
    L.mbik_skin_bounds.argtypes = [vp, C.c_int32, vp, vp, vp]
    L.mbik_skin_bounds.restype = C.c_int32
    L.mbik_skin_bounds_cpu.argtypes = [C.c_int32, vp, vp, C.c_int32, vp, vp]
    L.mbik_skin_bounds_cpu.restype = C.c_int32
    L.mbik_cull_boxes.argtypes = [vp, C.c_int32, vp, vp, C.c_float, C.c_int32, vp, vp, vp, vp, vp]
    L.mbik_cull_boxes.restype = C.c_int32
    L.mbik_cull_boxes_cpu.argtypes = [C.c_int32, vp, vp, C.c_float, C.c_int32, vp, vp, vp, vp]
    L.mbik_cull_boxes_cpu.restype = C.c_int32
    L.mbik_cull_lod.argtypes = [vp, C.c_int32, vp, vp, C.c_float, C.c_int32, vp, vp, C.c_int32, vp, C.c_uint32, vp, vp, vp, vp, vp]
    L.mbik_cull_lod.restype = C.c_int32
    L.mbik_cull_lod_cpu.argtypes = [C.c_int32, vp, vp, C.c_float, C.c_int32, vp, vp, C.c_int32, vp, C.c_uint32, vp, vp, vp, vp]
    L.mbik_cull_lod_cpu.restype = C.c_int32
    L.mbik_skin_vertices_listed.argtypes = [vp, C.c_int32, vp, vp, C.c_int32, vp, vp, C.c_uint32, vp, vp, vp]
    L.mbik_skin_vertices_listed.restype = C.c_int32
    L.mbik_skin_vertices_listed_cpu.argtypes = [C.c_int32, C.c_int32, C.c_int32, vp, vp, vp, vp, C.POINTER(MbikMeshShapes), C.c_int32,
                                                vp, vp, C.c_int32, vp, vp, C.c_uint32, vp, vp]
    L.mbik_skin_vertices_listed_cpu.restype = C.c_int32
    L.mbik_mesh_create_desc.argtypes = [C.POINTER(MbikMeshDesc), C.c_int32, C.POINTER(vp)]
    L.mbik_mesh_create_desc.restype = C.c_int32
    L.mbik_skin_vertices_call.argtypes = [vp, C.POINTER(MbikSkinCall), vp]
    L.mbik_skin_vertices_call.restype = C.c_int32
    L.mbik_skin_vertices_call_cpu.argtypes = [C.POINTER(MbikMeshDesc), C.POINTER(MbikSkinCall)]
    L.mbik_skin_vertices_call_cpu.restype = C.c_int32
    if hasattr(L, "mbik_clipset_create_desc"):  # (absent from older A/B builds)
        L.mbik_clipset_create_desc.argtypes = [C.POINTER(MbikClipsetDesc), C.c_int32, C.POINTER(vp)]
        L.mbik_clipset_create_desc.restype = C.c_int32
        L.mbik_clip_call_cpu.argtypes = [C.POINTER(MbikClipsetDesc), C.POINTER(MbikClipCall)]
        L.mbik_clip_call_cpu.restype = C.c_int32
    L.mbik_last_error.argtypes = []
    L.mbik_last_error.restype = C.c_char_p
    _lib = L
    return L


def check(rc: int) -> int:
    if rc < 0:
        raise MbikError(rc, load().mbik_last_error().decode(errors="replace"))
    return rc


def last_error() -> str:
    """mbik_last_error() of this thread."""
    return load().mbik_last_error().decode(errors="replace")
