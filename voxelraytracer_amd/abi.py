"""ctypes mirror of include/vrt.h (the C-ABI drop-in boundary).

The structs here are byte-for-byte the ones in include/vrt.h; tests/test_abi.py checks sizes and
that every function the header declares is exported by the built library.
"""
from __future__ import annotations

import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("VRT_LIB") or os.path.join(_HERE, "_lib", "libvrt.so")

VRT_OK = 0
VRT_ERR_INVALID = -1
VRT_ERR_DEVICE = -2
VRT_ERR_NO_VOLUME = -3
VRT_ERR_OOM = -4
VRT_ERR_UNSUPPORTED = -5

VRT_HIT_FLAG_TIE3 = 1
VRT_HIT_FLAG_STEP_CAP = 2
VRT_HIT_FLAG_STACK_FULL = 4
VRT_MAX_STEPS = 4096
VRT_COMM_ID_BYTES = 128

SCENE_TERRAIN = 0
SCENE_GLASS_CUBE = 1
SCENE_REFRACTION = 2
SCENES = {"terrain": SCENE_TERRAIN, "glass_cube": SCENE_GLASS_CUBE, "refraction": SCENE_REFRACTION}

COUNTER_NAMES = (
    "pixels",
    "primary_rays",
    "secondary_rays",
    "shadow_rays",
    "dda_steps",
    "shadow_steps",
    "refraction_probes",
    "tie3",
    "step_cap",
)
VRT_CNT_COUNT = len(COUNTER_NAMES)


class Camera(C.Structure):
    _fields_ = [("inv_pv", C.c_float * 16), ("width", C.c_int32), ("height", C.c_int32)]


class Volume(C.Structure):
    _fields_ = [("voxels", C.POINTER(C.c_uint8)), ("n", C.c_int32)]


class Params(C.Structure):
    _fields_ = [
        ("sun_dir", C.c_float * 3),
        ("time", C.c_float),
        ("ray_noise", C.c_float),
        ("reflection_noise", C.c_float),
        ("refraction_noise", C.c_float),
        ("max_ray_length", C.c_float),
        ("max_reflections", C.c_int32),
        ("max_transparencies", C.c_int32),
        ("color_only", C.c_int32),
        ("reserved0", C.c_int32),
        ("atlas_rgba", C.POINTER(C.c_uint8)),
        ("atlas_size", C.c_int32),
        ("atlas_texture_size", C.c_int32),
    ]


class Hit(C.Structure):
    _fields_ = [
        ("voxel_index", C.c_int32),
        ("ray_length", C.c_float),
        ("steps", C.c_uint32),
        ("flags", C.c_uint32),
    ]


VRT_STATS_COUNTERS = 1   # vrt_stats.request: count (runs the exact-walk instance)


class Stats(C.Structure):
    _fields_ = [
        ("counters", C.c_uint64 * VRT_CNT_COUNT),
        ("kernel_ms", C.c_float),
        ("request", C.c_uint32),
        ("reserved", C.c_float * 2),
    ]


# numpy dtype of one vrt_hit record
HIT_DTYPE = [("voxel_index", "<i4"), ("ray_length", "<f4"), ("steps", "<u4"), ("flags", "<u4")]

# ray queries (vrt_cast_rays*, vrt_pick_pixels)
VRT_RAY_FLAG_BLOCKED = 8
VRT_CAST_NEAREST = 0
VRT_CAST_OCCLUSION = 1
CAST_MODES = {"nearest": VRT_CAST_NEAREST, "occlusion": VRT_CAST_OCCLUSION}


class Ray(C.Structure):
    _fields_ = [
        ("origin", C.c_float * 3),
        ("max_length", C.c_float),
        ("dir", C.c_float * 3),
        ("reserved", C.c_uint32),
    ]


class RayHit(C.Structure):
    _fields_ = [
        ("voxel_index", C.c_int32),
        ("ray_length", C.c_float),
        ("steps", C.c_uint32),
        ("flags", C.c_uint32),
        ("point", C.c_float * 3),
        ("face", C.c_uint32),
    ]


# numpy dtypes of one vrt_ray and one vrt_ray_hit record (the latter starts with a vrt_hit)
RAY_DTYPE = [("origin", "<f4", (3,)), ("max_length", "<f4"), ("dir", "<f4", (3,)), ("reserved", "<u4")]
RAY_HIT_DTYPE = HIT_DTYPE + [("point", "<f4", (3,)), ("face", "<u4")]
# vrt_debug_cert_walks: a vrt_ray with the reserved word read as len0, and the walk's result
CERT_RAY_DTYPE = [("origin", "<f4", (3,)), ("max_length", "<f4"), ("dir", "<f4", (3,)), ("len0", "<f4")]
CERT_WALK_DTYPE = [("res", "<i4"), ("byte", "<u4"), ("axis", "<i4"), ("cell", "<i4", (3,)), ("u", "<f4"), ("eu", "<f4")]
CERT_MISS, CERT_HIT, CERT_UNSURE, CERT_NOT_STARTED = 0, 1, 2, 3


# shaded ray queries (vrt_trace_rays*, vrt_trace_pixels)
class RayColor(C.Structure):
    _fields_ = [
        ("voxel_index", C.c_int32),
        ("ray_length", C.c_float),
        ("steps", C.c_uint32),
        ("flags", C.c_uint32),
        ("rgba", C.c_float * 4),
    ]


# numpy dtype of one vrt_ray_color record (it starts with a vrt_hit)
RAY_COLOR_DTYPE = HIT_DTYPE + [("rgba", "<f4", (4,))]


# ID and depth pass (vrt_render_ids*)
class PixelId(C.Structure):
    _fields_ = [("voxel_index", C.c_int32), ("face", C.c_uint32)]


# numpy dtype of one vrt_pixel_id record (vrt_ray_hit's fields of the same names)
PIXEL_ID_DTYPE = [("voxel_index", "<i4"), ("face", "<u4")]

# history fetch of the reprojected temporal filter (vrt_reproject_temporal_fetch_async, vrt_set_reprojected_fetch)
FETCH_NEAREST = 0
FETCH_BILINEAR = 1

# ID-guided spatial filter (vrt_spatial_filter*): the guide's key, and the loop's modes (vrt_set_reprojected_spatial)
GUIDE_FACE = 0
GUIDE_PLANE = 1
SPATIAL_OFF = 0
SPATIAL_DISPLAY = 1
SPATIAL_FILL = 2

# name -> (restype, argtypes): every function include/vrt.h declares
# entry points added after ABI v12 (an older build loaded by VRT_LIB with VRT_LIB_ABI=<its version>
# may lack exactly these)
ADDED_IN = {"vrt_render_temporal_batch_async": 14, "vrt_set_cert_trees": 15,
            # added within v15 (in-place edits): a v15 build from before them lacks these three
            "vrt_update_volume_region": 16, "vrt_update_volume_region_device": 16, "vrt_volume_edit_plan": 16,
            # added within v15 after the edits (ray queries)
            "vrt_cast_rays_async": 16, "vrt_cast_rays": 16, "vrt_pick_pixels": 16,
            # added within v15 after the ray queries (shaded ray queries)
            "vrt_trace_rays_async": 16, "vrt_trace_rays": 16, "vrt_trace_pixels": 16,
            # added within v15 after the shaded ray queries (ID and depth pass)
            "vrt_render_ids_async": 16, "vrt_render_ids": 16, "vrt_ids_deferred": 16,
            # added within v15 after the ID and depth pass (reprojected temporal filter)
            "vrt_camera_forward": 16, "vrt_reproject_temporal_async": 16, "vrt_render_frame_reprojected": 16,
            "vrt_reprojected_history_reset": 16,
            # added within v15 after the reprojected filter (bilinear history fetch)
            "vrt_reproject_temporal_fetch_async": 16, "vrt_set_reprojected_fetch": 16,
            # added within v15 after the bilinear fetch (ID-guided spatial filter)
            "vrt_spatial_filter_async": 16, "vrt_spatial_filter": 16, "vrt_set_reprojected_spatial": 16,
            # added within v15 after the spatial filter (certified ID kernel)
            "vrt_set_ids_certified": 16, "vrt_ids_certified": 16}

SIGNATURES = {
    "vrt_abi_version": (C.c_int, []),
    "vrt_create": (C.c_int, [C.c_uint32, C.POINTER(C.c_void_p)]),
    "vrt_create_devices": (C.c_int, [C.c_void_p, C.c_int32, C.POINTER(C.c_void_p)]),
    "vrt_device_count": (C.c_int, [C.c_void_p]),
    "vrt_device_ordinal": (C.c_int, [C.c_void_p, C.c_int32]),
    "vrt_band_plan": (C.c_int, [C.c_int32, C.c_int32, C.c_int32, C.c_void_p]),
    "vrt_band_copy_plan": (C.c_int, [C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_void_p]),
    # ABI v12: block-cyclic whole-frame split, one process per GPU (RCCL gather + assembly)
    "vrt_frame_row_block": (C.c_int, [C.c_int32]),
    "vrt_block_band_plan": (C.c_int, [C.c_int32, C.c_int32, C.c_int32, C.c_void_p]),
    "vrt_block_copy_plan": (C.c_int, [C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_void_p]),
    "vrt_comm_unique_id": (C.c_int, [C.c_void_p, C.c_int32]),
    "vrt_comm_join": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int32]),
    "vrt_gather_band_async": (C.c_int, [C.c_void_p, C.c_int32, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p]),
    "vrt_assemble_blocks_async": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int32,
                                            C.c_int32, C.c_int32, C.c_void_p, C.c_int64, C.c_void_p]),
    "vrt_pack_rgb8_async": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p]),
    "vrt_assemble_blocks_rgb8_async": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int32,
                                                 C.c_int32, C.c_int32, C.c_void_p, C.c_int64, C.c_void_p]),
    "vrt_destroy": (None, [C.c_void_p]),
    "vrt_last_error": (C.c_char_p, [C.c_void_p]),
    "vrt_upload_volume": (C.c_int, [C.c_void_p, C.POINTER(Volume)]),
    "vrt_upload_volume_device": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p]),
    "vrt_volume_device_ptr": (C.c_void_p, [C.c_void_p]),
    # added within v15 (no version bump: detect by symbol lookup): in-place voxel edits
    "vrt_update_volume_region": (C.c_int, [C.c_void_p, C.POINTER(C.c_int32 * 3), C.POINTER(C.c_int32 * 3),
                                           C.c_void_p]),
    "vrt_update_volume_region_device": (C.c_int, [C.c_void_p, C.POINTER(C.c_int32 * 3),
                                                  C.POINTER(C.c_int32 * 3), C.c_void_p, C.c_void_p]),
    "vrt_volume_edit_plan": (C.c_int, [C.c_int32, C.c_int32, C.POINTER(C.c_int32 * 3),
                                       C.POINTER(C.c_int32 * 3), C.c_void_p]),
    # added within v15 (detect by symbol lookup): ray queries
    "vrt_cast_rays_async": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_int32, C.c_void_p, C.c_void_p]),
    "vrt_cast_rays": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_int32, C.c_void_p]),
    "vrt_pick_pixels": (C.c_int, [C.c_void_p, C.POINTER(Camera), C.POINTER(Params), C.c_void_p, C.c_int32,
                                  C.c_void_p]),
    # added within v15 (detect by symbol lookup): shaded ray queries
    "vrt_trace_rays_async": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.POINTER(Params), C.c_void_p,
                                       C.c_void_p]),
    "vrt_trace_rays": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.POINTER(Params), C.c_void_p]),
    "vrt_trace_pixels": (C.c_int, [C.c_void_p, C.POINTER(Camera), C.POINTER(Params), C.c_void_p, C.c_int32,
                                   C.c_void_p]),
    # added within v15 (detect by symbol lookup): ID and depth pass
    "vrt_render_ids_async": (C.c_int, [C.c_void_p, C.POINTER(Camera), C.POINTER(Params), C.c_int32, C.c_int32,
                                       C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p]),
    "vrt_render_ids": (C.c_int, [C.c_void_p, C.POINTER(Camera), C.POINTER(Params), C.c_void_p, C.c_void_p]),
    "vrt_ids_deferred": (C.c_int, [C.c_void_p, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]),
    # added within v15 (detect by symbol lookup): certified ID kernel
    "vrt_set_ids_certified": (C.c_int, [C.c_void_p, C.c_int32]),
    "vrt_ids_certified": (C.c_int, [C.c_void_p]),
    # added within v15 (detect by symbol lookup): reprojected temporal filter
    "vrt_camera_forward": (C.c_int, [C.POINTER(Camera), C.c_void_p]),
    "vrt_reproject_temporal_async": (C.c_int, [C.c_void_p, C.POINTER(Camera), C.POINTER(Params), C.c_void_p,
                                               C.c_float, C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p,
                                               C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p,
                                               C.c_void_p, C.c_void_p]),
    "vrt_render_frame_reprojected": (C.c_int, [C.c_void_p, C.POINTER(Camera), C.POINTER(Params), C.c_float,
                                               C.c_void_p, C.POINTER(Stats)]),
    "vrt_reprojected_history_reset": (C.c_int, [C.c_void_p]),
    # added within v15 (detect by symbol lookup): bilinear history fetch
    "vrt_reproject_temporal_fetch_async": (C.c_int, [C.c_void_p, C.POINTER(Camera), C.POINTER(Params), C.c_void_p,
                                                     C.c_float, C.c_int32, C.c_int32, C.c_int32, C.c_int32,
                                                     C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                                     C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "vrt_set_reprojected_fetch": (C.c_int, [C.c_void_p, C.c_int32]),
    # added within v15 (detect by symbol lookup): ID-guided spatial filter
    "vrt_spatial_filter_async": (C.c_int, [C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32,
                                           C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p,
                                           C.c_void_p, C.c_void_p, C.c_void_p]),
    "vrt_spatial_filter": (C.c_int, [C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_void_p,
                                     C.c_void_p, C.c_void_p, C.c_void_p]),
    "vrt_set_reprojected_spatial": (C.c_int, [C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_int32]),
    "vrt_build_scene_device": (C.c_int, [C.c_void_p, C.c_int32, C.c_int32, C.c_uint32, C.c_void_p]),
    "vrt_debug_packed_volume": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint64]),
    "vrt_debug_collectives": (C.c_int, [C.c_void_p]),
    "vrt_debug_fast_math": (C.c_int, [C.c_void_p, C.c_void_p]),
    # added within v15 (detect by symbol lookup): the proof run of the certified pass's power forms
    "vrt_debug_pow_forms": (C.c_int, [C.c_void_p, C.c_void_p]),
    "vrt_volume_octants": (C.c_int, [C.c_void_p]),
    "vrt_set_skip_layout": (C.c_int, [C.c_void_p, C.c_int32]),
    "vrt_set_certified": (C.c_int, [C.c_void_p, C.c_int32]),
    "vrt_certified": (C.c_int, [C.c_void_p]),
    "vrt_set_tile_order": (C.c_int, [C.c_void_p, C.c_int32]),
    "vrt_set_exact_pass": (C.c_int, [C.c_void_p, C.c_int32]),
    "vrt_set_cert_trees": (C.c_int, [C.c_void_p, C.c_int32]),
    "vrt_set_launch_timing": (C.c_int, [C.c_void_p, C.c_int32]),
    "vrt_launch_timing": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p]),
    "vrt_render": (
        C.c_int,
        [C.c_void_p, C.POINTER(Camera), C.POINTER(Params), C.c_void_p, C.c_void_p, C.POINTER(Stats)],
    ),
    "vrt_render_rows_async": (
        C.c_int,
        [
            C.c_void_p,
            C.POINTER(Camera),
            C.POINTER(Params),
            C.c_int32,
            C.c_int32,
            C.c_int32,
            C.c_void_p,
            C.c_void_p,
            C.c_void_p,
            C.c_void_p,
        ],
    ),
    "vrt_render_rows_pitched_async": (
        C.c_int,
        [C.c_void_p, C.POINTER(Camera), C.POINTER(Params), C.c_int32, C.c_int32, C.c_int32,
         C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p],
    ),
    "vrt_render_temporal_rows_pitched_async": (
        C.c_int,
        [C.c_void_p, C.POINTER(Camera), C.POINTER(Params), C.c_float, C.c_int32, C.c_int32,
         C.c_int32, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
         C.c_void_p],
    ),
    "vrt_render_blocks_pitched_async": (
        C.c_int,
        [C.c_void_p, C.POINTER(Camera), C.POINTER(Params), C.c_int32, C.c_int32, C.c_int32,
         C.c_int32, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p],
    ),
    "vrt_render_temporal_blocks_pitched_async": (
        C.c_int,
        [C.c_void_p, C.POINTER(Camera), C.POINTER(Params), C.c_float, C.c_int32, C.c_int32,
         C.c_int32, C.c_int32, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
         C.c_void_p, C.c_void_p],
    ),
    "vrt_render_temporal_batch_async": (
        C.c_int,
        [C.c_void_p, C.c_int32, C.POINTER(Camera), C.POINTER(Params), C.c_int32, C.c_int32,
         C.c_int32, C.c_int32, C.c_int64, C.POINTER(C.c_void_p), C.POINTER(C.c_void_p),
         C.c_void_p],
    ),
    "vrt_render_temporal_rows_async": (
        C.c_int,
        [C.c_void_p, C.POINTER(Camera), C.POINTER(Params), C.c_float, C.c_int32, C.c_int32,
         C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p],
    ),
    "vrt_render_frame": (
        C.c_int,
        [C.c_void_p, C.POINTER(Camera), C.POINTER(Params), C.c_float, C.c_void_p, C.POINTER(Stats)],
    ),
    "vrt_render_frame_device": (
        C.c_int,
        [C.c_void_p, C.POINTER(Camera), C.POINTER(Params), C.c_float, C.c_void_p,
         C.POINTER(C.c_void_p), C.POINTER(Stats)],
    ),
    "vrt_frame_stream": (C.c_void_p, [C.c_void_p]),
    "vrt_history_reset": (C.c_int, [C.c_void_p]),
    "vrt_upload_atlas": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32]),
    "vrt_debug_randomize": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_float,
                                      C.c_float, C.c_void_p]),
    # added within v15 (detect by symbol lookup): certified walks for a ray list
    "vrt_debug_cert_walks": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_int32, C.c_void_p]),
    "vrt_terrain_noise": (C.c_int, [C.c_int32, C.c_uint32, C.c_void_p]),
    "vrt_build_scene": (C.c_int, [C.c_int32, C.c_int32, C.c_uint32, C.c_void_p]),
    "vrt_camera_make": (
        C.c_int,
        [
            C.POINTER(C.c_float * 3),
            C.POINTER(C.c_float * 3),
            C.c_int32,
            C.c_int32,
            C.c_float,
            C.c_float,
            C.c_float,
            C.POINTER(Camera),
        ],
    ),
    "vrt_sun_dir": (None, [C.c_float, C.c_float, C.POINTER(C.c_float * 3)]),
    "vrt_params_default": (None, [C.POINTER(Params)]),
}

_lib = None


class VrtError(RuntimeError):
    def __init__(self, code: int, msg: str):
        super().__init__(f"vrt error {code}: {msg}")
        self.code = code


def load_library(path: str = LIB_PATH) -> C.CDLL:
    """Load the HIP library. Fails loudly: there is no CPU fallback for the product path."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(path):
        raise ImportError(
            f"{path} is missing: build it with `make` (or __graft_entry__.build()); "
            "the voxel ray tracer has no CPU fallback"
        )
    # One HIP runtime per process: if PyTorch is installed, let it load its libamdhip64.so.7 first
    # so the library binds to the same runtime (same soname) instead of /opt/rocm's copy; torch
    # tensors' device pointers are then valid in vrt_render_rows_async.
    try:
        import torch  # noqa: F401
    except ImportError:
        pass
    lib = C.CDLL(path)
    older = int(os.environ.get("VRT_LIB_ABI", "0"))   # A/B against an older ABI's build (VRT_LIB)
    for name, (res, args) in SIGNATURES.items():
        if not hasattr(lib, name) and name.startswith("vrt_debug_"):
            continue   # diagnostic entry points exist only in diagnostic builds (make variant)
        if not hasattr(lib, name) and os.environ.get("VRT_LIB") and older and older < ADDED_IN.get(name, 0):
            continue   # an entry point newer than the declared ABI of the VRT_LIB build
        # every other symbol must be there: A/B variants (VRT_LIB) are built from this tree, and an
        # ABI/build mismatch fails here, at load time, not at the first call
        fn = getattr(lib, name)
        fn.restype = res
        fn.argtypes = args
    _lib = lib
    return lib
