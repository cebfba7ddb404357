"""voxelraytracer_amd — MI355X-native drop-in for the per-pixel ray tracer of
Thraix/VoxelRayTracer (res/shaders/voxel.glsl).

The product is the C-ABI library voxelraytracer_amd/_lib/libvrt.so (include/vrt.h): a gfx950
HIP kernel plus the host harness that mirrors src/main.cpp. This module is a thin Python host
over that ABI with the reference's vocabulary (scene, camera, sun, frame, volume).
There is no CPU fallback: constructing a Renderer without the HIP library or a GPU raises.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import abi
from .abi import (  # noqa: F401  (re-exported vocabulary)
    COUNTER_NAMES,
    FETCH_BILINEAR,
    FETCH_NEAREST,
    GUIDE_FACE,
    GUIDE_PLANE,
    HIT_DTYPE,
    PIXEL_ID_DTYPE,
    RAY_COLOR_DTYPE,
    RAY_DTYPE,
    RAY_HIT_DTYPE,
    SCENE_GLASS_CUBE,
    SCENE_REFRACTION,
    SCENE_TERRAIN,
    SCENES,
    SPATIAL_DISPLAY,
    SPATIAL_FILL,
    SPATIAL_OFF,
    Camera,
    Params,
    PixelId,
    VrtError,
)

# Camera pose of AppScene (main.cpp:171-172) and projection (main.cpp:161): 90 deg, 0.01..100.
DEFAULT_CAM_POS = (-3.45, 2.17, 3.53)
DEFAULT_CAM_ROT = (-33.0, -48.0, 0.0)
FOV_DEG, NEAR, FAR = 90.0, 0.01, 100.0


def lib():
    return abi.load_library()


def build_scene(scene, n: int, seed: int = 0) -> np.ndarray:
    """N^3 uint8 volume, x fastest (main.cpp:218-288). `scene` is a name or SCENE_* id."""
    sid = SCENES[scene] if isinstance(scene, str) else int(scene)
    out = np.zeros(n * n * n, dtype=np.uint8)
    rc = lib().vrt_build_scene(sid, n, seed, out.ctypes.data)
    if rc != 0:
        raise VrtError(rc, "vrt_build_scene")
    return out


def terrain_noise(n: int, seed: int = 0) -> np.ndarray:
    out = np.zeros(n * n, dtype=np.float32)
    rc = lib().vrt_terrain_noise(n, seed, out.ctypes.data)
    if rc != 0:
        raise VrtError(rc, "vrt_terrain_noise")
    return out


def make_camera(width: int, height: int, pos=DEFAULT_CAM_POS, rot=DEFAULT_CAM_ROT,
                fov=FOV_DEG, near=NEAR, far=FAR) -> Camera:
    cam = Camera()
    p = (C.c_float * 3)(*pos)
    r = (C.c_float * 3)(*rot)
    rc = lib().vrt_camera_make(C.byref(p), C.byref(r), width, height, fov, near, far, C.byref(cam))
    if rc != 0:
        raise VrtError(rc, "vrt_camera_make")
    return cam


def camera_forward(cam: Camera) -> np.ndarray:
    """vrt_camera_forward: PV = inverse(cam.inv_pv) as 16 float32, column-major like inv_pv: the matrix that
    takes a world point to the camera's clip coordinates (Renderer.reproject_temporal_async's prev_pv)."""
    out = np.zeros(16, dtype=np.float32)
    rc = lib().vrt_camera_forward(C.byref(cam), out.ctypes.data)
    if rc != 0:
        raise VrtError(rc, "vrt_camera_forward")
    return out


def sun_dir(time_of_day: float, day_time: float = 50.0):
    out = (C.c_float * 3)()
    lib().vrt_sun_dir(time_of_day, day_time, C.byref(out))
    return tuple(out)


def default_params(max_reflections: int = 1, max_transparencies: int = 2, **kw) -> Params:
    """Bench defaults: "Make day" sun, u_Time=1, noise 0, 100 max length."""
    p = Params()
    lib().vrt_params_default(C.byref(p))
    p.max_reflections = max_reflections
    p.max_transparencies = max_transparencies
    for k, v in kw.items():
        if k == "sun_dir":
            p.sun_dir = (C.c_float * 3)(*v)
        else:
            setattr(p, k, v)
    return p


def counters_dict(values) -> dict:
    return {name: int(values[i]) for i, name in enumerate(COUNTER_NAMES)}


# ---- textured mode (voxel.glsl without _COLOR_ONLY) ---------------------
# Atlas layout (ABI): RGBA8 texels, atlas_size x atlas_size, row r at GL t = (r + 0.5) / size
# (row 0 = bottom, as glTexImage2D consumes rows). Slot (texX, texY) of a material
# (voxel.glsl:64-67) covers columns [texX*ts, (texX+1)*ts) and rows
# [size - (texY+1)*ts, size - texY*ts), which is where GetTextureCoordinate (:167-172) lands.
ATLAS_SLOTS = {"stone": (0, 0), "dirt": (1, 0), "glass": (0, 1), "grass": (1, 1)}


def atlas_slot_rows(size: int, ts: int, tex_x: int, tex_y: int):
    return slice(size - (tex_y + 1) * ts, size - tex_y * ts), slice(tex_x * ts, (tex_x + 1) * ts)


def make_atlas(atlas_size: int = 256, texture_size: int = 128, seed: int = 0) -> np.ndarray:
    """Deterministic synthetic atlas [size, size, 4] uint8 (the reference's PNG textures are not
    shipped): per-slot base colour x value noise; the glass slot has alpha 40..255 with a band of
    fully opaque texels (so both sides of GetColor(hit).a != 1, voxel.glsl:445, occur)."""
    rng = np.random.default_rng(seed)
    a = np.zeros((atlas_size, atlas_size, 4), np.uint8)
    base = {"stone": (128, 128, 128), "dirt": (120, 80, 40), "glass": (170, 220, 255),
            "grass": (30, 160, 40)}
    for name, (tx, ty) in ATLAS_SLOTS.items():
        rs, cs = atlas_slot_rows(atlas_size, texture_size, tx, ty)
        noise = rng.uniform(0.6, 1.0, (texture_size, texture_size, 1))
        rgb = np.clip(np.array(base[name], np.float64) * noise, 0, 255)
        a[rs, cs, :3] = rgb.astype(np.uint8)
        if name == "glass":
            alpha = rng.integers(40, 256, (texture_size, texture_size))
            alpha[:, : texture_size // 8] = 255
            a[rs, cs, 3] = alpha
        else:
            a[rs, cs, 3] = 255
    return a


def load_atlas(texture_dir: str, suffix: str = "128", atlas_size: int = 256) -> np.ndarray:
    """Atlas from the reference's res/textures/{stone,dirt,glass,grass}<suffix>.png (main.cpp:187-
    193), for demos on a host that has them (needs PIL); tests use make_atlas()."""
    from PIL import Image

    a = np.zeros((atlas_size, atlas_size, 4), np.uint8)
    for name, (tx, ty) in ATLAS_SLOTS.items():
        im = np.asarray(Image.open(f"{texture_dir}/{name}{suffix}.png").convert("RGBA"))
        ts = im.shape[0]
        rs, cs = atlas_slot_rows(atlas_size, ts, tx, ty)
        a[rs, cs] = im[::-1]   # image rows are top-down; atlas rows bottom-up
    return a


def textured_params(p: Params, atlas: np.ndarray, texture_size: int = 128) -> Params:
    """Switch params to textured mode with this atlas (kept alive on the Params object)."""
    atlas = np.ascontiguousarray(atlas, np.uint8)
    p.color_only = 0
    p.atlas_rgba = atlas.ctypes.data_as(C.POINTER(C.c_uint8))
    p.atlas_size = atlas.shape[0]
    p.atlas_texture_size = texture_size
    p._atlas_ref = atlas
    return p


def algorithmic_bytes(c: dict, pixel_bytes: int = 16) -> int:
    """1 B per DDA step (both marches) + 2 B per refraction probe + the per-pixel output bytes:
    16 for the float RGBA frame, 8 for the fused temporal RGB8 path (4 B history
    read + 4 B filtered write)."""
    return (c["dda_steps"] + c["shadow_steps"] + 2 * c["refraction_probes"]
            + pixel_bytes * c["pixels"])


def total_rays(c: dict) -> int:
    return c["primary_rays"] + c["secondary_rays"] + c["shadow_rays"]


def band_plan(height: int, k: int, parts: int = 2):
    """The library's whole-frame row plan (vrt_band_plan): ({(band j, part p): (row0, rows,
    row_step, band_row0)}, rows of the largest band). Band j holds frame rows j, j+k, ..."""
    out = np.zeros(k * parts * 4, np.int32)
    cap = lib().vrt_band_plan(height, k, parts, out.ctypes.data)
    if cap < 0:
        raise VrtError(cap, "vrt_band_plan")
    o = out.reshape(k, parts, 4)
    return {(j, p): tuple(int(v) for v in o[j, p]) for j in range(k) for p in range(parts)}, cap


def band_copy_plan(width: int, height: int, k: int, elem_bytes: int):
    """The library's frame-assembly copies (vrt_band_copy_plan): per band j, (dst_offset,
    dst_pitch, src_pitch, row_bytes, rows) of the 2-D copy of band j's packed rows into the frame."""
    out = np.zeros(k * 5, np.int64)
    r = lib().vrt_band_copy_plan(width, height, k, elem_bytes, out.ctypes.data)
    if r < 0:
        raise VrtError(r, "vrt_band_copy_plan")
    return [tuple(int(v) for v in row) for row in out.reshape(k, 5)]


def frame_row_block(k: int) -> int:
    """Rows per block of the bands the whole-frame entry points split a frame into over k devices
    (vrt_frame_row_block: 1 for one device, 16 for k > 1)."""
    return int(lib().vrt_frame_row_block(k))


def block_band_plan(height: int, k: int, row_block: int):
    """vrt_block_band_plan: ([(row0, rows, row_step)] per device, rows of the largest band) of the
    block-cyclic split of `height` rows over k devices in blocks of row_block rows."""
    out = np.zeros(k * 3, np.int32)
    cap = lib().vrt_block_band_plan(height, k, row_block, out.ctypes.data)
    if cap < 0:
        raise VrtError(cap, "vrt_block_band_plan")
    return [tuple(int(v) for v in row) for row in out.reshape(k, 3)], cap


def block_copy_plan(width: int, height: int, k: int, row_block: int, elem_bytes: int):
    """vrt_block_copy_plan: the 2-D copies (band, dst_offset, dst_pitch, src_offset, src_pitch,
    width_bytes, rows) that assemble a frame from k packed block-cyclic band buffers."""
    out = np.zeros(k * 2 * 7, np.int64)
    n = lib().vrt_block_copy_plan(width, height, k, row_block, elem_bytes, out.ctypes.data)
    if n < 0:
        raise VrtError(n, "vrt_block_copy_plan")
    return [tuple(int(v) for v in row) for row in out.reshape(k * 2, 7) if row[6] > 0]


def volume_edit_plan(n: int, octants: int, origin, extent):
    """vrt_volume_edit_plan: per packed volume o < octants (8 or 1), the half-open box (x0, y0, z0,
    x1, y1, z1) of packed texels in [0, n)^3 that an edit of the box [origin, origin + extent)
    (x, y, z order) may change. Host arithmetic, no GPU."""
    o3 = (C.c_int32 * 3)(*(int(v) for v in origin))
    e3 = (C.c_int32 * 3)(*(int(v) for v in extent))
    out = np.zeros(max(int(octants), 1) * 6, np.int32)
    k = lib().vrt_volume_edit_plan(n, octants, C.byref(o3), C.byref(e3), out.ctypes.data)
    if k < 0:
        raise VrtError(k, "vrt_volume_edit_plan")
    return [tuple(int(v) for v in row) for row in out.reshape(-1, 6)[:k]]


def make_rays(origins, dirs, max_length=100.0) -> np.ndarray:
    """vrt_ray records (RAY_DTYPE) from [count, 3] origins and directions in volume coordinates (the
    volume is [0, N]^3; directions are used as given) and a max_length, one value or one per ray."""
    o = np.asarray(origins, np.float32).reshape(-1, 3)
    d = np.asarray(dirs, np.float32).reshape(-1, 3)
    if len(o) != len(d):
        raise ValueError("make_rays: as many origins as directions")
    rays = np.zeros(len(o), dtype=RAY_DTYPE)
    rays["origin"] = o
    rays["dir"] = d
    rays["max_length"] = np.asarray(max_length, np.float32)
    return rays


def panorama_rays(width: int, height: int, pos, n: int, max_length=100.0) -> np.ndarray:
    """The ray list of an equirectangular panorama seen from the world position `pos` in a volume of
    size n, as RAY_DTYPE records of shape [height, width] for Renderer.trace_rays: a camera model the
    pinhole frame (inv_pv) cannot express. Row 0 is the bottom row. Column i looks along the longitude
    lon = 2 pi (i + 0.5) / width - pi and row j along the latitude lat = pi (j + 0.5) / height - pi / 2,
    direction (sin(lon) cos(lat), sin(lat), -cos(lon) cos(lat)): the image's centre looks along -z (the
    pinhole camera's view at zero rotation; for an odd width it is column (width - 1) / 2 exactly),
    longitude grows with the column towards +x, the left and right edges meet at +z, and the bottom and
    top rows are half a row from -y and +y. Directions have unit length in float32; every origin is
    pos + n / 2 (volume coordinates, voxel.glsl:430)."""
    lon = 2.0 * np.pi * (np.arange(width, dtype=np.float64) + 0.5) / width - np.pi
    lat = np.pi * (np.arange(height, dtype=np.float64) + 0.5) / height - 0.5 * np.pi
    d = np.empty((height, width, 3), np.float64)
    d[..., 0] = np.cos(lat)[:, None] * np.sin(lon)[None, :]
    d[..., 1] = np.sin(lat)[:, None]
    d[..., 2] = -np.cos(lat)[:, None] * np.cos(lon)[None, :]
    origin = np.asarray(pos, np.float32).reshape(3) + np.float32(n) * np.float32(0.5)
    rays = make_rays(np.broadcast_to(origin, (height * width, 3)), d.reshape(-1, 3), max_length)
    return rays.reshape(height, width)


def _cast_mode(mode) -> int:
    """VRT_CAST_* of a mode name ("nearest", "occlusion") or number."""
    return abi.CAST_MODES[mode] if isinstance(mode, str) else int(mode)


def hit_normal(hits) -> np.ndarray:
    """The hit face's outward normal per vrt_ray_hit record, int8 [count, 3]: +-1 on the face's axis
    (bits 0-1 of `face`; bit 2: negative), zero for records without a hit."""
    h = np.asarray(hits).reshape(-1)
    out = np.zeros((len(h), 3), np.int8)
    found = h["voxel_index"] >= 0
    axis = (h["face"] & 3).astype(np.intp)
    sign = np.where(h["face"] & 4, -1, 1).astype(np.int8)
    rows = np.nonzero(found)[0]
    out[rows, axis[rows]] = sign[rows]
    return out


def hit_cell(hits, n: int):
    """(i, j, k) of the hit voxels (voxel_index = i + j n + k n^2), -1 on every axis without a hit."""
    idx = np.asarray(hits).reshape(-1)["voxel_index"].astype(np.int64)
    found = idx >= 0
    return (np.where(found, idx % n, -1), np.where(found, idx // n % n, -1), np.where(found, idx // (n * n), -1))


def adjacent_cell(hits, n: int):
    """hit_cell + hit_normal: the cell in front of the hit face, where a placed block goes. It may lie
    outside [0, n) (a face on the volume's border); -1 on every axis without a hit."""
    nrm = hit_normal(hits).astype(np.int64)
    i, j, k = hit_cell(hits, n)
    return i + nrm[:, 0], j + nrm[:, 1], k + nrm[:, 2]


def comm_unique_id() -> bytes:
    """vrt_comm_unique_id: a new RCCL unique id (rank 0 of a one-process-per-GPU job creates one
    per communicator and the job distributes them)."""
    buf = (C.c_uint8 * abi.VRT_COMM_ID_BYTES)()
    r = lib().vrt_comm_unique_id(buf, abi.VRT_COMM_ID_BYTES)
    if r != abi.VRT_COMM_ID_BYTES:
        raise VrtError(r, "vrt_comm_unique_id")
    return bytes(buf)


class Renderer:
    """One vrt_ctx (replaces the GL context + FrameBuffer of the reference). `device` is a HIP
    device ordinal, or a sequence of ordinals: whole frames are then split into row bands across
    them (vrt_create's device mask; a repeated ordinal rehearses the split on one GPU)."""

    def __init__(self, device=0):
        self._lib = lib()
        h = C.c_void_p()
        if isinstance(device, int):
            rc = self._lib.vrt_create(1 << device, C.byref(h))
        else:
            devs = (C.c_int32 * len(device))(*device)
            rc = self._lib.vrt_create_devices(devs, len(device), C.byref(h))
        if rc != 0:
            raise VrtError(rc, f"vrt_create(device={device}) failed (no GPU?)")
        self._h = h
        self.n = None

    def device_count(self) -> int:
        return self._lib.vrt_device_count(self._h)

    def close(self):
        if getattr(self, "_h", None):
            self._lib.vrt_destroy(self._h)
            self._h = None

    def __del__(self):
        self.close()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def _check(self, rc: int, what: str):
        if rc != 0:
            msg = self._lib.vrt_last_error(self._h)
            raise VrtError(rc, f"{what}: {msg.decode() if msg else ''}")

    def upload_volume(self, voxels: np.ndarray, n: int):
        v = np.ascontiguousarray(voxels, dtype=np.uint8).reshape(-1)
        if v.size != n * n * n:
            raise ValueError("volume size mismatch")
        vol = abi.Volume(v.ctypes.data_as(C.POINTER(C.c_uint8)), n)
        self._check(self._lib.vrt_upload_volume(self._h, C.byref(vol)), "vrt_upload_volume")
        self.n = n

    def upload_volume_device(self, d_voxels: int, n: int, stream: int = 0):
        """Upload from a device buffer (e.g. a torch uint8 CUDA tensor's data_ptr())."""
        self._check(self._lib.vrt_upload_volume_device(self._h, d_voxels, n, stream or None),
                    "vrt_upload_volume_device")
        self.n = n

    def update_volume(self, origin, block: np.ndarray):
        """In-place edit (vrt_update_volume_region): `block`, a uint8 array indexed [z][y][x],
        replaces the voxels of the box at `origin` = (x, y, z); the packed skip-distance volumes
        become exactly those of a full upload of the edited volume, by a regional rebuild."""
        b = np.ascontiguousarray(block, dtype=np.uint8)
        if b.ndim != 3:
            raise ValueError("block must be indexed [z][y][x]")
        o3 = (C.c_int32 * 3)(*(int(v) for v in origin))
        e3 = (C.c_int32 * 3)(b.shape[2], b.shape[1], b.shape[0])
        self._check(self._lib.vrt_update_volume_region(self._h, C.byref(o3), C.byref(e3), b.ctypes.data),
                    "vrt_update_volume_region")

    def update_volume_device(self, origin, extent, d_ptr: int, stream: int = 0):
        """update_volume from a device buffer on the first device (extent[0] * extent[1] * extent[2]
        bytes, x fastest inside the box; e.g. a torch uint8 tensor's data_ptr()), ordered on
        `stream`. origin and extent are (x, y, z)."""
        o3 = (C.c_int32 * 3)(*(int(v) for v in origin))
        e3 = (C.c_int32 * 3)(*(int(v) for v in extent))
        self._check(self._lib.vrt_update_volume_region_device(self._h, C.byref(o3), C.byref(e3), d_ptr or None,
                                                              stream or None),
                    "vrt_update_volume_region_device")

    def cast_rays(self, rays: np.ndarray, mode="nearest") -> np.ndarray:
        """vrt_cast_rays: `rays` (RAY_DTYPE records, e.g. make_rays()) against the resident volume,
        synchronously; returns RAY_HIT_DTYPE records. mode "nearest": the first non-empty voxel on
        the ray within its max_length (glass included) with hit point and face; "occlusion": only
        whether an opaque voxel blocks it (flags & VRT_RAY_FLAG_BLOCKED; glass does not block)."""
        r = np.ascontiguousarray(rays, dtype=RAY_DTYPE).reshape(-1)
        hits = np.empty(len(r), dtype=RAY_HIT_DTYPE)
        self._check(self._lib.vrt_cast_rays(self._h, r.ctypes.data, len(r), _cast_mode(mode),
                                            hits.ctypes.data), "vrt_cast_rays")
        return hits

    def cast_rays_async(self, d_rays: int, count: int, d_hits: int, mode="nearest", stream: int = 0):
        """vrt_cast_rays_async: `count` vrt_ray records at the device pointer d_rays into vrt_ray_hit
        records at d_hits (both 16-byte aligned, e.g. torch tensors' data_ptr()), enqueued on a HIP
        stream: no host synchronisation, no allocation."""
        self._check(self._lib.vrt_cast_rays_async(self._h, d_rays or None, count, _cast_mode(mode),
                                                  d_hits or None, stream or None), "vrt_cast_rays_async")

    def pick(self, cam: Camera, params: Params, pixels) -> np.ndarray:
        """vrt_pick_pixels: what the primary rays of `pixels` ([count, 2] of (px, py), py = 0 the
        bottom row) of a frame of (cam, params) hit: RAY_HIT_DTYPE records whose voxel_index and
        ray_length equal render()'s hit records at those pixels, with the hit point and face."""
        px = np.ascontiguousarray(pixels, dtype=np.int32).reshape(-1, 2)
        hits = np.empty(len(px), dtype=RAY_HIT_DTYPE)
        self._check(self._lib.vrt_pick_pixels(self._h, C.byref(cam), C.byref(params), px.ctypes.data, len(px),
                                              hits.ctypes.data), "vrt_pick_pixels")
        return hits

    def trace_rays(self, rays: np.ndarray, params: Params) -> np.ndarray:
        """vrt_trace_rays: what each of `rays` (RAY_DTYPE records, e.g. make_rays() or panorama_rays())
        sees, synchronously: the shader's whole ray tree (shadow rays, reflections, refractions) from the
        ray as given, with the ray's own max_length as u_MaxRayLength and the rest of `params` as in a
        frame (ray_noise and max_ray_length are not read). Returns RAY_COLOR_DTYPE records in the shape of
        `rays`: the first march's hit, the tree's steps and flags, and the colour rgba (a = 1)."""
        r = np.ascontiguousarray(rays, dtype=RAY_DTYPE)
        out = np.empty(r.shape, dtype=RAY_COLOR_DTYPE)
        self._check(self._lib.vrt_trace_rays(self._h, r.ctypes.data, r.size, C.byref(params), out.ctypes.data),
                    "vrt_trace_rays")
        return out

    def trace_rays_async(self, d_rays: int, count: int, params: Params, d_out: int, stream: int = 0):
        """vrt_trace_rays_async: `count` vrt_ray records at the device pointer d_rays into vrt_ray_color
        records at d_out (both 16-byte aligned, e.g. torch tensors' data_ptr()), enqueued on a HIP
        stream: no host synchronisation, no allocation."""
        self._check(self._lib.vrt_trace_rays_async(self._h, d_rays or None, count, C.byref(params), d_out or None,
                                                   stream or None), "vrt_trace_rays_async")

    def trace_pixels(self, cam: Camera, params: Params, pixels) -> np.ndarray:
        """vrt_trace_pixels: the pixels `pixels` ([count, 2] of (px, py), py = 0 the bottom row) of a
        frame of (cam, params), without rendering it: RAY_COLOR_DTYPE records whose first four fields
        equal render()'s hit records at those pixels and whose rgba equals its float frame, bit for bit."""
        px = np.ascontiguousarray(pixels, dtype=np.int32).reshape(-1, 2)
        out = np.empty(len(px), dtype=RAY_COLOR_DTYPE)
        self._check(self._lib.vrt_trace_pixels(self._h, C.byref(cam), C.byref(params), px.ctypes.data, len(px),
                                               out.ctypes.data), "vrt_trace_pixels")
        return out

    def render_ids(self, cam: Camera, params: Params, want_depth: bool = True):
        """vrt_render_ids: what the frame of (cam, params) shows, per pixel and without shading. Returns
        (ids, depth): ids[H, W] of PIXEL_ID_DTYPE, whose voxel_index and face equal pick()'s record of
        each pixel (hit_normal, hit_cell and adjacent_cell read them), and depth[H, W] float32, the
        parameter of the hit face's plane along the normalised primary ray from its near-plane point
        (+inf for a miss), or None with want_depth=False. Row 0 is the bottom row."""
        ids = np.empty((cam.height, cam.width), dtype=PIXEL_ID_DTYPE)
        depth = np.empty((cam.height, cam.width), np.float32) if want_depth else None
        self._check(self._lib.vrt_render_ids(self._h, C.byref(cam), C.byref(params), ids.ctypes.data,
                                             depth.ctypes.data if want_depth else None), "vrt_render_ids")
        return ids, depth

    def render_ids_async(self, cam: Camera, params: Params, row0: int, rows: int, pitch: int, d_ids: int,
                         d_depth: int = 0, stream: int = 0):
        """vrt_render_ids_async: rows [row0, row0 + rows) into device buffers (e.g. torch tensors'
        data_ptr()), pixel (px, row0 + i) at record i * pitch + px of d_ids (8-byte records) and of
        d_depth (float32; 0: no depth), one kernel launch enqueued on a HIP stream: no host
        synchronisation, no allocation."""
        self._check(self._lib.vrt_render_ids_async(self._h, C.byref(cam), C.byref(params), row0, rows, pitch,
                                                   d_ids or None, d_depth or None, stream or None),
                    "vrt_render_ids_async")

    def ids_deferred(self):
        """vrt_ids_deferred: (pixels, deferred) of the last render_ids: how many pixels it rendered and
        how many of them the exact march walked: all of them when the exact ID kernel ran, and with the
        certified ID kernel (set_ids_certified(1) on an octant layout) those its walk could not settle."""
        px, de = C.c_uint64(), C.c_uint64()
        self._check(self._lib.vrt_ids_deferred(self._h, C.byref(px), C.byref(de)), "vrt_ids_deferred")
        return int(px.value), int(de.value)

    def set_ids_certified(self, mode: int):
        """vrt_set_ids_certified: the ID pass's kernel. 0 (the default): the exact ID kernel for every pixel;
        1: the certified ID kernel on an octant layout (certified walks, the exact march in the lane of a
        pixel they cannot settle). One launch either way; IDs and depths are the same bytes."""
        self._check(self._lib.vrt_set_ids_certified(self._h, int(mode)), "vrt_set_ids_certified")

    def ids_certified(self) -> int:
        """vrt_ids_certified: 1 when the next ID pass launches the certified ID kernel, else 0."""
        return int(self._lib.vrt_ids_certified(self._h))

    def reproject_temporal_async(self, cam: Camera, params: Params, prev_pv, alpha: float, row0: int, rows: int,
                                 pitch: int, d_raw: int, d_ids: int, d_depth: int, d_prev: int, d_prev_ids: int,
                                 prev_pitch: int, d_out: int, d_src: int = 0, stream: int = 0):
        """vrt_reproject_temporal_async: the reprojected temporal filter over rows [row0, row0 + rows), one
        kernel launch enqueued on a HIP stream. Device pointers (e.g. torch tensors' data_ptr()): d_raw,
        d_ids, d_depth, d_out and d_src (0: none) are band-indexed with `pitch` pixels per row, as
        render_ids_async writes them; d_prev and d_prev_ids are the whole previous frame and its IDs with
        prev_pitch pixels per row (both 0: no history). prev_pv: camera_forward() of the previous camera.
        d_src receives, per pixel, the previous frame's pixel index the history came from, or -1 (outside
        the previous image), -2 (behind the previous camera), -3 (another voxel, face or material there),
        -4 (no history)."""
        pv = np.ascontiguousarray(prev_pv, dtype=np.float32).reshape(16)
        self._check(self._lib.vrt_reproject_temporal_async(
            self._h, C.byref(cam), C.byref(params), pv.ctypes.data, alpha, row0, rows, pitch, d_raw or None,
            d_ids or None, d_depth or None, d_prev or None, d_prev_ids or None, prev_pitch, d_out or None,
            d_src or None, stream or None), "vrt_reproject_temporal_async")

    def reproject_temporal_fetch_async(self, cam: Camera, params: Params, prev_pv, alpha: float, fetch: int, row0: int,
                                       rows: int, pitch: int, d_raw: int, d_ids: int, d_depth: int, d_prev: int,
                                       d_prev_ids: int, prev_pitch: int, d_out: int, d_src: int = 0, d_taps: int = 0,
                                       stream: int = 0):
        """vrt_reproject_temporal_fetch_async: reproject_temporal_async with a history fetch mode, FETCH_NEAREST
        (that method's bytes) or FETCH_BILINEAR (the four texels around the reprojected position, each used
        only if it shows the pixel's own voxel face). d_src receives the nearest texel's index or the code,
        as there; d_taps (0: none) one byte per pixel at `pitch`, any alignment: the mask of the taps used
        (bit k: tap (x0 + (k & 1), y0 + (k >> 1))), 1 for a pixel the nearest fetch accepts, 0 for a pixel
        that is not accepted."""
        pv = np.ascontiguousarray(prev_pv, dtype=np.float32).reshape(16)
        self._check(self._lib.vrt_reproject_temporal_fetch_async(
            self._h, C.byref(cam), C.byref(params), pv.ctypes.data, alpha, fetch, row0, rows, pitch, d_raw or None,
            d_ids or None, d_depth or None, d_prev or None, d_prev_ids or None, prev_pitch, d_out or None,
            d_src or None, d_taps or None, stream or None), "vrt_reproject_temporal_fetch_async")

    def set_reprojected_fetch(self, mode: int):
        """vrt_set_reprojected_fetch: the history fetch of render_frame_reprojected's filter, FETCH_NEAREST (the
        default) or FETCH_BILINEAR; the history is kept across a switch."""
        self._check(self._lib.vrt_set_reprojected_fetch(self._h, mode), "vrt_set_reprojected_fetch")

    def render_frame_reprojected(self, cam: Camera, params: Params, alpha: float, timing: bool = False):
        """vrt_render_frame_reprojected: the frame loop with the reprojected temporal filter and a history of
        its own in the context (render_frame's is not touched). Returns the filtered frame rgba8[H, W, 4]
        uint8, or (frame, kernel_ms) with timing=True. The first call, the first after a change of the image
        size and the first after reprojected_history_reset() return the raw frame."""
        out = np.empty((cam.height, cam.width, 4), dtype=np.uint8)
        st = abi.Stats() if timing else None
        self._check(self._lib.vrt_render_frame_reprojected(self._h, C.byref(cam), C.byref(params), alpha,
                                                           out.ctypes.data, C.byref(st) if timing else None),
                    "vrt_render_frame_reprojected")
        return (out, float(st.kernel_ms)) if timing else out

    def reprojected_history_reset(self):
        """vrt_reprojected_history_reset: the next render_frame_reprojected has no history."""
        self._check(self._lib.vrt_reprojected_history_reset(self._h), "vrt_reprojected_history_reset")

    def spatial_filter_async(self, width: int, height: int, pitch: int, step: int, guide: int, range: int, row0: int,
                             rows: int, d_in: int, d_ids: int, d_keep: int, d_out: int, d_count: int = 0,
                             stream: int = 0):
        """vrt_spatial_filter_async: one ID-guided à-trous pass at `step` over rows [row0, row0 + rows) of a
        width x height frame, one kernel launch enqueued on a HIP stream. Device pointers, all indexed by the
        whole frame with `pitch` pixels per row: d_in and d_out RGBA8 words (they must differ), d_ids the
        frame's 8-byte ID records, d_keep (0: none) one byte per pixel, non-zero for a pixel that is copied
        through, d_count (0: none) one byte per pixel, the number of valid taps. guide: GUIDE_FACE or
        GUIDE_PLANE; range: the largest |dR| + |dG| + |dB| of a valid tap (765: no colour test)."""
        self._check(self._lib.vrt_spatial_filter_async(
            self._h, width, height, pitch, step, guide, range, row0, rows, d_in or None, d_ids or None,
            d_keep or None, d_out or None, d_count or None, stream or None), "vrt_spatial_filter_async")

    def spatial_filter(self, rgba8, ids, passes: int = 3, guide: int = GUIDE_FACE, range: int = 765, keep=None):
        """vrt_spatial_filter: `passes` passes (pass p at step 2^p) over the host frame rgba8[H, W, 4] uint8
        with the ID records ids[H, W] (PIXEL_ID_DTYPE, e.g. render_ids') and an optional keep[H, W] uint8
        (non-zero: the pixel is copied through). Returns the filtered frame [H, W, 4] uint8."""
        src = np.ascontiguousarray(rgba8, dtype=np.uint8)
        h, w = src.shape[:2]
        rec = np.ascontiguousarray(ids, dtype=PIXEL_ID_DTYPE).reshape(h, w)
        kp = None if keep is None else np.ascontiguousarray(keep, dtype=np.uint8).reshape(h, w)
        out = np.empty((h, w, 4), dtype=np.uint8)
        self._check(self._lib.vrt_spatial_filter(self._h, w, h, passes, guide, range, src.ctypes.data, rec.ctypes.data,
                                                 None if kp is None else kp.ctypes.data, out.ctypes.data),
                    "vrt_spatial_filter")
        return out

    def set_reprojected_spatial(self, mode: int, passes: int = 3, guide: int = GUIDE_FACE, range: int = 765):
        """vrt_set_reprojected_spatial: the spatial passes of render_frame_reprojected. SPATIAL_OFF (the default),
        SPATIAL_DISPLAY (the returned frame is filtered, the history is not) or SPATIAL_FILL (pixels without
        accepted history get their spatial estimate, in the returned frame and in the history). The history is
        kept across a switch."""
        self._check(self._lib.vrt_set_reprojected_spatial(self._h, mode, passes, guide, range),
                    "vrt_set_reprojected_spatial")

    def debug_packed_volume(self) -> np.ndarray:
        """The kernel's device volumes [octant][z][y][x] ((N+1)^3 u16 voxel | G << 8 each; 8
        octant volumes, or 1 for N = 1024), for tests."""
        p = self.n + 1
        k = self._lib.vrt_volume_octants(self._h)
        out = np.empty(k * p ** 3, np.uint16)
        self._check(self._lib.vrt_debug_packed_volume(self._h, out.ctypes.data, out.size),
                    "vrt_debug_packed_volume")
        return out.reshape(k, p, p, p)

    def set_skip_layout(self, octants: int):
        """Skip-distance layout of the next upload: 0 auto, 1 centred single volume, 8 octants."""
        self._check(self._lib.vrt_set_skip_layout(self._h, octants), "vrt_set_skip_layout")

    def set_certified(self, mode: int):
        """Certified walks for stats-free colour-only frames: 1 always, -1 never, 0 automatic."""
        self._check(self._lib.vrt_set_certified(self._h, mode), "vrt_set_certified")

    def certified(self) -> bool:
        """Whether the next stats-free colour-only frame uses certified walks."""
        return self._lib.vrt_certified(self._h) == 1

    def set_tile_order(self, on):
        """Heavy-first tile order for stats-free launches: False/0 off, True/1 automatic (default:
        launches of at least one dispatch round of waves), 2 every launch. Images are identical."""
        self._check(self._lib.vrt_set_tile_order(self._h, int(on)), "vrt_set_tile_order")

    def set_exact_pass(self, mode):
        """Deferred exact pass for certified launches: 0/False off, 1/True automatic (default:
        bands of at least two rounds of resident waves), 2 always. Images are identical."""
        self._check(self._lib.vrt_set_exact_pass(self._h, int(mode)), "vrt_set_exact_pass")

    def set_cert_trees(self, mode):
        """Certified bounce trees of glass pixels (ABI v15): 1 automatic (default: glass-heavy
        volumes), 2 always, 0 off. Images are identical."""
        self._check(self._lib.vrt_set_cert_trees(self._h, int(mode)), "vrt_set_cert_trees")

    def volume_device_ptr(self) -> int:
        return self._lib.vrt_volume_device_ptr(self._h) or 0

    def render(self, cam: Camera, params: Params, want_hits: bool = True, counters: bool = True):
        """Synchronous frame: returns (rgba[H,W,4] float32, hits[H,W] structured or None, stats).
        Hit records or counters run the exact-walk instance; with neither, the fast instance
        renders and stats holds kernel_ms only."""
        w, h = cam.width, cam.height
        rgba = np.empty((h, w, 4), dtype=np.float32)
        hits = np.empty((h, w), dtype=HIT_DTYPE) if want_hits else None
        st = abi.Stats()
        st.request = abi.VRT_STATS_COUNTERS if counters else 0
        self._check(
            self._lib.vrt_render(self._h, C.byref(cam), C.byref(params), rgba.ctypes.data,
                                 hits.ctypes.data if want_hits else None, C.byref(st)),
            "vrt_render",
        )
        stats = counters_dict(st.counters)
        stats["kernel_ms"] = float(st.kernel_ms)
        return rgba, hits, stats

    def render_rows_async(self, cam: Camera, params: Params, row0: int, rows: int, row_step: int,
                          d_out: int, d_hit: int = 0, d_counters: int = 0, stream: int = 0,
                          pitch: int = 0, row_block: int = 1):
        """Band render into device pointers (e.g. torch tensors' data_ptr()) on a HIP stream.
        pitch: pixels from one band row to the next (0 = width: a compact band buffer).
        row_block > 1: block-cyclic band (ABI v11): band row i is frame row
        row0 + (i // row_block) * row_step + i % row_block."""
        if row_block != 1:
            self._check(
                self._lib.vrt_render_blocks_pitched_async(
                    self._h, C.byref(cam), C.byref(params), row0, rows, row_step, row_block,
                    pitch or cam.width, d_out, d_hit or None, d_counters or None, stream or None),
                "vrt_render_blocks_pitched_async",
            )
            return
        if pitch:
            self._check(
                self._lib.vrt_render_rows_pitched_async(
                    self._h, C.byref(cam), C.byref(params), row0, rows, row_step, pitch, d_out,
                    d_hit or None, d_counters or None, stream or None),
                "vrt_render_rows_pitched_async",
            )
            return
        self._check(
            self._lib.vrt_render_rows_async(self._h, C.byref(cam), C.byref(params), row0, rows,
                                            row_step, d_out, d_hit or None, d_counters or None,
                                            stream or None),
            "vrt_render_rows_async",
        )

    def render_temporal_rows_async(self, cam: Camera, params: Params, alpha: float, row0: int,
                                   rows: int, row_step: int, d_prev: int, d_cur: int,
                                   d_raw: int = 0, d_hit: int = 0, d_counters: int = 0,
                                   stream: int = 0, pitch: int = 0, row_block: int = 1):
        """Band render with the fused temporal filter + RGB8 store (vrt_render_temporal_rows_async)
        into device RGBA8 buffers (e.g. torch uint8 [rows, W, 4] tensors' data_ptr()). pitch:
        pixels from one band row to the next in every buffer (0 = width). row_block > 1:
        block-cyclic band (vrt_render_temporal_blocks_pitched_async, ABI v11)."""
        if row_block != 1:
            self._check(
                self._lib.vrt_render_temporal_blocks_pitched_async(
                    self._h, C.byref(cam), C.byref(params), alpha, row0, rows, row_step,
                    row_block, pitch or cam.width, d_prev, d_cur, d_raw or None, d_hit or None,
                    d_counters or None, stream or None),
                "vrt_render_temporal_blocks_pitched_async",
            )
            return
        if pitch:
            self._check(
                self._lib.vrt_render_temporal_rows_pitched_async(
                    self._h, C.byref(cam), C.byref(params), alpha, row0, rows, row_step, pitch,
                    d_prev, d_cur, d_raw or None, d_hit or None, d_counters or None,
                    stream or None),
                "vrt_render_temporal_rows_pitched_async",
            )
            return
        self._check(
            self._lib.vrt_render_temporal_rows_async(
                self._h, C.byref(cam), C.byref(params), alpha, row0, rows, row_step, d_prev, d_cur,
                d_raw or None, d_hit or None, d_counters or None, stream or None),
            "vrt_render_temporal_rows_async",
        )

    def render_temporal_batch_async(self, cams, params, row0: int, rows: int, row_step: int,
                                    d_curs, d_raws=None, stream: int = 0, pitch: int = 0,
                                    row_block: int = 1):
        """The same band of len(cams) frames in one launch at alpha 1 (vrt_render_temporal_batch_async,
        ABI v14): cams / d_curs (/ d_raws) one per frame, params one Params or one per frame (ABI
        v15: frames whose params differ beyond u_Time take launches of their own, in order)."""
        nf = len(cams)
        if isinstance(params, Params):
            params = [params] * nf
        if len(params) != nf or len(d_curs) != nf or (d_raws is not None and len(d_raws) != nf):
            raise ValueError(f"render_temporal_batch_async: {nf} cameras need as many params, outputs "
                             "(and raw outputs, when given)")
        ca = (Camera * nf)(*cams)
        pa = (Params * nf)(*params)
        cur = (C.c_void_p * nf)(*d_curs)
        raw = (C.c_void_p * nf)(*d_raws) if d_raws else None
        self._check(
            self._lib.vrt_render_temporal_batch_async(self._h, nf, ca, pa, row0, rows, row_step, row_block,
                                                      pitch or cams[0].width, cur, raw, stream or None),
            "vrt_render_temporal_batch_async",
        )

    def render_frame(self, cam: Camera, params: Params, alpha: float = 1.0, counters: bool = False):
        """main.cpp's frame loop with the history in the context (vrt_render_frame): returns the
        new filtered frame as rgba8[H,W,4] uint8 and the stats (counters only when asked: they
        run the exact-walk instance)."""
        out = np.empty((cam.height, cam.width, 4), dtype=np.uint8)
        st = abi.Stats()
        st.request = abi.VRT_STATS_COUNTERS if counters else 0
        self._check(self._lib.vrt_render_frame(self._h, C.byref(cam), C.byref(params), alpha,
                                               out.ctypes.data, C.byref(st)), "vrt_render_frame")
        stats = counters_dict(st.counters)
        stats["kernel_ms"] = float(st.kernel_ms)
        return out, stats

    def render_frame_device(self, cam: Camera, params: Params, alpha: float, stream: int = 0,
                            timing: bool = False, counters: bool = False):
        """vrt_render_frame_device: the next filtered frame for display, on the first device,
        ordered on `stream`. Returns (device pointer of the W*H RGBA8 frame, owned by the context
        and valid until the fourth later call; stats dict or None). timing or counters wait for
        the frame (counters run the exact-walk instance); the dict then holds kernel_ms (and the
        counters)."""
        st = abi.Stats() if (timing or counters) else None
        if st is not None:
            st.request = abi.VRT_STATS_COUNTERS if counters else 0
        ptr = C.c_void_p()
        self._check(self._lib.vrt_render_frame_device(self._h, C.byref(cam), C.byref(params), alpha,
                                                      stream or None, C.byref(ptr),
                                                      C.byref(st) if st is not None else None),
                    "vrt_render_frame_device")
        if st is None:
            return ptr.value, None
        stats = counters_dict(st.counters)
        stats["kernel_ms"] = float(st.kernel_ms)
        return ptr.value, stats

    def frame_stream(self) -> int:
        """vrt_frame_stream: the HIP stream that produced the last device frame of a stream = 0
        (NULL) render_frame_device call; consume that frame there."""
        return self._lib.vrt_frame_stream(self._h) or 0

    def set_launch_timing(self, launches: int):
        """vrt_set_launch_timing: device start/end timestamps for the next `launches` async band
        launches (0: off)."""
        self._check(self._lib.vrt_set_launch_timing(self._h, int(launches)), "vrt_set_launch_timing")

    def launch_timing(self):
        """vrt_launch_timing: (sum of the recorded launches' kernel durations in ms, launches)."""
        total, n = C.c_double(), C.c_uint64()
        self._check(self._lib.vrt_launch_timing(self._h, C.byref(total), C.byref(n)),
                    "vrt_launch_timing")
        return total.value, n.value

    def debug_collectives(self):
        """vrt_debug_collectives: this one-device context takes the multi-GPU path through RCCL
        (one-rank communicator: ncclBroadcast of the volume, ncclGather of the band)."""
        self._check(self._lib.vrt_debug_collectives(self._h), "vrt_debug_collectives")

    def history_reset(self):
        """Key F (main.cpp:417-421): the last ray-traced frame becomes the temporal history."""
        self._check(self._lib.vrt_history_reset(self._h), "vrt_history_reset")


    def upload_atlas(self, atlas: np.ndarray):
        """Textured mode's atlas ([S, S, 4] uint8, row 0 = bottom) into the context."""
        a = np.ascontiguousarray(atlas, np.uint8)
        self._check(self._lib.vrt_upload_atlas(self._h, a.ctypes.data, a.shape[0]),
                    "vrt_upload_atlas")


    def debug_randomize(self, dirs: np.ndarray, pos: np.ndarray, randomness: float,
                        seed: float) -> np.ndarray:
        """The kernel's RandomizeDirection on [n, 3] inputs (vrt_debug_randomize), for tests."""
        d = np.ascontiguousarray(dirs, np.float32).reshape(-1, 3)
        p = np.ascontiguousarray(pos, np.float32).reshape(-1, 3)
        out = np.empty_like(d)
        self._check(self._lib.vrt_debug_randomize(self._h, d.ctypes.data, p.ctypes.data, len(d),
                                                  randomness, seed, out.ctypes.data),
                    "vrt_debug_randomize")
        return out


    def debug_cert_walks(self, rays: np.ndarray, kind: int) -> np.ndarray:
        """One certified walk per ray of `rays` (abi.CERT_RAY_DTYPE records) on the resident volume
        (vrt_debug_cert_walks), for tests -> abi.CERT_WALK_DTYPE records. kind 0: the air walk, 1: the
        shadow walk along the ray's direction, 2 and 3: the same in the certified pass's form."""
        r = np.ascontiguousarray(rays)
        if r.dtype.itemsize != 32 or r.ndim != 1:
            raise ValueError("debug_cert_walks: a one-dimensional array of 32-byte ray records")
        out = np.zeros(len(r), dtype=abi.CERT_WALK_DTYPE)
        self._check(self._lib.vrt_debug_cert_walks(self._h, r.ctypes.data, len(r), kind, out.ctypes.data),
                    "vrt_debug_cert_walks")
        return out

    def comm_join(self, ids, nranks: int, rank: int):
        """vrt_comm_join: one RCCL communicator per id (a list of VRT_COMM_ID_BYTES-byte ids), this
        context's device as `rank` of `nranks` (blocks until every rank joined each one)."""
        blob = b"".join(ids)
        buf = (C.c_uint8 * len(blob)).from_buffer_copy(blob)
        self._check(self._lib.vrt_comm_join(self._h, buf, len(ids), nranks, rank), "vrt_comm_join")

    def gather_band_async(self, comm: int, d_band: int, nbytes: int, d_gathered: int, stream: int):
        """vrt_gather_band_async: ncclGather of nbytes from every rank's d_band to rank 0's
        d_gathered (nranks x nbytes) on communicator `comm`, enqueued on `stream`."""
        self._check(self._lib.vrt_gather_band_async(self._h, comm, d_band, nbytes, d_gathered or None,
                                                    stream or None), "vrt_gather_band_async")

    def assemble_blocks_async(self, d_bands: int, k: int, band_rows_cap: int, width: int, height: int,
                              row_block: int, d_frame: int, frame_pitch: int, stream: int):
        """vrt_assemble_blocks_async: the frame's rows from k gathered block-cyclic bands."""
        self._check(self._lib.vrt_assemble_blocks_async(self._h, d_bands, k, band_rows_cap, width, height,
                                                        row_block, d_frame, frame_pitch, stream or None),
                    "vrt_assemble_blocks_async")

    def pack_rgb8_async(self, d_rgba8: int, pixels: int, d_rgb8: int, stream: int):
        """vrt_pack_rgb8_async: RGBA8 words -> 3-byte pixels (the RGB8 wire format of a gather)."""
        self._check(self._lib.vrt_pack_rgb8_async(self._h, d_rgba8, pixels, d_rgb8, stream or None),
                    "vrt_pack_rgb8_async")

    def assemble_blocks_rgb8_async(self, d_bands: int, k: int, band_rows_cap: int, width: int, height: int,
                                   row_block: int, d_frame: int, frame_pitch: int, stream: int):
        """vrt_assemble_blocks_rgb8_async: the frame's RGBA8 rows from k gathered RGB8 bands."""
        self._check(self._lib.vrt_assemble_blocks_rgb8_async(self._h, d_bands, k, band_rows_cap, width, height,
                                                             row_block, d_frame, frame_pitch, stream or None),
                    "vrt_assemble_blocks_rgb8_async")

    def build_scene_device(self, scene: str, n: int, seed: int = 0, stream: int = 0):
        """Build a scene's volume on the device (vrt_build_scene_device) and make it current."""
        self._check(self._lib.vrt_build_scene_device(self._h, SCENES[scene], n, seed,
                                                     stream or None), "vrt_build_scene_device")
        self.n = n
