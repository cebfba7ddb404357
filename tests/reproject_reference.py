"""The reprojected temporal filter restated in NumPy float32 (include/vrt.h, vrt_reproject_temporal_async):
the one reference of tests/test_reproject_cpu.py and tests/test_gpu_reproject.py, with the cameras and the
oracle's per-pixel geometry they share. Every operation is a float32 operation in the header's order, so
the restatement is exact: the GPU tests compare bytes. The blend is the oracle's (oracle.temporal_from_raw).
Plain helpers, no tests."""
import functools

import numpy as np

import oracle
import voxelraytracer_amd as vrt
from harness import first_records
from voxelraytracer_amd import abi

N, W, H = 16, 96, 54
SCENES = ("terrain", "glass_cube", "refraction")
# camera A is the default pose; B a small move (history mostly kept); C a turn of more than 90 degrees
# (points behind the previous camera occur)
CAMERAS = {
    "A": (vrt.DEFAULT_CAM_POS, vrt.DEFAULT_CAM_ROT),
    "B": ((-3.05, 2.02, 3.78), (-31.0, -53.0, 0.0)),
    "C": ((-3.05, 2.02, 3.78), (-20.0, -158.0, 0.0)),
}
NO_HISTORY, BEHIND, OUTSIDE, MISMATCH = -4, -2, -1, -3


def camera(name, w=W, h=H):
    pos, rot = CAMERAS[name]
    return vrt.make_camera(w, h, pos=pos, rot=rot)


@functools.lru_cache(maxsize=None)
def scene(name, n=N):
    v = vrt.build_scene(name, n)
    v.setflags(write=False)
    return v


def params(ray_noise=0.0, time=1.0, **kw):
    return vrt.default_params(1, 2, ray_noise=ray_noise, time=time, **kw)


@functools.lru_cache(maxsize=None)
def oracle_frame(name, cam_name, ray_noise=0.0, time=1.0, w=W, h=H, n=N):
    """What the oracle says about every pixel's primary ray (oracle.trace_pixel's first record,
    harness.first_records): pos and dir as the ray entered RayMarch, and the
    ID and depth pass restated from its hit: voxel_index (oracle.render's hit record), face = axis (a tie's
    3 clamped to 2) | 4 if the normal -sign(dir[axis]) is negative | voxel byte << 8, depth =
    (rint(point[axis]) - pos[axis]) / dir[axis] in float32, +inf and face 0 for a miss."""
    cam, p, vox = camera(cam_name, w, h), params(ray_noise, time), scene(name, n)
    _, hits, _ = oracle.render(cam, vox, n, p, threads=4)
    recs = first_records(cam, vox, n, p)
    pos, dirs = recs[..., 9:12].astype(np.float32), recs[..., 12:15].astype(np.float32)
    ids = np.zeros((h, w), dtype=abi.PIXEL_ID_DTYPE)
    depth = np.full((h, w), np.inf, np.float32)
    for py in range(h):
        for px in range(w):
            r = recs[py, px]
            found = r[1] != 0
            assert found == (hits["voxel_index"][py, px] >= 0), ((px, py), float(r[1]), int(hits["voxel_index"][py, px]))
            if found:
                a = min(int(r[3]), 2)
                ids[py, px] = (hits["voxel_index"][py, px], a | (4 if r[12 + a] > 0 else 0) | (int(r[2]) << 8))
                depth[py, px] = (np.rint(r[4 + a]) - r[9 + a]) / r[12 + a]
            else:
                ids[py, px] = (-1, 0)
    for arr in (pos, dirs, ids, depth):
        arr.setflags(write=False)
    return {"pos": pos, "dir": dirs, "ids": ids, "depth": depth}


def primary_rays(cam_name, ray_noise=0.0, time=1.0, w=W, h=H, n=N):
    """(pos, dir) of every pixel's primary ray. The ray depends on the volume through its size alone."""
    f = oracle_frame("terrain", cam_name, ray_noise, time, w, h, n)
    return f["pos"], f["dir"]


def reproject(ids, depth, pos, dirs, n, prev_pv, prev_ids, prev_rgba8, raw_rgba8, alpha):
    """vrt_reproject_temporal_async over a whole frame. ids [H, W] PIXEL_ID_DTYPE, depth [H, W] float32, pos
    and dirs [H, W, 3] float32: the current frame's; prev_pv: 16 float32, column-major; prev_ids [H, W] and
    prev_rgba8 [H, W, 4] uint8: the previous frame's (both None: no history); raw_rgba8 [H, W, 4] uint8.
    Returns (out [H, W, 4] uint8, src [H, W] int32)."""
    h, w = ids.shape
    raw = np.ascontiguousarray(raw_rgba8, np.uint8)
    if prev_ids is None and prev_rgba8 is None:
        return raw.copy(), np.full((h, w), NO_HISTORY, np.int32)
    f32 = np.float32
    m = np.asarray(prev_pv, f32).reshape(16)
    pos, dirs, depth = np.asarray(pos, f32), np.asarray(dirs, f32), np.asarray(depth, f32)
    hit = ids["voxel_index"] >= 0
    half = f32(n) * f32(0.5)
    with np.errstate(all="ignore"):
        v = [np.where(hit, (pos[..., i] + depth * dirs[..., i]) - half, dirs[..., i]) for i in range(3)]
        wc = np.where(hit, f32(1.0), f32(0.0)).astype(f32)
        clip = [((m[0 * 4 + r] * v[0] + m[1 * 4 + r] * v[1]) + m[2 * 4 + r] * v[2]) + m[3 * 4 + r] * wc
                for r in range(4)]
        assert all(c.dtype == f32 for c in clip)
        front = clip[3] > 0
        sx = ((clip[0] / clip[3]) * f32(0.5) + f32(0.5)) * f32(w)
        sy = ((clip[1] / clip[3]) * f32(0.5) + f32(0.5)) * f32(h)
        assert sx.dtype == f32 and sy.dtype == f32
        inside = (sx >= 0) & (sx < f32(w)) & (sy >= 0) & (sy < f32(h))
    ok = front & inside
    qx = np.where(ok, np.floor(np.where(ok, sx, 0)), 0).astype(np.int64)
    qy = np.where(ok, np.floor(np.where(ok, sy, 0)), 0).astype(np.int64)
    pid = prev_ids[qy, qx]
    same = (pid["voxel_index"] == ids["voxel_index"]) & (pid["face"] == ids["face"])
    accept = ok & same
    src = np.where(~front, BEHIND, np.where(~inside, OUTSIDE, np.where(~same, MISMATCH, qy * w + qx))).astype(np.int32)
    blended = oracle.temporal_from_raw(raw, np.ascontiguousarray(np.asarray(prev_rgba8, np.uint8)[qy, qx]), alpha)
    out = np.where(accept[..., None], blended, raw)
    return out, src


def counts(src):
    """How many pixels of src were accepted, and how many got each code."""
    return {"accepted": int(np.count_nonzero(src >= 0)), OUTSIDE: int(np.count_nonzero(src == OUTSIDE)),
            BEHIND: int(np.count_nonzero(src == BEHIND)), MISMATCH: int(np.count_nonzero(src == MISMATCH)),
            NO_HISTORY: int(np.count_nonzero(src == NO_HISTORY))}
