"""The ID-guided spatial filter restated in NumPy integers (include/vrt.h, vrt_spatial_filter_async): the one
reference of tests/test_spatial_cpu.py and tests/test_gpu_spatial.py. The pass, the multi-pass chain of
vrt_spatial_filter and the two modes of vrt_set_reprojected_spatial. Every operation is an integer operation, so
the restatement is exact: the GPU tests compare bytes. Scenes and cameras are reproject_reference's. Plain helpers,
no tests."""
import functools

import numpy as np

import oracle
import reproject_reference as ref
import voxelraytracer_amd as vrt
from voxelraytracer_amd import abi

FACE, PLANE = vrt.GUIDE_FACE, vrt.GUIDE_PLANE
KERNEL = (1, 4, 6, 4, 1)
NOISE = dict(reflection_noise=0.05, refraction_noise=0.01)   # beside ray_noise 0.05: the reference's settings


def keys(ids, guide, n):
    """The guide's key of every record as two int64 arrays: FACE both words; PLANE, for a hit, the cell coordinate
    along the face's axis in place of the voxel index (a miss keeps its negative word)."""
    v, f = ids["voxel_index"].astype(np.int64), ids["face"].astype(np.int64)
    if guide == PLANE:
        nlog = int(n).bit_length() - 1
        assert 1 << nlog == n, n
        v = np.where(v >= 0, (v >> ((f & 3) * nlog)) & (n - 1), v)
    else:
        assert guide == FACE, guide
    return v, f


def taps(h, w, step):
    """Per tap (i, j): its weight, whether it lies in the image, and its clamped coordinates, for every pixel."""
    ys, xs = np.arange(h)[:, None], np.arange(w)[None, :]
    for j in range(-2, 3):
        for i in range(-2, 3):
            ty, tx = ys + j * step, xs + i * step
            inside = (ty >= 0) & (ty < h) & (tx >= 0) & (tx < w)
            yield KERNEL[i + 2] * KERNEL[j + 2], inside, np.clip(ty, 0, h - 1) + 0 * tx, np.clip(tx, 0, w - 1) + 0 * ty


def spatial_pass(rgba8, ids, step, guide=FACE, rng=765, keep=None, n=ref.N, stats=None):
    """One pass over the whole frame. rgba8 [H, W, 4] uint8, ids [H, W] PIXEL_ID_DTYPE, keep [H, W] (non-zero: kept)
    or None. Returns (out [H, W, 4] uint8, count [H, W] uint8). stats (a dict, optional) receives per-pixel masks
    that ignore keep: "guide" (a tap in the image rejected by the key), "range" (a tap in the image with the
    pixel's key rejected by the colour test), "alone" (the centre is the only valid tap)."""
    src = np.ascontiguousarray(rgba8, np.uint8)
    h, w = src.shape[:2]
    c = src.astype(np.int64)
    k0, k1 = keys(ids, guide, n)
    acc = np.zeros((h, w, 3), np.int64)
    wsum = np.zeros((h, w), np.int64)
    count = np.zeros((h, w), np.int64)
    by_guide = np.zeros((h, w), bool)
    by_range = np.zeros((h, w), bool)
    for wt, inside, ty, tx in taps(h, w, step):
        same = inside & (k0[ty, tx] == k0) & (k1[ty, tx] == k1)
        tc = c[ty, tx]
        near = np.abs(tc[..., :3] - c[..., :3]).sum(-1) <= rng
        valid = same & near
        by_guide |= inside & ~same
        by_range |= same & ~near
        acc += np.where(valid[..., None], wt * tc[..., :3], 0)
        wsum += np.where(valid, wt, 0)
        count += valid
    assert wsum.min() >= 36 and wsum.max() <= 256 and count.min() >= 1, (wsum.min(), wsum.max(), count.min())
    out = np.empty((h, w, 4), np.uint8)
    out[..., :3] = (2 * acc + wsum[..., None]) // (2 * wsum[..., None])
    out[..., 3] = 255
    if stats is not None:
        stats.update(guide=by_guide, range=by_range, alone=count == 1)
    if keep is not None:
        kept = np.asarray(keep).reshape(h, w) != 0
        out[kept] = src[kept]
        count[kept] = 0
    return out, count.astype(np.uint8)


def chain(rgba8, ids, passes=3, guide=FACE, rng=765, keep=None, n=ref.N):
    """vrt_spatial_filter: pass p = 0 .. passes - 1 at step 2^p, each on the previous pass's output."""
    out = np.ascontiguousarray(rgba8, np.uint8)
    for p in range(passes):
        out, _ = spatial_pass(out, ids, 1 << p, guide, rng, keep, n)
    return out


def loop_frame(mode, temporal_out, tap_bytes, ids, passes=3, guide=FACE, rng=765, n=ref.N):
    """One frame of vrt_render_frame_reprojected after its temporal filter (temporal_out, tap_bytes: that filter's
    output and tap bytes; ids: the frame's noise-free records). Returns (returned frame, next history)."""
    if mode == vrt.SPATIAL_OFF:
        return temporal_out, temporal_out
    if mode == vrt.SPATIAL_DISPLAY:
        return chain(temporal_out, ids, passes, guide, rng, None, n), temporal_out
    assert mode == vrt.SPATIAL_FILL, mode
    filled = chain(temporal_out, ids, passes, guide, rng, tap_bytes, n)
    return filled, filled


def rmse(a, b):
    """Root mean square error over R, G and B, in 8-bit LSB."""
    d = a[..., :3].astype(np.float64) - b[..., :3].astype(np.float64)
    return float(np.sqrt(np.mean(d * d)))


@functools.lru_cache(maxsize=None)
def oracle_frames(name, cam_name):
    """The oracle's quantised frames of a scene and camera: (noisy at ray_noise 0.05, reflection_noise 0.05,
    refraction_noise 0.01; noise-free), each [H, W, 4] uint8, read-only."""
    cam, vox = ref.camera(cam_name), ref.scene(name)
    out = []
    for p in (ref.params(0.05, **NOISE), ref.params(0.0)):
        rgba, _, _ = oracle.render(cam, vox, ref.N, p, threads=4)
        raw, _ = oracle.temporal(rgba, np.zeros(rgba.shape, np.uint8), 1.0)
        raw.setflags(write=False)
        out.append(raw)
    return tuple(out)


def oracle_ids(name, cam_name):
    """The oracle's noise-free ID records of a scene and camera (reproject_reference.oracle_frame's cache)."""
    return ref.oracle_frame(name, cam_name)["ids"]


def random_frame(h, w, seed):
    """A seeded random RGBA8 frame with A = 255."""
    c = np.random.default_rng(seed).integers(0, 256, (h, w, 4), dtype=np.uint8)
    c[..., 3] = 255
    return c


def ids_from(voxel_index, face):
    """[H, W] PIXEL_ID_DTYPE records from two integer arrays."""
    v = np.asarray(voxel_index)
    ids = np.zeros(v.shape, abi.PIXEL_ID_DTYPE)
    ids["voxel_index"], ids["face"] = v, face
    return ids
