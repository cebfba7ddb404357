"""The fetch modes of the reprojected temporal filter restated in NumPy float32 (include/vrt.h,
vrt_reproject_temporal_fetch_async): the one reference of tests/test_reproject_bilinear_cpu.py and
tests/test_gpu_reproject_bilinear.py. Cameras, scenes and the oracle's per-pixel geometry are
reproject_reference's. Every operation is a float32 operation in the header's order, with a dtype assertion
on every intermediate, so the restatement is exact: the GPU tests compare bytes. The blend is written here
in NumPy (b / 255 as an IEEE float32 division, np.rint: half to even), with no call into the C oracle.
taps() and blend() stand alone so that each can be pinned by hand. Plain helpers, no tests."""
import numpy as np

import reproject_reference as ref
from reproject_reference import BEHIND, MISMATCH, NO_HISTORY, OUTSIDE  # noqa: F401  (re-exported)

f32 = np.float32
FETCH_NEAREST, FETCH_BILINEAR = 0, 1


def _f(*arrays):
    for a in arrays:
        assert a.dtype == f32, a.dtype
    return arrays[0] if len(arrays) == 1 else arrays


def screen(ids, depth, pos, dirs, n, prev_pv):
    """Steps 1-6 over a whole frame: (sx, sy, front, inside); sx and sy mean something where front & inside."""
    h, w = ids.shape
    m = np.asarray(prev_pv, f32).reshape(16)
    pos, dirs, depth = np.asarray(pos, f32), np.asarray(dirs, f32), np.asarray(depth, f32)
    hit = ids["voxel_index"] >= 0
    half = f32(n) * f32(0.5)
    with np.errstate(all="ignore"):
        v = [_f(np.where(hit, _f(_f(pos[..., i] + _f(depth * dirs[..., i])) - half), dirs[..., i])) for i in range(3)]
        wc = _f(np.where(hit, f32(1.0), f32(0.0)).astype(f32))
        clip = [_f(_f(_f(_f(m[0 * 4 + r] * v[0]) + _f(m[1 * 4 + r] * v[1])) + _f(m[2 * 4 + r] * v[2]))
                   + _f(m[3 * 4 + r] * wc)) for r in range(4)]
        front = clip[3] > 0
        sx = _f(_f(_f(_f(clip[0] / clip[3]) * f32(0.5)) + f32(0.5)) * f32(w))
        sy = _f(_f(_f(_f(clip[1] / clip[3]) * f32(0.5)) + f32(0.5)) * f32(h))
        inside = (sx >= 0) & (sx < f32(w)) & (sy >= 0) & (sy < f32(h))
    return sx, sy, front, inside


def taps(sx, sy):
    """Steps 7 and 8 for float32 arrays sx, sy of one shape S: coords int64 [S..., 4, 2] (x, y of tap k = 0..3,
    possibly -1 or width / height) and weights float32 [S..., 4]."""
    sx, sy = np.asarray(sx), np.asarray(sy)
    _f(sx, sy)
    tx, ty = _f(sx - f32(0.5)), _f(sy - f32(0.5))
    x0, y0 = _f(np.floor(tx)), _f(np.floor(ty))
    fx, fy = _f(tx - x0), _f(ty - y0)
    ix0, iy0 = x0.astype(np.int64), y0.astype(np.int64)
    gx, gy = _f(f32(1.0) - fx), _f(f32(1.0) - fy)
    weights = np.stack([_f(gx * gy), _f(fx * gy), _f(gx * fy), _f(fx * fy)], axis=-1)
    coords = np.stack([np.stack([ix0 + (k & 1), iy0 + (k >> 1)], axis=-1) for k in range(4)], axis=-2)
    return coords, _f(weights)


def in_image(coords, w, h):
    """Step 9's range test: [S..., 4] bool."""
    return (coords[..., 0] >= 0) & (coords[..., 0] < w) & (coords[..., 1] >= 0) & (coords[..., 1] < h)


def unorm8_read(b):
    return _f(np.asarray(b).astype(f32) / f32(255))


def unorm8(x):
    _f(x)
    return np.rint(_f(_f(np.minimum(np.maximum(x, f32(0.0)), f32(1.0))) * f32(255.0))).astype(np.uint8)


def blend(raw, tap_bytes, valid, weights, alpha):
    """Steps 10 and 11. raw uint8 [S..., 4]; tap_bytes uint8 [S..., 4 taps, 4 channels] (an invalid tap's bytes
    are not read); valid bool [S..., 4]; weights float32 [S..., 4]. Returns (out uint8 [S..., 4], wsum float32
    [S...]): the raw pixel where no tap is valid, else the blend with A = 255."""
    raw, tap_bytes = np.asarray(raw, np.uint8), np.asarray(tap_bytes, np.uint8)
    valid, weights = np.asarray(valid, bool), _f(np.asarray(weights))
    a = f32(alpha)
    om = f32(1.0) - a
    assert om.dtype == f32
    v = _f(np.where(valid, weights, f32(0.0)).astype(f32))
    wsum = _f(_f(_f(v[..., 0] + v[..., 1]) + v[..., 2]) + v[..., 3])
    accepted = valid.any(axis=-1)
    out = raw.copy()
    c = _f(np.where(valid[..., None], unorm8_read(tap_bytes), f32(0.0)).astype(f32))   # [S..., tap, channel]
    with np.errstate(all="ignore"):
        for ch in range(3):
            s = _f(_f(_f(_f(v[..., 0] * c[..., 0, ch]) + _f(v[..., 1] * c[..., 1, ch])) + _f(v[..., 2] * c[..., 2, ch]))
                   + _f(v[..., 3] * c[..., 3, ch]))
            hist = _f(s / wsum)
            mixed = _f(_f(a * unorm8_read(raw[..., ch])) + _f(om * hist))
            out[..., ch] = np.where(accepted, unorm8(np.where(accepted, mixed, f32(0.0)).astype(f32)), raw[..., ch])
    out[..., 3] = np.where(accepted, 255, raw[..., 3])
    return out, wsum


def bilinear(ids, depth, pos, dirs, n, prev_pv, prev_ids, prev_rgba8, raw_rgba8, alpha):
    """VRT_FETCH_BILINEAR over a whole frame, arguments as reproject_reference.reproject. Returns (out [H, W, 4]
    uint8, src [H, W] int32, taps [H, W] uint8, wsum [H, W] float32 (0 where not accepted))."""
    h, w = ids.shape
    raw = np.ascontiguousarray(raw_rgba8, np.uint8)
    if prev_ids is None and prev_rgba8 is None:
        return raw.copy(), np.full((h, w), NO_HISTORY, np.int32), np.zeros((h, w), np.uint8), np.zeros((h, w), f32)
    prev = np.asarray(prev_rgba8, np.uint8)
    sx, sy, front, inside = screen(ids, depth, pos, dirs, n, prev_pv)
    ok = front & inside
    sx0, sy0 = np.where(ok, sx, f32(0.0)).astype(f32), np.where(ok, sy, f32(0.0)).astype(f32)
    coords, weights = taps(sx0, sy0)
    inr = in_image(coords, w, h)
    cx, cy = np.where(inr, coords[..., 0], 0), np.where(inr, coords[..., 1], 0)   # a tap outside is never read
    pid = prev_ids[cy, cx]
    same = (pid["voxel_index"] == ids["voxel_index"][..., None]) & (pid["face"] == ids["face"][..., None])
    valid = ok[..., None] & inr & (weights > 0) & same
    out, wsum = blend(raw, prev[cy, cx], valid, weights, alpha)
    accepted = valid.any(axis=-1)
    qx, qy = np.floor(sx0).astype(np.int64), np.floor(sy0).astype(np.int64)
    src = np.where(~front, BEHIND, np.where(~inside, OUTSIDE, np.where(~accepted, MISMATCH, qy * w + qx))).astype(np.int32)
    mask = (valid * (1 << np.arange(4))).sum(axis=-1).astype(np.uint8)
    return out, src, mask, np.where(accepted, wsum, f32(0.0)).astype(f32)


def nearest(ids, depth, pos, dirs, n, prev_pv, prev_ids, prev_rgba8, raw_rgba8, alpha):
    """VRT_FETCH_NEAREST: reproject_reference.reproject plus the tap byte (1 for an accepted pixel)."""
    out, src = ref.reproject(ids, depth, pos, dirs, n, prev_pv, prev_ids, prev_rgba8, raw_rgba8, alpha)
    return out, src, (src >= 0).astype(np.uint8)


def fetch(mode, *args):
    """(out, src, taps) of either mode."""
    return bilinear(*args)[:3] if mode == FETCH_BILINEAR else nearest(*args)


def tap_stats(ids, depth, pos, dirs, n, prev_pv, prev_ids):
    """What a frame pair offers the tests, by colour-free outcome counts: the bilinear src and masks (grey
    colours), the nearest src, and per pixel whether a tap lies outside the image."""
    h, w = ids.shape
    grey = np.full((h, w, 4), 128, np.uint8)
    _, src, mask, wsum = bilinear(ids, depth, pos, dirs, n, prev_pv, prev_ids, grey, grey, 0.3)
    _, nsrc = ref.reproject(ids, depth, pos, dirs, n, prev_pv, prev_ids, grey, grey, 0.3)
    sx, sy, front, inside = screen(ids, depth, pos, dirs, n, prev_pv)
    ok = front & inside
    coords, _ = taps(np.where(ok, sx, f32(1.0)).astype(f32), np.where(ok, sy, f32(1.0)).astype(f32))
    border = ok & ~in_image(coords, w, h).all(axis=-1)
    # bit of the nearest texel among the four taps
    qx = np.where(ok, np.floor(np.where(ok, sx, 0)), 0).astype(np.int64)
    qy = np.where(ok, np.floor(np.where(ok, sy, 0)), 0).astype(np.int64)
    kx, ky = qx - coords[..., 0, 0], qy - coords[..., 0, 1]
    assert np.all((kx[ok] >= 0) & (kx[ok] <= 1) & (ky[ok] >= 0) & (ky[ok] <= 1))   # the nearest texel is a tap
    nbit = (1 << (np.clip(kx, 0, 1) + 2 * np.clip(ky, 0, 1))).astype(np.uint8)
    return {"src": src, "mask": mask, "wsum": wsum, "nearest_src": nsrc, "border": border, "nearest_bit": nbit,
            "ok": ok}


def counts(src, mask):
    c = ref.counts(src)
    c["partial"] = int(np.count_nonzero((src >= 0) & (mask != 15)))
    return c
