"""The skip field of the packed volume(s), restated twice, with the small edit helpers the tests share.

By brute force in NumPy (forward_reference, chebyshev_reference, packed_reference): the reference of
the GPU volume tests (tests/test_gpu_volume.py, tests/test_gpu_volume_edit.py) and of the edit plan's
CPU test (tests/test_volume_edit_plan.py) at N <= 32, where the caps clamp nothing and every regional
box is the whole volume.

By tests/skipfield_fast.c (forward_fast, chebyshev_fast, packed_fast): the largest-empty-cube dynamic
programme and the 26-neighbour chamfer, which share no algorithm with the kernels or with the brute
force, equal the brute force at N <= 32 (tests/test_skipfield_fast.py) and reach N = 256, where the
caps clamp and the boxes are regional (tests/test_gpu_skipfield_caps.py, tests/test_volume_edit_plan.py).
void256 is the volume of those tests. Plain helpers, no tests."""
import ctypes as C
import functools
import hashlib
import os
import subprocess

import numpy as np

CAP = 64  # kDistCap of csrc/vrt_walk.h
FWD_CAP = 128  # kFwdCap (VRT_FWD_CAP, csrc/vrt_tuning.h)
UNCAPPED = 255  # the largest cap the fast reference takes: nothing in a 256^3 volume reaches it

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)


# ---- the fast reference (tests/skipfield_fast.c) -------------------------------------------------

@functools.lru_cache(maxsize=None)
def load_skipfield_fast():
    """tests/skipfield_fast.c, built once per process into build/skipfield_fast.so, with its ctypes
    signatures."""
    so = os.path.join(ROOT, "build", "skipfield_fast.so")
    os.makedirs(os.path.dirname(so), exist_ok=True)
    subprocess.check_call(["gcc", "-O2", "-shared", "-fPIC", "-fopenmp", "-o", so,
                           os.path.join(HERE, "skipfield_fast.c")])
    L = C.CDLL(so)
    L.sf_forward.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p]
    L.sf_chebyshev.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p]
    L.sf_packed.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p]
    for fn in (L.sf_forward, L.sf_chebyshev, L.sf_packed):
        fn.restype = C.c_int
    return L


def volume_bytes(vox, n):
    v = np.ascontiguousarray(vox, np.uint8).reshape(-1)
    assert v.size == n ** 3, (v.size, n)
    return v


def forward_fast(vox, n, octant, cap=FWD_CAP):
    """F of `octant` at every anchor, [z][y][x] n^3 u8 (F, not G: G(w) = max(F(w - s) - 1, 0))."""
    v, out = volume_bytes(vox, n), np.empty((n, n, n), np.uint8)
    rc = load_skipfield_fast().sf_forward(v.ctypes.data, n, octant, cap, out.ctypes.data)
    assert rc == 0, ("sf_forward", rc)
    return out


def chebyshev_fast(vox, n, cap=CAP):
    """D at every voxel, [z][y][x] n^3 u8."""
    v, out = volume_bytes(vox, n), np.empty((n, n, n), np.uint8)
    rc = load_skipfield_fast().sf_chebyshev(v.ctypes.data, n, cap, out.ctypes.data)
    assert rc == 0, ("sf_chebyshev", rc)
    return out


_volumes = {}   # digest -> bytes, for the cached function's first call


@functools.lru_cache(maxsize=3)   # 271 MB per entry at N = 256, octants = 8
def _packed_fast(digest, n, octants, fwd_cap, dist_cap):
    v = _volumes.pop(digest)
    out = np.empty((octants,) + (n + 1,) * 3, np.uint16)
    rc = load_skipfield_fast().sf_packed(v.ctypes.data, n, octants, fwd_cap, dist_cap, out.ctypes.data)
    assert rc == 0, ("sf_packed", rc)
    out.setflags(write=False)
    return out


def packed_fast(vox, n, octants, fwd_cap=FWD_CAP, dist_cap=CAP):
    """packed_reference by the fast reference: [octant][z][y][x] (n+1)^3 u16, read-only, cached per
    volume (by its bytes' digest), layout and caps."""
    v = volume_bytes(vox, n)
    digest = hashlib.sha1(v).digest()
    _volumes[digest] = v
    try:
        return _packed_fast(digest, n, octants, fwd_cap, dist_cap)
    finally:
        _volumes.pop(digest, None)


@functools.lru_cache(maxsize=None)
def void256():
    """256^3 bytes, read-only: a void with an off-centre cluster (every in-volume cube of edge >= 129
    holds the voxel (128, 128, 128), so a centred object would keep kFwdCap from ever clamping), one
    glass block beside it, two lone voxels and a floor slab. Indexed [z][y][x]."""
    v = np.zeros((256, 256, 256), np.uint8)
    v[60:66, 60:66, 60:66] = 1
    v[60:66, 60:66, 66:72] = 2
    v[10, 10, 10] = 3
    v[30, 200, 245] = 200
    v[:, 20, :] = 3
    flat = v.reshape(-1)
    flat.setflags(write=False)
    return flat


# ---- the brute force -----------------------------------------------------------------------------


def forward_reference(vox, n, octant):
    """G of `octant` ([z][y][x] n^3): in coordinates flipped so that the octant's step is +1 on
    every axis, F(v) = the largest E <= FWD_CAP with v + E <= n and the cube [v, v+E-1]^3 empty
    (prefix-sum box counts), G(v) = F(v - 1) - 1 clamped at 0 (0 on the low faces)."""
    sl = tuple(slice(None, None, -1) if octant >> a & 1 else slice(None) for a in (2, 1, 0))
    occ = (vox.reshape(n, n, n) != 0)[sl].astype(np.int64)
    c = np.zeros((n + 1,) * 3, np.int64)
    c[1:, 1:, 1:] = occ.cumsum(0).cumsum(1).cumsum(2)
    f = np.zeros((n, n, n), np.int64)
    for e in range(1, min(FWD_CAP, n) + 1):
        m = n - e + 1   # anchors with v + e <= n on every axis
        i0 = np.arange(m)
        z0, y0, x0 = i0[:, None, None], i0[None, :, None], i0[None, None, :]
        z1, y1, x1 = z0 + e, y0 + e, x0 + e
        cnt = (c[z1, y1, x1] - c[z0, y1, x1] - c[z1, y0, x1] - c[z1, y1, x0] + c[z0, y0, x1]
               + c[z0, y1, x0] + c[z1, y0, x0] - c[z0, y0, x0])
        f[:m, :m, :m] = np.where(cnt == 0, e, f[:m, :m, :m])
    g = np.zeros((n, n, n), np.int64)
    g[1:, 1:, 1:] = np.maximum(f[:-1, :-1, :-1] - 1, 0)
    return g[sl]


def chebyshev_reference(vox, n):
    """D ([z][y][x] n^3): the smallest r < CAP with a non-empty voxel (or the outside) in the
    (2r+1)^3 box around the voxel, else CAP."""
    occ = np.ones((n + 2 * CAP,) * 3, bool)   # everything outside the volume is non-empty
    occ[CAP:CAP + n, CAP:CAP + n, CAP:CAP + n] = vox.reshape(n, n, n) != 0
    c = np.zeros((n + 2 * CAP + 1,) * 3, np.int64)
    c[1:, 1:, 1:] = occ.astype(np.int64).cumsum(0).cumsum(1).cumsum(2)
    d = np.full((n, n, n), CAP, np.int64)
    i = np.arange(n) + CAP
    for r in range(CAP - 1, -1, -1):
        l, h = i - r, i + r + 1
        z0, y0, x0 = l[:, None, None], l[None, :, None], l[None, None, :]
        z1, y1, x1 = h[:, None, None], h[None, :, None], h[None, None, :]
        cnt = (c[z1, y1, x1] - c[z0, y1, x1] - c[z1, y0, x1] - c[z1, y1, x0] + c[z0, y0, x1]
               + c[z0, y1, x0] + c[z1, y0, x0] - c[z0, y0, x0])
        d = np.where(cnt > 0, r, d)
    return d


def packed_texels(vox, n, octants):
    """[octant][z][y][x] n^3: voxel | skip distance << 8 (the texels in [0, n)^3 of the packed volumes)."""
    v = vox.reshape(n, n, n).astype(np.int64)
    if octants == 8:
        return np.stack([v | forward_reference(vox, n, o) << 8 for o in range(8)])
    return (v | chebyshev_reference(vox, n) << 8)[None]


def packed_reference(vox, n, octants):
    """[octant][z][y][x] (n+1)^3 u16, the whole of Renderer.debug_packed_volume(): packed_texels in
    [0, n)^3; texel n of an axis repeats voxel 0 of that axis (edges and the corner too) with skip
    distance 0."""
    wrap = np.arange(n + 1) % n
    out = np.empty((octants,) + (n + 1,) * 3, np.int64)
    out[:] = vox.reshape(n, n, n).astype(np.int64)[np.ix_(wrap, wrap, wrap)]
    out[:, :n, :n, :n] = packed_texels(vox, n, octants)
    return out.astype(np.uint16)


def random_edit(rng, n):
    """(origin (x, y, z), block [z][y][x]): a box of edge 1..6, carved, filled or random bytes."""
    e = rng.integers(1, 7, 3)
    o = [int(rng.integers(0, n - int(e[a]) + 1)) for a in range(3)]
    kind = int(rng.integers(0, 3))
    shape = (int(e[2]), int(e[1]), int(e[0]))
    if kind == 0:
        block = np.zeros(shape, np.uint8)
    elif kind == 1:
        block = np.full(shape, int(rng.integers(1, 4)), np.uint8)
    else:
        block = rng.integers(0, 4, shape).astype(np.uint8)
    return o, block


def apply_edit(vox, n, origin, block):
    """The edited copy of the n^3 bytes: `block` [z][y][x] at origin (x, y, z)."""
    out = vox.reshape(n, n, n).copy()
    ez, ey, ex = block.shape
    out[origin[2]:origin[2] + ez, origin[1]:origin[1] + ey, origin[0]:origin[0] + ex] = block
    return out.reshape(-1)
