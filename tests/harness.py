"""The tests' shared harness: the launches, render modes, fixtures, CPU model and comparisons that more than
one test file needs, each defined once. Importable without a GPU (the CPU tests use the comparisons, the
fixtures and the CPU model); the helpers that allocate device buffers import torch inside their bodies.
Helper modules are not assertion-rewritten by pytest, so every assert here carries the values it compares.
The ray queries' oracles are in tests/ray_oracle.py. Plain helpers, no tests."""
import ctypes as C
import functools
import glob
import json
import os
import subprocess

import numpy as np

import oracle
import voxelraytracer_amd as vrt
from adversarial_volumes import scene_volume
from voxelraytracer_amd import abi

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
COLOR_TOL = 1e-4   # the float-colour contract against the oracle (tests/test_gpu_parity.py)


# ---- launches ------------------------------------------------------------------------------------

def current_stream():
    import torch

    return torch.cuda.current_stream().cuda_stream


def band(r, cam, p, row0=0, rows=None, step=1, block=1, counters=False):
    """One band at alpha 1 as [rows, W] RGBA8 words (rows None: the whole frame); counters: by the exact
    STATS instance."""
    import torch

    rows = cam.height if rows is None else rows
    out = torch.zeros((rows, cam.width), dtype=torch.int32, device="cuda")
    cnt = torch.zeros(len(vrt.COUNTER_NAMES), dtype=torch.int64, device="cuda")
    r.render_temporal_rows_async(cam, p, 1.0, row0, rows, step, out.data_ptr(), out.data_ptr(),
                                 d_counters=cnt.data_ptr() if counters else 0,
                                 stream=current_stream(), row_block=block)
    torch.cuda.synchronize()
    return out.cpu().numpy()


def batch(r, cams, ps, row0=0, rows=None, step=1, block=1, fill=0):
    """The same band of len(cams) frames in one frame-batch launch, as a list of [rows, W] RGBA8 words.
    fill: what the buffers hold before the launch."""
    import torch

    rows = cams[0].height if rows is None else rows
    out = [torch.full((rows, cams[0].width), fill, dtype=torch.int32, device="cuda") for _ in cams]
    r.render_temporal_batch_async(cams, ps, row0, rows, step, [b.data_ptr() for b in out],
                                  stream=current_stream(), row_block=block)
    torch.cuda.synchronize()
    return [b.cpu().numpy() for b in out]


def frames(r, cam, n_frames, R, T, alpha, row0, rows, step, exact_pass=None, block=1, counters=False,
           atlas=None, **kw):
    """A temporal sequence: n_frames frames at times 1, 2, ... filtered in place into one history buffer
    that starts black; the [rows, W, 4] bytes after each frame. exact_pass: set on r first, when given;
    atlas: textured frames; kw: default_params keywords."""
    import torch

    if exact_pass is not None:
        r.set_exact_pass(exact_pass)
    hist = torch.zeros((rows, cam.width, 4), dtype=torch.uint8, device="cuda")
    cnt = torch.zeros(len(vrt.COUNTER_NAMES), dtype=torch.int64, device="cuda")
    out = []
    for t in range(n_frames):
        p = vrt.default_params(R, T, time=float(t + 1), **kw)
        if atlas is not None:
            p = vrt.textured_params(p, atlas)
        r.render_temporal_rows_async(cam, p, alpha, row0, rows, step, hist.data_ptr(), hist.data_ptr(),
                                     d_counters=cnt.data_ptr() if counters else 0,
                                     stream=current_stream(), row_block=block)
        torch.cuda.synchronize()
        out.append(hist.cpu().numpy().copy())
    return out


class View:
    """A raw device pointer as bytes of dst's shape, through __cuda_array_interface__."""

    def __init__(self, dst, ptr):
        self.__cuda_array_interface__ = {"shape": dst.shape, "typestr": "|u1", "data": (ptr, False), "version": 3}


def hipcopy(dst: np.ndarray, ptr: int, stream_handle=None):
    """Device -> host copy of a raw device pointer: after a device-wide wait, or, with stream_handle,
    enqueued on that raw HIP stream (the frame's own stream) and followed by a wait for it."""
    import torch

    if stream_handle is None:
        torch.cuda.synchronize()
        dst[...] = torch.as_tensor(View(dst, ptr), device="cuda").cpu().numpy()
        return
    ext = torch.cuda.ExternalStream(stream_handle)
    with torch.cuda.stream(ext):
        t = torch.as_tensor(View(dst, ptr), device="cuda").to("cpu", non_blocking=False)
    ext.synchronize()
    dst[...] = t.numpy()


# ---- render modes (fields of the context: a fresh Renderer has the default state) -----------------

def reset_modes(r):
    """The default state: certified automatic, certified trees automatic, exact pass automatic."""
    r.set_certified(0)
    r.set_cert_trees(1)
    r.set_exact_pass(1)


def certified_mode(r, trees, exact_pass=2):
    """The certified pass; exact_pass 2: deferred at any size, 0: in lane."""
    r.set_certified(1)
    r.set_cert_trees(trees)
    r.set_exact_pass(exact_pass)


def certified_modes(r):
    """The certified pass with the deferred exact pass at any size: plain and with bounce trees."""
    for trees in (0, 2):
        certified_mode(r, trees)
        yield trees


def all_modes(r):
    """set_certified x set_cert_trees x set_exact_pass, set on r one after another."""
    for cert in (-1, 0, 1):
        for trees in (0, 2):
            for exact in (0, 2):
                r.set_certified(cert)
                r.set_cert_trees(trees)
                r.set_exact_pass(exact)
                yield cert, trees, exact


# ---- fixtures ------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def ref_atlas_fixture():
    """tests/golden/atlas/atlas_ref128.npz (tests/golden/make_atlas_ref.py): the reference's own textures
    (res/textures/*128.png, main.cpp:187-193) decoded into the ABI atlas layout -> (atlas, read-only; meta)."""
    z = np.load(os.path.join(HERE, "golden", "atlas", "atlas_ref128.npz"), allow_pickle=False)
    a = z["atlas"]
    a.setflags(write=False)
    return a, json.loads(str(z["meta"]))


def ref_atlas():
    return ref_atlas_fixture()[0]


@functools.lru_cache(maxsize=None)
def synthetic_atlas(size=256, tile=128):
    a = vrt.make_atlas(size, tile)
    a.setflags(write=False)
    return a


GOLDEN = sorted(glob.glob(os.path.join(HERE, "golden", "*.npz")))


def load_golden(path):
    """(npz, meta, camera, params, volume bytes) of a fixture of tests/golden (make_golden.py)."""
    z = np.load(path, allow_pickle=False)
    meta = json.loads(str(z["meta"]))
    cam = abi.Camera()
    cam.inv_pv = (abi.C.c_float * 16)(*z["inv_pv"].tolist())
    cam.width, cam.height = meta["width"], meta["height"]
    p = vrt.default_params(meta["params"]["max_reflections"], meta["params"]["max_transparencies"])
    for k, v in meta["params"].items():
        if k == "sun_dir":
            p.sun_dir = (abi.C.c_float * 3)(*v)
        else:
            setattr(p, k, v)
    if "atlas" in z.files and z["atlas"].size:
        p = vrt.textured_params(p, z["atlas"], meta["params"]["atlas_texture_size"])
    vox = scene_volume(meta["scene"], meta["n"], meta["seed"])
    return z, meta, cam, p, vox


def params_dict(p):
    """A Params block as numpy_oracle's dict."""
    d = dict(sun_dir=list(p.sun_dir), time=p.time, ray_noise=p.ray_noise,
             reflection_noise=p.reflection_noise, refraction_noise=p.refraction_noise,
             max_ray_length=p.max_ray_length, max_reflections=p.max_reflections,
             max_transparencies=p.max_transparencies, color_only=p.color_only)
    if not p.color_only:
        d.update(atlas=p._atlas_ref, atlas_size=p.atlas_size,
                 atlas_texture_size=p.atlas_texture_size)
    return d


# ---- cameras -------------------------------------------------------------------------------------

# lattice cameras (pos, rot): rays through voxel edges and corners, where the exact walk ties
LATTICE = [((0.0, 0.0, 0.0), (-35.26439, 45.0, 0.0)), ((0.5, 0.5, 0.5), (-35.26439, 45.0, 0.0)),
           ((0.0, 0.0, 0.0), (0.0, 45.0, 0.0)), ((1.0, -2.0, 3.0), (-45.0, 0.0, 0.0)),
           ((0.25, 0.75, -0.5), (-30.0, 135.0, 0.0))]


def view_direction(cam):
    """The centre ray's direction (ndc (0, 0)), from the camera's inverse matrix."""
    m = np.array(cam.inv_pv[:], np.float64)
    near = np.array([-m[8 + i] + m[12 + i] for i in range(4)])
    far = np.array([m[8 + i] + m[12 + i] for i in range(4)])
    d = far[:3] / far[3] - near[:3] / near[3]
    return d / np.linalg.norm(d)


def edge_cameras(n, w, h):
    """Within one cell of each face and each corner of the volume (world coordinates: the volume is
    [-n/2, n/2]^3), on half-integer and integer lattice positions, looking outwards (the view
    direction within 60 degrees of the outward normal, or of the corner's diagonal) and along the
    faces (at right angles to the normal): of the six axis views, a face diagonal and a space
    diagonal, those that do. -> [(pos, rot, camera)]"""
    e = n / 2.0
    pos = []
    for axis in range(3):
        for sgn in (-1.0, 1.0):
            for inset in (0.5, 1.0):
                q = [0.5 if inset == 0.5 else 1.0] * 3
                q[axis] = sgn * (e - inset)
                o = [0.0, 0.0, 0.0]
                o[axis] = sgn
                pos.append((tuple(q), np.array(o), True))
    for sx in (-1.0, 1.0):
        for sy in (-1.0, 1.0):
            for sz in (-1.0, 1.0):
                pos.append(((sx * (e - 0.5), sy * (e - 0.5), sz * (e - 0.5)),
                            np.array([sx, sy, sz]) / np.sqrt(3.0), False))
    rots = [(0.0, 0.0, 0.0), (0.0, 90.0, 0.0), (0.0, 180.0, 0.0), (0.0, 270.0, 0.0), (-89.99, 0.0, 0.0),
            (89.99, 0.0, 0.0), (0.0, 45.0, 0.0), (0.0, 225.0, 0.0), (-35.26439, 225.0, 0.0), (35.26439, 45.0, 0.0)]
    cams = []
    for p, o, face in pos:
        for rt in rots:
            cam = vrt.make_camera(w, h, pos=p, rot=rt)
            c = float(view_direction(cam) @ o)
            if c > 0.5 or (face and abs(c) < 0.02):
                cams.append((p, rt, cam))
    return cams


def all_pixels(w, h):
    """[w * h, 2] int32 (x, y), row by row: a pixel list of the whole frame."""
    y, x = np.meshgrid(np.arange(h), np.arange(w), indexing="ij")
    return np.stack([x.reshape(-1), y.reshape(-1)], axis=1).astype(np.int32)


def first_records(cam, vox, n, p):
    """[H, W, :] float: every pixel's first record of oracle.trace_pixel, its primary ray (kind 1, no
    parent, depth 1) as it entered RayMarch: position in floats 9-11, direction in floats 12-14."""
    h, w = cam.height, cam.width
    out = None
    for py in range(h):
        for px in range(w):
            recs, _ = oracle.trace_pixel(cam, vox, n, p, px, py, cap=4)
            r = recs[0]
            assert r[0] == 1 and r[15] == 0 and r[16] == 1, ((px, py), float(r[0]), float(r[15]), float(r[16]))
            if out is None:
                out = np.zeros((h, w, len(r)), recs.dtype)
            out[py, px] = r
    return out


def primary_rays(cam, vox, n, p):
    """(pos, dir) [H, W, 3] float32 of every pixel's primary ray. The ray depends on the volume through
    its size alone (pos = near-plane point + n / 2)."""
    recs = first_records(cam, vox, n, p)
    return recs[..., 9:12].astype(np.float32), recs[..., 12:15].astype(np.float32)


# ---- the CPU model of the certified walks --------------------------------------------------------

@functools.lru_cache(maxsize=None)
def load_certsim():
    """scripts/certsim.c, built once per process into build/certsim.so, with its ctypes signatures."""
    so = os.path.join(ROOT, "build", "certsim.so")
    os.makedirs(os.path.dirname(so), exist_ok=True)
    subprocess.check_call(["gcc", "-O2", "-ffp-contract=off", "-fno-fast-math", "-fopenmp", "-shared",
                           "-fPIC", "-o", so, os.path.join(ROOT, "scripts", "certsim.c"), "-lm"])
    L = C.CDLL(so)
    L.cs_build.argtypes = [C.c_void_p, C.c_int, C.c_int]
    L.cs_run.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_float, C.c_double, C.c_float,
                         C.c_void_p]
    L.cs_exits.argtypes = [C.c_void_p]
    L.cs_exits.restype = C.c_int
    return L


# ---- the launch constants' host hook -------------------------------------------------------------

K_W, K_LEN, K_CELL = 1, 2, 4   # KArgs::setup's flags
ALL = K_W | K_LEN | K_CELL


def launch_consts_hook():
    fn = vrt.lib().vrt_debug_cert_launch_consts
    fn.restype = C.c_int
    fn.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_float, C.c_void_p]
    return fn


def consts(m, n, w, h, max_len=100.0, m2=None):
    """The hook's words as a dict; m, m2: 16 float32 (inv_pv, column-major)."""
    m = np.ascontiguousarray(m, np.float32)
    m2 = None if m2 is None else np.ascontiguousarray(m2, np.float32)
    out = np.zeros(20, np.uint32)
    rc = launch_consts_hook()(m.ctypes.data, None if m2 is None else m2.ctypes.data, n, w, h, max_len,
                              out.ctypes.data)
    assert rc == 0, ("vrt_debug_cert_launch_consts", rc)
    f = out.view(np.float32)
    return dict(setup=int(out[0]), wn=f[1], wf=f[2], rcp_wn=f[3], rcp_wf=f[4], fl1_up=f[5:8].copy(),
                fl1_dn=f[8:11].copy(), cell=out[11:14].view(np.int32).copy(), fw=f[14], fh=f[15], half_n=f[16],
                walk_b0=f[17], max_len2=f[18], vdiv_ok=int(out[19]))


# ---- comparisons ---------------------------------------------------------------------------------

def assert_equal(got, ref, what):
    """Element for element (RGBA8 words, as a rule); the message: what, how many differ, the first five
    positions."""
    got, ref = np.asarray(got), np.asarray(ref)
    assert got.shape == ref.shape, (what, "shapes", got.shape, ref.shape)
    bad = np.argwhere(got != ref)
    assert bad.size == 0, (what, len(bad), bad[:5].tolist())


def words_to_bytes(a):
    """[H, W] RGBA8 words -> [H, W, 4] bytes (a view when a is contiguous)."""
    return np.ascontiguousarray(a).view(np.uint8).reshape(a.shape[0], a.shape[1], 4)


def float_bits(a):
    """The float32 bit patterns of an array (made contiguous) or a scalar (-> shape (1,)): +0 and -0, and
    two NaN payloads, differ."""
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def same_bytes(a, b):
    """Whether two arrays of any dtypes and shapes hold the same bytes."""
    return np.array_equal(np.ascontiguousarray(a).view(np.uint8).reshape(-1),
                          np.ascontiguousarray(b).view(np.uint8).reshape(-1))


def compare(rgba_g, hits_g, cnt_g, rgba_o, hits_o, cnt_o):
    """tests/test_gpu_parity.py's contract: hit records and counters equal, clamped colour within COLOR_TOL,
    alpha 1."""
    assert_equal(hits_g["voxel_index"], hits_o["voxel_index"], "voxel_index")
    assert_equal(hits_g["ray_length"].view(np.uint32), hits_o["ray_length"].view(np.uint32), "ray_length bits")
    assert_equal(hits_g["steps"], hits_o["steps"], "steps")
    assert_equal(hits_g["flags"], hits_o["flags"], "flags")
    for k in oracle.COUNTER_NAMES:
        assert cnt_g[k] == cnt_o[k], (k, cnt_g[k], cnt_o[k])
    d = np.abs(np.clip(rgba_g[..., :3], 0, 1) - np.clip(rgba_o[..., :3], 0, 1))
    assert d.max() <= COLOR_TOL, ("max |clamped colour difference|", float(d.max()), COLOR_TOL)
    assert_equal(rgba_g[..., 3], np.ones_like(rgba_g[..., 3]), "alpha")


def check_raw(raw_g, rgba_o):
    """tests/test_gpu_temporal.py's contract: device RGB8 bytes against the oracle's float colour quantised
    by the oracle; one LSB only where that colour is within COLOR_TOL of a rounding boundary of x * 255.
    -> how many bytes differ."""
    raw_o, _ = oracle.temporal(rgba_o, np.zeros(rgba_o.shape, np.uint8), 1.0)
    diff = raw_g[..., :3].astype(np.int16) - raw_o[..., :3].astype(np.int16)
    bad = diff != 0
    worst = int(np.abs(diff).max(initial=0))
    assert worst <= 1, ("bytes from the oracle's", worst, np.argwhere(np.abs(diff) > 1)[:5].tolist())
    if bad.any():   # only where the oracle colour is within COLOR_TOL of a .5 boundary
        x = np.clip(rgba_o[..., :3][bad], 0, 1).astype(np.float64) * 255.0
        off = np.abs(x - np.floor(x) - 0.5)
        assert np.all(off <= COLOR_TOL * 255.0), ("one LSB off away from a rounding boundary", float(off.max()),
                                                  COLOR_TOL * 255.0, np.argwhere(bad)[:5].tolist())
    assert np.all(raw_g[..., 3] == 255), ("alpha != 255", np.argwhere(raw_g[..., 3] != 255)[:5].tolist())
    return int(bad.sum())


def assert_ids_equal_pick(ids, picks, what=""):
    bad = np.argwhere((ids["voxel_index"] != picks["voxel_index"]) | (ids["face"] != picks["face"]))
    assert bad.size == 0, (what, len(bad), bad[:5].tolist())


def depth_restated(picks, pos, dirs):
    """(np.rint(point[a]) - pos[a]) / dir[a] in float32, a the face's axis; +inf for a miss."""
    a = (picks["face"] & 3).astype(np.intp)[..., None]
    pt = np.take_along_axis(picks["point"], a, -1)[..., 0]
    pa, da = np.take_along_axis(pos, a, -1)[..., 0], np.take_along_axis(dirs, a, -1)[..., 0]
    with np.errstate(all="ignore"):
        d = ((np.rint(pt) - pa) / da).astype(np.float32)
    assert (np.rint(pt) - pa).dtype == np.float32 and da.dtype == np.float32, ((np.rint(pt) - pa).dtype, da.dtype)
    return np.where(picks["voxel_index"] >= 0, d, np.float32(np.inf)).astype(np.float32)


def assert_same_packed(got, want):
    """The packed skip field, texel for texel."""
    assert got.shape == want.shape, (got.shape, want.shape)
    if not np.array_equal(got, want):
        bad = np.argwhere(got != want)
        raise AssertionError(f"{len(bad)} packed texels differ, first [octant, z, y, x] = {bad[:4].tolist()}: "
                             f"{[hex(int(got[tuple(b)])) for b in bad[:4]]} != "
                             f"{[hex(int(want[tuple(b)])) for b in bad[:4]]}")
