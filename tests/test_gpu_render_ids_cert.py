"""The certified ID kernel (GPU): vrt_set_ids_certified(1) on an octant layout launches ids_cert_kernel, whose
certified walks settle most pixels and whose lanes walk the rest exactly. Everything it writes is held to the
exact ID kernel's bytes (mode 0 on the same renderer), to vrt_pick_pixels of every pixel, to the oracle's hit
records and to the NumPy restatement of the depth; vrt_ids_deferred's count of exact-path pixels is held to the
caps that tests/test_render_ids_cert_cpu.py proves on the CPU model. Volumes are 16^3 unless a camera brings
its own size, frames 96x54 or smaller; picks, oracle frames and primary rays are computed once and shared."""
import ctypes as C
import functools

import numpy as np
import pytest

import harness
import ids_cert_model as model
import oracle
import reproject_reference as ref
import voxelraytracer_amd as vrt
from adversarial_volumes import volumes as adversarial_volumes
from harness import all_pixels, assert_ids_equal_pick, depth_restated, edge_cameras
from ids_cert_model import CAP_DEFAULT, CAP_HARD, H, SCENES, W, params, scene
from voxelraytracer_amd import abi

pytestmark = pytest.mark.gpu

N = 16
ID_SENTINEL, DEPTH_SENTINEL = 0x5A5A5A5A, -7.25


def pick_frame(r, cam, p):
    return r.pick(cam, p, all_pixels(cam.width, cam.height)).reshape(cam.height, cam.width)


def certified(layout=8):
    """A renderer in mode 1 (set before the upload: the mode survives it)."""
    r = vrt.Renderer(0)
    r.set_skip_layout(layout)
    r.set_ids_certified(1)
    return r


def same_depth(a, b):
    return np.array_equal(a.view(np.uint32), b.view(np.uint32))


@functools.lru_cache(maxsize=None)
def oracle_hits(name, n, ray_noise):
    _, hits, _ = oracle.render(vrt.make_camera(W, H), scene(name, n), n, params(ray_noise), threads=4)
    return hits


@functools.lru_cache(maxsize=None)
def primary_rays(n, ray_noise, max_len=None):
    kw = {} if max_len is None else dict(max_ray_length=max_len)
    return harness.primary_rays(vrt.make_camera(W, H), scene("terrain", n), n, params(ray_noise, **kw))


# ---- 1. parity -----------------------------------------------------------------------------------

PARITY = [(s, N, noise) for s in SCENES for noise in (0.0, 0.05)] + [("terrain", 32, 0.0)]


def test_default_mode_is_the_exact_kernel(built):
    cam, p = vrt.make_camera(W, H), params()
    with vrt.Renderer(0) as r:
        assert r.ids_certified() == 0
        r.upload_volume(scene("terrain", N), N)
        assert r.ids_certified() == 0
        r.render_ids(cam, p)
        assert r.ids_deferred() == (W * H, W * H)


@pytest.mark.parametrize("name,n,ray_noise", PARITY)
def test_certified_ids_and_depth_are_the_exact_kernels(built, name, n, ray_noise):
    """Mode 1's bytes equal mode 0's on the same renderer, the pick's records, the oracle's voxel_index and the
    restated depth; ids_deferred counts at most 1 % of the frame (the model: 0 to 3 pixels). With the exact kernel
    behind mode 1 by mistake the count would be every pixel."""
    cam, p = vrt.make_camera(W, H), params(ray_noise)
    with certified() as r:
        r.upload_volume(scene(name, n), n)
        assert r.ids_certified() == 1
        ids, depth = r.render_ids(cam, p)
        pixels, deferred = r.ids_deferred()
        ids_only, none = r.render_ids(cam, p, want_depth=False)
        assert r.ids_deferred() == (pixels, deferred)
        picks = pick_frame(r, cam, p)
        r.set_ids_certified(0)
        assert r.ids_certified() == 0
        ids0, depth0 = r.render_ids(cam, p)
        assert r.ids_deferred() == (W * H, W * H)
    modelled = model.model_frame(name, n, ray_noise)[0] if n == N else None
    print(f"{name} {n}^3 noise {ray_noise}: {deferred} of {pixels} pixels on the exact path (model: {modelled})")
    assert none is None and ids.shape == depth.shape == (H, W) and depth.dtype == np.float32
    assert ids.tobytes() == ids0.tobytes()
    assert same_depth(depth, depth0)
    assert ids.tobytes() == ids_only.tobytes()
    assert_ids_equal_pick(ids, picks, (name, n, ray_noise))
    assert np.array_equal(ids["voxel_index"], oracle_hits(name, n, ray_noise)["voxel_index"])
    found = picks["voxel_index"] >= 0
    assert np.count_nonzero(found) > 0
    assert np.all(np.isposinf(depth[~found]))
    pos, dirs = primary_rays(n, ray_noise)
    want = depth_restated(picks, pos, dirs)
    bad = np.argwhere(depth.view(np.uint32) != want.view(np.uint32))
    assert bad.size == 0, (len(bad), bad[:5].tolist())
    assert pixels == W * H
    assert 0 <= deferred <= CAP_DEFAULT


@pytest.mark.parametrize("name", SCENES)
def test_single_layout_keeps_the_exact_kernel(built, name):
    cam, p = vrt.make_camera(W, H), params(0.05)
    with certified(layout=1) as r:
        r.upload_volume(scene(name, N), N)
        assert r.ids_certified() == 0
        ids, depth = r.render_ids(cam, p)
        assert r.ids_deferred() == (W * H, W * H)
        r.set_ids_certified(0)
        ids0, depth0 = r.render_ids(cam, p)
    assert ids.tobytes() == ids0.tobytes() and same_depth(depth, depth0)


# ---- 2. frame shapes -----------------------------------------------------------------------------

@pytest.mark.parametrize("w,h", [(37, 19), (16, 8)])
def test_frame_shapes(built, w, h):
    cam, p = vrt.make_camera(w, h), params()
    for name in SCENES:
        with certified() as r:
            r.upload_volume(scene(name, N), N)
            ids, depth = r.render_ids(cam, p)
            pixels, deferred = r.ids_deferred()
            picks = pick_frame(r, cam, p)
        assert pixels == w * h and deferred < pixels
        assert_ids_equal_pick(ids, picks, (name, w, h))
        assert np.array_equal(np.isposinf(depth), picks["voxel_index"] < 0)


# ---- 3. length-limited walks ---------------------------------------------------------------------

@pytest.mark.parametrize("max_len", [6.0, 0.75])
def test_length_limited_walks(built, max_len):
    """Rays that end at the length test, before a crossing and at one: the walk's length stop and its tie."""
    cam, p = vrt.make_camera(W, H), params(max_ray_length=max_len)
    pos, dirs = primary_rays(N, 0.0, max_len)
    for name in SCENES:
        with certified() as r:
            r.upload_volume(scene(name, N), N)
            ids, depth = r.render_ids(cam, p)
            picks = pick_frame(r, cam, p)
        assert_ids_equal_pick(ids, picks, (name, max_len))
        assert same_depth(depth, depth_restated(picks, pos, dirs)), (name, max_len)


# ---- 4. adversarial volumes ----------------------------------------------------------------------

@pytest.mark.parametrize("vname", ["lattice", "glass_clutter"])
def test_adversarial_volumes(built, vname):
    w, h = 64, 48
    vox = adversarial_volumes(N)[vname]
    cam, p = vrt.make_camera(w, h), params()
    with certified() as r:
        r.upload_volume(vox, N)
        assert r.ids_certified() == 1
        ids, depth = r.render_ids(cam, p)
        picks = pick_frame(r, cam, p)
    pos, dirs = harness.primary_rays(cam, vox, N, p)
    assert_ids_equal_pick(ids, picks, vname)
    assert same_depth(depth, depth_restated(picks, pos, dirs)), vname


# ---- 5. pitched band -----------------------------------------------------------------------------

def test_async_band_with_pitch_on_a_torch_stream(built):
    import torch

    cam, p = vrt.make_camera(W, H), params(0.05)
    row0, rows, pitch = 5, 9, W + 7
    with certified() as r:
        r.upload_volume(scene("refraction", N), N)
        ids, depth = r.render_ids(cam, p)
        s = torch.cuda.Stream()
        with torch.cuda.stream(s):
            # one sentinel row before the band and one after it
            d_ids = torch.full(((rows + 2) * pitch * 2,), ID_SENTINEL, dtype=torch.int32, device="cuda")
            d_depth = torch.full(((rows + 2) * pitch,), DEPTH_SENTINEL, dtype=torch.float32, device="cuda")
            r.render_ids_async(cam, p, row0, rows, pitch, d_ids.data_ptr() + pitch * 8, d_depth.data_ptr() + pitch * 4,
                               s.cuda_stream)
            # rows == 0: success, nothing written
            z_ids = torch.full((pitch * 2,), ID_SENTINEL, dtype=torch.int32, device="cuda")
            z_depth = torch.full((pitch,), DEPTH_SENTINEL, dtype=torch.float32, device="cuda")
            r.render_ids_async(cam, p, row0, 0, pitch, z_ids.data_ptr(), z_depth.data_ptr(), s.cuda_stream)
        s.synchronize()
    band_ids = d_ids.cpu().numpy().reshape(rows + 2, pitch, 2)
    band_depth = d_depth.cpu().numpy().reshape(rows + 2, pitch)
    got = np.ascontiguousarray(band_ids[1:rows + 1, :W]).view(abi.PIXEL_ID_DTYPE).reshape(rows, W)
    assert got.tobytes() == np.ascontiguousarray(ids[row0:row0 + rows]).tobytes()
    assert same_depth(np.ascontiguousarray(band_depth[1:rows + 1, :W]), np.ascontiguousarray(depth[row0:row0 + rows]))
    for untouched in (band_ids[0], band_ids[rows + 1], band_ids[:, W:]):
        assert np.all(untouched == ID_SENTINEL)
    for untouched in (band_depth[0], band_depth[rows + 1], band_depth[:, W:]):
        assert np.all(untouched == np.float32(DEPTH_SENTINEL))
    assert np.all(z_ids.cpu().numpy() == ID_SENTINEL) and np.all(z_depth.cpu().numpy() == np.float32(DEPTH_SENTINEL))


# ---- 6. captured graph ---------------------------------------------------------------------------

def test_async_pass_is_capturable(built):
    """One call is one launch of one kernel with no counter, memset or list: captured into a graph, every replay
    over sentinel-filled buffers writes the synchronous result."""
    import torch

    cam, p = vrt.make_camera(W, H), params()
    with certified() as r:
        r.upload_volume(scene("refraction", N), N)
        assert r.ids_certified() == 1
        ids, depth = r.render_ids(cam, p)
        d_ids = torch.zeros((H * W * 2,), dtype=torch.int32, device="cuda")
        d_depth = torch.zeros((H * W,), dtype=torch.float32, device="cuda")
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):   # warm the stream outside the capture
            r.render_ids_async(cam, p, 0, H, W, d_ids.data_ptr(), d_depth.data_ptr(), s.cuda_stream)
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            r.render_ids_async(cam, p, 0, H, W, d_ids.data_ptr(), d_depth.data_ptr(),
                               torch.cuda.current_stream().cuda_stream)
        for _ in range(3):
            d_ids.fill_(ID_SENTINEL)
            d_depth.fill_(DEPTH_SENTINEL)
            g.replay()
            torch.cuda.synchronize()
            assert d_ids.cpu().numpy().tobytes() == ids.tobytes()
            assert same_depth(d_depth.cpu().numpy(), depth.reshape(-1))


# ---- 7. edge cameras -----------------------------------------------------------------------------

@pytest.mark.parametrize("name", SCENES)
def test_edge_cameras(built, name):
    """The 118 cameras within a cell of the volume's faces and corners: IDs equal the pick at every pixel; over a
    scene's cameras the exact path takes under 2 % of the pixels (the model without start checks: 0.35 to 0.83 %),
    and no frame leaves every pixel to it."""
    w, h = 40, 24
    p = params()
    cams = edge_cameras(N, w, h)
    assert len(cams) == 118
    px = all_pixels(w, h)
    total = 0
    with certified() as r:
        r.upload_volume(scene(name, N), N)
        for pos, rot, cam in cams:
            ids, _ = r.render_ids(cam, p)
            pixels, deferred = r.ids_deferred()
            picks = r.pick(cam, p, px).reshape(h, w)
            assert_ids_equal_pick(ids, picks, (name, pos, rot))
            assert pixels == w * h and deferred < pixels, (name, pos, rot, deferred)
            total += deferred
    print(f"{name}: {total} of {len(cams) * w * h} pixels on the exact path over the edge cameras")
    assert total < 0.02 * len(cams) * w * h


# ---- 8. lattice and open cameras -----------------------------------------------------------------

# tests/test_gpu_render_ids.py's HARD_CAMERAS: the four lattice cameras and the two cameras of the certified
# trees' open cases, at their own volume sizes
HARD_CAMERAS = [
    (64, (1.0, 20.0, -22.0), (-90.0, 315.0, 0.0)),
    (128, (0.0, 50.0, -44.0), (-90.0, 315.0, 0.0)),
    (64, (0.0, 10.0, -8.5), (-90.0, 225.0, 0.0)),
    (64, (1.0, 2.0, -3.0), (0.0, 0.0, 0.0)),
    (128, (-29.0, -44.5, 21.5), (-89.99, 225.0, 0.0)),
    (64, (-21.0, 1.0, 16.0), (90.0, 0.0, 0.0)),
]


@pytest.mark.parametrize("n,pos,rot", HARD_CAMERAS)
def test_lattice_and_open_cameras(built, n, pos, rot):
    """At most 10 % of a frame on the exact path (the model's worst: 298 of 5184, 5.7 %)."""
    cam, p = vrt.make_camera(W, H, pos=pos, rot=rot), params()
    for name in SCENES:
        with certified() as r:
            r.upload_volume(scene(name, n), n)
            ids, depth = r.render_ids(cam, p)
            pixels, deferred = r.ids_deferred()
            picks = pick_frame(r, cam, p)
        print(f"{name} {n}^3 {pos} {rot}: {deferred} of {pixels} pixels on the exact path")
        assert_ids_equal_pick(ids, picks, (name, n, pos, rot))
        assert np.array_equal(np.isposinf(depth), picks["voxel_index"] < 0)
        assert pixels == W * H and deferred <= CAP_HARD, (name, deferred)


# ---- 9. edit loop --------------------------------------------------------------------------------

def test_edits_are_seen(built):
    vox = scene("terrain", N).copy()
    cam, p = vrt.make_camera(W, H), params()
    with certified() as r:
        r.upload_volume(vox, N)
        before, _ = r.render_ids(cam, p)
        centre = before[H // 2, W // 2]
        assert centre["voxel_index"] >= 0
        i, j, k = (int(c[0]) for c in vrt.hit_cell(before[H // 2:H // 2 + 1, W // 2:W // 2 + 1], N))
        r.update_volume((i, j, k), np.zeros((1, 1, 1), np.uint8))
        vox[centre["voxel_index"]] = 0
        assert r.ids_certified() == 1
        after, after_depth = r.render_ids(cam, p)
        assert r.ids_deferred()[1] < W * H
        r.set_ids_certified(0)
        exact, exact_depth = r.render_ids(cam, p)
    with certified() as fresh:
        fresh.upload_volume(vox, N)
        want, want_depth = fresh.render_ids(cam, p)
    assert after.tobytes() == want.tobytes() == exact.tobytes()
    assert same_depth(after_depth, want_depth) and same_depth(after_depth, exact_depth)
    assert after[H // 2, W // 2]["voxel_index"] != centre["voxel_index"]


# ---- 10. reprojected loop ------------------------------------------------------------------------

@pytest.mark.parametrize("spatial", [False, True])
def test_reprojected_loop_is_the_same_bytes(built, spatial):
    """vrt_render_frame_reprojected goes through the same ID pass: along cameras A, B, A, C every frame of a
    mode 1 renderer equals the mode 0 renderer's."""
    with vrt.Renderer(0) as a, certified() as b:
        for q in (a, b):
            q.upload_volume(ref.scene("refraction"), N)
            if spatial:
                q.set_reprojected_spatial(vrt.SPATIAL_FILL, 3, vrt.GUIDE_FACE, 765)
                q.set_reprojected_fetch(vrt.FETCH_BILINEAR)
        assert (a.ids_certified(), b.ids_certified()) == (0, 1)
        for f, cn in enumerate("ABAC"):
            cam, p = ref.camera(cn), ref.params(0.05, float(f + 1))
            fa, fb = a.render_frame_reprojected(cam, p, 0.2), b.render_frame_reprojected(cam, p, 0.2)
            assert fa.tobytes() == fb.tobytes(), (f, cn, spatial)


# ---- 11. launch timing ---------------------------------------------------------------------------

def test_launch_timing_counts_one_launch_per_call(built):
    import torch

    cam, p = vrt.make_camera(W, H), params()
    with certified() as r:
        r.upload_volume(scene("refraction", N), N)
        d_ids = torch.zeros((H * W * 2,), dtype=torch.int32, device="cuda")
        d_depth = torch.zeros((H * W,), dtype=torch.float32, device="cuda")
        r.set_launch_timing(2)
        r.render_ids_async(cam, p, 0, H, W, d_ids.data_ptr(), d_depth.data_ptr())
        r.render_ids_async(cam, p, 0, H, W, d_ids.data_ptr(), 0)
        total, launches = r.launch_timing()
        r.set_launch_timing(0)
    assert launches == 2 and total > 0.0


# ---- 12. errors ----------------------------------------------------------------------------------

def test_errors(built):
    import torch

    cam, p = vrt.make_camera(W, H), params()
    d_ids = torch.full((H * W * 2 + 2,), ID_SENTINEL, dtype=torch.int32, device="cuda")
    d_depth = torch.full((H * W + 2,), DEPTH_SENTINEL, dtype=torch.float32, device="cuda")
    pi, pd = d_ids.data_ptr(), d_depth.data_ptr()
    inv = abi.VRT_ERR_INVALID
    with vrt.Renderer(0) as r:
        L, ctx = r._lib, r._h
        cr, pr = C.byref(cam), C.byref(p)

        def a(cam_=cr, p_=pr, row0=0, rows=H, pitch=W, ids=pi, depth=pd):
            return L.vrt_render_ids_async(ctx, cam_, p_, row0, rows, pitch, ids, depth, None)

        assert L.vrt_set_ids_certified(None, 1) == inv
        r.set_ids_certified(1)
        assert r.ids_certified() == 0   # no volume resident
        assert a() == abi.VRT_ERR_NO_VOLUME
        r.upload_volume(scene("terrain", N), N)
        assert r.ids_certified() == 1   # the mode survived the upload
        for mode in (-1, 2, 7):
            assert L.vrt_set_ids_certified(ctx, mode) == inv, mode
            assert r.ids_certified() == 1
        assert a(cam_=None) == inv and a(p_=None) == inv and a(ids=None) == inv
        assert a(rows=-1) == inv and a(row0=-1, rows=1) == inv
        assert a(row0=H - 3, rows=4) == inv and a(row0=H, rows=1) == inv
        assert a(pitch=W - 1) == inv and a(pitch=0) == inv
        assert a(ids=pi + 4) == inv and a(depth=pd + 2) == inv and a(depth=pd + 1) == inv
        assert L.vrt_render_ids_async(None, cr, pr, 0, H, W, pi, pd, None) == inv
        torch.cuda.synchronize()
        assert np.all(d_ids.cpu().numpy() == ID_SENTINEL)
        assert np.all(d_depth.cpu().numpy() == np.float32(DEPTH_SENTINEL))
        assert a(rows=0) == abi.VRT_OK
        torch.cuda.synchronize()
        assert np.all(d_ids.cpu().numpy() == ID_SENTINEL)
        r.set_ids_certified(0)
        assert r.ids_certified() == 0
        for mode in (-1, 2, 7):
            assert L.vrt_set_ids_certified(ctx, mode) == inv, mode
            assert r.ids_certified() == 0
        r.set_ids_certified(1)
        r.upload_volume(scene("refraction", N), N)
        assert r.ids_certified() == 1
