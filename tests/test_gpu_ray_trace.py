"""Shaded ray queries (GPU): vrt_trace_rays / vrt_trace_rays_async / vrt_trace_pixels run fragment main
(exact_pixel with exact walks only) for a list of rays or pixels.

Arbitrary rays are held against numpy_oracle.Tracer: tests/ray_oracle.py's oracle_trace() restates the loop of
Tracer.pixel (the stack, the STACK_FULL rule, the first pop's record) for a given first ray over
Tracer's own methods, with a Tracer per distinct max_length. voxel_index, steps and flags are equal,
ray_length is bit-equal, the colour is within COLOR_TOL = 1e-4 (tests/test_gpu_parity.py) after the
[0, 1] clamp, and alpha is 1. The clamp is the framebuffer store's (NaN -> 0, DESIGN.md "Numerics"), and a
NaN channel must be NaN on both sides: an all-zero direction gives a NaN sky in the shader itself
(normalize(0)), which a plain difference would fail on either side. Listed pixels are held bit for bit
against the frame: the hit-record (exact, counted) instance, the default stats-free frame, and the C
oracle's hits. Primary rays come from oracle.trace_pixel's first record, whose position is in floats
9-11 and direction in floats 12-14 (oracle/vrt_oracle.c trace_with_shadow), as tests/test_gpu_ray_query.py
reads them. All volumes are 16^3 unless stated, frames 96x54; oracle results are computed once and shared."""
import ctypes
import functools

import numpy as np
import pytest

import oracle
import voxelraytracer_amd as vrt
from harness import float_bits as bits, same_bytes
from oracle import numpy_oracle
from ray_oracle import NOISE, ONE, F, N, Z, assert_matches_oracle, make_params, oracle_records, ray_list, tracer
from voxelraytracer_amd import abi

pytestmark = pytest.mark.gpu

COUNT = 300
ASYNC_COUNT = 4099     # not a multiple of 64: the last wave is partial
W, H = 96, 54
SCENES = ("terrain", "glass_cube", "refraction")
BOUNCES = ((1, 2), (4, 4))


@functools.lru_cache(maxsize=None)
def scene_rays(scene):
    vox = vrt.build_scene(scene, N)
    vox.setflags(write=False)
    return vox, ray_list(100 + SCENES.index(scene), COUNT)


@functools.lru_cache(maxsize=None)
def scene_oracle(scene, bounces, noise, textured=False):
    vox, rays = scene_rays(scene)
    return oracle_records(vox, rays, make_params(bounces, noise, textured))


# ---- 1. arbitrary rays against the NumPy oracle ------------------------------------------------

@pytest.mark.parametrize("noise", sorted(NOISE))
@pytest.mark.parametrize("bounces", BOUNCES, ids=lambda b: f"R{b[0]}T{b[1]}")
@pytest.mark.parametrize("scene", SCENES)
def test_rays_match_the_numpy_oracle(built, scene, bounces, noise):
    vox, rays = scene_rays(scene)
    want, pops = scene_oracle(scene, bounces, noise)
    # asserted on the oracle, so the case cannot pass empty
    hits = int(np.count_nonzero(want["voxel_index"] >= 0))
    print(f"{scene} {bounces} {noise}: {hits} hits, {COUNT - hits} misses, {np.count_nonzero(pops)} rays with "
          f"secondary rays, at most {pops.max()} per ray")
    assert hits >= 100 and COUNT - hits >= 25
    if scene == "glass_cube":
        assert np.count_nonzero(pops) >= 100
        if bounces == (4, 4):
            assert pops.max() > 6
    with vrt.Renderer(0) as r:
        r.upload_volume(vox, N)
        got = r.trace_rays(rays, make_params(bounces, noise))
    assert_matches_oracle(got, want, f"{scene} {bounces} {noise}")


# ---- 2. textured ------------------------------------------------------------------------------

def test_textured_rays_match_the_numpy_oracle(built):
    vox, rays = scene_rays("glass_cube")
    want, pops = scene_oracle("glass_cube", (1, 2), "noisy", True)
    hits = int(np.count_nonzero(want["voxel_index"] >= 0))
    assert hits >= 100 and COUNT - hits >= 25 and np.count_nonzero(pops) >= 100
    with vrt.Renderer(0) as r:
        r.upload_volume(vox, N)
        got = r.trace_rays(rays, make_params((1, 2), "noisy", True))
        # the atlas stays in the context: atlas_rgba = NULL traces with it, as the render calls do
        p = make_params((1, 2), "noisy", True)
        p.atlas_rgba = None
        again = r.trace_rays(rays, p)
    assert_matches_oracle(got, want, "textured glass_cube")
    assert same_bytes(again, got)
    plain, _ = scene_oracle("glass_cube", (1, 2), "noisy")
    assert not np.array_equal(got["rgba"], plain["rgba"])   # and the atlas is what colours it


# ---- 3. fixed rays -----------------------------------------------------------------------------

def fixed_volume():
    """refraction 16^3 (a glass voxel at the centre, grass plates on the six sides) plus a stone voxel at
    (3, 1, 1), as tests/test_gpu_ray_query.py."""
    vox = vrt.build_scene("refraction", N).copy()
    assert vox[8 + 8 * N + 8 * N * N] == 2 and vox[3 + 1 * N + 1 * N * N] == 0
    vox[3 + 1 * N + 1 * N * N] = 1
    return vox


FIXED = [
    # origin, direction, max_length
    ((16.0, 8.5, 8.5), (-1.0, 0.0, 0.0), 100.0),      # an origin on coordinate N; +0 components
    ((16.0, 8.5, 8.5), (-1.0, -0.0, 0.0), 100.0),     # a -0 component
    ((8.5, 8.5, -3.0), (0.0, -0.0, 1.0), 100.0),      # from outside, inward, with a -0 component: the glass voxel
    ((8.0, 8.0, 20.0), (0.0, 0.0, -1.0), 100.0),      # from outside, inward, along a lattice line
    ((-3.0, -2.0, -1.0), (0.63, 0.575, 0.52), 100.0),  # from outside, inward, at the centre voxel
    ((20.0, 8.5, 8.5), (1.0, 0.0, 0.0), 100.0),       # outside, moving away: the sky
    ((-2.0, -3.0, 19.0), (-0.3, -0.5, 0.8), 100.0),   # outside, moving away, every component non-zero: the sky
    ((0.0, 0.0, 0.0), (1.0, 1.0, 1.0), 100.0),        # the lattice diagonal: x+y+z ties, VRT_HIT_FLAG_TIE3
    ((0.5, 8.5, 8.5), (1.0, 1e-30, -1e-30), 100.0),   # components of 1e-30
    ((0.5, 8.5, 8.5), (1.0, 1e-30, 0.25), 100.0),
    ((8.5, 8.5, 3.5), (0.0, 0.0, 0.0), 100.0),        # an all-zero direction
    ((0.5, 1.5, 1.5), (1.0, 0.0, 0.0), 2.0),          # a short ray that still lands on the stone voxel
]
AWAY = (5, 6)


@pytest.mark.parametrize("bounces", BOUNCES, ids=lambda b: f"R{b[0]}T{b[1]}")
def test_fixed_rays(built, bounces):
    vox = fixed_volume()
    rays = vrt.make_rays([f[0] for f in FIXED], [f[1] for f in FIXED], [f[2] for f in FIXED])
    p = make_params(bounces)
    want, pops = oracle_records(vox, rays, p)
    # the cases are what their comments say, on the oracle
    centre = 8 + 8 * N + 8 * N * N
    assert [want["voxel_index"][i] for i in (0, 4, 7, 8)] == [centre] * 4 and all(pops[i] > 0 for i in (0, 4, 7, 8))
    assert want["voxel_index"][3] >= 0 and pops[3] == 0                   # a grass plate
    assert [want["voxel_index"][i] for i in (1, 2, 9)] == [-1] * 3 and all(want["steps"][i] > 0 for i in (1, 2, 9))
    assert want["voxel_index"][11] == 3 + 1 * N + 1 * N * N and want["ray_length"][11] == 2.5
    assert want["flags"][7] & abi.VRT_HIT_FLAG_TIE3 and not want["flags"][4] & abi.VRT_HIT_FLAG_TIE3
    with np.errstate(all="ignore"):
        tr = tracer(vox, p, F(100.0))
        for i in AWAY:   # a ray that leaves at once sees the sky: the skybox through the loop's two mixes
            assert want["voxel_index"][i] == -1 and want["steps"][i] == 0
            ray = dict(dir=tuple(F(x) for x in FIXED[i][1]), energy=ONE)
            sky = tr.skybox(ray, (Z, Z, Z))
            mixed = tuple(numpy_oracle.g_mix(s, Z, ONE - ONE) for s in sky)
            assert np.array_equal(bits(want["rgba"][i, :3]), bits(np.array(mixed, np.float32)))
            assert max(mixed) > 0.0
    assert want["voxel_index"][10] == -1 and np.isnan(want["rgba"][10, :3]).any()   # normalize(0) in the skybox
    with vrt.Renderer(0) as r:
        r.upload_volume(vox, N)
        got = r.trace_rays(rays, p)
    assert_matches_oracle(got, want, f"fixed rays {bounces}")


# ---- 4. pixels equal the frame ------------------------------------------------------------------

def all_pixels():
    y, x = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    return np.stack([x.reshape(-1), y.reshape(-1)], axis=1).astype(np.int32)   # row by row


PIXEL_CASES = [
    # scene, n, ray_noise, skip layout
    ("glass_cube", 16, 0.0, 0),
    ("glass_cube", 16, 0.0, 1),
    ("glass_cube", 16, 0.0, 8),
    ("refraction", 16, 0.0, 0),
    ("refraction", 16, 0.05, 0),
    ("terrain", 32, 0.0, 0),
]


@pytest.mark.parametrize("scene,n,ray_noise,layout", PIXEL_CASES)
def test_pixels_equal_the_frame(built, scene, n, ray_noise, layout):
    vox = vrt.build_scene(scene, n)
    cam = vrt.make_camera(W, H)
    p = vrt.default_params(2, 2, ray_noise=ray_noise, reflection_noise=0.05, refraction_noise=0.01, time=3.0)
    with vrt.Renderer(0) as r:
        r.set_skip_layout(layout)
        r.upload_volume(vox, n)
        assert r._lib.vrt_volume_octants(r._h) == (1 if layout == 1 else 8)
        got = r.trace_pixels(cam, p, all_pixels()).reshape(H, W)
        exact_rgba, exact_hits, _ = r.render(cam, p, want_hits=True, counters=False)
        fast_rgba, _, _ = r.render(cam, p, want_hits=False, counters=False)
    for name, _ in abi.Hit._fields_:
        assert np.array_equal(bits(got[name]) if name == "ray_length" else got[name],
                              bits(exact_hits[name]) if name == "ray_length" else exact_hits[name]), name
    assert same_bytes(got.view(np.uint8).reshape(H, W, 32)[..., :16], exact_hits)
    assert np.array_equal(bits(got["rgba"]), bits(exact_rgba))
    assert np.array_equal(bits(got["rgba"]), bits(fast_rgba))
    _, oracle_hits, _ = oracle.render(cam, vox, n, p, threads=4)
    assert np.array_equal(got["voxel_index"], oracle_hits["voxel_index"])
    assert np.array_equal(bits(got["ray_length"]), bits(oracle_hits["ray_length"]))
    found = np.count_nonzero(got["voxel_index"] >= 0)
    # voxels and sky; glass_cube's camera looks at the glass walls with every pixel
    assert found > 0 and (found < W * H) == (scene != "glass_cube")


# ---- 5. rays equal pixels -----------------------------------------------------------------------

def test_rays_equal_pixels(built):
    vox = vrt.build_scene("refraction", N)
    cam = vrt.make_camera(W, H)
    p = vrt.default_params(2, 2, ray_noise=0.0, reflection_noise=0.05, refraction_noise=0.01, time=3.0)
    pixels = all_pixels()[np.random.default_rng(5).choice(W * H, 200, replace=False)]
    origins, dirs = [], []
    for x, y in pixels:
        recs, _ = oracle.trace_pixel(cam, vox, N, p, int(x), int(y))
        assert recs[0, 0] == 1 and recs[0, 15] == 0 and recs[0, 16] == 1   # a first ray: from length 0, energy 1
        origins.append(recs[0, 9:12].copy())
        dirs.append(recs[0, 12:15].copy())
    rays = vrt.make_rays(origins, dirs, p.max_ray_length)
    with vrt.Renderer(0) as r:
        r.upload_volume(vox, N)
        by_pixel = r.trace_pixels(cam, p, pixels)
        by_ray = r.trace_rays(rays, p)
    assert 0 < np.count_nonzero(by_pixel["voxel_index"] >= 0) < len(pixels)
    assert same_bytes(by_ray, by_pixel)


# ---- 6. async equals sync -----------------------------------------------------------------------

def device_bytes(a):
    import torch

    return torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).cuda()


def test_async_on_a_torch_stream_equals_the_synchronous_trace(built):
    import torch

    vox = vrt.build_scene("glass_cube", N)
    rays = ray_list(77, ASYNC_COUNT)
    p = make_params((2, 2), "noisy")
    pad = 64   # records allocated after the last one written
    with vrt.Renderer(0) as r:
        r.upload_volume(vox, N)
        want = r.trace_rays(rays, p)
        assert want.shape == (ASYNC_COUNT,) and np.count_nonzero(want["voxel_index"] >= 0) > ASYNC_COUNT // 4
        s = torch.cuda.Stream()
        outs = {}
        with torch.cuda.stream(s):
            d_rays = device_bytes(rays)
            for count in (ASYNC_COUNT, 1, 64):
                d_out = torch.full(((count + pad) * 32,), 0xAB, dtype=torch.uint8, device="cuda")
                r.trace_rays_async(d_rays.data_ptr(), count, p, d_out.data_ptr(), s.cuda_stream)
                outs[count] = d_out
        s.synchronize()
        for count, d_out in outs.items():
            raw = d_out.cpu().numpy()
            assert same_bytes(raw[:count * 32], want[:count]), count
            assert np.all(raw[count * 32:] == 0xAB), count   # nothing past `count`
        assert same_bytes(r.trace_rays(rays[:64], p), want[:64]) and same_bytes(r.trace_rays(rays[:1], p), want[:1])


# ---- 7. edits are seen ---------------------------------------------------------------------------

def test_edits_are_seen(built):
    vox = vrt.build_scene("terrain", N).copy()
    cam = vrt.make_camera(W, H)
    p = vrt.default_params(2, 2)
    pixels = all_pixels()
    centre = (H // 2) * W + W // 2
    with vrt.Renderer(0) as r:
        r.upload_volume(vox, N)
        before = r.trace_pixels(cam, p, pixels)
        assert before["voxel_index"][centre] >= 0
        i, j, k = (int(c[0]) for c in vrt.hit_cell(before[centre:centre + 1], N))
        r.update_volume((i, j, k), np.zeros((1, 1, 1), np.uint8))
        vox[before["voxel_index"][centre]] = 0
        after = r.trace_pixels(cam, p, pixels)
    with vrt.Renderer(0) as fresh:
        fresh.upload_volume(vox, N)
        rgba, hits, _ = fresh.render(cam, p, want_hits=True, counters=False)
    assert same_bytes(after.view(np.uint8).reshape(-1, 32)[:, :16], hits.reshape(-1))
    assert np.array_equal(bits(after["rgba"]), bits(rgba.reshape(-1, 4)))
    assert after["voxel_index"][centre] != before["voxel_index"][centre]
    assert np.any(bits(after["rgba"]) != bits(before["rgba"]))


# ---- 8. errors -----------------------------------------------------------------------------------

def test_errors(built):
    import torch

    vox, rays = scene_rays("terrain")
    cam = vrt.make_camera(W, H)
    p = make_params((2, 2))
    d_rays = device_bytes(rays[:64])
    d_out = torch.full((65 * 32,), 0xAB, dtype=torch.uint8, device="cuda")
    rp, op = d_rays.data_ptr(), d_out.data_ptr()
    assert rp % 16 == 0 and op % 16 == 0
    with vrt.Renderer(0) as r:
        for call in (lambda: r.trace_rays(rays[:4], p), lambda: r.trace_pixels(cam, p, [(1, 1)]),
                     lambda: r.trace_rays_async(rp, 4, p, op)):
            with pytest.raises(vrt.VrtError) as e:
                call()
            assert e.value.code == abi.VRT_ERR_NO_VOLUME
        r.upload_volume(vox, N)
        want = r.trace_rays(rays[:64], p)
        want_px = r.trace_pixels(cam, p, [(1, 1), (W - 1, H - 1)])
        deeper = make_params((9, 2))   # max_reflections = 9: outside 0..8 (vrt_params)
        lib, h, pp = r._lib, r._h, ctypes.byref(p)

        def still_works():
            assert lib.vrt_last_error(h)
            torch.cuda.synchronize()
            assert bool((d_out == 0xAB).all())   # the rejected call wrote no record
            assert same_bytes(r.trace_rays(rays[:64], p), want)
            assert same_bytes(r.trace_pixels(cam, p, [(1, 1), (W - 1, H - 1)]), want_px)

        for args in ((rp, -1, pp, op), (rp, (1 << 30) + 1, pp, op), (rp + 8, 4, pp, op), (rp, 4, pp, op + 8),
                     (None, 4, pp, op), (rp, 4, pp, None), (rp, 4, None, op), (rp, 4, ctypes.byref(deeper), op)):
            assert lib.vrt_trace_rays_async(h, *args, None) == abi.VRT_ERR_INVALID, args
            still_works()
        for args in ((rays.ctypes.data, -1, pp, None), (None, 4, pp, None), (rays.ctypes.data, 4, ctypes.byref(deeper), None)):
            assert lib.vrt_trace_rays(h, *args) == abi.VRT_ERR_INVALID, args
            still_works()
        for bad in ((W, 0), (0, H), (-1, 3), (3, -1)):
            with pytest.raises(vrt.VrtError) as e:
                r.trace_pixels(cam, p, [(1, 1), bad])
            assert e.value.code == abi.VRT_ERR_INVALID
            still_works()
        for call in (lambda: r.trace_pixels(cam, deeper, [(1, 1)]), lambda: r.trace_rays(rays[:4], deeper)):
            with pytest.raises(vrt.VrtError) as e:
                call()
            assert e.value.code == abi.VRT_ERR_INVALID
            still_works()
        assert lib.vrt_trace_pixels(h, None, None, None, 1, None) == abi.VRT_ERR_INVALID
        assert lib.vrt_trace_pixels(h, ctypes.byref(cam), pp, None, 1, None) == abi.VRT_ERR_INVALID
        assert lib.vrt_trace_pixels(h, ctypes.byref(cam), pp, None, -1, None) == abi.VRT_ERR_INVALID
        still_works()
        assert len(r.trace_rays(rays[:4], make_params((8, 8)))) == 4   # the largest stack traces
        # count == 0 is a successful no-op and needs no buffers
        assert lib.vrt_trace_rays_async(h, None, 0, pp, None, None) == abi.VRT_OK
        assert lib.vrt_trace_rays(h, None, 0, pp, None) == abi.VRT_OK
        assert lib.vrt_trace_pixels(h, ctypes.byref(cam), pp, None, 0, None) == abi.VRT_OK
        assert len(r.trace_rays(rays[:0], p)) == 0 and len(r.trace_pixels(cam, p, np.zeros((0, 2), np.int32))) == 0
        # and a valid asynchronous call still works afterwards
        assert lib.vrt_trace_rays_async(h, rp, 64, pp, op, None) == abi.VRT_OK
        torch.cuda.synchronize()
        assert same_bytes(d_out.cpu().numpy()[:64 * 32], want)


# ---- 9. launch timing ----------------------------------------------------------------------------

def test_launch_timing_covers_the_trace_launches(built):
    vox, rays = scene_rays("refraction")
    cam = vrt.make_camera(W, H)
    p = make_params((2, 2))
    with vrt.Renderer(0) as r:
        r.upload_volume(vox, N)
        r.set_launch_timing(2)
        r.trace_rays(rays, p)
        r.trace_pixels(cam, p, all_pixels())
        total, launches = r.launch_timing()
        r.set_launch_timing(0)
    assert launches == 2 and total > 0.0
