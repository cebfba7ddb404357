"""Ray queries (GPU): vrt_cast_rays / vrt_cast_rays_async / vrt_pick_pixels run the frame kernels' exact
walks for a list of rays, so every record is held bit for bit against the CPU oracles' march of the
same ray: oracle.march_one (the C restatement of RayMarch), numpy_oracle.Tracer.march (the independent
one, which also yields the flags) and Tracer.march_shadow (RayMarchShadow along any direction). All
volumes are 16^3; the oracle results of a scene are computed once and shared."""
import functools
import os
import re
import subprocess

import numpy as np
import pytest

import oracle
import voxelraytracer_amd as vrt
from harness import float_bits as bits
from ray_oracle import N, assert_nearest_matches, march_all, numpy_march, numpy_shadow, ray_list
from voxelraytracer_amd import abi

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
COUNT = 4099          # not a multiple of 64 or 256: the last wave is partial
NUMPY_COUNT = 300     # rays also held against the NumPy oracle (flags; occlusion)
SCENES = ("terrain", "glass_cube", "refraction")


@functools.lru_cache(maxsize=None)
def scene_rays(scene):
    """The scene's bytes and its COUNT rays (ray_oracle.ray_list's distribution)."""
    return vrt.build_scene(scene, N), ray_list(SCENES.index(scene) + 1, COUNT)


@functools.lru_cache(maxsize=None)
def oracle_nearest(scene):
    vox, rays = scene_rays(scene)
    return march_all(vox, rays)


def assert_matches_numpy(hit_rec, vox, ray):
    hit, steps, flags = numpy_march(vox, ray)
    assert (hit_rec["voxel_index"] >= 0) == hit["found"]
    assert hit_rec["steps"] == steps and hit_rec["flags"] == flags
    if hit["found"]:
        assert hit_rec["voxel_index"] == hit["vidx"]
        assert bits(hit_rec["ray_length"]) == bits(hit["len"])
        assert np.array_equal(bits(hit_rec["point"]), bits(np.array(hit["point"], np.float32)))
        assert np.array_equal(vrt.hit_normal(hit_rec)[0], np.array(hit["normal"]).astype(np.int8))
    else:
        assert hit_rec["ray_length"] == 0 and np.all(hit_rec["point"] == 0) and hit_rec["face"] == 0


@pytest.mark.parametrize("layout", [0, 1])
@pytest.mark.parametrize("scene", SCENES)
def test_nearest_matches_the_oracle(built, scene, layout):
    vox, rays = scene_rays(scene)
    want = oracle_nearest(scene)
    # asserted on the oracle, so the case cannot pass empty: hits, misses, and hits that the ray's own
    # shorter max_length removes
    short = rays["max_length"] < 100.0
    far = march_all(vox, rays[short], max_len=100.0)
    cut = int(np.count_nonzero(far["found"] & ~want["found"][short]))
    share = want["found"].mean()
    print(f"{scene}: {share:.0%} hits, {1 - share:.0%} misses, {cut} hits cut by max_length")
    assert share >= 0.10 and 1.0 - share >= 0.10 and cut >= 100
    with vrt.Renderer(0) as r:
        r.set_skip_layout(layout)
        r.upload_volume(vox, N)
        assert r._lib.vrt_volume_octants(r._h) == (1 if layout == 1 else 8)
        hits = r.cast_rays(rays, "nearest")
    assert hits.dtype == np.dtype(abi.RAY_HIT_DTYPE) and hits.shape == (COUNT,)
    assert_nearest_matches(hits, want, vox, rays)
    for i in range(NUMPY_COUNT):
        assert_matches_numpy(hits[i:i + 1][0], vox, rays[i])


def fixed_volume():
    """refraction 16^3 (a glass voxel at the centre, grass plates on the six sides) plus the stone voxel
    of tests/test_oracle_kat.py's length test at (3, 1, 1)."""
    vox = vrt.build_scene("refraction", N).copy()
    assert vox[8 + 8 * N + 8 * N * N] == 2 and vox[3 + 1 * N + 1 * N * N] == 0
    vox[3 + 1 * N + 1 * N * N] = 1
    return vox


FIXED = [
    # origin, direction, max_length
    ((16.0, 8.5, 8.5), (-1.0, 0.0, 0.0), 100.0),      # an origin on coordinate N; +0 components (dda_walk)
    ((16.0, 8.5, 8.5), (-1.0, -0.0, 0.0), 100.0),     # a -0 component: t = -inf, the literal replay's miss
    ((8.0, 8.0, 20.0), (0.0, 0.0, -1.0), 100.0),      # from outside, inward, along a lattice line
    ((8.5, 8.5, -3.0), (0.0, -0.0, 1.0), 100.0),      # from outside, inward, with a -0 component
    ((20.0, 8.5, 8.5), (1.0, 0.0, 0.0), 100.0),       # outside, moving away: 0 steps
    ((-2.0, -3.0, 19.0), (-0.3, -0.5, 0.8), 100.0),   # outside, moving away, every component non-zero
    ((-3.0, -2.0, -1.0), (0.63, 0.575, 0.52), 100.0),  # from outside, inward, at the centre voxel (fast path)
    ((0.0, 0.0, 0.0), (1.0, 1.0, 1.0), 100.0),        # the lattice diagonal: x+y+z ties, VRT_HIT_FLAG_TIE3
    ((0.5, 8.5, 8.5), (1.0, 1e-30, -1e-30), 100.0),   # components below fast_path_ok's 2^-64
    ((0.5, 8.5, 8.5), (1.0, 1e-30, 0.25), 100.0),
    ((0.5, 1.5, 1.5), (1.0, 0.0, 0.0), 1.5),          # test_oracle_kat's length test: stops before x = 3
    ((0.5, 1.5, 1.5), (1.0, 0.0, 0.0), 2.0),          # still takes the step that lands on x = 3 (2.5)
    ((0.5, 1.5, 1.5), (1.0, 0.0, 0.0), 100.0),
]


def test_fixed_rays(built):
    vox = fixed_volume()
    rays = vrt.make_rays([f[0] for f in FIXED], [f[1] for f in FIXED], [f[2] for f in FIXED])
    want = march_all(vox, rays)
    # the cases are what their comments say, on the oracle
    centre = 8 + 8 * N + 8 * N * N
    assert want["found"].tolist() == [True, False, True, False, False, False, True, True, True, False, False, True, True]
    assert want["steps"][4] == 0 and want["steps"][5] == 0 and want["steps"][1] > 0 and want["steps"][9] > 8
    assert [want["vidx"][i] for i in (0, 6, 7, 8)] == [centre] * 4
    assert want["len"][11] == 2.5 and want["len"][12] == 2.5 and want["vidx"][11] == 3 + 1 * N + 1 * N * N
    with vrt.Renderer(0) as r:
        r.upload_volume(vox, N)
        hits = r.cast_rays(rays)
        occ = r.cast_rays(rays, "occlusion")
    assert_nearest_matches(hits, want, vox, rays)
    for i in range(len(rays)):
        assert_matches_numpy(hits[i:i + 1][0], vox, rays[i])
        blocked, steps, flags = numpy_shadow(vox, rays[i])
        assert bool(occ["flags"][i] & abi.VRT_RAY_FLAG_BLOCKED) == blocked, i
        assert occ["steps"][i] == steps and occ["flags"][i] & ~np.uint32(abi.VRT_RAY_FLAG_BLOCKED) == flags, i
    assert hits["flags"][7] & abi.VRT_HIT_FLAG_TIE3     # as the NumPy oracle (checked above), and set
    assert not hits["flags"][6] & abi.VRT_HIT_FLAG_TIE3


def occlusion_case(scene):
    """The scene's bytes and its first NUMPY_COUNT rays. "glass_walls" is glass_cube without its one
    opaque voxel (the grass voxel at the centre, which 1 % of the rays meet): a volume that is all glass."""
    vox, rays = scene_rays("glass_cube" if scene == "glass_walls" else scene)
    if scene == "glass_walls":
        vox = vox.copy()
        assert np.count_nonzero((vox != 0) & (vox != 2)) == 1 and vox[8 + 8 * N + 8 * N * N] == 3
        vox[8 + 8 * N + 8 * N * N] = 0
    return vox, rays[:NUMPY_COUNT]


@pytest.mark.parametrize("scene", SCENES + ("glass_walls",))
def test_occlusion_matches_the_numpy_oracle(built, scene):
    """The blocked bit, the steps and the flags of RayMarchShadow along each ray. glass_cube at 16^3 is glass
    walls around one grass voxel: its rays are blocked only by that voxel, and with it removed (glass_walls)
    never, while nearest mode hits the walls."""
    vox, rays = occlusion_case(scene)
    want = [numpy_shadow(vox, r) for r in rays]
    blocked = np.array([w[0] for w in want])
    near_want = march_all(vox, rays)
    share, near_share = blocked.mean(), near_want["found"].mean()
    print(f"{scene}: {share:.0%} blocked, {near_share:.0%} nearest hits")
    if scene == "glass_walls":
        assert not blocked.any() and near_share >= 0.10
    elif scene == "glass_cube":
        assert near_share >= 0.10 and share <= 0.05
        assert np.all(near_want["found"][blocked])   # a blocked ray has a nearest hit, not the reverse
    else:
        assert share >= 0.10 and 1.0 - share >= 0.10
    with vrt.Renderer(0) as r:
        r.upload_volume(vox, N)
        occ = r.cast_rays(rays, "occlusion")
        near = r.cast_rays(rays, "nearest")
    assert np.array_equal((occ["flags"] & abi.VRT_RAY_FLAG_BLOCKED) != 0, blocked)
    assert np.array_equal(occ["steps"], np.array([w[1] for w in want], np.uint32))
    assert np.array_equal(occ["flags"] & ~np.uint32(abi.VRT_RAY_FLAG_BLOCKED), np.array([w[2] for w in want], np.uint32))
    assert np.all(occ["voxel_index"] == -1) and np.all(occ["ray_length"] == 0)
    assert np.all(occ["point"] == 0) and np.all(occ["face"] == 0)
    assert_nearest_matches(near, near_want, vox, rays)


def device_bytes(a):
    import torch

    return torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).copy()).cuda()


@pytest.mark.parametrize("mode", ["nearest", "occlusion"])
def test_counts_and_untouched_tail(built, mode):
    import torch

    vox, rays = scene_rays("terrain")
    pad = 3   # records allocated after the last one written
    with vrt.Renderer(0) as r:
        r.upload_volume(vox, N)
        full = r.cast_rays(rays, mode)
        d_rays = device_bytes(rays)
        for count in (0, 1, 63, 64, 65, 257):
            assert np.array_equal(r.cast_rays(rays[:count], mode), full[:count])
            d_hits = torch.full(((count + pad) * 32,), 0xAB, dtype=torch.uint8, device="cuda")
            torch.cuda.synchronize()
            r.cast_rays_async(d_rays.data_ptr(), count, d_hits.data_ptr(), mode)
            torch.cuda.synchronize()
            got = d_hits.cpu().numpy()
            assert np.array_equal(got[:count * 32].view(abi.RAY_HIT_DTYPE), full[:count])
            assert np.all(got[count * 32:] == 0xAB)
        # count == 0 needs no buffers
        r.cast_rays_async(0, 0, 0, mode)


def test_staging_grows_and_is_reused(built):
    """One renderer's casts of 5, 4 097, 9 000 and 5 rays: the synchronous staging's first allocation (its
    4 096-record floor), two growths, then the larger buffers reused for a short list."""
    vox, rays = scene_rays("terrain")
    want = oracle_nearest("terrain")
    with vrt.Renderer(0) as r:
        r.upload_volume(vox, N)
        for count in (5, 4097, 9000, 5):
            idx = np.arange(count) % COUNT
            hits = r.cast_rays(rays[idx], "nearest")
            assert hits.shape == (count,)
            assert_nearest_matches(hits, {key: v[idx] for key, v in want.items()}, vox, rays[idx])


def test_async_on_a_torch_stream_equals_the_synchronous_cast(built):
    import torch

    vox, rays = scene_rays("refraction")
    with vrt.Renderer(0) as r:
        r.upload_volume(vox, N)
        s = torch.cuda.Stream()
        out = {}
        with torch.cuda.stream(s):
            d_rays = device_bytes(rays)
            for mode in ("nearest", "occlusion"):
                d_hits = torch.zeros(COUNT * 32, dtype=torch.uint8, device="cuda")
                r.cast_rays_async(d_rays.data_ptr(), COUNT, d_hits.data_ptr(), mode, s.cuda_stream)
                out[mode] = d_hits
        s.synchronize()
        for mode, d_hits in out.items():
            assert np.array_equal(d_hits.cpu().numpy().view(abi.RAY_HIT_DTYPE), r.cast_rays(rays, mode))
    assert_nearest_matches(out["nearest"].cpu().numpy().view(abi.RAY_HIT_DTYPE), oracle_nearest("refraction"), vox, rays)


PICK_W, PICK_H = 64, 36


def pick_pixels():
    px = [(x, y) for y in (0, 17, PICK_H - 1) for x in range(PICK_W)]
    px += [(0, 0), (PICK_W - 1, 0), (0, PICK_H - 1), (PICK_W - 1, PICK_H - 1)]
    return np.array(px, np.int32)


def primary_ray(cam, vox, p, px, py):
    """The pixel's primary ray as it entered RayMarch: oracle.trace_pixel's first record (a
    TraceWithShadow call: position in floats 9-11, direction in 12-14, ray length in 15)."""
    recs, _ = oracle.trace_pixel(cam, vox, N, p, int(px), int(py))
    assert recs[0, 0] == 1 and recs[0, 15] == 0 and recs[0, 16] == 1   # from ray length 0, energy 1
    return recs[0, 9:12].copy(), recs[0, 12:15].copy()


def march_pixels(cam, vox, p, pixels):
    rays = [primary_ray(cam, vox, p, x, y) for x, y in pixels]
    return march_all(vox, vrt.make_rays([r[0] for r in rays], [r[1] for r in rays], p.max_ray_length))


@pytest.mark.parametrize("ray_noise", [0.0, 0.05])
@pytest.mark.parametrize("scene", ["refraction", "terrain"])
def test_pick_matches_the_frame_and_the_oracle(built, scene, ray_noise):
    vox = vrt.build_scene(scene, N)
    cam = vrt.make_camera(PICK_W, PICK_H)
    p = vrt.default_params(2, 2, ray_noise=ray_noise, time=3.0)
    pixels = pick_pixels()
    xs, ys = pixels[:, 0], pixels[:, 1]
    with vrt.Renderer(0) as r:
        r.upload_volume(vox, N)
        picks = r.pick(cam, p, pixels)
        _, frame_hits, _ = r.render(cam, p, want_hits=True, counters=False)
        for bad in ((PICK_W, 0), (0, PICK_H), (-1, 3), (3, -1)):
            with pytest.raises(vrt.VrtError) as e:
                r.pick(cam, p, [(1, 1), bad])
            assert e.value.code == abi.VRT_ERR_INVALID
        assert len(r.pick(cam, p, np.zeros((0, 2), np.int32))) == 0
    _, oracle_hits, _ = oracle.render(cam, vox, N, p, threads=4)
    for ref in (frame_hits, oracle_hits):
        assert np.array_equal(picks["voxel_index"], ref["voxel_index"][ys, xs])
        assert np.array_equal(bits(picks["ray_length"]), bits(ref["ray_length"][ys, xs]))
    assert 0 < np.count_nonzero(picks["voxel_index"] >= 0) < len(pixels)   # hits and sky
    assert_nearest_matches(picks, march_pixels(cam, vox, p, pixels), vox, None)


def test_pick_edit_pick_loop(built):
    scene, centre = "terrain", np.array([[PICK_W // 2, PICK_H // 2]], np.int32)
    vox = vrt.build_scene(scene, N).copy()
    cam = vrt.make_camera(PICK_W, PICK_H)
    p = vrt.default_params(2, 2)
    with vrt.Renderer(0) as r:
        r.upload_volume(vox, N)
        first = r.pick(cam, p, centre)
        assert first["voxel_index"][0] >= 0
        assert_nearest_matches(first, march_pixels(cam, vox, p, centre), vox, None)
        # remove the voxel under the cursor: the next pick is behind it, or sky
        i, j, k = (int(c[0]) for c in vrt.hit_cell(first, N))
        r.update_volume((i, j, k), np.zeros((1, 1, 1), np.uint8))
        vox[first["voxel_index"][0]] = 0
        second = r.pick(cam, p, centre)
        assert_nearest_matches(second, march_pixels(cam, vox, p, centre), vox, None)
        assert second["voxel_index"][0] < 0 or second["ray_length"][0] > first["ray_length"][0]
        assert second["voxel_index"][0] != first["voxel_index"][0]
        # place a block on the face first seen: the pick then hits that cell
        ai, aj, ak = (int(c[0]) for c in vrt.adjacent_cell(first, N))
        assert all(0 <= c < N for c in (ai, aj, ak)), "the centre pixel's face lies inside the volume"
        r.update_volume((ai, aj, ak), np.ones((1, 1, 1), np.uint8))
        vox[ai + aj * N + ak * N * N] = 1
        third = r.pick(cam, p, centre)
        want = march_pixels(cam, vox, p, centre)
        assert_nearest_matches(third, want, vox, None)
        assert third["voxel_index"][0] == ai + aj * N + ak * N * N
        assert np.array_equal(bits(third["point"]), bits(want["point"]))
        assert third["ray_length"][0] < first["ray_length"][0]


def raw_cast(r, d_rays, count, mode, d_hits):
    return r._lib.vrt_cast_rays_async(r._h, d_rays, count, mode, d_hits, None)


def test_errors(built):
    import torch

    vox, rays = scene_rays("terrain")
    cam = vrt.make_camera(PICK_W, PICK_H)
    p = vrt.default_params(2, 2)
    d_rays = device_bytes(rays[:64])
    d_hits = torch.full((65 * 32,), 0xAB, dtype=torch.uint8, device="cuda")
    with vrt.Renderer(0) as r:
        for call in (lambda: r.cast_rays(rays[:4]), lambda: r.pick(cam, p, [(1, 1)]),
                     lambda: r.cast_rays_async(d_rays.data_ptr(), 4, d_hits.data_ptr())):
            with pytest.raises(vrt.VrtError) as e:
                call()
            assert e.value.code == abi.VRT_ERR_NO_VOLUME
        r.upload_volume(vox, N)
        rp, hp = d_rays.data_ptr(), d_hits.data_ptr()
        assert rp % 16 == 0 and hp % 16 == 0
        for args in ((rp + 4, 4, 0, hp), (rp, 4, 0, hp + 8), (rp, -1, 0, hp), (rp, (1 << 30) + 1, 0, hp),
                     (rp, 4, 7, hp), (rp, 4, -1, hp), (None, 4, 0, hp), (rp, 4, 0, None)):
            assert raw_cast(r, *args) == abi.VRT_ERR_INVALID, args
            assert r._lib.vrt_last_error(r._h)
        with pytest.raises(vrt.VrtError) as e:
            r.cast_rays(rays[:4], 7)
        assert e.value.code == abi.VRT_ERR_INVALID
        assert r._lib.vrt_cast_rays(r._h, None, 4, 0, None) == abi.VRT_ERR_INVALID
        assert r._lib.vrt_pick_pixels(r._h, None, None, None, 1, None) == abi.VRT_ERR_INVALID
        torch.cuda.synchronize()
        assert bool((d_hits == 0xAB).all())   # no rejected call wrote a record
        # and a valid call still works afterwards
        assert raw_cast(r, rp, 64, 0, hp) == abi.VRT_OK
        torch.cuda.synchronize()
        assert np.array_equal(d_hits.cpu().numpy()[:64 * 32].view(abi.RAY_HIT_DTYPE), r.cast_rays(rays[:64]))


def headless_pick_line(x, y):
    app = os.path.join(ROOT, "build", "bin", "vrt_headless")
    run = subprocess.run([app, "--scene", "refraction", "--n", "16", "--size", "64x36", "--frames", "1",
                          "--pick", f"{x},{y}"], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, run.stderr
    line = [ln for ln in run.stdout.splitlines() if ln.startswith("pick ")]
    assert len(line) == 1, run.stdout
    return line[0]


def test_headless_pick(built):
    """vrt_headless --pick prints the fields of Renderer.pick's record: for the centre pixel (32, 18), which
    shows the sky in this frame, and for a pixel that the oracle's frame says shows a voxel."""
    # the app's frame 0: u_Time 1, the default camera and sun, bounces 4 / 4 (a pick reads neither)
    vox = vrt.build_scene("refraction", N)
    cam, p = vrt.make_camera(64, 36), vrt.default_params(4, 4)
    _, oracle_hits, _ = oracle.render(cam, vox, N, p, threads=4)
    ys, xs = np.nonzero(oracle_hits["voxel_index"] >= 0)
    assert len(xs) > 0
    hx, hy = int(xs[len(xs) // 2]), int(ys[len(xs) // 2])
    with vrt.Renderer(0) as r:
        r.upload_volume(vox, N)
        h = r.pick(cam, p, [(32, 18), (hx, hy)])
    assert np.array_equal(h["voxel_index"], oracle_hits["voxel_index"][[18, hy], [32, hx]]) and h["voxel_index"][1] >= 0
    for i, (x, y) in enumerate(((32, 18), (hx, hy))):
        line = headless_pick_line(x, y)
        if h["voxel_index"][i] < 0:
            assert line == f"pick {x} {y} voxel=-1 byte=0 len=0 face=none cell=none"
            continue
        m = re.fullmatch(rf"pick {x} {y} voxel=(\d+) byte=(\d+) len=(\S+) face=([+-])([xyz]) cell=(\d+),(\d+),(\d+)", line)
        assert m, line
        assert int(m.group(1)) == h["voxel_index"][i] and int(m.group(2)) == (h["face"][i] >> 8) & 0xFF
        assert np.float32(float(m.group(3))) == h["ray_length"][i]
        nrm = vrt.hit_normal(h[i:i + 1])[0]
        axis = "xyz".index(m.group(5))
        assert nrm[axis] == (1 if m.group(4) == "+" else -1) and np.count_nonzero(nrm) == 1
        assert tuple(int(m.group(g)) for g in (6, 7, 8)) == tuple(int(c[0]) for c in vrt.hit_cell(h[i:i + 1], N))
