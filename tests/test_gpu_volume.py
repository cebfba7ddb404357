"""The kernel's device volume format (GPU): per direction octant a padded (N+1)^3 u16 = voxel |
G << 8, with plane N a copy of plane 0 (GL_REPEAT) and G the forward skip distance of the octant
(G(v) = F(v - s) - 1, F = edge of the largest empty in-volume cube anchored at a voxel and
extending along the octant's step s) — checked against a brute-force NumPy transform; for
N = 1024 one volume with the centred Chebyshev distance (tested at small N through the same
reference). G drives the empty-space step skipping, so an over-estimate would skip geometry
(DESIGN.md §6)."""
import numpy as np
import pytest

import voxelraytracer_amd as vrt
from skipfield_reference import chebyshev_reference, forward_reference, packed_reference

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("scene,n", [("terrain", 16), ("glass_cube", 16), ("refraction", 32),
                                     ("terrain", 32)])
def test_packed_volume_layout_and_distance(built, scene, n):
    vox = vrt.build_scene(scene, n)
    with vrt.Renderer(0) as r:
        r.upload_volume(vox, n)
        vols = r.debug_packed_volume()   # [octant][z][y][x], 8 x (n+1)^3
    assert vols.shape[0] == 8
    v = vox.reshape(n, n, n)
    for o, packed in enumerate(vols):
        assert np.array_equal(packed[:n, :n, :n] & 0xFF, v)
        assert np.array_equal(packed[n, :n, :n] & 0xFF, v[0])        # plane z = N repeats z = 0
        assert np.array_equal(packed[:n, n, :n] & 0xFF, v[:, 0])
        assert np.array_equal(packed[:n, :n, n] & 0xFF, v[:, :, 0])
        assert np.all(packed[n] >> 8 == 0) and np.all(packed[:, n] >> 8 == 0)
        assert np.all(packed[:, :, n] >> 8 == 0)
        assert np.array_equal(packed[:n, :n, :n] >> 8, forward_reference(vox, n, o)), o
        # the guarantee the skip walk relies on, stated directly: the box from one voxel behind
        # to G - 1 voxels ahead (along the octant's step) holds no non-empty voxel
        g = packed[:n, :n, :n] >> 8
        s = [(-1 if o >> a & 1 else 1) for a in range(3)]   # x, y, z steps
        zz, yy, xx = np.nonzero(g >= 1)
        for q in range(0, len(zz), max(1, len(zz) // 300)):
            k, j, i, e = zz[q], yy[q], xx[q], int(g[zz[q], yy[q], xx[q]])
            lo = [min(c - sc, c + (e - 1) * sc) for c, sc in zip((i, j, k), s)]
            hi = [max(c - sc, c + (e - 1) * sc) for c, sc in zip((i, j, k), s)]
            assert min(lo) >= 0 and max(hi) < n
            assert not v[lo[2]:hi[2] + 1, lo[1]:hi[1] + 1, lo[0]:hi[0] + 1].any()


@pytest.mark.parametrize("scene,n", [("terrain", 16), ("refraction", 32)])
def test_single_layout_centred_distance(built, scene, n):
    """The N = 1024 layout (one volume, centred Chebyshev D), forced at small N."""
    vox = vrt.build_scene(scene, n)
    with vrt.Renderer(0) as r:
        r.set_skip_layout(1)
        r.upload_volume(vox, n)
        vols = r.debug_packed_volume()
    assert vols.shape[0] == 1
    packed = vols[0]
    assert np.array_equal(packed[:n, :n, :n] & 0xFF, vox.reshape(n, n, n))
    assert np.all(packed[n] >> 8 == 0) and np.all(packed[:, n] >> 8 == 0)
    assert np.array_equal(packed[:n, :n, :n] >> 8, chebyshev_reference(vox, n))


@pytest.mark.parametrize("layout", [8, 1])
@pytest.mark.parametrize("n", [2, 4, 8])
def test_smallest_volumes(built, n, layout):
    """Random bytes (0..3, about half empty) at the smallest edges, both layouts, every texel of
    the (N+1)^3 volumes against the NumPy reference. At n = 2 every texel neighbours plane N and
    every scan is cut by a volume face: the whole-volume boxes of the upload clip on every side."""
    rng = np.random.default_rng(n)
    vox = np.where(rng.random(n ** 3) < 0.5, 0, rng.integers(1, 4, n ** 3)).astype(np.uint8)
    assert 0 < np.count_nonzero(vox) < n ** 3
    with vrt.Renderer(0) as r:
        r.set_skip_layout(layout)
        r.upload_volume(vox, n)
        vols = r.debug_packed_volume()
    assert vols.shape == (layout,) + (n + 1,) * 3
    v = vox.reshape(n, n, n)
    for packed in vols:
        assert np.array_equal(packed[n, :n, :n] & 0xFF, v[0])        # plane z = N repeats z = 0
        assert np.array_equal(packed[:n, n, :n] & 0xFF, v[:, 0])
        assert np.array_equal(packed[:n, :n, n] & 0xFF, v[:, :, 0])
        assert packed[n, n, n] & 0xFF == v[0, 0, 0]
        assert np.all(packed[n] >> 8 == 0) and np.all(packed[:, n] >> 8 == 0)
        assert np.all(packed[:, :, n] >> 8 == 0)
    want = packed_reference(vox, n, layout)
    assert np.array_equal(vols, want), np.argwhere(vols != want)[:4].tolist()


@pytest.mark.parametrize("scene,n,w,h,rt", [("terrain", 64, 160, 90, (4, 2)),
                                            ("refraction", 64, 160, 90, (4, 4)),
                                            ("glass_cube", 32, 128, 96, (1, 2))])
def test_layouts_render_identically(built, scene, n, w, h, rt):
    """Octant and single (centred) layouts skip different steps but replay the same walk: images,
    hit records and every counter are identical."""
    vox = vrt.build_scene(scene, n)
    cam = vrt.make_camera(w, h)
    p = vrt.default_params(*rt)
    res = []
    for layout in (8, 1):
        with vrt.Renderer(0) as r:
            r.set_skip_layout(layout)
            r.upload_volume(vox, n)
            res.append(r.render(cam, p))
    (ra, ha, sa), (rb, hb, sb) = res
    assert np.array_equal(ra.view(np.uint32), rb.view(np.uint32))
    assert np.array_equal(ha, hb)
    assert {k: v for k, v in sa.items() if k != "kernel_ms"} == \
        {k: v for k, v in sb.items() if k != "kernel_ms"}


@pytest.mark.parametrize("scene", ["terrain", "glass_cube", "refraction"])
@pytest.mark.parametrize("n", [16, 32, 64, 128])
def test_device_scene_builder_matches_host(built, scene, n):
    """vrt_build_scene_device (main.cpp:218-288 on the GPU) yields the same packed volume (voxel
    bytes + distance field) as uploading vrt_build_scene's host bytes, and the same frame."""
    with vrt.Renderer(0) as a, vrt.Renderer(0) as b:
        a.upload_volume(vrt.build_scene(scene, n), n)
        b.build_scene_device(scene, n)
        assert np.array_equal(a.debug_packed_volume(), b.debug_packed_volume())
        cam = vrt.make_camera(96, 54)
        p = vrt.default_params(4, 2)
        ra, _, _ = a.render(cam, p, want_hits=False)
        rb, _, _ = b.render(cam, p, want_hits=False)
        assert np.array_equal(ra.view(np.uint32), rb.view(np.uint32))


def test_device_scene_builder_512_terrain(built):
    with vrt.Renderer(0) as a, vrt.Renderer(0) as b:
        a.upload_volume(vrt.build_scene("terrain", 512), 512)
        b.build_scene_device("terrain", 512)
        assert np.array_equal(a.debug_packed_volume(), b.debug_packed_volume())
