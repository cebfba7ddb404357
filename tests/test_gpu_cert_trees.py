"""GPU: certified bounce trees (vrt_set_cert_trees, ABI v15) in the certified pass's tree instance,
with the deferred exact pass (vrt_set_exact_pass 2) and in lane: a glass pixel's tree
(voxel.glsl:425-452) walked ray by ray with certified walks, trees that cannot be certified
rendered by the exact path. Frames must be bit-identical to the exact STATS instance, frame after
frame (temporal history read at alpha 0.5), on glass-heavy volumes at full size, bands with row
steps, frame batches, noise (every tree then takes the exact path), lattice cameras (ties; exact
march continuations after in-volume refraction that start on or just before a lattice plane) and
the modes toggled between frames on one stream."""
import numpy as np
import pytest
import torch

import voxelraytracer_amd as vrt
from harness import band, batch, current_stream, frames
from voxelraytracer_amd.tiles import block_band_spec

pytestmark = pytest.mark.gpu


def glass_volume(n, seed):
    rng = np.random.default_rng(seed)
    vox = np.zeros((n, n, n), np.uint8)
    m = rng.random((n, n, n)) < 0.04
    vox[m] = rng.choice(np.array([2, 2, 2, 1, 3], np.uint8), size=int(m.sum()))
    vox[n // 4: n // 2, n // 4: n // 2, n // 4: n // 2] = 2
    vox[:, :2, :] = 1
    return vox.reshape(-1)


CASES = [
    # scene, n, w, h, R, T, row0, rows, step, noise
    ("glass_cube", 128, 1920, 1080, 1, 2, 0, 1080, 1, {}),
    ("glass_cube", 128, 1920, 1080, 4, 4, 0, 1080, 1, {}),
    ("glass_cube", 64, 640, 360, 2, 6, 3, 90, 4, {}),
    ("glass", 64, 480, 270, 4, 4, 0, 270, 1, {}),
    ("glass", 32, 320, 200, 3, 5, 1, 67, 3, {}),
    ("glass_cube", 64, 320, 180, 1, 2, 0, 180, 1, dict(refraction_noise=0.01)),
    ("refraction", 128, 480, 270, 4, 4, 0, 270, 1, {}),
]


@pytest.mark.parametrize("case", CASES, ids=[f"{c[0]}{c[1]}_{c[2]}x{c[3]}_{c[4]}{c[5]}_s{c[8]}" for c in CASES])
def test_cert_trees_are_bit_identical(built, case):
    scene, n, w, h, R, T, row0, rows, step, kw = case
    vox = glass_volume(n, n) if scene == "glass" else vrt.build_scene(scene, n)
    with vrt.Renderer(0) as r:
        r.upload_volume(vox, n)
        r.set_certified(1)
        r.set_cert_trees(2)
        r.set_exact_pass(2)   # deferred at any size
        cam = vrt.make_camera(w, h)
        a = frames(r, cam, 2, R, T, 0.5, row0, rows, step, **kw)
        r.set_exact_pass(0)
        b = frames(r, cam, 2, R, T, 0.5, row0, rows, step, **kw)
        ref = frames(r, cam, 2, R, T, 0.5, row0, rows, step, counters=True, **kw)
    for k in range(2):
        assert np.array_equal(a[k], ref[k]), f"deferred, frame {k}: {int(np.any(a[k] != ref[k], -1).sum())} px"
        assert np.array_equal(b[k], ref[k]), f"in lane, frame {k}"


@pytest.mark.parametrize("trees", [2, 0])
def test_cert_trees_lattice_cameras(built, trees):
    """Cameras on lattice points and diagonals: many trees start on ties and take the exact path,
    whose march continuations into air after an in-volume refraction are certified walks. At (1, 2,
    -3) one pixel's continuation started 8e-6 before the glass cube's face plane x = 63, so the
    exact walk sampled the face voxel (63, 8, 25) at a y crossing 3.7e-6 after the start, which
    the certified continuation, started beyond the plane, did not see (every certified mode
    differed in that pixel until cert_continuation checked that layer)."""
    n, w, h = 64, 320, 180
    with vrt.Renderer(0) as r:
        r.upload_volume(vrt.build_scene("glass_cube", n), n)
        r.set_certified(1)
        r.set_cert_trees(trees)
        for ep in (2, 0):
            r.set_exact_pass(ep)
            for pos, rot in [((0.0, 0.0, 0.0), (-45.0, -45.0, 0.0)), ((1.0, 2.0, -3.0), (0.0, 0.0, 0.0)),
                             ((-2.5, 0.5, 1.5), (-35.26439, 45.0, 0.0)), ((0.5, 0.5, -40.0), (0.0, 0.0, 0.0)),
                             ((3.0, -1.0, -7.0), (0.0, 90.0, 0.0)), ((0.0, 0.0, -20.0), (-45.0, 0.0, 0.0))]:
                cam = vrt.make_camera(w, h, pos=pos, rot=rot)
                a = frames(r, cam, 1, 4, 4, 1.0, 0, h, 1)
                ref = frames(r, cam, 1, 4, 4, 1.0, 0, h, 1, counters=True)
                bad = np.argwhere(np.any(a[0] != ref[0], axis=-1))
                assert bad.size == 0, (pos, rot, ep, bad[:5].tolist())


def test_cert_trees_toggled_between_frames(built):
    """Trees and the exact pass switched on and off between frames on one stream."""
    n, w, h = 64, 480, 270
    with vrt.Renderer(0) as r:
        r.upload_volume(vrt.build_scene("glass_cube", n), n)
        r.set_certified(1)
        r.set_exact_pass(2)
        cam = vrt.make_camera(w, h)
        hist = torch.zeros((h, w, 4), dtype=torch.uint8, device="cuda")
        ref = torch.zeros_like(hist)
        cnt = torch.zeros(len(vrt.COUNTER_NAMES), dtype=torch.int64, device="cuda")
        s = current_stream()
        for t, (trees, ep) in enumerate([(2, 2), (1, 2), (2, 2), (0, 2), (2, 2), (2, 0), (2, 2),
                                         (2, 2), (0, 0), (2, 2)]):
            p = vrt.default_params(4, 4, time=float(t + 1))
            r.set_cert_trees(trees)
            r.set_exact_pass(ep)
            r.render_temporal_rows_async(cam, p, 0.5, 0, h, 1, hist.data_ptr(), hist.data_ptr(), stream=s)
            r.render_temporal_rows_async(cam, p, 0.5, 0, h, 1, ref.data_ptr(), ref.data_ptr(),
                                         d_counters=cnt.data_ptr(), stream=s)
            torch.cuda.synchronize()
            assert torch.equal(hist, ref), f"frame {t}"


@pytest.mark.parametrize("ranks,rank,nf", [(1, 0, 3), (8, 3, 8)])
def test_cert_trees_frame_batches(built, ranks, rank, nf):
    """Frame batches (one launch, up to 8 frames: their own cameras and times) with certified
    trees equal one launch per frame."""
    w, h, n = 640, 360, 64
    block = 16 if ranks > 1 else 1
    row0, rows, step = block_band_spec(rank, ranks, h, block) if ranks > 1 else (0, h, 1)
    cams = [vrt.make_camera(w, h, pos=(0.5 * f, 0.25 * f, -2.0), rot=(-10.0 + f, 20.0 + 2 * f, 0.0))
            for f in range(nf)]
    ps = [vrt.default_params(2, 4, time=float(f + 1)) for f in range(nf)]
    with vrt.Renderer(0) as r:
        r.upload_volume(vrt.build_scene("glass_cube", n), n)
        r.set_certified(1)
        r.set_cert_trees(2)
        r.set_exact_pass(2)
        ref = [band(r, cams[f], ps[f], row0, rows, step, block) for f in range(nf)]
        got = batch(r, cams, ps, row0, rows, step, block)
    for f in range(nf):
        assert np.array_equal(got[f], ref[f]), f"frame {f}"


@pytest.mark.parametrize("scene,n,pos,rot,R,T", [
    ("terrain", 64, (1.0, 20.0, -22.0), (-90.0, 315.0, 0.0), 4, 4),
    ("glass_cube", 128, (0.0, 50.0, -44.0), (-90.0, 315.0, 0.0), 4, 4),
    ("refraction", 64, (0.0, 10.0, -8.5), (-90.0, 225.0, 0.0), 1, 2),
    ("glass_cube", 64, (1.0, 2.0, -3.0), (0.0, 0.0, 0.0), 4, 4),
])
def test_certified_start_slivers(built, scene, n, pos, rot, R, T):
    """The cameras scripts/lattice_stress.py found (HISTORY r06_s25-s34): straight-down views whose
    rays have a zero or 2e-8 component, so shadow and primary walks start on a lattice plane (a
    shadow from x = 33.0 going -x whose exact walk never sampled the solid cell the certified walk
    blamed; a ray along x = 64 reading plane N's GL_REPEAT copy for 170 units), and a march
    continuation started 8e-6 before a face plane. Every certified mode equals the exact instance."""
    w, h = 320, 180
    with vrt.Renderer(0) as r:
        r.upload_volume(vrt.build_scene(scene, n), n)
        cam = vrt.make_camera(w, h, pos=pos, rot=rot)
        ref = frames(r, cam, 1, R, T, 1.0, 0, h, 1, counters=True)
        for cert, trees, ep in ((1, 2, 2), (1, 2, 0), (1, 0, 2), (1, 0, 0), (0, 0, 0)):
            r.set_certified(cert)
            r.set_cert_trees(trees)
            r.set_exact_pass(ep)
            a = frames(r, cam, 1, R, T, 1.0, 0, h, 1)
            bad = np.argwhere(np.any(a[0] != ref[0], axis=-1))
            assert bad.size == 0, (cert, trees, ep, bad[:5].tolist())


@pytest.mark.parametrize("scene,n", [("glass_cube", 64), ("refraction", 64), ("terrain", 64)])
def test_lattice_camera_sample(built, scene, n):
    """A sample of scripts/lattice_stress.py (its full runs: 19 200 frames, HISTORY r06_s36): 40
    lattice-aligned cameras (integer / half-integer positions; axis, diagonal, (1,1,1) and
    straight-down views) per scene, every certified mode against the exact instance."""
    rng = np.random.default_rng(sum(map(ord, scene)) + n)
    pitches = [0.0, -45.0, 45.0, -35.26439, -90.0, 90.0, -30.0, -60.0, -89.99]
    yaws = [0.0, 45.0, 90.0, 135.0, 180.0, 225.0, 270.0, 315.0, 30.0, 60.0]
    w, h = 160, 90
    with vrt.Renderer(0) as r:
        r.upload_volume(vrt.build_scene(scene, n), n)
        r.set_certified(1)
        for k in range(40):
            pos = tuple(float(x) for x in np.round(rng.uniform(-n / 2.5, n / 2.5, 3) * 2) / 2)
            if k % 3 == 0:
                pos = tuple(float(round(x)) for x in pos)
            rot = (float(rng.choice(pitches)), float(rng.choice(yaws)), 0.0)
            R, T = [(4, 4), (1, 2), (2, 6)][k % 3]
            cam = vrt.make_camera(w, h, pos=pos, rot=rot)
            ref = frames(r, cam, 1, R, T, 1.0, 0, h, 1, counters=True)
            for trees, ep in ((2, 2), (2, 0), (0, 2), (0, 0)):
                r.set_cert_trees(trees)
                r.set_exact_pass(ep)
                a = frames(r, cam, 1, R, T, 1.0, 0, h, 1)
                bad = np.argwhere(np.any(a[0] != ref[0], axis=-1))
                assert bad.size == 0, (pos, rot, (R, T), trees, ep, bad[:3].tolist())


@pytest.mark.parametrize("scene,n,pos,rot,R,T", [
    ("refraction", 128, (-29.0, -44.5, 21.5), (-89.99, 225.0, 0.0), 1, 2),
    ("terrain", 64, (-21.0, 1.0, 16.0), (90.0, 0.0, 0.0), 4, 4),
])
def test_certified_shadow_open_cases(built, scene, n, pos, rot, R, T):
    """The two cameras of the 72 000-frame lattice stress (r06_s38) that differed, in one or two
    pixels, in every certified mode including exact primaries with certified shadows (set_certified
    0 on these glass-light volumes keeps certified shadow walks from exact hit points), until the
    shadow walk's one-flag hit was corrected (DESIGN.md §6 "Certified walks, ray by ray": the tie,
    the plane's copy and the second step's length; tests/test_gpu_cert_rays.py). Each camera was a
    strict expected failure until then; both render bit-identically now."""
    w, h = 320, 180
    with vrt.Renderer(0) as r:
        r.upload_volume(vrt.build_scene(scene, n), n)
        cam = vrt.make_camera(w, h, pos=pos, rot=rot)
        ref = frames(r, cam, 1, R, T, 1.0, 0, h, 1, counters=True)
        r.set_certified(1)
        a = frames(r, cam, 1, R, T, 1.0, 0, h, 1)
        r.set_certified(0)
        assert np.array_equal(a[0], ref[0])
