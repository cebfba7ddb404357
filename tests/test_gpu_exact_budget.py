"""GPU: the deferred exact pass after its register budget changed (the launch's arguments read late, the
deferred list's segment counters read per batch, the whole-frame instances under a VGPR cap). Each case
forces the deferred path, set_exact_pass(2), and compares the frames byte for byte with the exact STATS
instance's on the same history. The cases reach what changed: bounce stacks that grow past their LDS
bottom entry into scratch, up to the full stack (R + T = 16) on the glass-clutter volume; the glass cube
at its default depths; the refraction scene; a frame batch (the FB instances, whose entries carry their
frame); and a textured frame (the textured whole-frame instance). Those colour bands are under four
rounds of waves, so their launches take the short-band instance, which shares the body; the last case
renders 1920x1080 frames, one launch each and three in a batch, which take the whole-frame instances
under the VGPR cap (exact_pass_kernel_capped, one-frame and frame-batch)."""
import numpy as np
import pytest

import voxelraytracer_amd as vrt
from harness import GOLDEN, assert_equal, band, batch, frames, load_golden

pytestmark = pytest.mark.gpu

N = 16


def golden(name):
    """(camera, params, volume bytes) of the fixture tests/golden/<name>*.npz."""
    _, _, cam, p, vox = load_golden(next(q for q in GOLDEN if name in q))
    return cam, p, vox


def clutter():
    """The glass-clutter adversarial volume, 16^3, and its fixture's 64x48 camera."""
    cam, _, vox = golden("adversarial_glass_clutter16_64x48")
    assert (cam.width, cam.height) == (64, 48), (cam.width, cam.height)
    return cam, vox


def deferred_and_stats(r, cam, R, T, n_frames=2, **kw):
    """n_frames at alpha 0.5 (the second frame reads the first as history): deferred, then STATS."""
    h = cam.height
    got = frames(r, cam, n_frames, R, T, 0.5, 0, h, 1, 2, **kw)
    ref = frames(r, cam, n_frames, R, T, 0.5, 0, h, 1, 2, counters=True, **kw)
    return got, ref


@pytest.mark.parametrize("R,T", [(4, 4), (4, 12)])
def test_glass_clutter_stacks_reach_scratch(built, R, T):
    """30 % glass beside glass: bounce trees as deep as the depth limits allow, so the stack holds more
    than its LDS bottom entry; (4, 12) is the largest stack a launch accepts."""
    cam, vox = clutter()
    with vrt.Renderer(0) as r:
        r.upload_volume(vox, N)
        r.set_certified(1)
        got, ref = deferred_and_stats(r, cam, R, T, reflection_noise=0.02)
    assert not np.array_equal(ref[0], np.zeros_like(ref[0]))
    for t in range(len(ref)):
        assert_equal(got[t], ref[t], f"glass clutter ({R}, {T}), frame {t}")


@pytest.mark.parametrize("scene,R,T", [("glass_cube", 1, 2), ("refraction", 4, 4)])
def test_built_scenes(built, scene, R, T):
    cam = vrt.make_camera(64, 64)
    with vrt.Renderer(0) as r:
        r.upload_volume(vrt.build_scene(scene, N), N)
        r.set_certified(1)
        got, ref = deferred_and_stats(r, cam, R, T)
    for t in range(len(ref)):
        assert_equal(got[t], ref[t], f"{scene}, frame {t}")


def test_frame_batch_of_glass_clutter(built):
    """Three frames, each with its own camera and time, in one frame-batch launch
    (render_temporal_batch_async): the FB instance decodes a deferred entry's frame for its ray, its time
    and its output buffer."""
    cam0, vox = clutter()
    # the fixture's pose, a generic pose inside the volume and one outside it
    cams = [cam0, vrt.make_camera(64, 48, pos=(0.3, -0.2, 0.1), rot=(10.0, 170.0, 0.0)),
            vrt.make_camera(64, 48, pos=(0.0, 0.0, N / 2 + 6.0), rot=(0.0, 0.0, 0.0))]
    ps = [vrt.default_params(4, 4, time=float(2 * f + 1), reflection_noise=0.02) for f in range(len(cams))]
    with vrt.Renderer(0) as r:
        r.upload_volume(vox, N)
        r.set_certified(1)
        r.set_exact_pass(2)
        ref = [band(r, cam, p, counters=True) for cam, p in zip(cams, ps)]
        got = batch(r, cams, ps, fill=7)
    assert not all(np.array_equal(ref[0], x) for x in ref[1:])
    for f in range(len(cams)):
        assert_equal(got[f], ref[f], f"batch frame {f}")


def test_whole_frames_take_the_capped_instances(built):
    """1920x1080 on refraction 128^3 (the benchmark's C3 shape): 16 200 two-wave tiles, more than four
    rounds of waves, so the deferred launch is not a short band. One frame per launch and the same three
    frames in one frame-batch launch, each against the STATS instance's frame."""
    n, w, h = 128, 1920, 1080
    cams = [vrt.make_camera(w, h, pos=(0.5 * f, 0.25 * f, -0.5 * f), rot=(-3.0 * f, 5.0 * f, 0.0)) for f in range(3)]
    ps = [vrt.default_params(4, 4, time=float(3 * f + 1), ray_noise=0.02) for f in range(3)]
    with vrt.Renderer(0) as r:
        r.upload_volume(vrt.build_scene("refraction", n), n)
        r.set_exact_pass(2)
        ref = [band(r, cam, p, counters=True) for cam, p in zip(cams, ps)]
        one = [band(r, cam, p) for cam, p in zip(cams, ps)]
        got = batch(r, cams, ps, fill=7)
    assert not all(np.array_equal(ref[0], x) for x in ref[1:])
    for f in range(3):
        assert_equal(one[f], ref[f], f"one-frame launch, frame {f}")
        assert_equal(got[f], ref[f], f"batch frame {f}")


def test_textured_glass_cube(built):
    """The fixture textured_ref_glass_cube16 (the reference's atlas): the textured whole-frame instance."""
    cam, p, vox = golden("textured_ref_glass_cube16")
    with vrt.Renderer(0) as r:
        r.upload_volume(vox, N)
        r.set_certified(1)
        r.set_exact_pass(2)
        got = band(r, cam, p)
        ref = band(r, cam, p, counters=True)
    assert_equal(got, ref, "textured_ref_glass_cube16")
