"""The certified pass's ray set-up and walk start from the launch's host proofs (KArgs::setup: the constant w
column, the straight-line normalize, the uniform start cell; csrc/vrt_render.hip primary_ray<LEAN>,
csrc/vrt_cert.h cert_pixel<LEAN>) on cameras that set and cameras that clear each flag. The timed path (the
certified pass with the deferred exact pass forced, set_exact_pass(2): the DEFER instances run at these
frame sizes) must equal the exact STATS instance byte for byte: as a whole frame, as a 16-row block band,
as a two-frame batch of two different cameras (flags clear: the constants are the launch's) and of one
camera at two times (flags set in the frame-batch instance, the bench's case); colour-only with certified
trees off and forced, and textured with the reference atlas.
For each camera the expected flag state is asserted through the host's test hook first, so that a fallback
that always runs cannot pass for the fast form.
Frames 64x48 at 16^3 and 96x54 at 32^3: refraction, terrain (with its glass walls at 32^3), glass cube and
the adversarial material bytes volume. Certified trees are a colour-only mode, so textured launches run
with them off only. The CPU test's group of non-finite matrices stays on the host (its flags are asserted
through the hook there): such a frame's rays are all NaN and say nothing about the set-up."""
import numpy as np
import pytest

import voxelraytracer_amd as vrt
from adversarial_volumes import scene_volume
from harness import (ALL, K_CELL, K_LEN, K_W, assert_equal, band, batch, certified_mode, consts, ref_atlas,
                     reset_modes)

pytestmark = pytest.mark.gpu

CASES = (("refraction", 16, 64, 48), ("terrain", 32, 96, 54), ("glass_cube", 16, 64, 48), ("adversarial/bytes", 32, 96, 54))


def cameras(n, w, h):
    """(id, camera, expected flags). One camera from each group of tests/test_cert_launch_consts.py."""
    def edited(i, v, **kw):
        cam = vrt.make_camera(w, h, **kw)
        cam.inv_pv[i] = v
        return cam

    def scaled(f):
        cam = vrt.make_camera(w, h)
        for i in (0, 1, 2):
            for j in range(4):
                cam.inv_pv[4 * j + i] = float(np.float32(cam.inv_pv[4 * j + i]) * np.float32(f))
        return cam

    out = n / 2 + 3.0
    return (
        ("default", vrt.make_camera(w, h), ALL),
        ("inside", vrt.make_camera(w, h, pos=(1.37, -2.41, 0.58), rot=(-20.0, 140.0, 10.0)), ALL),
        # the lattice camera of tests/test_gpu_cert_start_lit.py: every ray moves down y from 0.01 below a plane
        ("straight_down", vrt.make_camera(w, h, pos=(0.5, 2.0, 0.5), rot=(-90.0, 0.0, 0.0)), ALL),
        ("lattice_axis", vrt.make_camera(w, h, pos=(0.0, 0.0, 0.0), rot=(0.0, 0.0, 0.0)), K_W | K_LEN),
        ("near_plane", vrt.make_camera(w, h, pos=(3.0005, 0.4, 0.61), rot=(0.0, 0.0, 0.0)), K_W | K_LEN),
        ("outside", vrt.make_camera(w, h, pos=(0.3, 0.4, out), rot=(0.0, 0.0, 0.0)), K_W | K_LEN),
        ("w_above", edited(3, 1e-6), 0),
        ("w_below", edited(3, 1e-8), ALL),
        ("scaled_short", scaled(1.0 / 64.0), K_W | K_CELL),
    )


def params(textured, **kw):
    p = vrt.default_params(4, 4, **kw)
    return vrt.textured_params(p, ref_atlas(), 128) if textured else p


def matrix_of(cam):
    return np.array(cam.inv_pv, np.float32)


@pytest.mark.parametrize("textured", (False, True), ids=("colour", "textured"))
@pytest.mark.parametrize("scene,n,w,h", CASES)
def test_timed_path_equals_exact_instance(built, scene, n, w, h, textured):
    cams = cameras(n, w, h)
    seen = 0
    for cid, cam, want in cams:  # the flag state the host reports for this launch
        k = consts(matrix_of(cam), n, w, h)
        assert k["setup"] == want, (cid, k["setup"], want)
        seen |= k["setup"] | ((ALL & ~k["setup"]) << 4)
    assert seen == ALL | (ALL << 4)  # every flag set by some camera and clear for another
    assert consts(matrix_of(cams[0][1]), n, w, h, m2=matrix_of(cams[1][1]))["setup"] == 0
    with vrt.Renderer(0) as r:
        r.upload_volume(scene_volume(scene, n), n)
        for i, (cid, cam, _) in enumerate(cams):
            p = params(textured)
            p2 = [params(textured, time=1.0), params(textured, time=2.0)]
            other = cams[(i + 1) % len(cams)][1]
            reset_modes(r)
            ref = band(r, cam, p, counters=True)
            ref2 = [band(r, cam, p2[0], counters=True), band(r, other, p2[1], counters=True),
                    band(r, cam, p2[1], counters=True)]
            for t in ((0,) if textured else (0, 2)):
                certified_mode(r, t)
                what = (scene, n, cid, textured, t)
                assert_equal(band(r, cam, p), ref, what + ("frame",))
                assert_equal(band(r, cam, p, row0=16, rows=16), ref[16:32], what + ("band",))
                if not textured:  # frame batches are colour-only launches
                    got = batch(r, [cam, other], p2)
                    assert_equal(got[0], ref2[0], what + ("batch", 0))
                    assert_equal(got[1], ref2[1], what + ("batch", 1))
                    got = batch(r, [cam, cam], p2)
                    assert_equal(got[0], ref2[0], what + ("same-camera batch", 0))
                    assert_equal(got[1], ref2[2], what + ("same-camera batch", 1))
