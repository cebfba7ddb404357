"""GPU: the certified pass's once-per-pixel cuts (csrc: the sun disc of a wave of primary misses away from the
sun, apply_sky_color<FAR>; the specular power of a colour-only primary hit by the bare log and exp, gpow_raw)
change no bit of a frame. The deferred pair is forced (set_certified(1), set_exact_pass(2): the DEFER instances
run at these frame sizes) and its RGBA8 and float frames must equal the exact STATS instance's, element for
element.

Volumes: the sparse material-byte volume of tests/adversarial_volumes.py at 16^3 and 32^3 (stone, grass and
glass hits beside many primary misses), from a camera outside it and one inside. Frames 96x64, 33x17 and 50x40
(widths that are no multiple of the 16-pixel tile, an odd height).
Suns, relative to the camera's view direction v: inside the view 30 degrees off v (the 0.75 threshold, 41
degrees from the sun, crosses the frame, so single waves mix pixels either side of it), behind the camera, below
the horizon (the sky factor is 0), straight along v, and one with a zero component (the generic lit term).
Launch shapes: frame sizes A, B, A on one context and then five more distinct sizes and A once more, a cyclic
band and a block-cyclic band, a frame batch of three cameras (the frame-batch instances carry the cuts too), and
frames in flight on the context's lanes. (The sizes and the lanes were chosen for per-frame-size NDC tables,
which were measured and not kept; they stay as cheap cases of the forced pair.)"""
import numpy as np
import pytest

import voxelraytracer_amd as vrt
from adversarial_volumes import camera_poses, volumes
from harness import (assert_equal, band, batch, certified_mode, current_stream, float_bits, hipcopy, reset_modes,
                     view_direction, words_to_bytes)

pytestmark = pytest.mark.gpu

SHAPES = ((96, 64), (33, 17), (50, 40))
CAMS = ("c4", "c3")   # outside the volume; a generic pose inside it


def unit(v):
    v = np.asarray(v, np.float64)
    return v / np.linalg.norm(v)


def suns(cam):
    v = unit(view_direction(cam))
    side = unit(np.cross(v, (0.0, 1.0, 0.0)) if abs(v[1]) < 0.9 else np.cross(v, (1.0, 0.0, 0.0)))
    a = np.radians(30.0)
    return {
        "in_view": tuple(np.cos(a) * v + np.sin(a) * side),
        "behind": tuple(-v),
        "below_horizon": (0.3, -0.9, 0.3),
        "straight_at": tuple(v),
        "zero_component": (0.0, 0.8, 0.6),
    }


def band_f32(r, cam, p, counters=False):
    """The whole frame as [H, W, 4] float32; counters: by the exact STATS instance."""
    import torch

    out = torch.zeros((cam.height, cam.width, 4), dtype=torch.float32, device="cuda")
    cnt = torch.zeros(len(vrt.COUNTER_NAMES), dtype=torch.int64, device="cuda")
    r.render_rows_async(cam, p, 0, cam.height, 1, out.data_ptr(), d_counters=cnt.data_ptr() if counters else 0,
                        stream=current_stream())
    torch.cuda.synchronize()
    return out.cpu().numpy()


def both_equal(r, cam, p, what):
    """RGBA8 and float frames of the forced deferred pair against the STATS instance's. -> the reference words"""
    reset_modes(r)
    ref, ref_f = band(r, cam, p, counters=True), band_f32(r, cam, p, counters=True)
    certified_mode(r, 0)
    assert_equal(band(r, cam, p), ref, what + ("rgba8",))
    assert_equal(float_bits(band_f32(r, cam, p)), float_bits(ref_f), what + ("float",))
    return ref


@pytest.mark.parametrize("n", (16, 32))
def test_suns(built, n):
    vox = volumes(n)["bytes"]
    with vrt.Renderer(0) as r:
        r.upload_volume(vox, n)
        for cid in CAMS:
            for w, h in SHAPES:
                cam = vrt.make_camera(w, h, **camera_poses(n)[cid])
                for sid, sun in suns(cam).items():
                    ref = both_equal(r, cam, vrt.default_params(4, 4, sun_dir=sun), (n, cid, (w, h), sid))
                    if (w, h) == SHAPES[0] and cid == "c4":   # the case is not empty: sky and lit faces both
                        assert len(np.unique(ref)) > 16, (n, cid, sid, len(np.unique(ref)))


@pytest.mark.parametrize("n", (16, 32))
def test_frame_sizes_on_one_context(built, n):
    """A, B, A, then five more sizes and A again; widths and heights both vary, and two sizes share a width."""
    vox = volumes(n)["bytes"]
    sizes = [(96, 64), (33, 17), (96, 64), (50, 40), (64, 48), (33, 33), (80, 24), (96, 40), (96, 64), (33, 17)]
    p = vrt.default_params(4, 4)
    with vrt.Renderer(0) as r:
        r.upload_volume(vox, n)
        for i, (w, h) in enumerate(sizes):
            cam = vrt.make_camera(w, h, **camera_poses(n)["c4"])
            both_equal(r, cam, p, (n, i, (w, h)))


@pytest.mark.parametrize("n", (16, 32))
def test_bands_and_batches(built, n):
    vox = volumes(n)["bytes"]
    with vrt.Renderer(0) as r:
        r.upload_volume(vox, n)
        for w, h in SHAPES:
            cams = [vrt.make_camera(w, h, **camera_poses(n)[cid]) for cid in ("c4", "c3", "c0")]
            p = vrt.default_params(4, 4, sun_dir=suns(cams[0])["in_view"])
            # a cyclic band (every third row from row 1) and a block-cyclic band (blocks of 4 rows, 8 apart, from row 4)
            for kw in (dict(row0=1, rows=(h - 1 + 2) // 3, step=3),
                       dict(row0=4, rows=4 * ((h - 8) // 8 + 1), step=8, block=4)):
                last = kw["row0"] + ((kw["rows"] - 1) // kw.get("block", 1)) * kw["step"] + (kw["rows"] - 1) % kw.get("block", 1)
                assert 0 < kw["rows"] and last < h, (kw, h)
                reset_modes(r)
                ref = band(r, cams[0], p, counters=True, **kw)
                certified_mode(r, 0)
                assert_equal(band(r, cams[0], p, **kw), ref, (n, (w, h), kw))
            # a frame batch of three cameras, whole frames and the cyclic band
            ps = [vrt.default_params(4, 4, sun_dir=suns(cams[0])["in_view"], time=float(t + 1)) for t in range(3)]
            for kw in (dict(), dict(row0=1, rows=(h - 1 + 2) // 3, step=3)):
                reset_modes(r)
                refs = [band(r, cams[f], ps[f], counters=True, **kw) for f in range(3)]
                certified_mode(r, 0)
                got = batch(r, cams, ps, **kw)
                for f in range(3):
                    assert_equal(got[f], refs[f], (n, (w, h), "batch", kw, f))


@pytest.mark.parametrize("n", (16, 32))
def test_frames_in_flight_on_the_lanes(built, n):
    """Six device-output frames back to back at u_Alpha = 1: they rotate over the context's lanes, each lane a
    stream of its own."""
    import torch

    vox = volumes(n)["bytes"]
    w, h = SHAPES[0]
    cam = vrt.make_camera(w, h, **camera_poses(n)["c4"])
    ps = [vrt.default_params(4, 4, sun_dir=suns(cam)["in_view"], time=float(t + 1)) for t in range(6)]
    with vrt.Renderer(0) as r:
        r.upload_volume(vox, n)
        reset_modes(r)
        refs = [words_to_bytes(band(r, cam, p, counters=True)) for p in ps]
        certified_mode(r, 0)
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        ptrs = [r.render_frame_device(cam, p, 1.0, s.cuda_stream)[0] for p in ps]
        torch.cuda.current_stream().wait_stream(s)
        for f in (2, 3, 4, 5):   # a frame stays valid for three more frames
            got = np.empty((h, w, 4), np.uint8)
            hipcopy(got, ptrs[f])
            assert_equal(got, refs[f], (n, "lane frame", f))
