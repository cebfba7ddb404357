"""The ID-guided spatial filter (GPU): vrt_spatial_filter_async byte for byte against the NumPy integer restatement
(tests/spatial_reference.py): d_out and d_count; vrt_spatial_filter against the composed restatement; and
vrt_render_frame_reprojected after vrt_set_reprojected_spatial against the restatement composed frame by frame.
The restatement is exact, so there is no tolerance anywhere. The layout follows tests/test_gpu_reproject_bilinear.py.
Volumes are 16^3, frames 96x54 or smaller."""
import itertools

import numpy as np
import pytest

import voxelraytracer_amd as vrt
from voxelraytracer_amd import abi

import reproject_bilinear_reference as bil
import reproject_reference as ref
import spatial_reference as sp
from reproject_reference import H, N, W
from spatial_reference import FACE, PLANE

pytestmark = pytest.mark.gpu

ALPHA = 0.3
OUT_SENTINEL, COUNT_SENTINEL = 0x5A5A5A5A, 0xA5
STEPS = (1, 2, 4, 16)   # the three LDS-staged steps and a direct-gather step
OFF, DISPLAY, FILL = vrt.SPATIAL_OFF, vrt.SPATIAL_DISPLAY, vrt.SPATIAL_FILL


def dev(a):
    import torch

    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def ids_words(ids):
    """[H, W] PIXEL_ID_DTYPE records as [H, 2 W] int32 words."""
    return np.ascontiguousarray(ids).view(np.int32).reshape(ids.shape[0], -1)


def random_keep(h, w, seed):
    """A seeded random keep mask: about a third of the pixels kept, with various non-zero bytes."""
    g = np.random.default_rng(seed)
    return (g.integers(1, 256, (h, w)) * (g.random((h, w)) < 0.35)).astype(np.uint8)


def run_pass(r, img, ids, step, guide=FACE, rng=765, keep=None, stream=0, count=True):
    """One whole-frame call on packed buffers; returns (out [H, W, 4] uint8, count [H, W] uint8)."""
    import torch

    h, w = ids.shape
    d_in, d_ids = dev(img), dev(ids_words(ids))
    d_keep = dev(keep) if keep is not None else None
    d_out = torch.full((h, w), OUT_SENTINEL, dtype=torch.int32, device="cuda")
    d_count = torch.full((h, w), COUNT_SENTINEL, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    r.spatial_filter_async(w, h, w, step, guide, rng, 0, h, d_in.data_ptr(), d_ids.data_ptr(),
                           d_keep.data_ptr() if d_keep is not None else 0, d_out.data_ptr(),
                           d_count.data_ptr() if count else 0, stream)
    torch.cuda.synchronize()
    return d_out.cpu().numpy().view(np.uint8).reshape(h, w, 4), d_count.cpu().numpy()


def assert_same(got, want, what=""):
    """(out, count) against (out, count)."""
    bad = np.argwhere(got[1] != want[1])
    assert bad.size == 0, (what, "count", len(bad), bad[:5].tolist(), got[1][tuple(bad[:5].T)].tolist(),
                           want[1][tuple(bad[:5].T)].tolist())
    bad = np.argwhere(np.any(got[0] != want[0], axis=-1))
    assert bad.size == 0, (what, "out", len(bad), bad[:5].tolist(), got[0][tuple(bad[:5].T)].tolist(),
                           want[0][tuple(bad[:5].T)].tolist())


# ---- the pass, byte for byte -------------------------------------------------------------------------

@pytest.mark.parametrize("source", ["rendered", "random"])
@pytest.mark.parametrize("name,layout", [("terrain", 8), ("glass_cube", 8), ("refraction", 8), ("refraction", 1)])
def test_pass_equals_the_restatement(built, name, layout, source):
    """Both guides, steps 1, 2, 4 and 16, range 765 and 48, keep absent and a seeded random keep, on the context's
    own frame at noise 0.05 with its IDs, and on a seeded random frame: d_out and d_count equal the restatement."""
    cam, p = ref.camera("B"), ref.params(0.05, **sp.NOISE)
    seen = {"range": 0, "guide": 0, "alone": 0}
    with vrt.Renderer(0) as r:
        r.set_skip_layout(layout)
        r.upload_volume(ref.scene(name), N)
        ids, _ = r.render_ids(cam, p)
        img = r.render_frame(cam, p, 1.0)[0] if source == "rendered" else sp.random_frame(H, W, 31)
        keep = random_keep(H, W, 32)
        for guide, step, rng, kp in itertools.product((FACE, PLANE), STEPS, (765, 48), (None, keep)):
            got = run_pass(r, img, ids, step, guide, rng, kp)
            st = {}
            want = sp.spatial_pass(img, ids, step, guide, rng, kp, N, stats=st)
            assert_same(got, want, (name, layout, source, guide, step, rng, kp is not None))
            for k in seen:
                seen[k] += int(st[k].sum())
    print(name, layout, source, seen)
    assert min(seen.values()) > 0   # rejected by the guide, by the range, and pixels left alone, all occur


def test_without_a_count_buffer(built):
    cam, p = ref.camera("A"), ref.params(0.05)
    with vrt.Renderer(0) as r:
        r.upload_volume(ref.scene("terrain"), N)
        ids, _ = r.render_ids(cam, p)
        img = sp.random_frame(H, W, 33)
        for step in STEPS:
            out, count = run_pass(r, img, ids, step, PLANE, 100, random_keep(H, W, 34), count=False)
            assert np.array_equal(out, sp.spatial_pass(img, ids, step, PLANE, 100, random_keep(H, W, 34), N)[0])
            assert np.all(count == COUNT_SENTINEL)


@pytest.mark.parametrize("guide", [FACE, PLANE])
def test_host_chain_equals_the_composed_restatement(built, guide):
    cam, p = ref.camera("A"), ref.params(0.05, **sp.NOISE)
    with vrt.Renderer(0) as r:
        r.upload_volume(ref.scene("refraction"), N)
        ids, _ = r.render_ids(cam, ref.params())
        img, _ = r.render_frame(cam, p, 1.0)
        keep = random_keep(H, W, 35)
        assert np.array_equal(r.spatial_filter(img, ids, guide=guide), sp.chain(img, ids, 3, guide, 765, None, N))
        assert np.array_equal(r.spatial_filter(img, ids, 5, guide, 48, keep), sp.chain(img, ids, 5, guide, 48, keep, N))
        assert np.array_equal(r.spatial_filter(img, ids, 1, guide, 0), sp.chain(img, ids, 1, guide, 0, None, N))
        small = sp.random_frame(19, 37, 36)   # a smaller frame through the same staging
        sids, _ = r.render_ids(ref.camera("A", 37, 19), ref.params())
        assert np.array_equal(r.spatial_filter(small, sids, 3, guide), sp.chain(small, sids, 3, guide, 765, None, N))
        for bad in (dict(passes=0), dict(passes=6), dict(guide=2), dict(range=-1)):
            with pytest.raises(vrt.VrtError):
                r.spatial_filter(img, ids, **bad)


@pytest.mark.parametrize("w,h", [(37, 19), (16, 8), (5, 3)])
def test_frame_shapes(built, w, h):
    """Sizes that are no multiple of the 16x16 tile, one tile of two waves, and a frame smaller than a wave's tile,
    where most taps fall outside the image."""
    cam, p = ref.camera("B", w, h), ref.params()
    img = sp.random_frame(h, w, 37)
    keep = random_keep(h, w, 38)
    with vrt.Renderer(0) as r:
        r.upload_volume(ref.scene("refraction"), N)
        ids, _ = r.render_ids(cam, p)
        for guide, step, kp in itertools.product((FACE, PLANE), STEPS, (None, keep)):
            got = run_pass(r, img, ids, step, guide, 765, kp)
            assert_same(got, sp.spatial_pass(img, ids, step, guide, 765, kp, N), (w, h, guide, step, kp is not None))
    if (w, h) == (5, 3):   # tests/test_spatial_cpu.py::test_count_on_a_small_image, on the device
        with vrt.Renderer(0) as r:
            r.upload_volume(ref.scene("refraction"), N)
            one = sp.ids_from(np.zeros((3, 5)), 0)
            assert run_pass(r, img, one, 1)[1].tolist() == [[9, 12, 15, 12, 9]] * 3
            assert run_pass(r, img, one, 4)[1].tolist() == [[2, 1, 1, 1, 2]] * 3


@pytest.mark.parametrize("step", STEPS)
def test_pitched_band_on_a_torch_stream(built, step):
    """pitch = W + 7, row0 = 5, rows = 20, d_keep and d_count at odd addresses: the band equals the whole-frame
    call's rows, and every byte outside the band is unchanged."""
    import torch

    cam, p = ref.camera("B"), ref.params(0.05)
    row0, rows, pitch = 5, 20, W + 7
    img = sp.random_frame(H, W, 39)
    keep = random_keep(H, W, 40)
    with vrt.Renderer(0) as r:
        r.upload_volume(ref.scene("terrain"), N)
        ids, _ = r.render_ids(cam, p)
        want = sp.spatial_pass(img, ids, step, PLANE, 90, keep, N)

        def pitched(a, fill, width=1):   # the whole frame at `pitch`, the padding filled
            b = np.full((H, pitch * width), fill, a.dtype)
            b[:, :W * width] = a.reshape(H, -1)
            return b

        s = torch.cuda.Stream()
        with torch.cuda.stream(s):
            d_in = dev(pitched(img.view(np.int32).reshape(H, W), 0x01020304))
            d_ids = dev(pitched(ids_words(ids), -9, 2))
            d_keep = dev(np.concatenate([[np.uint8(1)], pitched(keep, 1).reshape(-1)]))   # the mask from byte 1 on
            d_out = torch.full((H, pitch), OUT_SENTINEL, dtype=torch.int32, device="cuda")
            d_count = torch.full((H * pitch + 1,), COUNT_SENTINEL, dtype=torch.uint8, device="cuda")
            assert d_keep.data_ptr() % 2 == 0 and d_count.data_ptr() % 2 == 0
            r.spatial_filter_async(W, H, pitch, step, PLANE, 90, row0, rows, d_in.data_ptr(), d_ids.data_ptr(),
                                   d_keep.data_ptr() + 1, d_out.data_ptr(), d_count.data_ptr() + 1, s.cuda_stream)
            # rows == 0: success, nothing written
            r.spatial_filter_async(W, H, pitch, step, PLANE, 90, H, 0, d_in.data_ptr(), d_ids.data_ptr(), 0,
                                   d_out.data_ptr(), d_count.data_ptr(), s.cuda_stream)
        s.synchronize()
    out = d_out.cpu().numpy()
    count = d_count.cpu().numpy()
    assert count[0] == COUNT_SENTINEL
    count = count[1:].reshape(H, pitch)
    band = slice(row0, row0 + rows)
    assert np.array_equal(out[band, :W].copy().view(np.uint8).reshape(rows, W, 4), want[0][band])
    assert np.array_equal(count[band, :W], want[1][band])
    for buf, sentinel in ((out, OUT_SENTINEL), (count, COUNT_SENTINEL)):
        for untouched in (buf[:row0], buf[row0 + rows:], buf[:, W:]):
            assert np.all(untouched == np.array(sentinel).astype(buf.dtype))
    assert want[1][band].max() > 1 and (want[1][band] == 0).any()


def test_three_passes_are_capturable(built):
    """Three calls are three kernel launches without allocation (counted by the launch timing): captured into a
    graph and replayed three times, each time with another frame and keep mask in the same buffers: every replay
    writes what the eager calls write."""
    import torch

    cam, p = ref.camera("B"), ref.params()
    with vrt.Renderer(0) as r:
        r.upload_volume(ref.scene("refraction"), N)
        ids, _ = r.render_ids(cam, p)
        inputs = [(sp.random_frame(H, W, 41 + k), random_keep(H, W, 51 + k)) for k in range(3)]
        wants = [sp.chain(img, ids, 3, PLANE, 200, kp, N) for img, kp in inputs]
        d_ids = dev(ids_words(ids))
        d_a, d_keep = dev(inputs[0][0]), dev(inputs[0][1])
        d_b = torch.zeros((H, W), dtype=torch.int32, device="cuda")
        d_c = torch.zeros((H, W), dtype=torch.int32, device="cuda")
        d_out = torch.zeros((H, W), dtype=torch.int32, device="cuda")

        def calls(stream):   # a -> b -> c -> out at steps 1, 2, 4
            for q, (src, dst) in enumerate(((d_a, d_b), (d_b, d_c), (d_c, d_out))):
                r.spatial_filter_async(W, H, W, 1 << q, PLANE, 200, 0, H, src.data_ptr(), d_ids.data_ptr(),
                                       d_keep.data_ptr(), dst.data_ptr(), 0, stream)

        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        r.set_launch_timing(4)
        with torch.cuda.stream(s):   # warm the stream outside the capture
            calls(s.cuda_stream)
        torch.cuda.synchronize()
        total, launches = r.launch_timing()
        r.set_launch_timing(0)
        assert launches == 3 and total > 0.0
        assert np.array_equal(d_out.cpu().numpy().view(np.uint8).reshape(H, W, 4), wants[0])   # the eager bytes
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            calls(torch.cuda.current_stream().cuda_stream)
        for (img, kp), want in zip(inputs, wants):
            d_a.copy_(dev(img))
            d_keep.copy_(dev(kp))
            d_out.fill_(OUT_SENTINEL)
            torch.cuda.synchronize()
            g.replay()
            torch.cuda.synchronize()
            got = d_out.cpu().numpy().view(np.uint8).reshape(H, W, 4)
            bad = np.argwhere(np.any(got != want, axis=-1))
            assert bad.size == 0, ("replay", len(bad), bad[:5].tolist())
    assert not np.array_equal(wants[0], wants[1]) and not np.array_equal(wants[0], wants[2])


@pytest.mark.parametrize("step,count", [(1, True), (4, False), (8, True)])
def test_launch_timing_counts_one_launch(built, step, count):
    import torch

    cam, p = ref.camera("A"), ref.params()
    with vrt.Renderer(0) as r:
        r.upload_volume(ref.scene("terrain"), N)
        ids, _ = r.render_ids(cam, p)
        r.set_launch_timing(2)
        run_pass(r, sp.random_frame(H, W, 61), ids, step, count=count)
        total, launches = r.launch_timing()
        r.set_launch_timing(0)
        torch.cuda.synchronize()
    assert launches == 1 and total > 0.0


# ---- the synchronous frame loop --------------------------------------------------------------------

def loop_parts(parts, cn, t):
    """What a frame of the loop is made from, by a second context: the raw frame with ray_noise 0.05, and the
    noise-free IDs and depth."""
    cam = ref.camera(cn)
    raw, _ = parts.render_frame(cam, ref.params(0.05, t), 1.0)
    ids, depth = parts.render_ids(cam, ref.params(0.0, t))
    return raw, ids, depth


def test_loop_off_is_todays_loop(built):
    """With nothing set (context a), and after set_reprojected_spatial(SPATIAL_OFF, ...) with other passes, guide
    and range (context b), the frames along A, B, A, C equal each other byte for byte, and both are the loop as it
    was: the nearest temporal restatement composed frame by frame, with no spatial pass."""
    prev_out = prev_ids = prev_cam = None
    with vrt.Renderer(0) as a, vrt.Renderer(0) as b, vrt.Renderer(0) as parts:
        for q in (a, b, parts):
            q.upload_volume(ref.scene("refraction"), N)
        b.set_reprojected_spatial(OFF, 2, PLANE, 48)
        for f, cn in enumerate("ABAC"):
            t = float(f + 1)
            cam, p = ref.camera(cn), ref.params(0.05, t)
            fa, fb = a.render_frame_reprojected(cam, p, ALPHA), b.render_frame_reprojected(cam, p, ALPHA)
            assert np.array_equal(fa, fb), (f, cn)
            raw, ids, depth = loop_parts(parts, cn, t)
            pos, dirs = ref.primary_rays(cn, 0.0, t)
            pv = vrt.camera_forward(prev_cam) if prev_cam is not None else np.zeros(16, np.float32)
            want, _, _ = bil.nearest(ids, depth, pos, dirs, N, pv, prev_ids, prev_out, raw, ALPHA)
            assert np.array_equal(fa, want), (f, cn)
            prev_out, prev_ids, prev_cam = fa, ids, cam


@pytest.mark.parametrize("name,guide,passes", [("terrain", FACE, 3), ("refraction", PLANE, 2)])
def test_loop_display(built, name, guide, passes):
    """Along A, B, A, C each frame equals the restated passes applied to the lock-step OFF context's frame, with
    this frame's noise-free IDs and no keep mask: so the history chain is the OFF context's."""
    with vrt.Renderer(0) as r, vrt.Renderer(0) as off, vrt.Renderer(0) as parts:
        for q in (r, off, parts):
            q.upload_volume(ref.scene(name), N)
        r.set_reprojected_spatial(DISPLAY, passes, guide, 765)
        for f, cn in enumerate("ABAC"):
            t = float(f + 1)
            cam, p = ref.camera(cn), ref.params(0.05, t)
            got, ms = r.render_frame_reprojected(cam, p, ALPHA, timing=True)
            plain = off.render_frame_reprojected(cam, p, ALPHA)
            ids, _ = parts.render_ids(cam, ref.params(0.0, t))
            want = sp.chain(plain, ids, passes, guide, 765, None, N)
            bad = np.argwhere(np.any(got != want, axis=-1))
            assert bad.size == 0, (name, f, cn, len(bad), bad[:5].tolist())
            assert ms > 0.0 and not np.array_equal(got, plain)


@pytest.mark.parametrize("name,guide", [("terrain", FACE), ("refraction", PLANE)])
def test_loop_fill(built, name, guide):
    """Each frame equals the restatement composed from the previous RETURNED frame: the nearest temporal filter
    against it, then the passes with keep = the tap byte. From the second frame on there are kept and filled
    pixels, and the filled ones are exactly those with tap byte 0."""
    prev_out = prev_ids = prev_cam = None
    with vrt.Renderer(0) as r, vrt.Renderer(0) as parts:
        r.upload_volume(ref.scene(name), N)
        parts.upload_volume(ref.scene(name), N)
        r.set_reprojected_spatial(FILL, 3, guide, 765)
        for f, cn in enumerate("ABAC"):
            t = float(f + 1)
            got = r.render_frame_reprojected(ref.camera(cn), ref.params(0.05, t), ALPHA)
            raw, ids, depth = loop_parts(parts, cn, t)
            pos, dirs = ref.primary_rays(cn, 0.0, t)
            pv = vrt.camera_forward(prev_cam) if prev_cam is not None else np.zeros(16, np.float32)
            temporal, src, taps = bil.nearest(ids, depth, pos, dirs, N, pv, prev_ids, prev_out, raw, ALPHA)
            want, hist = sp.loop_frame(FILL, temporal, taps, ids, 3, guide, 765, N)
            bad = np.argwhere(np.any(got != want, axis=-1))
            assert bad.size == 0, (name, f, cn, len(bad), bad[:5].tolist())
            kept = taps != 0
            print(name, f, cn, "kept", int(kept.sum()), "filled", int((~kept).sum()))
            assert np.array_equal(got[kept], temporal[kept])
            if f == 0:
                assert not kept.any() and np.array_equal(got, sp.chain(raw, ids, 3, guide, 765, None, N))
            else:
                assert kept.any() and (~kept).any()
                # a filled pixel is its spatial estimate, which the count of the first pass tells from a copy
                _, count = sp.spatial_pass(temporal, ids, 1, guide, 765, taps, N)
                assert np.array_equal(count == 0, kept)
            prev_out, prev_ids, prev_cam = got, ids, ref.camera(cn)


def test_loop_switches_keep_the_history(built):
    """OFF, then FILL, then DISPLAY, then OFF on camera A, B, A, C: frame 2 is not a first frame (it has kept
    pixels), an unknown mode, guide or pass count in between is refused and changes nothing."""
    modes = (OFF, FILL, DISPLAY, OFF)
    prev_hist = prev_ids = prev_cam = None
    with vrt.Renderer(0) as r, vrt.Renderer(0) as parts:
        r.upload_volume(ref.scene("refraction"), N)
        parts.upload_volume(ref.scene("refraction"), N)
        for f, (cn, mode) in enumerate(zip("ABAC", modes)):
            t = float(f + 1)
            r.set_reprojected_spatial(mode, 2, PLANE, 300)
            for bad in ((3, 2, PLANE, 300), (-1, 2, PLANE, 300), (mode ^ 1, 0, PLANE, 300), (mode ^ 1, 6, PLANE, 300),
                        (mode ^ 1, 2, 2, 300), (mode ^ 1, 2, -1, 300), (mode ^ 1, 2, FACE, -1)):
                assert r._lib.vrt_set_reprojected_spatial(r._h, *bad) == abi.VRT_ERR_INVALID, bad
            got = r.render_frame_reprojected(ref.camera(cn), ref.params(0.05, t), ALPHA)
            raw, ids, depth = loop_parts(parts, cn, t)
            pos, dirs = ref.primary_rays(cn, 0.0, t)
            pv = vrt.camera_forward(prev_cam) if prev_cam is not None else np.zeros(16, np.float32)
            temporal, src, taps = bil.nearest(ids, depth, pos, dirs, N, pv, prev_ids, prev_hist, raw, ALPHA)
            want, hist = sp.loop_frame(mode, temporal, taps, ids, 2, PLANE, 300, N)
            assert np.array_equal(got, want), (f, cn, mode)
            if f > 0:
                assert np.count_nonzero(src >= 0) > 0
            prev_hist, prev_ids, prev_cam = hist, ids, ref.camera(cn)


def test_edited_voxels_are_filled(built):
    """FILL, the camera stays: the material bytes of a small box under the centre pixel change between two frames.
    The box's pixels find no history (tap byte 0), so they are filled, not kept; the frame equals the restatement."""
    cam = ref.camera("A")
    vox = ref.scene("terrain").copy()
    with vrt.Renderer(0) as r, vrt.Renderer(0) as parts:
        r.upload_volume(vox, N)
        parts.upload_volume(vox, N)
        r.set_reprojected_spatial(FILL, 3, FACE, 765)
        f1 = r.render_frame_reprojected(cam, ref.params(0.05, 1.0), ALPHA)
        _, ids1, _ = loop_parts(parts, "A", 1.0)
        assert ids1[H // 2, W // 2]["voxel_index"] >= 0
        i, j, k = (int(c[0]) for c in vrt.hit_cell(ids1[H // 2:H // 2 + 1, W // 2:W // 2 + 1], N))
        lo = [max(c - 1, 0) for c in (i, j, k)]
        hi = [min(c + 2, N) for c in (i, j, k)]
        box = vox.reshape(N, N, N)[lo[2]:hi[2], lo[1]:hi[1], lo[0]:hi[0]].copy()
        swap = np.array([0, 3, 2, 1], np.uint8)   # stone <-> grass: every cell keeps its emptiness
        assert box.max() <= 3
        for q in (r, parts):
            q.update_volume(lo, swap[box])
        got = r.render_frame_reprojected(cam, ref.params(0.05, 3.0), ALPHA)
        raw, ids2, depth2 = loop_parts(parts, "A", 3.0)
    changed = ids1["face"] != ids2["face"]
    assert changed[H // 2, W // 2] and 0 < np.count_nonzero(changed) < W * H
    pos, dirs = ref.primary_rays("A", 0.0, 3.0)
    temporal, src, taps = bil.nearest(ids2, depth2, pos, dirs, N, vrt.camera_forward(cam), ids1, f1, raw, ALPHA)
    assert not taps[changed].any() and taps[~changed].all()
    want, _ = sp.loop_frame(FILL, temporal, taps, ids2, 3, FACE, 765, N)
    assert np.array_equal(got, want)
    _, count = sp.spatial_pass(temporal, ids2, 1, FACE, 765, taps, N)
    assert np.all(count[changed] >= 1) and np.all(count[~changed] == 0)   # filled, and the others kept
    assert np.array_equal(got[~changed], temporal[~changed])


# ---- errors ------------------------------------------------------------------------------------------

def test_errors_leave_the_outputs_untouched(built):
    import torch

    d_in = torch.zeros((H * W + 2,), dtype=torch.int32, device="cuda")
    d_ids = torch.zeros((H * W * 2 + 2,), dtype=torch.int32, device="cuda")
    d_keep = torch.zeros((H * W + 2,), dtype=torch.uint8, device="cuda")
    d_out = torch.full((H * W + 2,), OUT_SENTINEL, dtype=torch.int32, device="cuda")
    d_count = torch.full((H * W + 2,), COUNT_SENTINEL, dtype=torch.uint8, device="cuda")

    def untouched():
        torch.cuda.synchronize()
        return np.all(d_out.cpu().numpy() == OUT_SENTINEL) and np.all(d_count.cpu().numpy() == COUNT_SENTINEL)

    with vrt.Renderer(0) as r:
        L, ctx = r._lib, r._h
        good = dict(w=W, h=H, pitch=W, step=1, guide=FACE, range=765, row0=0, rows=H, src=d_in.data_ptr(),
                    ids=d_ids.data_ptr(), keep=d_keep.data_ptr(), out=d_out.data_ptr(), count=d_count.data_ptr())

        def a(**kw):
            g = dict(good, **kw)
            return L.vrt_spatial_filter_async(ctx, g["w"], g["h"], g["pitch"], g["step"], g["guide"], g["range"], g["row0"],
                                              g["rows"], g["src"], g["ids"], g["keep"], g["out"], g["count"], None)

        assert a() == abi.VRT_ERR_NO_VOLUME and a(guide=PLANE) == abi.VRT_ERR_NO_VOLUME
        host = np.zeros((H, W, 4), np.uint8)
        with pytest.raises(vrt.VrtError) as e:
            r.spatial_filter(host, np.zeros((H, W), abi.PIXEL_ID_DTYPE))
        assert e.value.code == abi.VRT_ERR_NO_VOLUME
        r.upload_volume(ref.scene("terrain"), N)
        inv = abi.VRT_ERR_INVALID
        for guide in (FACE, PLANE):
            good["guide"] = guide
            for name in ("src", "ids", "out"):
                assert a(**{name: None}) == inv, name
            for w, h in ((0, H), (W, 0), (-1, H), (40000, H), (W, 40000)):
                assert a(w=w, h=h, pitch=max(w, W), rows=1) == inv, (w, h)
            assert a(pitch=W - 1) == inv and a(pitch=0) == inv
            assert a(rows=-1) == inv and a(row0=-1, rows=1) == inv
            assert a(row0=H - 3, rows=4) == inv and a(row0=H, rows=1) == inv
            assert a(step=0) == inv and a(step=65) == inv and a(step=-1) == inv
            assert a(range=-1) == inv
            assert a(out=good["src"]) == inv
            assert a(ids=good["ids"] + 4) == inv
            for name in ("src", "out"):
                assert a(**{name: good[name] + 2}) == inv and a(**{name: good[name] + 1}) == inv, name
        for guide in (2, -1):   # unknown guides, also on an empty band
            assert a(guide=guide) == inv and a(guide=guide, rows=0) == inv, guide
        assert b"guide" in L.vrt_last_error(ctx)
        assert L.vrt_spatial_filter_async(None, W, H, W, 1, FACE, 765, 0, H, good["src"], good["ids"], good["keep"],
                                          good["out"], good["count"], None) == inv
        assert untouched()
        # rows == 0 is a successful no-op; step 64 and range 0 are valid; no keep and no count are valid
        assert a(rows=0) == abi.VRT_OK and a(row0=H, rows=0) == abi.VRT_OK
        assert untouched()
        assert a(row0=H - 1, rows=1, step=64, range=0, keep=None, count=None) == abi.VRT_OK
        torch.cuda.synchronize()
        got = d_out.cpu().numpy()
        first = (H - 1) * W
        assert np.all(got[:first] == OUT_SENTINEL) and np.all(got[first + W:] == OUT_SENTINEL)
        assert np.all(got[first:first + W].view(np.uint32) == 0xFF000000)   # the mean of zeros, A = 255
        assert np.all(d_count.cpu().numpy() == COUNT_SENTINEL)
        # d_keep and d_count at odd addresses are valid
        assert a(row0=0, rows=1, keep=good["keep"] + 1, count=good["count"] + 1) == abi.VRT_OK
        torch.cuda.synchronize()
        c = d_count.cpu().numpy()
        assert c[0] == COUNT_SENTINEL and np.all(c[1:W + 1] >= 9) and np.all(c[W + 1:] == COUNT_SENTINEL)
