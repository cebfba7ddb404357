"""The reprojected temporal filter (GPU): vrt_reproject_temporal_async byte for byte against the NumPy float32
restatement (tests/reproject_reference.py), and vrt_render_frame_reprojected against vrt_render_frame (static
camera) and against the restatement composed frame by frame (moving camera). Volumes are 16^3, frames 96x54
or smaller; the oracle's primary rays of a camera are computed once and shared."""
import ctypes as C

import numpy as np
import pytest

import voxelraytracer_amd as vrt
from voxelraytracer_amd import abi

import reproject_reference as ref
from reproject_reference import H, N, SCENES, W

pytestmark = pytest.mark.gpu

ALPHA = 0.3
OUT_SENTINEL, SRC_SENTINEL = 0x5A5A5A5A, -77


def history(w=W, h=H, seed=11):
    """A seeded random RGBA8 frame with A = 255."""
    c = np.random.default_rng(seed).integers(0, 256, (h, w, 4), dtype=np.uint8)
    c[..., 3] = 255
    return c


def dev(a):
    import torch

    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def ids_words(ids):
    """[H, W] PIXEL_ID_DTYPE records as [H, 2 W] int32 words."""
    return np.ascontiguousarray(ids).view(np.int32).reshape(ids.shape[0], -1)


def run_whole(r, cam, p, prev_pv, raw, ids, depth, prev, prev_ids, alpha=ALPHA, stream=0):
    """One whole-frame call on packed buffers; returns (out [H, W, 4] uint8, src [H, W] int32)."""
    import torch

    h, w = ids.shape
    d_raw, d_ids, d_depth = dev(raw), dev(ids_words(ids)), dev(depth)
    d_prev = dev(prev) if prev is not None else None
    d_pids = dev(ids_words(prev_ids)) if prev_ids is not None else None
    d_out = torch.full((h, w), OUT_SENTINEL, dtype=torch.int32, device="cuda")
    d_src = torch.full((h, w), SRC_SENTINEL, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    r.reproject_temporal_async(cam, p, prev_pv, alpha, 0, h, w, d_raw.data_ptr(), d_ids.data_ptr(), d_depth.data_ptr(),
                               d_prev.data_ptr() if d_prev is not None else 0,
                               d_pids.data_ptr() if d_pids is not None else 0, w, d_out.data_ptr(), d_src.data_ptr(),
                               stream)
    torch.cuda.synchronize()
    return d_out.cpu().numpy().view(np.uint8).reshape(h, w, 4), d_src.cpu().numpy()


def assert_same(got_out, got_src, want_out, want_src, what=""):
    bad = np.argwhere(got_src != want_src)
    assert bad.size == 0, (what, "src", len(bad), bad[:5].tolist(), got_src[tuple(bad[:5].T)].tolist(),
                           want_src[tuple(bad[:5].T)].tolist())
    bad = np.argwhere(np.any(got_out != want_out, axis=-1))
    assert bad.size == 0, (what, "out", len(bad), bad[:5].tolist())


# ---- the primitive, bit for bit --------------------------------------------------------------------

@pytest.mark.parametrize("ray_noise", [0.0, 0.05])
@pytest.mark.parametrize("layout", [8, 1])
@pytest.mark.parametrize("name", SCENES)
def test_primitive_equals_the_restatement(built, name, layout, ray_noise):
    """Previous camera A, current camera A, B and C; ids and depth from render_ids, raw from render_frame at
    alpha 1, ray_noise passed through to the ID pass and the kernel alike: d_src and d_out equal the
    restatement at every pixel. The restatement is exact, so there is no tolerance."""
    p = ref.params(ray_noise)
    prev_rgb = history()
    pv_a = vrt.camera_forward(ref.camera("A"))
    seen = {}
    with vrt.Renderer(0) as r:
        r.set_skip_layout(layout)
        r.upload_volume(ref.scene(name), N)
        prev_ids, _ = r.render_ids(ref.camera("A"), p)
        for cur in ("A", "B", "C"):
            cam = ref.camera(cur)
            ids, depth = r.render_ids(cam, p)
            raw, _ = r.render_frame(cam, p, 1.0)
            out, src = run_whole(r, cam, p, pv_a, raw, ids, depth, prev_rgb, prev_ids)
            pos, dirs = ref.primary_rays(cur, ray_noise)
            want_out, want_src = ref.reproject(ids, depth, pos, dirs, N, pv_a, prev_ids, prev_rgb, raw, ALPHA)
            assert_same(out, src, want_out, want_src, (name, layout, ray_noise, cur))
            assert np.all(out[..., 3] == 255)
            seen[cur] = ref.counts(src)
            print(name, layout, ray_noise, "A->" + cur, seen[cur])
    if ray_noise == 0.0:
        assert seen["A"]["accepted"] == W * H
    if name != "glass_cube":
        assert seen["B"]["accepted"] > 0 and seen["B"][ref.OUTSIDE] > 0 and seen["B"][ref.MISMATCH] > 0
        assert seen["C"]["accepted"] > 0 and seen["C"][ref.BEHIND] > 0


def test_no_history(built):
    cam, p = ref.camera("B"), ref.params()
    with vrt.Renderer(0) as r:
        r.upload_volume(ref.scene("refraction"), N)
        ids, depth = r.render_ids(cam, p)
        raw, _ = r.render_frame(cam, p, 1.0)
        out, src = run_whole(r, cam, p, np.zeros(16, np.float32), raw, ids, depth, None, None)
    assert np.array_equal(out, raw) and np.all(src == ref.NO_HISTORY)


def test_edits_drop_history(built):
    """pick -> edit -> render: the material bytes of a small box under the centre pixel change, the camera
    stays: the box's pixels reject their history (-3, out = raw), every other pixel keeps its own."""
    cam, p = ref.camera("A"), ref.params()
    vox = ref.scene("terrain").copy()
    prev_rgb = history()
    with vrt.Renderer(0) as r:
        r.upload_volume(vox, N)
        ids1, _ = r.render_ids(cam, p)
        assert ids1[H // 2, W // 2]["voxel_index"] >= 0
        i, j, k = (int(c[0]) for c in vrt.hit_cell(ids1[H // 2:H // 2 + 1, W // 2:W // 2 + 1], N))
        lo = [max(c - 1, 0) for c in (i, j, k)]
        hi = [min(c + 2, N) for c in (i, j, k)]
        box = vox.reshape(N, N, N)[lo[2]:hi[2], lo[1]:hi[1], lo[0]:hi[0]].copy()
        swap = np.array([0, 3, 2, 1], np.uint8)   # stone <-> grass: every cell keeps its emptiness
        assert box.max() <= 3
        r.update_volume(lo, swap[box])
        ids2, depth2 = r.render_ids(cam, p)
        raw2, _ = r.render_frame(cam, p, 1.0)
        out, src = run_whole(r, cam, p, vrt.camera_forward(cam), raw2, ids2, depth2, prev_rgb, ids1)
    assert np.array_equal(ids1["voxel_index"], ids2["voxel_index"])
    ci, cj, ck = vrt.hit_cell(ids2, N)
    hit = ids2["voxel_index"].reshape(-1) >= 0
    inbox = hit & (ci >= lo[0]) & (ci < hi[0]) & (cj >= lo[1]) & (cj < hi[1]) & (ck >= lo[2]) & (ck < hi[2])
    changed = inbox & ((ids1["face"].reshape(-1) >> 8) != 2)   # (glass keeps its byte under the swap)
    changed = changed.reshape(H, W)
    assert changed[H // 2, W // 2] and 0 < np.count_nonzero(changed) < W * H
    own = np.arange(W * H, dtype=np.int32).reshape(H, W)
    assert np.all(src[changed] == ref.MISMATCH) and np.array_equal(out[changed], raw2[changed])
    assert np.array_equal(src[~changed], own[~changed])
    want = ref.reproject(ids2, depth2, *ref.primary_rays("A"), N, vrt.camera_forward(cam), ids1, prev_rgb, raw2, ALPHA)
    assert_same(out, src, *want, "edit")


# ---- bands, pitches, streams, shapes ---------------------------------------------------------------

def test_band_with_pitches_on_a_torch_stream(built):
    import torch

    cam, p = ref.camera("B"), ref.params(0.05)
    row0, rows, pitch, ppitch = 5, 24, W + 7, W + 3
    prev_rgb = history()
    pv_a = vrt.camera_forward(ref.camera("A"))
    with vrt.Renderer(0) as r:
        r.upload_volume(ref.scene("terrain"), N)
        prev_ids, _ = r.render_ids(ref.camera("A"), p)
        ids, depth = r.render_ids(cam, p)
        raw, _ = r.render_frame(cam, p, 1.0)
        whole_out, whole_src = run_whole(r, cam, p, pv_a, raw, ids, depth, prev_rgb, prev_ids)

        def band(a, fill, width=1):   # rows of the band at `pitch`, the padding filled
            b = np.full((rows, pitch * width), fill, a.dtype)
            b[:, :W * width] = a[row0:row0 + rows].reshape(rows, -1)
            return b

        def pitched(a, fill, width=1):   # the whole previous frame at `ppitch`
            b = np.full((H, ppitch * width), fill, a.dtype)
            b[:, :W * width] = a.reshape(H, -1)
            return b

        s = torch.cuda.Stream()
        with torch.cuda.stream(s):
            d_raw = dev(band(raw.view(np.int32).reshape(H, W), 0))
            d_ids = dev(band(ids_words(ids), -9, 2))
            d_depth = dev(band(depth, np.float32(np.nan)))
            d_prev = dev(pitched(prev_rgb.view(np.int32).reshape(H, W), 0))
            d_pids = dev(pitched(ids_words(prev_ids), -9, 2))
            # one sentinel row before the band and one after it
            d_out = torch.full(((rows + 2), pitch), OUT_SENTINEL, dtype=torch.int32, device="cuda")
            d_src = torch.full(((rows + 2), pitch), SRC_SENTINEL, dtype=torch.int32, device="cuda")
            r.reproject_temporal_async(cam, p, pv_a, ALPHA, row0, rows, pitch, d_raw.data_ptr(), d_ids.data_ptr(),
                                       d_depth.data_ptr(), d_prev.data_ptr(), d_pids.data_ptr(), ppitch,
                                       d_out.data_ptr() + pitch * 4, d_src.data_ptr() + pitch * 4, s.cuda_stream)
            # rows == 0: success, nothing written
            z_out = torch.full((pitch,), OUT_SENTINEL, dtype=torch.int32, device="cuda")
            r.reproject_temporal_async(cam, p, pv_a, ALPHA, row0, 0, pitch, d_raw.data_ptr(), d_ids.data_ptr(),
                                       d_depth.data_ptr(), d_prev.data_ptr(), d_pids.data_ptr(), ppitch,
                                       z_out.data_ptr(), 0, s.cuda_stream)
        s.synchronize()
    out, src = d_out.cpu().numpy(), d_src.cpu().numpy()
    assert np.array_equal(out[1:rows + 1, :W].copy().view(np.uint8).reshape(rows, W, 4), whole_out[row0:row0 + rows])
    assert np.array_equal(src[1:rows + 1, :W], whole_src[row0:row0 + rows])
    for untouched in (out[0], out[rows + 1], out[:, W:]):
        assert np.all(untouched == OUT_SENTINEL)
    for untouched in (src[0], src[rows + 1], src[:, W:]):
        assert np.all(untouched == SRC_SENTINEL)
    assert np.all(z_out.cpu().numpy() == OUT_SENTINEL)


@pytest.mark.parametrize("w,h", [(37, 19), (16, 8)])
def test_frame_shapes(built, w, h):
    """Sizes that are no multiple of the 16x16 tile, and one smaller than a tile's row of waves."""
    p = ref.params()
    prev_rgb = history(w, h)
    cam_a, cam_b = ref.camera("A", w, h), ref.camera("B", w, h)
    pv_a = vrt.camera_forward(cam_a)
    with vrt.Renderer(0) as r:
        r.upload_volume(ref.scene("refraction"), N)
        prev_ids, _ = r.render_ids(cam_a, p)
        ids, depth = r.render_ids(cam_b, p)
        raw, _ = r.render_frame(cam_b, p, 1.0)
        out, src = run_whole(r, cam_b, p, pv_a, raw, ids, depth, prev_rgb, prev_ids)
    pos, dirs = ref.primary_rays("B", 0.0, 1.0, w, h)
    want = ref.reproject(ids, depth, pos, dirs, N, pv_a, prev_ids, prev_rgb, raw, ALPHA)
    assert_same(out, src, *want, (w, h))
    assert np.count_nonzero(src >= 0) > 0


def test_call_is_capturable(built):
    """One call is one kernel launch without allocation: captured into a graph like the ID pass
    (tests/test_gpu_render_ids.py::test_async_pass_is_capturable), every replay writes the same bytes."""
    import torch

    cam, p = ref.camera("B"), ref.params()
    prev_rgb = history()
    pv_a = vrt.camera_forward(ref.camera("A"))
    with vrt.Renderer(0) as r:
        r.upload_volume(ref.scene("refraction"), N)
        prev_ids, _ = r.render_ids(ref.camera("A"), p)
        ids, depth = r.render_ids(cam, p)
        raw, _ = r.render_frame(cam, p, 1.0)
        want_out, want_src = run_whole(r, cam, p, pv_a, raw, ids, depth, prev_rgb, prev_ids)
        d_raw, d_ids, d_depth = dev(raw), dev(ids_words(ids)), dev(depth)
        d_prev, d_pids = dev(prev_rgb), dev(ids_words(prev_ids))
        d_out = torch.zeros((H, W), dtype=torch.int32, device="cuda")
        d_src = torch.zeros((H, W), dtype=torch.int32, device="cuda")

        def call(stream):
            r.reproject_temporal_async(cam, p, pv_a, ALPHA, 0, H, W, d_raw.data_ptr(), d_ids.data_ptr(),
                                       d_depth.data_ptr(), d_prev.data_ptr(), d_pids.data_ptr(), W, d_out.data_ptr(),
                                       d_src.data_ptr(), stream)

        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):   # warm the stream outside the capture
            call(s.cuda_stream)
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            call(torch.cuda.current_stream().cuda_stream)
        for _ in range(3):
            d_out.fill_(OUT_SENTINEL)
            d_src.fill_(SRC_SENTINEL)
            g.replay()
            torch.cuda.synchronize()
            assert np.array_equal(d_out.cpu().numpy().view(np.uint8).reshape(H, W, 4), want_out)
            assert np.array_equal(d_src.cpu().numpy(), want_src)


# ---- the synchronous frame loop --------------------------------------------------------------------

@pytest.mark.parametrize("name", SCENES)
def test_frame_loop_with_a_static_camera_is_the_plain_filter(built, name):
    """Five frames with u_Time advancing, ray_noise 0 and reflection_noise 0.05: with an unmoved camera every
    pixel fetches its own history (tests/test_reproject_cpu.py), so the loop is vrt_render_frame's filter.
    The two loops start differently: the reprojected loop's first frame has no history and is the raw frame,
    vrt_render_frame's first frame blends with black. The comparison therefore gives vrt_render_frame the
    same start, its first frame at u_Alpha = 1 (the raw frame, which becomes its history), and then
    compares all five frames byte for byte, frames 2-5 at alpha 0.3 on both sides. A third Renderer runs all
    five frames at alpha 0.3 with vrt_history_reset after the first (the raw frame becomes the history): its
    frames 2-5 are the same bytes again."""
    cam = ref.camera("A")
    with vrt.Renderer(0) as r, vrt.Renderer(0) as plain, vrt.Renderer(0) as keyf:
        for q in (r, plain, keyf):
            q.upload_volume(ref.scene(name), N)
        for f in range(5):
            p = ref.params(0.0, float(f + 1), reflection_noise=0.05)
            got = r.render_frame_reprojected(cam, p, ALPHA)
            want, _ = plain.render_frame(cam, p, 1.0 if f == 0 else ALPHA)
            bad = np.argwhere(np.any(got != want, axis=-1))
            assert bad.size == 0, (name, f, len(bad), bad[:5].tolist())
            also, _ = keyf.render_frame(cam, p, ALPHA)
            if f == 0:
                keyf.history_reset()
            else:
                assert np.array_equal(got, also), (name, f)


@pytest.mark.parametrize("name", ["terrain", "refraction"])
def test_frame_loop_with_a_moving_camera(built, name):
    """Frames along A, B, A, C with ray_noise 0.05 in the colour pass only: each equals the restatement
    composed from the previous output, the previous noise-free IDs, camera_forward(previous camera) and this
    frame's raw frame, noise-free IDs and depth."""
    prev_out = prev_ids = prev_cam = None
    with vrt.Renderer(0) as r, vrt.Renderer(0) as parts:
        r.upload_volume(ref.scene(name), N)
        parts.upload_volume(ref.scene(name), N)
        for f, cn in enumerate("ABAC"):
            cam, t = ref.camera(cn), float(f + 1)
            p, geom = ref.params(0.05, t), ref.params(0.0, t)
            got, ms = r.render_frame_reprojected(cam, p, ALPHA, timing=True)
            assert ms > 0.0
            raw, _ = parts.render_frame(cam, p, 1.0)
            ids, depth = parts.render_ids(cam, geom)
            pos, dirs = ref.primary_rays(cn, 0.0, t)
            want, src = ref.reproject(ids, depth, pos, dirs, N,
                                      vrt.camera_forward(prev_cam) if prev_cam is not None else np.zeros(16),
                                      prev_ids, prev_out, raw, ALPHA)
            bad = np.argwhere(np.any(got != want, axis=-1))
            assert bad.size == 0, (name, f, cn, len(bad), bad[:5].tolist())
            print(name, f, cn, ref.counts(src))
            if f > 0:
                assert 0 < np.count_nonzero(src >= 0) < W * H
            prev_out, prev_ids, prev_cam = got, ids, cam


def test_resets_and_the_plain_history(built):
    """After reprojected_history_reset and after a change of the image size the next frame is raw; the
    reprojected calls do not disturb render_frame's history; counters are unsupported."""
    cam, small = ref.camera("A"), ref.camera("A", 37, 19)
    # the sun moves from frame to frame, so that every frame differs from its history
    ps = [ref.params(0.0, float(t), sun_dir=vrt.sun_dir(40.0 + t)) for t in range(1, 8)]
    with vrt.Renderer(0) as r, vrt.Renderer(0) as plain:
        r.upload_volume(ref.scene("refraction"), N)
        plain.upload_volume(ref.scene("refraction"), N)
        raws = [plain.render_frame(cam, q, 1.0)[0] for q in ps]
        raw_small = plain.render_frame(small, ps[4], 1.0)[0]
        f0 = r.render_frame_reprojected(cam, ps[0], ALPHA)
        f1 = r.render_frame_reprojected(cam, ps[1], ALPHA)
        assert np.array_equal(f0, raws[0]) and not np.array_equal(f1, raws[1])
        r.reprojected_history_reset()
        assert np.array_equal(r.render_frame_reprojected(cam, ps[2], ALPHA), raws[2])
        assert not np.array_equal(r.render_frame_reprojected(cam, ps[3], ALPHA), raws[3])
        assert np.array_equal(r.render_frame_reprojected(small, ps[4], ALPHA), raw_small)   # size change
        assert np.array_equal(r.render_frame_reprojected(cam, ps[5], ALPHA), raws[5])       # and back
        st = abi.Stats()
        st.request = abi.VRT_STATS_COUNTERS
        out = np.zeros((H, W, 4), np.uint8)
        assert r._lib.vrt_render_frame_reprojected(r._h, C.byref(cam), C.byref(ps[6]), ALPHA, out.ctypes.data,
                                                   C.byref(st)) == abi.VRT_ERR_UNSUPPORTED
        assert r._lib.vrt_render_frame_reprojected(r._h, C.byref(cam), C.byref(ps[6]), ALPHA, None,
                                                   None) == abi.VRT_ERR_INVALID
        assert not out.any()
    # render_frame's own history, with reprojected calls in between
    with vrt.Renderer(0) as r, vrt.Renderer(0) as plain:
        r.upload_volume(ref.scene("refraction"), N)
        plain.upload_volume(ref.scene("refraction"), N)
        for f in range(4):
            a, _ = r.render_frame(cam, ps[f], ALPHA)
            r.render_frame_reprojected(cam, ps[f + 1], ALPHA)
            b, _ = plain.render_frame(cam, ps[f], ALPHA)
            assert np.array_equal(a, b), f


def test_staging_grows_and_is_reused(built):
    """One renderer's frames of 16x8 twice, 96x54 twice and 16x8 twice: the staging's first allocation, its
    growth and the larger buffers reused. Every first frame of a size has no history (it is the raw frame);
    every second one is the frame a fresh renderer gives after the same two calls."""
    ps = [ref.params(0.0, float(t), sun_dir=vrt.sun_dir(40.0 + t)) for t in range(1, 7)]
    with vrt.Renderer(0) as r, vrt.Renderer(0) as plain:
        r.upload_volume(ref.scene("refraction"), N)
        plain.upload_volume(ref.scene("refraction"), N)
        for i, (w, h) in enumerate(((16, 8), (W, H), (16, 8))):
            cam, p0, p1 = ref.camera("A", w, h), ps[2 * i], ps[2 * i + 1]
            first = r.render_frame_reprojected(cam, p0, ALPHA)
            second = r.render_frame_reprojected(cam, p1, ALPHA)
            assert np.array_equal(first, plain.render_frame(cam, p0, 1.0)[0]), (w, h)
            assert not np.array_equal(second, plain.render_frame(cam, p1, 1.0)[0]), (w, h)
            with vrt.Renderer(0) as fresh:
                fresh.upload_volume(ref.scene("refraction"), N)
                fresh.render_frame_reprojected(cam, p0, ALPHA)
                assert np.array_equal(second, fresh.render_frame_reprojected(cam, p1, ALPHA)), (w, h)


# ---- errors, timing --------------------------------------------------------------------------------

def test_errors_leave_the_outputs_untouched(built):
    import torch

    cam, p = ref.camera("A"), ref.params()
    pv = vrt.camera_forward(cam)
    d_raw = torch.zeros((H * W + 2,), dtype=torch.int32, device="cuda")
    d_ids = torch.zeros((H * W * 2 + 2,), dtype=torch.int32, device="cuda")
    d_depth = torch.ones((H * W + 2,), dtype=torch.float32, device="cuda")
    d_prev = torch.zeros((H * W + 2,), dtype=torch.int32, device="cuda")
    d_pids = torch.zeros((H * W * 2 + 2,), dtype=torch.int32, device="cuda")
    d_out = torch.full((H * W + 2,), OUT_SENTINEL, dtype=torch.int32, device="cuda")
    d_src = torch.full((H * W + 2,), SRC_SENTINEL, dtype=torch.int32, device="cuda")

    def bad_size(w, h):
        c = ref.camera("A")
        c.width, c.height = w, h
        return c

    with vrt.Renderer(0) as r:
        L, ctx = r._lib, r._h
        good = dict(cam=C.byref(cam), p=C.byref(p), pv=pv.ctypes.data, row0=0, rows=H, pitch=W, raw=d_raw.data_ptr(),
                    ids=d_ids.data_ptr(), depth=d_depth.data_ptr(), prev=d_prev.data_ptr(), pids=d_pids.data_ptr(),
                    ppitch=W, out=d_out.data_ptr(), src=d_src.data_ptr())

        def a(**kw):
            g = dict(good, **kw)
            return L.vrt_reproject_temporal_async(ctx, g["cam"], g["p"], g["pv"], ALPHA, g["row0"], g["rows"],
                                                  g["pitch"], g["raw"], g["ids"], g["depth"], g["prev"], g["pids"],
                                                  g["ppitch"], g["out"], g["src"], None)

        assert a() == abi.VRT_ERR_NO_VOLUME
        r.upload_volume(ref.scene("terrain"), N)
        inv = abi.VRT_ERR_INVALID
        for name in ("cam", "p", "pv", "raw", "ids", "depth", "out"):
            assert a(**{name: None}) == inv, name
        for w, h in ((0, H), (W, 0), (-1, H), (40000, H), (W, 40000)):
            assert a(cam=C.byref(bad_size(w, h)), rows=1) == inv, (w, h)
        assert a(rows=-1) == inv and a(row0=-1, rows=1) == inv
        assert a(row0=H - 3, rows=4) == inv and a(row0=H, rows=1) == inv
        assert a(pitch=W - 1) == inv and a(pitch=0) == inv
        assert a(ppitch=W - 1) == inv and a(ppitch=0) == inv
        assert a(prev=None) == inv and a(pids=None) == inv   # exactly one of the two
        assert a(out=good["prev"]) == inv
        assert a(ids=good["ids"] + 4) == inv and a(pids=good["pids"] + 4) == inv
        for name in ("raw", "depth", "prev", "out", "src"):
            assert a(**{name: good[name] + 2}) == inv and a(**{name: good[name] + 1}) == inv, name
        assert L.vrt_reproject_temporal_async(None, good["cam"], good["p"], good["pv"], ALPHA, 0, H, W, good["raw"],
                                              good["ids"], good["depth"], good["prev"], good["pids"], W, good["out"],
                                              good["src"], None) == inv
        torch.cuda.synchronize()
        assert np.all(d_out.cpu().numpy() == OUT_SENTINEL) and np.all(d_src.cpu().numpy() == SRC_SENTINEL)
        # rows == 0 is a successful no-op; no history and no d_src are valid; the last row is a valid band
        assert a(rows=0) == abi.VRT_OK and a(row0=H, rows=0) == abi.VRT_OK
        torch.cuda.synchronize()
        assert np.all(d_out.cpu().numpy() == OUT_SENTINEL) and np.all(d_src.cpu().numpy() == SRC_SENTINEL)
        assert a(row0=H - 1, rows=1, prev=None, pids=None, src=None) == abi.VRT_OK
        torch.cuda.synchronize()
        got = d_out.cpu().numpy()
        assert np.all(got[:W] == 0) and np.all(got[W:] == OUT_SENTINEL)   # out = raw (zeros) in the band's row
        assert np.all(d_src.cpu().numpy() == SRC_SENTINEL)


def test_launch_timing_counts_one_launch(built):
    import torch

    cam, p = ref.camera("A"), ref.params()
    with vrt.Renderer(0) as r:
        r.upload_volume(ref.scene("terrain"), N)
        ids, depth = r.render_ids(cam, p)
        raw, _ = r.render_frame(cam, p, 1.0)
        r.set_launch_timing(2)
        run_whole(r, cam, p, vrt.camera_forward(cam), raw, ids, depth, history(), ids)
        total, launches = r.launch_timing()
        r.set_launch_timing(0)
        torch.cuda.synchronize()
    assert launches == 1 and total > 0.0
