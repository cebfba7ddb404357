"""The fetch modes of the reprojected temporal filter (GPU): vrt_reproject_temporal_fetch_async byte for byte
against the NumPy float32 restatement (tests/reproject_bilinear_reference.py): d_out, d_src and d_taps, and
vrt_render_frame_reprojected after vrt_set_reprojected_fetch against the restatement composed frame by frame.
The layout follows tests/test_gpu_reproject.py. Volumes are 16^3, frames 96x54 or smaller; the oracle's primary
rays of a camera are computed once and shared (reproject_reference.oracle_frame's cache)."""
import ctypes as C

import numpy as np
import pytest

import voxelraytracer_amd as vrt
from voxelraytracer_amd import abi

import reproject_bilinear_reference as bil
import reproject_reference as ref
from reproject_reference import H, N, SCENES, W

pytestmark = pytest.mark.gpu

ALPHA = 0.3
OUT_SENTINEL, SRC_SENTINEL, TAP_SENTINEL = 0x5A5A5A5A, -77, 0xA5
NEAREST, BILINEAR = vrt.FETCH_NEAREST, vrt.FETCH_BILINEAR


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


def run_whole(r, fetch, cam, p, prev_pv, raw, ids, depth, prev, prev_ids, alpha=ALPHA, stream=0, taps=True):
    """One whole-frame call on packed buffers; returns (out [H, W, 4] uint8, src [H, W] int32, taps [H, W] uint8)."""
    import torch

    h, w = ids.shape
    d_raw, d_ids, d_depth = dev(raw), dev(ids_words(ids)), dev(depth)
    d_prev = dev(prev) if prev is not None else None
    d_pids = dev(ids_words(prev_ids)) if prev_ids is not None else None
    d_out = torch.full((h, w), OUT_SENTINEL, dtype=torch.int32, device="cuda")
    d_src = torch.full((h, w), SRC_SENTINEL, dtype=torch.int32, device="cuda")
    d_taps = torch.full((h, w), TAP_SENTINEL, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    r.reproject_temporal_fetch_async(cam, p, prev_pv, alpha, fetch, 0, h, w, d_raw.data_ptr(), d_ids.data_ptr(),
                                     d_depth.data_ptr(), d_prev.data_ptr() if d_prev is not None else 0,
                                     d_pids.data_ptr() if d_pids is not None else 0, w, d_out.data_ptr(),
                                     d_src.data_ptr(), d_taps.data_ptr() if taps else 0, stream)
    torch.cuda.synchronize()
    return d_out.cpu().numpy().view(np.uint8).reshape(h, w, 4), d_src.cpu().numpy(), d_taps.cpu().numpy()


def assert_same(got, want, what=""):
    """(out, src, taps) against (out, src, taps)."""
    for name, g, w in zip(("src", "taps"), got[1:], want[1:]):
        bad = np.argwhere(g != w)
        assert bad.size == 0, (what, name, len(bad), bad[:5].tolist(), g[tuple(bad[:5].T)].tolist(),
                               w[tuple(bad[:5].T)].tolist())
    bad = np.argwhere(np.any(got[0] != want[0], axis=-1))
    assert bad.size == 0, (what, "out", len(bad), bad[:5].tolist(), got[0][tuple(bad[:5].T)].tolist(),
                           want[0][tuple(bad[:5].T)].tolist())


# ---- the primitive, bit for bit --------------------------------------------------------------------

@pytest.mark.parametrize("ray_noise", [0.0, 0.05])
@pytest.mark.parametrize("name,layout", [(s, 8) for s in SCENES] + [("refraction", 1)])
def test_bilinear_equals_the_restatement(built, name, layout, ray_noise):
    """Previous camera A, current camera A, B and C; ids and depth from render_ids, raw from render_frame at
    alpha 1: d_out, d_src and d_taps equal the restatement at every pixel. The restatement is exact, so there
    is no tolerance."""
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
            got = run_whole(r, BILINEAR, cam, p, pv_a, raw, ids, depth, prev_rgb, prev_ids)
            pos, dirs = ref.primary_rays(cur, ray_noise)
            want = bil.bilinear(ids, depth, pos, dirs, N, pv_a, prev_ids, prev_rgb, raw, ALPHA)[:3]
            assert_same(got, want, (name, layout, ray_noise, cur))
            assert np.all(got[0][..., 3] == 255)
            seen[cur] = bil.counts(got[1], got[2])
            print(name, layout, ray_noise, "A->" + cur, seen[cur])
    if ray_noise == 0.0:
        assert seen["A"]["accepted"] == W * H
        assert seen["B"]["partial"] >= 100 and seen["C"]["partial"] >= 100   # tests/test_reproject_bilinear_cpu.py


@pytest.mark.parametrize("name", SCENES)
def test_nearest_through_the_new_entry_point(built, name):
    """VRT_FETCH_NEAREST: d_out and d_src are the old entry point's bytes on the same buffers, with and without
    d_taps (without: the same kernel), and d_taps = (src >= 0); all equal the restatement."""
    import torch

    p = ref.params(0.05)
    prev_rgb = history()
    pv_a = vrt.camera_forward(ref.camera("A"))
    with vrt.Renderer(0) as r:
        r.upload_volume(ref.scene(name), N)
        prev_ids, _ = r.render_ids(ref.camera("A"), p)
        for cur in ("A", "B", "C"):
            cam = ref.camera(cur)
            ids, depth = r.render_ids(cam, p)
            raw, _ = r.render_frame(cam, p, 1.0)
            d_raw, d_ids, d_depth = dev(raw), dev(ids_words(ids)), dev(depth)
            d_prev, d_pids = dev(prev_rgb), dev(ids_words(prev_ids))
            d_out = torch.full((3, H, W), OUT_SENTINEL, dtype=torch.int32, device="cuda")
            d_src = torch.full((3, H, W), SRC_SENTINEL, dtype=torch.int32, device="cuda")
            d_taps = torch.full((H, W), TAP_SENTINEL, dtype=torch.uint8, device="cuda")
            torch.cuda.synchronize()
            common = (d_raw.data_ptr(), d_ids.data_ptr(), d_depth.data_ptr(), d_prev.data_ptr(), d_pids.data_ptr(), W)
            r.reproject_temporal_async(cam, p, pv_a, ALPHA, 0, H, W, *common, d_out[0].data_ptr(), d_src[0].data_ptr())
            r.reproject_temporal_fetch_async(cam, p, pv_a, ALPHA, NEAREST, 0, H, W, *common, d_out[1].data_ptr(),
                                             d_src[1].data_ptr(), d_taps.data_ptr())
            r.reproject_temporal_fetch_async(cam, p, pv_a, ALPHA, NEAREST, 0, H, W, *common, d_out[2].data_ptr(),
                                             d_src[2].data_ptr(), 0)
            torch.cuda.synchronize()
            out, src, taps = d_out.cpu().numpy(), d_src.cpu().numpy(), d_taps.cpu().numpy()
            for k in (1, 2):
                assert np.array_equal(out[k], out[0]) and np.array_equal(src[k], src[0]), (name, cur, k)
            assert np.array_equal(taps, (src[0] >= 0).astype(np.uint8)), (name, cur)
            pos, dirs = ref.primary_rays(cur, 0.05)
            want = bil.nearest(ids, depth, pos, dirs, N, pv_a, prev_ids, prev_rgb, raw, ALPHA)
            assert_same((out[1].view(np.uint8).reshape(H, W, 4), src[1], taps), want, (name, cur))
            print(name, "A->" + cur, ref.counts(src[0]))


@pytest.mark.parametrize("fetch", [NEAREST, BILINEAR])
def test_no_history(built, fetch):
    cam, p = ref.camera("B"), ref.params()
    with vrt.Renderer(0) as r:
        r.upload_volume(ref.scene("refraction"), N)
        ids, depth = r.render_ids(cam, p)
        raw, _ = r.render_frame(cam, p, 1.0)
        out, src, taps = run_whole(r, fetch, cam, p, np.zeros(16, np.float32), raw, ids, depth, None, None)
    assert np.array_equal(out, raw) and np.all(src == bil.NO_HISTORY) and not taps.any()


def test_edits_drop_history(built):
    """tests/test_gpu_reproject.py::test_edits_drop_history with the bilinear fetch: the material bytes of a
    small box under the centre pixel change, the camera stays: the box's pixels find no tap with their record
    (-3, out = raw), everything equals the restatement, and a pixel next to the box keeps its history through
    the taps that do not show the box (a partial mask)."""
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
        got = run_whole(r, BILINEAR, cam, p, vrt.camera_forward(cam), raw2, ids2, depth2, prev_rgb, ids1)
    out, src, taps = got
    assert np.array_equal(ids1["voxel_index"], ids2["voxel_index"])
    ci, cj, ck = vrt.hit_cell(ids2, N)
    hit = ids2["voxel_index"].reshape(-1) >= 0
    inbox = hit & (ci >= lo[0]) & (ci < hi[0]) & (cj >= lo[1]) & (cj < hi[1]) & (ck >= lo[2]) & (ck < hi[2])
    changed = inbox & ((ids1["face"].reshape(-1) >> 8) != 2)   # (glass keeps its byte under the swap)
    changed = changed.reshape(H, W)
    assert changed[H // 2, W // 2] and 0 < np.count_nonzero(changed) < W * H
    assert np.all(src[changed] == bil.MISMATCH) and np.array_equal(out[changed], raw2[changed])
    assert not taps[changed].any()
    own = np.arange(W * H, dtype=np.int32).reshape(H, W)
    assert np.array_equal(src[~changed], own[~changed])
    want = bil.bilinear(ids2, depth2, *ref.primary_rays("A"), N, vrt.camera_forward(cam), ids1, prev_rgb, raw2, ALPHA)
    assert_same(got, want[:3], "edit")
    near = np.zeros_like(changed)   # the 8-neighbourhood of the changed pixels, without them
    for dy in (-1, 0, 1):
        for dx in (-1, 0, 1):
            near[max(dy, 0):H + min(dy, 0), max(dx, 0):W + min(dx, 0)] |= \
                changed[max(-dy, 0):H + min(-dy, 0), max(-dx, 0):W + min(-dx, 0)]
    near &= ~changed
    partial = near & (src >= 0) & (taps != 15)
    print("edit: changed", int(changed.sum()), "next to the box", int(near.sum()), "of them partial", int(partial.sum()))
    assert partial.any()


# ---- bands, pitches, streams, shapes ---------------------------------------------------------------

@pytest.mark.parametrize("fetch", [NEAREST, BILINEAR])
def test_band_with_pitches_on_a_torch_stream(built, fetch):
    """row0 > 0, pitch > width, prev_pitch > width, d_taps at an odd address, sentinel rows and columns around
    d_out, d_src and d_taps."""
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
        whole = run_whole(r, fetch, cam, p, pv_a, raw, ids, depth, prev_rgb, prev_ids)

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
            d_taps = torch.full(((rows + 2), pitch), TAP_SENTINEL, dtype=torch.uint8, device="cuda")
            taps_ptr = d_taps.data_ptr() + pitch
            assert pitch % 2 == 1 and d_taps.data_ptr() % 2 == 0 and taps_ptr % 2 == 1
            r.reproject_temporal_fetch_async(cam, p, pv_a, ALPHA, fetch, row0, rows, pitch, d_raw.data_ptr(),
                                             d_ids.data_ptr(), d_depth.data_ptr(), d_prev.data_ptr(), d_pids.data_ptr(),
                                             ppitch, d_out.data_ptr() + pitch * 4, d_src.data_ptr() + pitch * 4, taps_ptr,
                                             s.cuda_stream)
            # rows == 0: success, nothing written
            z_out = torch.full((pitch,), OUT_SENTINEL, dtype=torch.int32, device="cuda")
            z_taps = torch.full((pitch,), TAP_SENTINEL, dtype=torch.uint8, device="cuda")
            r.reproject_temporal_fetch_async(cam, p, pv_a, ALPHA, fetch, row0, 0, pitch, d_raw.data_ptr(),
                                             d_ids.data_ptr(), d_depth.data_ptr(), d_prev.data_ptr(), d_pids.data_ptr(),
                                             ppitch, z_out.data_ptr(), 0, z_taps.data_ptr(), s.cuda_stream)
        s.synchronize()
    out, src, taps = d_out.cpu().numpy(), d_src.cpu().numpy(), d_taps.cpu().numpy()
    assert np.array_equal(out[1:rows + 1, :W].copy().view(np.uint8).reshape(rows, W, 4), whole[0][row0:row0 + rows])
    assert np.array_equal(src[1:rows + 1, :W], whole[1][row0:row0 + rows])
    assert np.array_equal(taps[1:rows + 1, :W], whole[2][row0:row0 + rows])
    for buf, sentinel in ((out, OUT_SENTINEL), (src, SRC_SENTINEL), (taps, TAP_SENTINEL)):
        for untouched in (buf[0], buf[rows + 1], buf[:, W:]):
            assert np.all(untouched == np.array(sentinel).astype(buf.dtype))
    assert np.all(z_out.cpu().numpy() == OUT_SENTINEL) and np.all(z_taps.cpu().numpy() == TAP_SENTINEL)
    assert np.count_nonzero(whole[1][row0:row0 + rows] >= 0) > 0


@pytest.mark.parametrize("w,h", [(37, 19), (16, 8)])
def test_frame_shapes(built, w, h):
    """Sizes that are no multiple of the 16x16 tile, and one smaller than a tile's row of waves: partial
    workgroups, and taps past every border of the previous image."""
    p = ref.params()
    prev_rgb = history(w, h)
    cam_a, cam_b = ref.camera("A", w, h), ref.camera("B", w, h)
    pv_a = vrt.camera_forward(cam_a)
    with vrt.Renderer(0) as r:
        r.upload_volume(ref.scene("refraction"), N)
        prev_ids, _ = r.render_ids(cam_a, p)
        ids, depth = r.render_ids(cam_b, p)
        raw, _ = r.render_frame(cam_b, p, 1.0)
        got = run_whole(r, BILINEAR, cam_b, p, pv_a, raw, ids, depth, prev_rgb, prev_ids)
    pos, dirs = ref.primary_rays("B", 0.0, 1.0, w, h)
    want = bil.bilinear(ids, depth, pos, dirs, N, pv_a, prev_ids, prev_rgb, raw, ALPHA)
    assert_same(got, want[:3], (w, h))
    assert np.count_nonzero(got[1] >= 0) > 0
    stats = bil.tap_stats(ids, depth, pos, dirs, N, pv_a, prev_ids)
    print((w, h), bil.counts(got[1], got[2]), "pixels with a tap outside", int(stats["border"].sum()))
    assert stats["border"].any()


def test_call_is_capturable(built):
    """One call is one kernel launch without allocation (test_launch_timing_counts_one_launch counts it):
    captured into a graph like the old entry point, and replayed three times, each time with another raw
    frame and another history in the same buffers: every replay writes what an eager call writes."""
    import torch

    cam, p = ref.camera("B"), ref.params()
    pv_a = vrt.camera_forward(ref.camera("A"))
    with vrt.Renderer(0) as r:
        r.upload_volume(ref.scene("refraction"), N)
        prev_ids, _ = r.render_ids(ref.camera("A"), p)
        ids, depth = r.render_ids(cam, p)
        raw, _ = r.render_frame(cam, p, 1.0)
        inputs = [(raw, history(seed=21)), (history(seed=22), history(seed=23)), (raw[::-1].copy(), history(seed=24))]
        wants = [run_whole(r, BILINEAR, cam, p, pv_a, rw, ids, depth, pr, prev_ids) for rw, pr in inputs]
        d_raw, d_ids, d_depth = dev(raw), dev(ids_words(ids)), dev(depth)
        d_prev, d_pids = dev(inputs[0][1]), dev(ids_words(prev_ids))
        d_out = torch.zeros((H, W), dtype=torch.int32, device="cuda")
        d_src = torch.zeros((H, W), dtype=torch.int32, device="cuda")
        d_taps = torch.zeros((H, W), dtype=torch.uint8, device="cuda")

        def call(stream):
            r.reproject_temporal_fetch_async(cam, p, pv_a, ALPHA, BILINEAR, 0, H, W, d_raw.data_ptr(), d_ids.data_ptr(),
                                             d_depth.data_ptr(), d_prev.data_ptr(), d_pids.data_ptr(), W,
                                             d_out.data_ptr(), d_src.data_ptr(), d_taps.data_ptr(), stream)

        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):   # warm the stream outside the capture
            call(s.cuda_stream)
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            call(torch.cuda.current_stream().cuda_stream)
        for (rw, pr), want in zip(inputs, wants):
            d_raw.copy_(dev(rw))
            d_prev.copy_(dev(pr))
            d_out.fill_(OUT_SENTINEL)
            d_src.fill_(SRC_SENTINEL)
            d_taps.fill_(TAP_SENTINEL)
            torch.cuda.synchronize()
            g.replay()
            torch.cuda.synchronize()
            got = (d_out.cpu().numpy().view(np.uint8).reshape(H, W, 4), d_src.cpu().numpy(), d_taps.cpu().numpy())
            assert_same(got, want, "replay")
    assert not np.array_equal(wants[0][0], wants[1][0]) and not np.array_equal(wants[0][0], wants[2][0])


@pytest.mark.parametrize("fetch,taps", [(NEAREST, True), (BILINEAR, True), (BILINEAR, False)])
def test_launch_timing_counts_one_launch(built, fetch, taps):
    import torch

    cam, p = ref.camera("A"), ref.params()
    with vrt.Renderer(0) as r:
        r.upload_volume(ref.scene("terrain"), N)
        ids, depth = r.render_ids(cam, p)
        raw, _ = r.render_frame(cam, p, 1.0)
        r.set_launch_timing(2)
        run_whole(r, fetch, cam, p, vrt.camera_forward(cam), raw, ids, depth, history(), ids, taps=taps)
        total, launches = r.launch_timing()
        r.set_launch_timing(0)
        torch.cuda.synchronize()
    assert launches == 1 and total > 0.0


# ---- the synchronous frame loop --------------------------------------------------------------------

def restated_frame(parts, mode, cn, t, prev_out, prev_ids, prev_cam):
    """One frame of the loop from its parts: the raw frame with ray_noise 0.05, noise-free IDs and depth, and
    the restatement of `mode` against the previous output. Returns (frame, src, taps, ids)."""
    cam = ref.camera(cn)
    p, geom = ref.params(0.05, t), ref.params(0.0, t)
    raw, _ = parts.render_frame(cam, p, 1.0)
    ids, depth = parts.render_ids(cam, geom)
    pos, dirs = ref.primary_rays(cn, 0.0, t)
    pv = vrt.camera_forward(prev_cam) if prev_cam is not None else np.zeros(16, np.float32)
    out, src, taps = bil.fetch(mode, ids, depth, pos, dirs, N, pv, prev_ids, prev_out, raw, ALPHA)
    return out, src, taps, ids


@pytest.mark.parametrize("name", ["terrain", "refraction"])
def test_frame_loop_with_a_moving_camera(built, name):
    """set_reprojected_fetch(FETCH_BILINEAR), then frames along A, B, A, C with ray_noise 0.05 in the colour pass
    only: each equals the bilinear restatement composed from the previous output."""
    prev_out = prev_ids = prev_cam = None
    with vrt.Renderer(0) as r, vrt.Renderer(0) as parts:
        r.upload_volume(ref.scene(name), N)
        parts.upload_volume(ref.scene(name), N)
        r.set_reprojected_fetch(BILINEAR)
        for f, cn in enumerate("ABAC"):
            t = float(f + 1)
            got, ms = r.render_frame_reprojected(ref.camera(cn), ref.params(0.05, t), ALPHA, timing=True)
            assert ms > 0.0
            want, src, taps, ids = restated_frame(parts, BILINEAR, cn, t, prev_out, prev_ids, prev_cam)
            bad = np.argwhere(np.any(got != want, axis=-1))
            assert bad.size == 0, (name, f, cn, len(bad), bad[:5].tolist())
            print(name, f, cn, bil.counts(src, taps))
            if f > 0:
                assert 0 < np.count_nonzero(src >= 0) < W * H
            prev_out, prev_ids, prev_cam = got, ids, ref.camera(cn)


def test_mode_switches_keep_the_history(built):
    """Frames at A, B, A: `r` switches to the bilinear fetch after frame 1 and back to nearest after frame 2 (an
    unknown mode in between is refused and changes nothing); `plain` never calls the setter. Frame 2 of `r` is
    not the raw frame: it is the bilinear restatement against frame 1; frame 3 the nearest restatement against
    frame 2. Every frame of `plain` is the nearest restatement."""
    with vrt.Renderer(0) as r, vrt.Renderer(0) as plain, vrt.Renderer(0) as parts:
        for q in (r, plain, parts):
            q.upload_volume(ref.scene("refraction"), N)
        prev = {"r": (None, None, None), "plain": (None, None, None)}
        for f, (cn, mode) in enumerate((("A", NEAREST), ("B", BILINEAR), ("A", NEAREST))):
            t = float(f + 1)
            cam, p = ref.camera(cn), ref.params(0.05, t)
            if f > 0:
                assert r._lib.vrt_set_reprojected_fetch(r._h, 2) == abi.VRT_ERR_INVALID
                assert r._lib.vrt_set_reprojected_fetch(r._h, -1) == abi.VRT_ERR_INVALID
                r.set_reprojected_fetch(mode)
                with pytest.raises(vrt.VrtError):
                    r.set_reprojected_fetch(7)
            got = r.render_frame_reprojected(cam, p, ALPHA)
            want, src, taps, ids = restated_frame(parts, mode, cn, t, *prev["r"])
            assert np.array_equal(got, want), (f, cn, mode)
            if f > 0:
                raw, _ = parts.render_frame(cam, p, 1.0)
                assert not np.array_equal(got, raw) and np.count_nonzero(src >= 0) > 0
            prev["r"] = (got, ids, cam)
            got_p = plain.render_frame_reprojected(cam, p, ALPHA)
            want_p, _, _, ids_p = restated_frame(parts, NEAREST, cn, t, *prev["plain"])
            assert np.array_equal(got_p, want_p), (f, cn)
            prev["plain"] = (got_p, ids_p, cam)
        assert not np.array_equal(prev["r"][0], prev["plain"][0])   # (the two loops did differ)
    assert r._lib.vrt_set_reprojected_fetch(None, BILINEAR) == abi.VRT_ERR_INVALID


def test_resets_still_drop_the_history(built):
    """In the bilinear mode too: after reprojected_history_reset and after a change of the image size the next
    frame is the raw frame."""
    cam, small = ref.camera("A"), ref.camera("A", 37, 19)
    # the sun moves from frame to frame, so that every frame differs from its history
    ps = [ref.params(0.0, float(t), sun_dir=vrt.sun_dir(40.0 + t)) for t in range(1, 7)]
    with vrt.Renderer(0) as r, vrt.Renderer(0) as plain:
        r.upload_volume(ref.scene("refraction"), N)
        plain.upload_volume(ref.scene("refraction"), N)
        r.set_reprojected_fetch(BILINEAR)
        raws = [plain.render_frame(cam, q, 1.0)[0] for q in ps]
        raw_small = plain.render_frame(small, ps[4], 1.0)[0]
        assert np.array_equal(r.render_frame_reprojected(cam, ps[0], ALPHA), raws[0])
        assert not np.array_equal(r.render_frame_reprojected(cam, ps[1], ALPHA), raws[1])
        r.reprojected_history_reset()
        assert np.array_equal(r.render_frame_reprojected(cam, ps[2], ALPHA), raws[2])
        assert not np.array_equal(r.render_frame_reprojected(cam, ps[3], ALPHA), raws[3])
        assert np.array_equal(r.render_frame_reprojected(small, ps[4], ALPHA), raw_small)   # size change
        assert np.array_equal(r.render_frame_reprojected(cam, ps[5], ALPHA), raws[5])       # and back


# ---- errors ------------------------------------------------------------------------------------------

def test_errors_leave_the_outputs_untouched(built):
    """Every error case of tests/test_gpu_reproject.py::test_errors_leave_the_outputs_untouched through the new
    entry point, in both modes, and the unknown modes."""
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
    d_taps = torch.full((H * W + 2,), TAP_SENTINEL, dtype=torch.uint8, device="cuda")

    def bad_size(w, h):
        c = ref.camera("A")
        c.width, c.height = w, h
        return c

    def untouched():
        torch.cuda.synchronize()
        return (np.all(d_out.cpu().numpy() == OUT_SENTINEL) and np.all(d_src.cpu().numpy() == SRC_SENTINEL)
                and np.all(d_taps.cpu().numpy() == TAP_SENTINEL))

    with vrt.Renderer(0) as r:
        L, ctx = r._lib, r._h
        good = dict(cam=C.byref(cam), p=C.byref(p), pv=pv.ctypes.data, fetch=BILINEAR, row0=0, rows=H, pitch=W,
                    raw=d_raw.data_ptr(), ids=d_ids.data_ptr(), depth=d_depth.data_ptr(), prev=d_prev.data_ptr(),
                    pids=d_pids.data_ptr(), ppitch=W, out=d_out.data_ptr(), src=d_src.data_ptr(), taps=d_taps.data_ptr())

        def a(**kw):
            g = dict(good, **kw)
            return L.vrt_reproject_temporal_fetch_async(ctx, g["cam"], g["p"], g["pv"], ALPHA, g["fetch"], g["row0"],
                                                        g["rows"], g["pitch"], g["raw"], g["ids"], g["depth"], g["prev"],
                                                        g["pids"], g["ppitch"], g["out"], g["src"], g["taps"], None)

        assert a() == abi.VRT_ERR_NO_VOLUME and a(fetch=NEAREST) == abi.VRT_ERR_NO_VOLUME
        r.upload_volume(ref.scene("terrain"), N)
        inv = abi.VRT_ERR_INVALID
        for fetch in (NEAREST, BILINEAR):
            good["fetch"] = fetch
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
            assert L.vrt_reproject_temporal_fetch_async(None, good["cam"], good["p"], good["pv"], ALPHA, fetch, 0, H, W,
                                                        good["raw"], good["ids"], good["depth"], good["prev"],
                                                        good["pids"], W, good["out"], good["src"], good["taps"],
                                                        None) == inv
        # unknown modes, also on an empty band
        for fetch in (2, -1):
            assert a(fetch=fetch) == inv and a(fetch=fetch, rows=0) == inv, fetch
        assert b"fetch" in L.vrt_last_error(ctx)
        assert untouched()
        # rows == 0 is a successful no-op; no history, no d_src and no d_taps are valid; the last row is a valid band
        assert a(rows=0) == abi.VRT_OK and a(row0=H, rows=0) == abi.VRT_OK
        assert untouched()
        assert a(row0=H - 1, rows=1, prev=None, pids=None, src=None, taps=None) == abi.VRT_OK
        torch.cuda.synchronize()
        got = d_out.cpu().numpy()
        assert np.all(got[:W] == 0) and np.all(got[W:] == OUT_SENTINEL)   # out = raw (zeros) in the band's row
        assert np.all(d_src.cpu().numpy() == SRC_SENTINEL) and np.all(d_taps.cpu().numpy() == TAP_SENTINEL)
        # d_taps at an odd address is valid
        assert a(row0=H - 1, rows=1, prev=None, pids=None, src=None, taps=good["taps"] + 1) == abi.VRT_OK
        torch.cuda.synchronize()
        t = d_taps.cpu().numpy()
        assert t[0] == TAP_SENTINEL and not t[1:W + 1].any() and np.all(t[W + 1:] == TAP_SENTINEL)
