"""In-place voxel edits (GPU): vrt_update_volume_region rebuilds only the packed texels of its plan, by
the kernels that build the whole skip field for an upload (csrc/vrt_skipfield_kernels.h) run on the
plan's boxes, and the result must be, byte for byte, what a full upload of the edited volume produces.
The reference is a fresh Renderer with a full upload_volume of the edited bytes (its
debug_packed_volume() must be array_equal, its frames bit-identical, its certified() the same) and,
since upload and edit share their kernels, the brute-force NumPy transform of
tests/skipfield_reference.py on small volumes."""
import ctypes as C
import os

import numpy as np
import pytest

import oracle
import voxelraytracer_amd as vrt
from harness import COLOR_TOL, assert_same_packed
from skipfield_reference import apply_edit, packed_reference, random_edit
from voxelraytracer_amd import abi

pytestmark = pytest.mark.gpu

THREADS = min(16, os.cpu_count() or 1)


def current_block(vox, n, origin, extent):
    ex, ey, ez = extent
    return vox.reshape(n, n, n)[origin[2]:origin[2] + ez, origin[1]:origin[1] + ey,
                                origin[0]:origin[0] + ex].copy()


def edit_sequence(vox, n, count, seed):
    """`count` cumulative edits [(origin, block)] of `vox` and the edited bytes after each. Three are
    fixed: a box on x = y = z = 0 (the plane-N rule, corner texel included), a box on N - 1 of every
    axis, and a box whose materials change while no cell's emptiness does; the rest are random boxes
    of edge 1..9 that cycle through carving (0), fills with 1..3 and random bytes."""
    rng = np.random.default_rng(seed)
    edits, states = [], []
    for i in range(count):
        if i == 0:
            origin, block = (0, 0, 0), rng.integers(0, 4, (4, 2, 3)).astype(np.uint8)
        elif i == 1:
            origin, block = (n - 5, n - 3, n - 2), rng.integers(0, 4, (2, 3, 5)).astype(np.uint8)
        elif i == 2:
            origin = (10, 0, 10)
            cur = current_block(vox, n, origin, (6, 4, 6))
            block = np.where(cur != 0, cur % 3 + 1, 0).astype(np.uint8)
            assert np.any(block != cur) and np.array_equal(block != 0, cur != 0)
        else:
            e = rng.integers(1, 10, 3)
            origin = tuple(int(rng.integers(0, n - int(e[a]) + 1)) for a in range(3))
            shape = (int(e[2]), int(e[1]), int(e[0]))
            if i % 3 == 0:
                block = np.zeros(shape, np.uint8)
            elif i % 3 == 1:
                block = np.full(shape, int(rng.integers(1, 4)), np.uint8)
            else:
                block = rng.integers(0, 4, shape).astype(np.uint8)
        vox = apply_edit(vox, n, origin, block)
        edits.append((origin, block))
        states.append(vox)
    return edits, states


def fresh_packed(vox, n, layout=0):
    with vrt.Renderer(0) as f:
        f.set_skip_layout(layout)
        f.upload_volume(vox, n)
        return f.debug_packed_volume()


@pytest.mark.parametrize("scene", ["terrain", "glass_cube"])
def test_edit_sequence_matches_full_uploads(built, scene):
    n = 64
    vox = vrt.build_scene(scene, n)
    edits, states = edit_sequence(vox, n, 20, seed=11)
    kinds = {int(b.max()) == 0 for _, b in edits[3:]}
    assert kinds == {True, False}   # carving and filling both occur
    with vrt.Renderer(0) as r:
        r.upload_volume(vox, n)
        assert r._lib.vrt_volume_octants(r._h) == 8
        for i, (origin, block) in enumerate(edits):
            r.update_volume(origin, block)
            if i in (0, 9, 19):
                assert_same_packed(r.debug_packed_volume(), fresh_packed(states[i], n))
        # the canonical bytes (vrt_volume_device_ptr consumers, later edits) are the edited ones
        import torch

        class View:
            __cuda_array_interface__ = {"shape": (n ** 3,), "typestr": "|u1", "version": 3,
                                        "data": (r.volume_device_ptr(), False)}
        torch.cuda.synchronize()
        assert np.array_equal(torch.as_tensor(View(), device="cuda").cpu().numpy(), states[-1])


def test_edit_sequence_single_layout(built):
    n = 64
    vox = vrt.build_scene("terrain", n)
    edits, states = edit_sequence(vox, n, 8, seed=5)
    with vrt.Renderer(0) as r:
        r.set_skip_layout(1)
        r.upload_volume(vox, n)
        assert r._lib.vrt_volume_octants(r._h) == 1
        for i, (origin, block) in enumerate(edits):
            r.update_volume(origin, block)
            if i in (0, 7):
                assert_same_packed(r.debug_packed_volume(), fresh_packed(states[i], n, 1))


@pytest.mark.parametrize("layout", [8, 1])
@pytest.mark.parametrize("scene,n,seed", [("terrain", 16, 3), ("refraction", 16, 2), ("glass_cube", 16, 7),
                                          ("terrain", 32, 10), ("refraction", 32, 11)])
def test_edits_match_the_numpy_reference(built, scene, n, seed, layout):
    """Upload and edit run the same kernels, so an edit is also held against the independent NumPy
    transform: the four seeded edits of tests/test_volume_edit_plan.py (each changes emptiness), then a
    box on x = y = z = 0 with its emptiness inverted (plane N, corner texel included); after every
    edit every texel of the (N+1)^3 volume(s) equals the reference of the edited bytes."""
    rng = np.random.default_rng(seed)
    vox = vrt.build_scene(scene, n)
    with vrt.Renderer(0) as r:
        r.set_skip_layout(layout)
        r.upload_volume(vox, n)
        assert r._lib.vrt_volume_octants(r._h) == layout
        for i in range(5):
            if i < 4:
                origin, block = random_edit(rng, n)
            else:
                origin = (0, 0, 0)
                block = np.where(current_block(vox, n, origin, (4, 3, 2)) != 0, 0, 3).astype(np.uint8)
            new = apply_edit(vox, n, origin, block)
            assert np.any((new != 0) != (vox != 0)), "the edit changes no emptiness"
            vox = new
            r.update_volume(origin, block)
            assert_same_packed(r.debug_packed_volume(), packed_reference(vox, n, layout))


@pytest.mark.parametrize("n,layout,probe", [(256, 8, (200, 200, 200)), (128, 1, (100, 100, 100))])
def test_edits_where_the_caps_bind(built, n, layout, probe):
    """refraction is mostly empty, so the skip distances reach their caps and a one-voxel edit changes
    texels up to the caps away: an under-dilated region fails here and nowhere smaller."""
    vox = vrt.build_scene("refraction", n)
    c = n // 2
    assert vox.reshape(n, n, n)[c, c, c] == 2 and vox.reshape(n, n, n)[probe[2], probe[1], probe[0]] == 0
    with vrt.Renderer(0) as r:
        r.set_skip_layout(layout)
        r.upload_volume(vox, n)
        assert r._lib.vrt_volume_octants(r._h) == layout
        for origin, byte in ((probe, 1), ((c, c, c), 0)):   # one voxel set, the one glass voxel cleared
            block = np.full((1, 1, 1), byte, np.uint8)
            vox = apply_edit(vox, n, origin, block)
            r.update_volume(origin, block)
            assert_same_packed(r.debug_packed_volume(), fresh_packed(vox, n, layout))


def test_device_variant_matches_host_variant(built):
    import torch

    n = 64
    vox = vrt.build_scene("terrain", n)
    rng = np.random.default_rng(3)
    origin, block = (0, 20, 30), rng.integers(0, 4, (5, 7, 9)).astype(np.uint8)   # [z][y][x], on x = 0
    extent = block.shape[::-1]
    with vrt.Renderer(0) as a, vrt.Renderer(0) as b:
        a.upload_volume(vox, n)
        b.upload_volume(vox, n)
        a.update_volume(origin, block)
        s = torch.cuda.Stream()
        with torch.cuda.stream(s):
            t = torch.from_numpy(block.reshape(-1)).to("cuda", non_blocking=False)
            b.update_volume_device(origin, extent, t.data_ptr(), s.cuda_stream)
        pa, pb = a.debug_packed_volume(), b.debug_packed_volume()
    assert_same_packed(pb, pa)
    assert_same_packed(pa, fresh_packed(apply_edit(vox, n, origin, block), n))


def test_rendering_after_the_edit_sequence(built):
    n, w, h = 64, 160, 90
    vox = vrt.build_scene("terrain", n)
    edits, states = edit_sequence(vox, n, 20, seed=11)
    cam = vrt.make_camera(w, h)
    p = vrt.default_params(4, 2)
    with vrt.Renderer(0) as r, vrt.Renderer(0) as f:
        r.upload_volume(vox, n)
        for origin, block in edits:
            r.update_volume(origin, block)
        f.upload_volume(states[-1], n)
        assert r.certified() == f.certified()
        rg, rh, rs = r.render(cam, p)
        fg, fh, fs = f.render(cam, p)
        frame_r, _ = r.render_frame(cam, p)   # stats-free: the certified path, which reads G
        frame_f, _ = f.render_frame(cam, p)
    assert np.array_equal(rg.view(np.uint32), fg.view(np.uint32))
    assert np.array_equal(rh, fh)
    assert {k: v for k, v in rs.items() if k != "kernel_ms"} == {k: v for k, v in fs.items() if k != "kernel_ms"}
    assert np.array_equal(frame_r, frame_f)
    og, oh, _ = oracle.render(cam, states[-1], n, p, threads=THREADS)
    for field in ("voxel_index", "steps", "flags"):
        assert np.array_equal(rh[field], oh[field]), field
    assert np.array_equal(rh["ray_length"].view(np.uint32), oh["ray_length"].view(np.uint32))
    d = np.abs(np.clip(rg[..., :3], 0, 1) - np.clip(og[..., :3], 0, 1)).max()
    print(f"max colour difference against the oracle: {d:.3e}")
    assert d <= COLOR_TOL, d


@pytest.mark.parametrize("trees", [0, 1])
def test_glass_share_follows_edits(built, trees):
    """The automatic certified mode's glass share moves with an edit's box counts. With certified
    bounce trees off (trees = 0) certified() shows that rule alone; with the default (1) glass-heavy
    volumes stay certified through the trees, on the edited and the fresh context alike."""
    n, w, h = 32, 96, 54
    vox = vrt.build_scene("refraction", n)
    cam = vrt.make_camera(w, h)
    p = vrt.default_params(2, 2)
    origin = (4, 4, 4)
    glass = np.full((8, 8, 8), 2, np.uint8)
    filled = apply_edit(vox, n, origin, glass)
    assert np.count_nonzero(filled == 2) * 8 > np.count_nonzero(filled)
    carved = apply_edit(filled, n, origin, np.zeros_like(glass))
    assert np.array_equal(carved, vox)
    with vrt.Renderer(0) as r:
        r.set_cert_trees(trees)
        r.upload_volume(vox, n)
        assert r.certified() is True
        for block, state, expect in ((glass, filled, False), (np.zeros_like(glass), carved, True)):
            r.update_volume(origin, block)
            with vrt.Renderer(0) as f:
                f.set_cert_trees(trees)
                f.upload_volume(state, n)
                assert r.certified() == f.certified()
                if trees == 0:
                    assert f.certified() is expect
                assert_same_packed(r.debug_packed_volume(), f.debug_packed_volume())
                frame_r, _ = r.render_frame(cam, p)
                frame_f, _ = f.render_frame(cam, p)
                assert np.array_equal(frame_r, frame_f)


def test_repeated_device_context_edits_every_replica(built):
    """Renderer([0, 0]) keeps two replicas and renders half of the frame's row blocks from each:
    the frame after an edit equals the single-device fresh frame only if both were rebuilt."""
    n, w, h = 64, 160, 90
    vox = vrt.build_scene("terrain", n)
    edits, states = edit_sequence(vox, n, 6, seed=7)
    cam = vrt.make_camera(w, h)
    p = vrt.default_params(4, 2)
    with vrt.Renderer([0, 0]) as r, vrt.Renderer(0) as f:
        assert r.device_count() == 2
        r.upload_volume(vox, n)
        before, _ = r.render_frame(cam, p)
        for origin, block in edits:
            r.update_volume(origin, block)
        f.upload_volume(states[-1], n)
        frame_r, _ = r.render_frame(cam, p)
        frame_f, _ = f.render_frame(cam, p)
        assert_same_packed(r.debug_packed_volume(), f.debug_packed_volume())
    assert not np.array_equal(before, frame_f)   # the edits are visible
    assert np.array_equal(frame_r, frame_f)


def raw_update(r, origin, extent, buf):
    o3, e3 = (C.c_int32 * 3)(*origin), (C.c_int32 * 3)(*extent)
    return r._lib.vrt_update_volume_region(r._h, C.byref(o3), C.byref(e3), buf)


def test_errors_leave_the_volume_alone(built):
    n = 32
    vox = vrt.build_scene("glass_cube", n)
    buf = np.ones(64, np.uint8)
    with vrt.Renderer(0) as r:
        assert raw_update(r, (0, 0, 0), (1, 1, 1), buf.ctypes.data) == abi.VRT_ERR_NO_VOLUME
        assert r._lib.vrt_last_error(r._h)
        with pytest.raises(vrt.VrtError) as e:
            r.update_volume((0, 0, 0), np.ones((1, 1, 1), np.uint8))
        assert e.value.code == abi.VRT_ERR_NO_VOLUME
        r.upload_volume(vox, n)
        before = r.debug_packed_volume()
        for origin, extent in (((n - 1, 0, 0), (2, 1, 1)), ((0, n, 0), (1, 1, 1)), ((0, 0, -1), (1, 1, 1)),
                               ((0, 0, 0), (1, n + 1, 1)), ((3, 3, 3), (0, 1, 1)), ((3, 3, 3), (1, 1, -2))):
            assert raw_update(r, origin, extent, buf.ctypes.data) == abi.VRT_ERR_INVALID, (origin, extent)
            assert r._lib.vrt_last_error(r._h)
        assert raw_update(r, (3, 3, 3), (1, 1, 1), None) == abi.VRT_ERR_INVALID
        assert r._lib.vrt_update_volume_region(r._h, None, None, buf.ctypes.data) == abi.VRT_ERR_INVALID
        with pytest.raises(vrt.VrtError) as e:
            r.update_volume((n - 1, 0, 0), np.ones((1, 1, 2), np.uint8))
        assert e.value.code == abi.VRT_ERR_INVALID
        assert np.array_equal(r.debug_packed_volume(), before)
        # and a valid edit still works afterwards
        r.update_volume((3, 3, 3), np.ones((1, 1, 1), np.uint8))
        assert_same_packed(r.debug_packed_volume(), fresh_packed(apply_edit(vox, n, (3, 3, 3),
                                                                            np.ones((1, 1, 1), np.uint8)), n))
