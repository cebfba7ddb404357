"""GPU: the packed skip field where its caps bind and its regional boxes are regional, against the fast
exact reference (tests/skipfield_fast.c through tests/skipfield_reference.py), which shares no algorithm
with the kernels. At N <= 32 (tests/test_gpu_volume.py, tests/test_gpu_volume_edit.py) kFwdCap = 128 and
kDistCap = 64 clamp nothing and every box of an edit is the whole volume; at N >= 64 those files compare
the kernels with themselves. Here, at N = 256 on void256 (an off-centre cluster in a void: uncapped F
reaches 190, uncapped D 95):

  a. uploads, every texel of debug_packed_volume() in both layouts, also of the built scenes and two
     adversarial volumes at 64 to 256
  b. cumulative edits, the field compared with the reference of the edited bytes after each one (never with
     a fresh upload): strict-interior plans, an occupied voxel exactly 127 and exactly 128 cells ahead of an
     anchor at the cap, a box across x = 0 (plane N), a material-only edit, a voxel cleared
  c. frames whose walks are made of capped jumps, against the oracle: hit records, every stats-free mode,
     the RGB8 temporal frame, render_ids and pick, in both layouts

The floors that keep a case from passing empty are asserted on the reference and on the oracle."""
import functools
import os

import numpy as np
import pytest
import torch

import oracle
import voxelraytracer_amd as vrt
from adversarial_volumes import volumes
from harness import (all_modes, all_pixels, assert_ids_equal_pick, assert_same_packed, check_raw, compare,
                     reset_modes)
from harness import float_bits as bits
from skipfield_reference import (CAP, FWD_CAP, UNCAPPED, apply_edit, chebyshev_fast, forward_fast, packed_fast,
                                 void256)
from voxelraytracer_amd import abi

pytestmark = pytest.mark.gpu

THREADS = min(16, os.cpu_count() or 1)
N = 256


def volume(name, n):
    if name == "void256":
        assert n == N
        return void256()
    if name in ("bytes", "lattice"):
        return volumes(n)[name]
    return vrt.build_scene(name, n)


def step(octant):
    """(sx, sy, sz) of an octant: bit a set, the step is -1 on axis a."""
    return tuple(-1 if octant >> a & 1 else 1 for a in range(3))


def forward_at(vox, octant, anchor, cap=FWD_CAP):
    """The reference's F of `octant` at the anchor (x, y, z)."""
    return int(forward_fast(vox, N, octant, cap)[anchor[2], anchor[1], anchor[0]])


# ---- a. uploads ----------------------------------------------------------------------------------

def test_void256_reference_floors(built):
    """On the reference, so that (a) and (b) cannot pass with caps that clamp nothing: some anchor of every
    octant has uncapped F > 128, some cell uncapped D > 64, and the capped field holds G = 127 and D = 64."""
    vox = void256()
    for o in range(8):
        assert int(forward_fast(vox, N, o, UNCAPPED).max()) > FWD_CAP, o
    assert int(chebyshev_fast(vox, N, UNCAPPED).max()) > CAP
    assert int((packed_fast(vox, N, 8) >> 8).max()) == FWD_CAP - 1
    assert int((packed_fast(vox, N, 1) >> 8).max()) == CAP


UPLOADS = [("void256", 256), ("refraction", 256), ("terrain", 64), ("glass_cube", 64), ("refraction", 64),
           ("terrain", 128), ("glass_cube", 128), ("refraction", 128), ("bytes", 64), ("lattice", 64)]


@pytest.mark.parametrize("layout", [8, 1])
@pytest.mark.parametrize("name,n", UPLOADS)
def test_uploads_match_the_fast_reference(built, name, n, layout):
    """Every texel, plane N included."""
    vox = volume(name, n)
    with vrt.Renderer(0) as r:
        r.set_skip_layout(layout)
        r.upload_volume(vox, n)
        assert r._lib.vrt_volume_octants(r._h) == layout
        got = r.debug_packed_volume()
    assert_same_packed(got, packed_fast(vox, n, layout))


# ---- b. edits ------------------------------------------------------------------------------------

CENTRE = (128, 128, 128)
# An anchor of octant 0 (+x, +y, +z) whose cube of edge 128 is empty once the centre voxel is set: x in
# [0, 127] stops short of the centre, y in [100, 227] clears the floor slab and the cluster. F = 128.
ANCHOR_127, OCTANT_127 = (0, 100, 100), 0
AHEAD_127 = (127, 227, 227)   # the far corner of that cube, 127 cells ahead on every axis: F becomes 127
# An anchor of octant 1 (-x, +y, +z) with F = 128: x in [128, 255] clears the cluster and AHEAD_127, y in
# [40, 167] the floor slab and the byte 200 at y = 200, z in [0, 127] the centre.
ANCHOR_128, OCTANT_128 = (255, 40, 0), 1
AHEAD_128 = (127, 168, 128)   # 128 cells ahead on every axis, just outside that cube: F stays 128


def edits_256():
    """[(what, origin (x, y, z), block [z][y][x], whether emptiness changes)], cumulative on void256."""
    one = np.full((1, 1, 1), 1, np.uint8)
    rng = np.random.default_rng(256)
    return [("centre set", CENTRE, one, True),
            ("127 ahead of an anchor at the cap", AHEAD_127, one, True),
            ("128 ahead of an anchor at the cap", AHEAD_128, one, True),
            ("random bytes across x = 0", (0, 100, 50), rng.integers(0, 4, (2, 3, 5)).astype(np.uint8), True),
            ("the glass block rewritten as byte 1", (66, 60, 60), np.full((6, 6, 6), 1, np.uint8), False),
            ("centre cleared", CENTRE, np.zeros((1, 1, 1), np.uint8), True)]


def test_edit_anchors_on_the_reference(built):
    """The named anchors of edits 2 and 3, on the reference: F = 128 before; 127 after a voxel 127 cells
    ahead; still 128 after a voxel 128 cells ahead. And the steps point from anchor to voxel."""
    states = [void256()]
    for _, origin, block, _ in edits_256():
        states.append(apply_edit(states[-1], N, origin, block))
    assert tuple(a + 127 * s for a, s in zip(ANCHOR_127, step(OCTANT_127))) == AHEAD_127
    assert tuple(a + 128 * s for a, s in zip(ANCHOR_128, step(OCTANT_128))) == AHEAD_128
    assert forward_at(states[1], OCTANT_127, ANCHOR_127) == FWD_CAP
    assert forward_at(states[2], OCTANT_127, ANCHOR_127) == FWD_CAP - 1
    assert forward_at(states[2], OCTANT_128, ANCHOR_128) == FWD_CAP
    assert forward_at(states[3], OCTANT_128, ANCHOR_128) == FWD_CAP


@pytest.mark.parametrize("layout", [8, 1])
def test_edits_match_the_fast_reference(built, layout):
    """One Renderer, the six cumulative edits of edits_256(); after each, every texel against the reference
    of the edited bytes. Every plan is a strict sub-box, so the passes run on regional boxes with
    region-local offsets; edit 5 changes no emptiness (the packs alone run, the distances stand)."""
    vox, wrong = void256(), []
    with vrt.Renderer(0) as r:
        r.set_skip_layout(layout)
        r.upload_volume(vox, N)
        assert r._lib.vrt_volume_octants(r._h) == layout
        for i, (what, origin, block, changes) in enumerate(edits_256()):
            new = apply_edit(vox, N, origin, block)
            assert not np.array_equal(new, vox), what
            assert bool(np.any((new != 0) != (vox != 0))) is changes, what
            plan = vrt.volume_edit_plan(N, layout, origin, block.shape[::-1])
            # a regional rebuild: some plan is a strict sub-range of every axis
            assert any(all(row[a] > 0 or row[3 + a] < N for a in range(3)) for row in plan), (what, plan)
            vox = new
            r.update_volume(origin, block)
            try:
                assert_same_packed(r.debug_packed_volume(), packed_fast(vox, N, layout))
            except AssertionError as e:   # go on: the report names every edit after which the field is wrong
                wrong.append(f"after edit {i + 1} ({what}): {e}")
    assert not wrong, "\n".join(wrong)


# ---- c. frames whose walks are capped jumps ------------------------------------------------------

W, H = 64, 48
CAMERAS = {   # name: (pos, rot, the max_ray_lengths)
    "near": ((-68.45, -62.83, -61.47), (-33.0, -48.0, 0.0), (100.0, 600.0)),
    "corner": ((100.0, 90.0, 110.0), (-30.0, 45.0, 0.0), (600.0,)),
    "outside": ((0.0, 0.0, 134.0), (0.0, 0.0, 0.0), (600.0,)),
    "lattice": ((0.5, 40.5, 0.5), (-35.26439, 45.0, 0.0), (200.0, 600.0)),
}
FRAMES = [(name, length) for name, (_, _, lengths) in CAMERAS.items() for length in lengths]


def camera(name):
    pos, rot, _ = CAMERAS[name]
    return vrt.make_camera(W, H, pos=pos, rot=rot)


def params(length):
    return vrt.default_params(4, 4, reflection_noise=0.02, time=3.0, max_ray_length=length)


@functools.lru_cache(maxsize=None)
def oracle_frame(name, length):
    """The oracle's frame, with the floors asserted on it: near sees the cluster through glass; the other
    cameras' hits lie beyond one capped jump, and corner and lattice meet three-way ties."""
    vox = void256()
    rgba, hits, cnt = oracle.render(camera(name), vox, N, params(length), threads=THREADS)
    for a in (rgba, hits):
        a.setflags(write=False)
    found = hits["voxel_index"] >= 0
    nhit, nmiss = int(np.count_nonzero(found)), int(np.count_nonzero(~found))
    far = int(np.count_nonzero(found & (hits["ray_length"] > FWD_CAP)))
    glass = int(np.count_nonzero(vox[hits["voxel_index"][found]] == 2))
    what = (name, length, nhit, nmiss, far, glass, cnt["secondary_rays"], cnt["tie3"])
    print("void256 oracle frame (name, max_ray_length, hits, misses, hits beyond 128, glass hits, secondary "
          f"rays, tie3): {what}")
    if name == "near":
        assert nhit >= 2000 and cnt["secondary_rays"] >= 50 and glass > 0, what
        if length == 600.0:
            assert far > 0, what
    else:
        assert far >= 500 and nmiss >= 2000, what
    if name in ("corner", "lattice"):
        assert cnt["tie3"] > 0 and np.any(hits["flags"] & abi.VRT_HIT_FLAG_TIE3), what
    return rgba, hits, cnt


def float_frame(r, cam, p):
    """The stats-free float frame (no hit records, no counters) through render_rows_async."""
    out = torch.full((cam.height, cam.width, 4), -1.0, dtype=torch.float32, device="cuda")
    r.render_rows_async(cam, p, 0, cam.height, 1, out.data_ptr())
    torch.cuda.synchronize()
    return out.cpu().numpy()


@pytest.fixture(scope="module")
def renderers(built):
    """void256 uploaded once per layout."""
    out = {}
    try:
        for layout in (8, 1):
            r = vrt.Renderer(0)
            out[layout] = r
            r.set_skip_layout(layout)
            r.upload_volume(void256(), N)
            assert r._lib.vrt_volume_octants(r._h) == layout
        yield out
    finally:
        for r in out.values():
            r.close()


@pytest.mark.parametrize("layout", [8, 1])
@pytest.mark.parametrize("name,length", FRAMES)
def test_frames_of_capped_jumps(renderers, name, length, layout):
    r = renderers[layout]
    cam, p = camera(name), params(length)
    rgba_o, hits_o, cnt_o = oracle_frame(name, length)
    reset_modes(r)
    try:
        exact, hits, st = r.render(cam, p)
        compare(exact, hits, st, rgba_o, hits_o, cnt_o)
        for mode in all_modes(r):
            got = float_frame(r, cam, p)
            bad = np.argwhere(np.any(bits(got) != bits(exact), axis=-1))
            assert bad.size == 0, (mode, len(bad), bad[:5].tolist())
        reset_modes(r)
        d_prev = torch.zeros((H, W, 4), dtype=torch.uint8, device="cuda")
        d_cur = torch.zeros((H, W, 4), dtype=torch.uint8, device="cuda")
        d_raw = torch.zeros((H, W, 4), dtype=torch.uint8, device="cuda")
        r.render_temporal_rows_async(cam, p, 0.5, 0, H, 1, d_prev.data_ptr(), d_cur.data_ptr(), d_raw.data_ptr())
        torch.cuda.synchronize()
        near = check_raw(d_raw.cpu().numpy(), rgba_o)
        print(f"{name} {length} layout {layout}: {near} bytes one LSB from the oracle's")
        picks = r.pick(cam, p, all_pixels(W, H)).reshape(H, W)
        ids, _ = r.render_ids(cam, p)
        assert np.array_equal(picks["voxel_index"], hits_o["voxel_index"])
        assert np.array_equal(bits(picks["ray_length"]), bits(hits_o["ray_length"]))
        assert np.array_equal(ids["voxel_index"], hits_o["voxel_index"])
        assert_ids_equal_pick(ids, picks, (name, length, layout))
    finally:
        reset_modes(r)
