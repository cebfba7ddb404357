"""The ID-guided spatial filter on the CPU: properties of the NumPy integer restatement
(tests/spatial_reference.py) that the GPU tests compare bytes against, conditions on the oracle's ID buffers
that make those comparisons meaningful (colour-free), and what the filter is for: it lowers the error of the
oracle's noisy frames against its noise-free ones. Volumes are 16^3, frames 96x54 or smaller. No GPU."""
import numpy as np
import pytest

import spatial_reference as sp
from reproject_reference import H, N, SCENES, W
from spatial_reference import FACE, PLANE

FRAMES = [(s, c) for s in SCENES for c in "AB"]


def blur_1d(a, axis):
    """(1, 4, 6, 4, 1) along an axis of an int64 array, zero outside."""
    pad = [(0, 0)] * a.ndim
    pad[axis] = (2, 2)
    p = np.pad(a, pad)
    n = a.shape[axis]
    return sum(k * np.take(p, np.arange(d, d + n), axis=axis) for d, k in enumerate(sp.KERNEL))


def test_constant_colour_is_a_fixed_point():
    rng = np.random.default_rng(1)
    ids = sp.ids_from(rng.integers(-1, 40, (19, 37)), rng.integers(0, 3, (19, 37)) | (rng.integers(1, 4, (19, 37)) << 8))
    img = np.empty((19, 37, 4), np.uint8)
    img[...] = (13, 200, 255, 255)
    for guide in (FACE, PLANE):
        for step in (1, 2, 4, 16):
            out, count = sp.spatial_pass(img, ids, step, guide, 0)
            assert np.array_equal(out, img), (guide, step)
            assert count.min() >= 1 and count.max() <= 25


def test_one_key_is_the_binomial_blur():
    """One key and range 765: the interior is the 5x5 binomial blur rounded to nearest (ties up), and the border
    renormalises by the weights inside the image."""
    h, w = 19, 37
    img = sp.random_frame(h, w, 2)
    ids = sp.ids_from(np.full((h, w), 7), np.full((h, w), 1 | (2 << 8)))
    out, count = sp.spatial_pass(img, ids, 1)
    c = img[..., :3].astype(np.int64)
    acc = blur_1d(blur_1d(c, 0), 1)
    wsum = blur_1d(blur_1d(np.ones((h, w), np.int64), 0), 1)
    assert np.all(wsum[2:-2, 2:-2] == 256) and wsum[0, 0] == 121 and wsum[0, 5] == 176
    want = (2 * acc + wsum[..., None]) // (2 * wsum[..., None])
    assert np.array_equal(out[..., :3], want) and np.all(out[..., 3] == 255)
    assert np.all(count[2:-2, 2:-2] == 25) and count[0, 0] == 9 and count[0, 5] == 15
    # the stated rounding on one interior pixel, by hand
    y, x = 9, 20
    a = sum(sp.KERNEL[i + 2] * sp.KERNEL[j + 2] * int(img[y + j, x + i, 0]) for i in range(-2, 3) for j in range(-2, 3))
    assert out[y, x, 0] == (2 * a + 256) // 512 == int(np.floor(a / 256 + 0.5))


def test_two_regions_never_mix():
    h, w = 16, 24
    left = np.arange(w)[None, :] < 11
    img = np.where(left[..., None], np.uint8(10), np.uint8(250)) * np.ones((h, w, 4), np.uint8)
    img[..., 3] = 255
    for guide, vi, face in ((FACE, np.where(left, 5, 6), 0x100), (PLANE, 5, np.where(left, 0x100, 0x104)),
                            (FACE, np.where(left, -1, 6), np.where(left, 0, 0x100))):
        ids = sp.ids_from(np.broadcast_to(vi, (h, w)), np.broadcast_to(face, (h, w)))
        for step in (1, 2, 4):
            out, count = sp.spatial_pass(img, ids, step, guide)
            assert np.array_equal(out, img), (guide, step)
            assert count[8, 10] < 25 and count[8, 20 if step < 4 else 19] >= 15


def test_plane_guide_joins_coplanar_faces_only():
    """Voxels of one layer seen through the same face join under PLANE and stay apart under FACE; another
    layer, another orientation or another material byte stays apart under both."""
    h, w = 5, 10
    img = sp.random_frame(h, w, 3)
    x = np.arange(w)[None, :] + np.zeros((h, 1), np.int64)
    face = 1 | (2 << 8)                      # axis y
    row = sp.ids_from(x + N * 3 + N * N * 2, face)   # cells (x, 3, 2): one layer along y
    _, cf = sp.spatial_pass(img, row, 1, FACE)
    _, cp = sp.spatial_pass(img, row, 1, PLANE)
    assert np.all(cf[2] == 5) and cp[2, 5] == 25       # FACE: the pixel's own column only
    for other in (sp.ids_from(x + N * (3 + x % 2) + N * N * 2, face),          # alternating layers
                  sp.ids_from(x + N * 3 + N * N * 2, face | (4 * (x % 2))),    # alternating orientation
                  sp.ids_from(x + N * 3 + N * N * 2, 1 | ((2 + x % 2) << 8))):  # alternating material
        _, c = sp.spatial_pass(img, other, 1, PLANE)
        assert c[2, 5] == 15
    miss = sp.ids_from(np.full((h, w), -1), 0)
    for guide in (FACE, PLANE):
        assert sp.spatial_pass(img, miss, 1, guide)[1][2, 5] == 25    # all misses share one key


def test_kept_pixels_pass_through_and_still_serve_as_taps():
    h, w = 9, 9
    img = np.zeros((h, w, 4), np.uint8)
    img[..., 3] = 7                     # (a kept pixel keeps its A byte too)
    img[4, 4, :3] = 255
    ids = sp.ids_from(np.zeros((h, w)), 0)
    keep = np.zeros((h, w), np.uint8)
    keep[4, 4] = 3
    out, count = sp.spatial_pass(img, ids, 1, keep=keep)
    assert np.array_equal(out[4, 4], img[4, 4]) and count[4, 4] == 0
    assert out[4, 5, 0] == (2 * 255 * 24 + 256) // 512 and out[4, 5, 3] == 255 and count[4, 5] == 25
    free, _ = sp.spatial_pass(img, ids, 1)
    other = np.ones((h, w), bool)
    other[4, 4] = False
    assert np.array_equal(out[other], free[other]) and free[4, 4, 0] == (2 * 255 * 36 + 256) // 512


def test_count_on_a_small_image():
    """5x3, one key: count = the taps inside the image, by hand. Step 1: a pixel's columns x - 2 .. x + 2 hold 3,
    4, 5, 4, 3 image columns and its rows all 3 image rows; step 4: no other row is in reach and only columns 0
    and 4 reach each other; step 2: columns 0, 2, 4 reach each other, 1 and 3 each other, rows 0 and 2 each other."""
    ids = sp.ids_from(np.zeros((3, 5)), 0)
    img = sp.random_frame(3, 5, 4)
    _, c1 = sp.spatial_pass(img, ids, 1)
    assert c1.tolist() == [[9, 12, 15, 12, 9]] * 3
    _, c4 = sp.spatial_pass(img, ids, 4)
    assert c4.tolist() == [[2, 1, 1, 1, 2]] * 3
    _, c2 = sp.spatial_pass(img, ids, 2)
    assert c2.tolist() == [[6, 4, 6, 4, 6], [3, 2, 3, 2, 3], [6, 4, 6, 4, 6]]


def test_range_test_uses_rgb_only():
    h, w = 5, 5
    img = np.zeros((h, w, 4), np.uint8)
    img[..., 3] = np.arange(25, dtype=np.uint8).reshape(5, 5) * 10   # A differs everywhere: ignored
    img[2, 3, :3] = (10, 20, 18)    # |d| = 48
    img[2, 1, :3] = (10, 20, 19)    # |d| = 49
    ids = sp.ids_from(np.zeros((h, w)), 0)
    st = {}
    _, c = sp.spatial_pass(img, ids, 1, rng=48, stats=st)
    assert c[2, 2] == 24 and st["range"][2, 2] and not st["guide"].any()
    assert sp.spatial_pass(img, ids, 1, rng=49)[1][2, 2] == 25
    assert sp.spatial_pass(img, ids, 1, rng=0)[1][2, 2] == 23


# ---- conditions on the oracle's IDs (colour-free) ------------------------------------------------

@pytest.mark.parametrize("name,cam", FRAMES)
def test_oracle_ids_exercise_both_guides(built, name, cam):
    ids = sp.oracle_ids(name, cam)
    img = sp.random_frame(H, W, 5)
    outs = {}
    for guide in (FACE, PLANE):
        st = {}
        outs[guide], _ = sp.spatial_pass(img, ids, 1, guide, stats=st)
        n = int(st["guide"].sum())
        print(name, cam, "guide", guide, "pixels with a tap rejected by the guide at step 1:", n)
        assert n >= 500
    differ = int(np.any(outs[FACE] != outs[PLANE], axis=-1).sum())
    print(name, cam, "pixels where FACE and PLANE differ:", differ)
    assert differ >= 500


@pytest.mark.parametrize("name,cam", FRAMES)
def test_oracle_ids_leave_pixels_alone_at_step_4(built, name, cam):
    st = {}
    sp.spatial_pass(sp.random_frame(H, W, 6), sp.oracle_ids(name, cam), 4, FACE, stats=st)
    n = int(st["alone"].sum())
    print(name, cam, "pixels whose only valid tap is the centre, step 4, FACE:", n)
    assert n >= 1


@pytest.mark.parametrize("name,cam", FRAMES)
def test_range_48_rejects_taps_on_the_noisy_frame(built, name, cam):
    noisy, _ = sp.oracle_frames(name, cam)
    st = {}
    sp.spatial_pass(noisy, sp.oracle_ids(name, cam), 1, FACE, 48, stats=st)
    n = int(st["range"].sum())
    print(name, cam, "pixels with a range-rejected tap at range 48:", n)
    assert n >= (400 if name in ("terrain", "refraction") else 30)


# ---- usefulness ----------------------------------------------------------------------------------

@pytest.mark.parametrize("name,cam", FRAMES)
def test_three_passes_lower_the_error(built, name, cam):
    """Against the oracle's noise-free frame, RMSE over R, G, B in 8-bit LSB: three passes with the FACE guide at
    range 765 lower it on all six frames; PLANE lowers it on terrain and refraction (glass shows view-dependent
    content across a plane: DESIGN.md §6 "Spatial filter")."""
    noisy, clean = sp.oracle_frames(name, cam)
    ids = sp.oracle_ids(name, cam)
    raw = sp.rmse(noisy, clean)
    face = sp.rmse(sp.chain(noisy, ids, 3, FACE), clean)
    plane = sp.rmse(sp.chain(noisy, ids, 3, PLANE), clean)
    print(f"{name} {cam}: raw {raw:.2f}, FACE {face:.2f}, PLANE {plane:.2f}")
    assert face < raw
    if name != "glass_cube":
        assert plane < raw
