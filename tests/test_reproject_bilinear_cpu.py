"""The bilinear history fetch on the CPU: header, Python mirror and built library agree on the two new entry
points; the restatement (tests/reproject_bilinear_reference.py) gives hand-computed answers; and the conditions
the GPU tests (tests/test_gpu_reproject_bilinear.py) rely on hold on the oracle's data at ray_noise 0: 16^3
volumes, 96x54 frames. No GPU."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import voxelraytracer_amd as vrt
from voxelraytracer_amd import abi

import reproject_bilinear_reference as bil
import reproject_reference as ref
from reproject_reference import H, N, W

f32 = np.float32
HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "vrt.h")
PAIRS = (("B", "A"), ("C", "A"), ("A", "B"))   # (current, previous): A->B, A->C, B->A


def test_header_mirror_and_library_agree(built):
    with open(HEADER) as f:
        text = f.read()
    assert re.search(r"^#define VRT_ABI_VERSION 15$", text, re.M)
    assert re.search(r"enum \{ VRT_FETCH_NEAREST = 0, VRT_FETCH_BILINEAR = 1 \};", text)
    lib = C.CDLL(abi.LIB_PATH)
    for name, nargs in (("vrt_reproject_temporal_fetch_async", 19), ("vrt_set_reprojected_fetch", 2)):
        decl = re.search(r"^int " + name + r"\(([^;]*)\);", text, re.M)
        assert decl, name
        assert len(decl.group(1).split(",")) == nargs, (name, decl.group(1))
        restype, argtypes = abi.SIGNATURES[name]
        assert restype is C.c_int and len(argtypes) == nargs, name
        assert abi.ADDED_IN[name] == 16, name
        assert getattr(lib, name) is not None
    assert lib.vrt_abi_version() == 15
    assert vrt.FETCH_NEAREST == 0 and vrt.FETCH_BILINEAR == 1
    assert callable(vrt.Renderer.reproject_temporal_fetch_async) and callable(vrt.Renderer.set_reprojected_fetch)


# ---- known answers by hand ---------------------------------------------------------------------------

def test_taps_of_a_point_on_a_texel_row():
    """sx = 2.0, sy = 1.5: tx = 1.5, ty = 1.0, so ix0 = 1, fx = 0.5, iy0 = 1, fy = 0: taps 0 and 1 weigh 0.5
    each, taps 2 and 3 weigh 0 and are invalid whatever they show."""
    coords, w = bil.taps(f32(2.0), f32(1.5))
    assert coords.tolist() == [[1, 1], [2, 1], [1, 2], [2, 2]]
    assert w.dtype == f32 and w.tolist() == [0.5, 0.5, 0.0, 0.0]
    raw = np.array([9, 9, 9, 255], np.uint8)
    tb = np.array([[0, 0, 0, 255], [255, 255, 255, 255], [77, 77, 77, 255], [77, 77, 77, 255]], np.uint8)
    # bytes 0 and 255 at alpha 0: 255 * 0.5 = 127.5, rint to even = 128
    out, wsum = bil.blend(raw, tb, w > 0, w, 0.0)
    assert out.tolist() == [128, 128, 128, 255] and wsum == f32(1.0)
    # only tap 1 valid: exactly tap 1's byte, for every byte
    for b in range(256):
        tb[1, :3] = b
        out, wsum = bil.blend(raw, tb, np.array([False, True, False, False]), w, 0.0)
        assert out.tolist() == [b, b, b, 255] and wsum == f32(0.5), b


def test_taps_of_a_corner_point():
    """sx = sy = 0.25: tx = ty = -0.25, ix0 = iy0 = -1, fx = fy = 0.75: only tap 3 = (0, 0) lies in the image,
    with w3 = 0.5625; alone it returns its own byte exactly, for every byte, at alpha 0."""
    coords, w = bil.taps(f32(0.25), f32(0.25))
    assert coords.tolist() == [[-1, -1], [0, -1], [-1, 0], [0, 0]]
    assert w.tolist() == [0.0625, 0.1875, 0.1875, 0.5625]
    for (iw, ih) in ((1, 1), (16, 8), (W, H)):
        assert bil.in_image(coords, iw, ih).tolist() == [False, False, False, True]
    valid = bil.in_image(coords, W, H) & (w > 0)
    raw = np.array([1, 2, 3, 255], np.uint8)
    tb = np.zeros((4, 4), np.uint8)
    for b in range(256):
        tb[3] = (b, 255 - b, b ^ 0x55, 255)
        out, wsum = bil.blend(raw, tb, valid, w, 0.0)
        assert out.tolist() == [b, 255 - b, b ^ 0x55, 255] and wsum == f32(0.5625), b


def test_a_pixel_no_tap_agrees_with_is_rejected():
    """Static camera A, one pixel's ID changed so that it differs from all four taps' IDs: code -3, raw colour;
    every other pixel is as before."""
    f = ref.oracle_frame("terrain", "A")
    pv = vrt.camera_forward(ref.camera("A"))
    rng = np.random.default_rng(5)
    raw = rng.integers(0, 256, (H, W, 4), dtype=np.uint8)
    prev = rng.integers(0, 256, (H, W, 4), dtype=np.uint8)
    base = bil.bilinear(f["ids"], f["depth"], f["pos"], f["dir"], N, pv, f["ids"], prev, raw, 0.3)
    ids = f["ids"].copy()
    py, px = H // 2, W // 2
    assert base[1][py, px] == py * W + px
    ids["face"][py, px] ^= 0x100   # another material byte: no previous record has it
    out, src, mask, _ = bil.bilinear(ids, f["depth"], f["pos"], f["dir"], N, pv, f["ids"], prev, raw, 0.3)
    assert src[py, px] == bil.MISMATCH and mask[py, px] == 0 and np.array_equal(out[py, px], raw[py, px])
    keep = np.ones((H, W), bool)
    keep[py, px] = False
    assert np.array_equal(out[keep], base[0][keep]) and np.array_equal(src[keep], base[1][keep])
    assert np.array_equal(mask[keep], base[2][keep])


def test_no_history_is_raw():
    f = ref.oracle_frame("terrain", "A")
    raw = np.random.default_rng(3).integers(0, 256, (H, W, 4), dtype=np.uint8)
    for mode in (bil.FETCH_NEAREST, bil.FETCH_BILINEAR):
        out, src, mask = bil.fetch(mode, f["ids"], f["depth"], f["pos"], f["dir"], N, np.zeros(16, f32), None, None,
                                   raw, 0.3)
        assert np.array_equal(out, raw) and np.all(src == bil.NO_HISTORY) and not mask.any()


# ---- conditions the GPU tests rely on, on the oracle's data --------------------------------------------

def stats(name, cur, prev):
    f, g = ref.oracle_frame(name, cur), ref.oracle_frame(name, prev)
    return bil.tap_stats(f["ids"], f["depth"], f["pos"], f["dir"], N, vrt.camera_forward(ref.camera(prev)), g["ids"])


@pytest.mark.parametrize("name", ref.SCENES)
def test_static_camera_accepts_every_pixel(built, name):
    s = stats(name, "A", "A")
    own = np.arange(W * H, dtype=np.int32).reshape(H, W)
    assert np.array_equal(s["src"], own)
    print(name, "A->A wsum min", float(s["wsum"].min()), "masks", np.bincount(s["mask"].ravel(), minlength=16).tolist())
    assert np.all(s["wsum"] > f32(0.999))


@pytest.mark.parametrize("cur,prev", PAIRS)
@pytest.mark.parametrize("name", ref.SCENES)
def test_moved_cameras_meet_every_tap_outcome(built, name, cur, prev):
    s = stats(name, cur, prev)
    src, mask, nsrc = s["src"], s["mask"], s["nearest_src"]
    acc = src >= 0
    partial = int(np.count_nonzero(acc & (mask != 15)))
    rescued = int(np.count_nonzero(acc & ((mask & s["nearest_bit"]) == 0)))
    none = int(np.count_nonzero(src == bil.MISMATCH))
    border = int(np.count_nonzero(s["border"]))
    print(name, prev + "->" + cur, "accepted", int(acc.sum()), "partial", partial, "rescued", rescued, "no valid tap", none,
          "tap outside", border)
    assert partial >= 100 and rescued >= 20 and none >= 1 and border >= 12
    # the codes -4, -2 and -1 fall where the nearest restatement puts them
    for code in (bil.NO_HISTORY, bil.BEHIND, bil.OUTSIDE):
        assert np.array_equal(src == code, nsrc == code), code
    # what the nearest restatement accepts is accepted, with its nearest tap's bit set and the same src
    nacc = nsrc >= 0
    assert np.all(acc[nacc]) and np.all((mask[nacc] & s["nearest_bit"][nacc]) != 0)
    assert np.array_equal(src[nacc], nsrc[nacc])
    # and the rescued pixels are exactly those the nearest restatement rejects by the IDs
    assert rescued == int(np.count_nonzero(acc & (nsrc == bil.MISMATCH)))
    assert np.all(mask[~acc] == 0)
