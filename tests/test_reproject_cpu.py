"""The reprojected temporal filter on the CPU: vrt_camera_forward against NumPy's inverse, and the conditions
the GPU tests (tests/test_gpu_reproject.py) rely on, asserted on the oracle's data with the NumPy restatement
(tests/reproject_reference.py): a static camera fetches every pixel's own history, a moved camera meets every
outcome. 16^3 volumes, 96x54 frames. No GPU."""
import ctypes as C

import numpy as np
import pytest

import voxelraytracer_amd as vrt
from voxelraytracer_amd import abi

import reproject_reference as ref
from reproject_reference import H, N, W


@pytest.mark.parametrize("name", ["A", "B", "C"])
def test_camera_forward_is_the_inverse(built, name):
    """Both inverses are computed in double; the library's is rounded to float32: one ulp (6e-8 relative)
    plus the conditioning of a well-conditioned 4x4 inverse is far inside rtol 1e-6, atol 1e-6 max|PV|."""
    cam = ref.camera(name)
    pv = vrt.camera_forward(cam)
    assert pv.dtype == np.float32 and pv.shape == (16,)
    inv = np.array(cam.inv_pv, np.float64).reshape(4, 4).T   # column-major -> [row][col]
    want = np.linalg.inv(inv).T.reshape(16)
    assert np.allclose(pv.astype(np.float64), want, rtol=1e-6, atol=1e-6 * np.abs(want).max())
    # and it is a forward matrix: PV * invPV = I
    prod = pv.astype(np.float64).reshape(4, 4).T @ inv
    assert np.allclose(prod, np.eye(4), atol=1e-4)


def test_camera_forward_rejects(built):
    L = vrt.lib()
    cam = ref.camera("A")
    out = np.full(16, 7.0, np.float32)
    assert L.vrt_camera_forward(None, out.ctypes.data) == abi.VRT_ERR_INVALID
    assert L.vrt_camera_forward(C.byref(cam), None) == abi.VRT_ERR_INVALID
    zero = vrt.make_camera(W, H)
    for i in range(16):
        zero.inv_pv[i] = 0.0
    twin = ref.camera("A")   # two equal columns
    for r in range(4):
        twin.inv_pv[1 * 4 + r] = twin.inv_pv[0 * 4 + r]
    nan = ref.camera("A")
    nan.inv_pv[5] = float("nan")
    for bad in (zero, twin, nan):
        assert L.vrt_camera_forward(C.byref(bad), out.ctypes.data) == abi.VRT_ERR_INVALID
        with pytest.raises(vrt.VrtError):
            vrt.camera_forward(bad)
    assert np.all(out == 7.0)   # a failed call writes nothing
    assert L.vrt_camera_forward(C.byref(cam), out.ctypes.data) == abi.VRT_OK


def restated(name, cur, prev):
    """src of a frame of camera `cur` against a previous frame of camera `prev`, all from the oracle, at
    ray_noise 0, with a constant grey history (the colours do not enter src)."""
    f, g = ref.oracle_frame(name, cur), ref.oracle_frame(name, prev)
    grey = np.full((H, W, 4), 128, np.uint8)
    out, src = ref.reproject(f["ids"], f["depth"], f["pos"], f["dir"], N, vrt.camera_forward(ref.camera(prev)),
                             g["ids"], grey, grey, 0.3)
    assert out.shape == (H, W, 4) and src.shape == (H, W) and src.dtype == np.int32
    return src


@pytest.mark.parametrize("name", ref.SCENES)
def test_static_camera_fetches_the_own_pixel(built, name):
    """The frame loop's static-camera test needs this: with an unmoved camera at ray_noise 0, every pixel's
    surface point (and the sky's point at infinity) lands in the pixel it came from."""
    src = restated(name, "A", "A")
    own = np.arange(W * H, dtype=np.int32).reshape(H, W)
    bad = np.argwhere(src != own)
    assert bad.size == 0, (len(bad), bad[:5].tolist(), src[tuple(bad[:5].T)].tolist())


@pytest.mark.parametrize("name", ["terrain", "refraction"])
def test_moved_cameras_meet_every_outcome(built, name):
    """A -> B: accepted samples, -1 and -3; A -> C (a turn past 90 degrees): -2 as well."""
    b = ref.counts(restated(name, "B", "A"))
    print(name, "A->B", b)
    assert b["accepted"] > 0 and b[ref.OUTSIDE] > 0 and b[ref.MISMATCH] > 0 and b[ref.NO_HISTORY] == 0
    c = ref.counts(restated(name, "C", "A"))
    print(name, "A->C", c)
    assert c["accepted"] > 0 and c[ref.OUTSIDE] > 0 and c[ref.BEHIND] > 0 and c[ref.MISMATCH] > 0
    assert sum(c.values()) == W * H


def test_no_history_is_raw(built):
    f = ref.oracle_frame("terrain", "A")
    raw = np.random.default_rng(3).integers(0, 256, (H, W, 4), dtype=np.uint8)
    out, src = ref.reproject(f["ids"], f["depth"], f["pos"], f["dir"], N, np.zeros(16, np.float32), None, None, raw,
                             0.3)
    assert np.array_equal(out, raw) and np.all(src == ref.NO_HISTORY)
