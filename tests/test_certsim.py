"""CPU model check of the certified walks (DESIGN.md §6 "Certified walks"): scripts/certsim.c runs a
certified primary and shadow walk beside the oracle's exact walks (test infrastructure) for every
pixel and counts the rays where a certified outcome (miss / first event byte + face axis / shadow
bit) disagrees with the exact walk's. Lattice cameras put rays through voxel edges and corners,
where the exact walk ties. The GPU tests (test_gpu_certified.py) check the kernel itself."""
import ctypes as C

import numpy as np
import pytest

import voxelraytracer_amd as vrt
from harness import LATTICE, load_certsim


@pytest.fixture(scope="module")
def sim(built):
    return load_certsim()


def run(L, vox, n, w, h, pos=None, rot=None):
    vox = np.ascontiguousarray(vox, np.uint8)
    L.cs_build(vox.ctypes.data, n, 64)
    kw = {} if pos is None else dict(pos=pos, rot=rot)
    cam = vrt.make_camera(w, h, **kw)
    p = vrt.default_params(4, 4)
    sun = np.array(p.sun_dir[:], np.float32)
    inv = np.array(cam.inv_pv[:], np.float32)
    o = np.zeros(32, np.float64)
    L.cs_run(inv.ctypes.data, w, h, sun.ctypes.data, C.c_float(p.max_ray_length), 1.0,
             C.c_float(1.0 / 64), o.ctypes.data)
    return o


def check(o):
    assert o[6] == 0, f"{o[6]:.0f} primary rays disagree with the exact walk"
    assert o[18] == 0, f"{o[18]:.0f} shadow rays disagree with the exact walk"
    assert o[5] + o[7] > 0.5 * o[0], "most primaries should certify"


@pytest.mark.parametrize("scene,n", [("refraction", 32), ("terrain", 64), ("glass_cube", 16),
                                     ("refraction", 128)])
def test_certified_default_camera(sim, scene, n):
    check(run(sim, vrt.build_scene(scene, n), n, 160, 90))


@pytest.mark.parametrize("li", range(len(LATTICE)))
def test_certified_lattice_cameras(sim, li):
    pos, rot = LATTICE[li]
    for scene, n in (("terrain", 32), ("refraction", 32)):
        o = run(sim, vrt.build_scene(scene, n), n, 97, 65, pos, rot)
        assert o[6] == 0 and o[18] == 0


def test_certified_random_scenes(sim):
    rng = np.random.default_rng(7)
    for n, dens in ((16, 0.05), (32, 0.01), (64, 0.002)):
        vox = np.zeros((n, n, n), np.uint8)
        m = rng.random((n, n, n)) < dens
        vox[m] = rng.choice(np.array([1, 2, 3, 200], np.uint8), size=int(m.sum()))
        vox[:, : n // 8, :] = 1
        for _ in range(2):
            pos = tuple(float(x) for x in np.round(rng.uniform(-n / 3, n / 3, 3) * 2) / 2)
            rot = (float(rng.choice([-45, -35.26439, -20])), float(rng.choice([0, 45, 135, 33.3])), 0.0)
            o = run(sim, vox.reshape(-1), n, 80, 60, pos, rot)
            assert o[6] == 0 and o[18] == 0
