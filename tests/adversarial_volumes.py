"""Adversarial volumes, their cameras and the oracle-side conditions that keep a case from passing
empty: the inputs of tests/test_oracle_adversarial.py (the C oracle against the NumPy oracle) and of
tests/test_gpu_adversarial.py (every render path against the C oracle). The built scenes hold bytes 0
to 3, one glass block and tidy faces; these hold material bytes up to 255 (min(voxel, 3) in the colour
table, the textured slot table and the eta lookup), glass beside glass and beside opaque voxels, filled
voxels on all six faces (a sample at coordinate N reads plane 0), the empty and the all-solid volume,
and a 3-D checker lattice of glass and grass whose bounce trees are the deepest. Plain helpers, no tests."""
import functools

import numpy as np

import voxelraytracer_amd as vrt
from voxelraytracer_amd import abi

NAMES = ("bytes", "glass_clutter", "shell", "solid", "glass_solid", "empty", "lattice")
W, H = 96, 64
CAMERA_IDS = ("c0", "c1", "c2", "c3", "c4", "c5")


def build_volumes(n):
    """The seven volumes as [z][y][x] arrays (use v.reshape(-1)). The draw order is part of the
    definition: the conditions below were measured with it."""
    rng = np.random.default_rng(n)
    out = {}
    v = np.zeros((n, n, n), np.uint8)
    m = rng.random((n, n, n)) < 0.06
    v[m] = rng.choice(np.array([1, 2, 3, 4, 7, 200, 255], np.uint8), size=int(m.sum()))
    out["bytes"] = v
    v = np.zeros((n, n, n), np.uint8)
    r = rng.random((n, n, n))
    v[r < 0.30] = 2
    v[r < 0.05] = 1
    v[(r > 0.30) & (r < 0.33)] = 3
    out["glass_clutter"] = v
    v = np.zeros((n, n, n), np.uint8)
    v[0] = 1
    v[-1] = 2
    v[:, 0] = 3
    v[:, -1] = 2
    v[:, :, 0] = 200
    v[:, :, -1] = 1
    out["shell"] = v
    out["solid"] = np.full((n, n, n), 1, np.uint8)
    out["glass_solid"] = np.full((n, n, n), 2, np.uint8)
    out["empty"] = np.zeros((n, n, n), np.uint8)
    v = np.zeros((n, n, n), np.uint8)
    v[::2, ::2, ::2] = 2
    v[1::2, 1::2, 1::2] = 3
    out["lattice"] = v
    return out


@functools.lru_cache(maxsize=None)
def volumes(n):
    """{name: n^3 bytes, x fastest, read-only}."""
    out = {}
    for name, v in build_volumes(n).items():
        flat = np.ascontiguousarray(v.reshape(-1))
        flat.setflags(write=False)
        out[name] = flat
    return out


def camera_poses(n):
    """make_camera keyword arguments by id; pos is relative to the volume's centre."""
    return {
        "c0": {},                                                            # the default pose
        "c1": dict(pos=(0.0, 0.0, 0.0), rot=(0.0, 0.0, 0.0)),                # on a lattice point; inside a filled voxel of solid / glass_solid
        "c2": dict(pos=(0.5, 0.5, 0.5), rot=(-35.26439, 45.0, 0.0)),         # along the lattice diagonal
        "c3": dict(pos=(0.3, -0.2, 0.1), rot=(10.0, 170.0, 0.0)),            # a generic pose inside the volume
        "c4": dict(pos=(0.0, 0.0, n / 2 + 6.0), rot=(0.0, 0.0, 0.0)),        # outside the volume
        "c5": dict(pos=(n / 2 + 6.0, 0.5, 0.5), rot=(0.0, 90.0, 0.0)),       # outside, along an axis: TIE3 occurs
    }


def camera(n, cid, w=W, h=H):
    return vrt.make_camera(w, h, **camera_poses(n)[cid])


def base_params(refl=4, transp=4, **kw):
    kw.setdefault("reflection_noise", 0.02)
    kw.setdefault("time", 3.0)
    return vrt.default_params(refl, transp, **kw)


INSIDE = ("c0", "c1", "c2", "c3")


def check_conditions(name, cid, vox, hits, cnt):
    """The conditions of a (volume, camera) on the oracle's 96x64 colour-only frame at (R, T) = (4, 4)
    with base_params(), N = 16 or 32. The bounds are floors, not estimates; the oracle's narrowest figures,
    all at 16^3: bytes 2 048 hits (c4) and 630 secondary rays (c2), glass_clutter 44 323 (c5), lattice
    19 088 (c5), shell 11 058 (c3), glass_solid 55 296 (one tree of nine secondary rays per pixel). The
    golden fixtures of bytes and glass_clutter pin the generator's draws at 16^3."""
    found = hits["voxel_index"] >= 0
    nhit, nmiss = int(np.count_nonzero(found)), int(np.count_nonzero(~found))
    sec = cnt["secondary_rays"]
    what = (name, cid, nhit, nmiss, sec)
    if name == "bytes":
        assert nhit >= 2000 and nmiss >= 800 and sec >= 600, what
    if name == "glass_clutter":
        assert sec >= 40000, what
    if name == "lattice":
        assert sec >= 19000, what
    if name == "shell" and cid in ("c3", "c4"):
        assert sec >= 10000, what
    if name == "glass_solid" and cid in INSIDE:
        assert sec >= 55000, what
    if name == "empty":
        assert nhit == 0, what
    if name == "solid" and cid in INSIDE:
        assert nmiss == 0 and int(hits["steps"].max()) <= 2, what + (int(hits["steps"].max()),)
    if cid == "c5":
        assert cnt["tie3"] > 0 and np.any(hits["flags"] & abi.VRT_HIT_FLAG_TIE3), what + (cnt["tie3"],)


def sees_a_clamped_byte(vox, hits):
    """Whether some pixel's primary hit voxel holds a byte >= 4 (the material clamp)."""
    vi = hits["voxel_index"]
    return bool(np.any(vox[vi[vi >= 0]] >= 4))


GOLDEN_PREFIX = "adversarial/"


def scene_volume(scene, n, seed=0):
    """The bytes of a golden fixture's scene: a built scene's name, or GOLDEN_PREFIX + a name above."""
    if scene.startswith(GOLDEN_PREFIX):
        return volumes(n)[scene[len(GOLDEN_PREFIX):]]
    return vrt.build_scene(scene, n, seed)
