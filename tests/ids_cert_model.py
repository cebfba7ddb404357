"""The certified ID kernel's frames on the CPU model (scripts/certsim.c's listed-ray walk, which runs the
kernel's start checks): a frame's primary rays as CERT_RAY_DTYPE records, the model's walk and the oracle's
exact walk of each. Shared by tests/test_render_ids_cert_cpu.py and tests/test_gpu_render_ids_cert.py; a
frame is computed once per process. Plain helpers, no tests."""
import functools

import numpy as np

import cert_rays
import harness
import voxelraytracer_amd as vrt
from voxelraytracer_amd import abi

W, H = 96, 54
SCENES = ("terrain", "glass_cube", "refraction")
# the share of exact-path pixels a frame may have: 1 % of the default camera's 16^3 frames, 10 % at the
# lattice and open cameras (conditions of the GPU tests, proved on the model by the CPU test)
CAP_DEFAULT, CAP_HARD = (W * H) // 100, (W * H) // 10


@functools.lru_cache(maxsize=None)
def scene(name, n):
    v = vrt.build_scene(name, n)
    v.setflags(write=False)
    return v


def params(ray_noise=0.0, **kw):
    return vrt.default_params(1, 2, ray_noise=ray_noise, **kw)


def camera(pos=None, rot=None, w=W, h=H):
    return vrt.make_camera(w, h) if pos is None else vrt.make_camera(w, h, pos=pos, rot=rot)


def frame_rays(cam, vox, n, p):
    """Every pixel's primary ray as it enters the march, row by row, as the walk hook's records: len0 0,
    max_length the params'."""
    pos, dirs = harness.primary_rays(cam, vox, n, p)
    r = np.zeros(cam.width * cam.height, abi.CERT_RAY_DTYPE)
    r["origin"], r["dir"] = pos.reshape(-1, 3), dirs.reshape(-1, 3)
    r["max_length"], r["len0"] = np.float32(p.max_ray_length), np.float32(0.0)
    return r


@functools.lru_cache(maxsize=None)
def model_frame(name, n, ray_noise=0.0, pos=None, rot=None):
    """-> (exact-path pixels: the model's res neither HIT nor MISS, unsound pixels: a certain outcome that is
    not the exact walk's) of the 96x54 frame."""
    vox, p = scene(name, n), params(ray_noise)
    rays = frame_rays(camera(pos, rot), vox, n, p)
    exact = cert_rays.exact_walks(vox, n, rays, 0)
    model = cert_rays.model_walks(vox, n, rays, 0)
    fallback = (model["res"] != cert_rays.HIT) & (model["res"] != cert_rays.MISS)
    return int(np.count_nonzero(fallback)), int(np.count_nonzero(cert_rays.unsound(exact, model, 0)))
