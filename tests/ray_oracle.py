"""The ray queries' CPU side, shared by tests/test_gpu_ray_query.py, tests/test_gpu_ray_trace.py and
tests/test_gpu_adversarial.py: the ray lists, the oracles' march, shadow march and whole ray tree of a listed
ray at N = 16 (oracle.march_one, numpy_oracle.Tracer), and the comparisons of the device's records with
them. Helper modules are not assertion-rewritten by pytest, so every assert here carries the values it
compares. Plain helpers, no tests."""
import numpy as np

import oracle
import voxelraytracer_amd as vrt
from harness import COLOR_TOL, assert_equal, float_bits, synthetic_atlas
from oracle import numpy_oracle
from voxelraytracer_amd import abi

N = 16
NOISE = {"noisy": (0.05, 0.01), "clean": (0.0, 0.0)}   # (reflection_noise, refraction_noise)
F = np.float32
Z, ONE = F(0.0), F(1.0)


def unit(d):
    d = np.asarray(d, np.float32)
    return d / np.sqrt((d * d).sum(axis=-1, keepdims=True), dtype=np.float32)


def ray_list(seed, count, n=N):
    """count rays, read-only: origins uniform in [-4, n + 4]^3; three of every four rays aimed at a uniform
    point of the volume, every fourth with an unaimed Gaussian direction (aimed rays alone never miss the
    glass cube's walls); directions normalised in float32; max_length 100, but uniform in [0.5, 12] for
    every eighth ray (among the aimed ones)."""
    rng = np.random.default_rng(seed)
    origins = rng.uniform(-4.0, n + 4.0, (count, 3)).astype(np.float32)
    targets = rng.uniform(0.0, n, (count, 3)).astype(np.float32)
    dirs = targets - origins
    unaimed = np.arange(count) % 4 == 3
    dirs[unaimed] = rng.standard_normal((count, 3)).astype(np.float32)[unaimed]
    max_len = np.full(count, 100.0, np.float32)
    short = np.arange(count) % 8 == 0
    max_len[short] = rng.uniform(0.5, 12.0, count).astype(np.float32)[short]
    rays = vrt.make_rays(origins, unit(dirs), max_len)
    rays.setflags(write=False)
    return rays


# ---- one march: oracle.march_one and numpy_oracle.Tracer.march / march_shadow --------------------

def march_all(vox, rays, max_len=None):
    """oracle.march_one per ray -> dict of arrays (found, vidx, len, point, normal, steps)."""
    n = len(rays)
    out = dict(found=np.zeros(n, bool), vidx=np.zeros(n, np.int32), len=np.zeros(n, np.float32),
               point=np.zeros((n, 3), np.float32), normal=np.zeros((n, 3), np.float32), steps=np.zeros(n, np.uint32))
    for i, r in enumerate(rays):
        m = oracle.march_one(vox, N, r["origin"], r["dir"], float(r["max_length"]) if max_len is None else max_len)
        for key in out:
            out[key][i] = m[key]
    return out


def march_tracer(vox, max_len):
    p = vrt.default_params(1, 2)
    return numpy_oracle.Tracer(vox, N, dict(sun_dir=list(p.sun_dir), time=p.time, ray_noise=0.0, reflection_noise=0.0,
                                            refraction_noise=0.0, max_ray_length=max_len, max_reflections=1,
                                            max_transparencies=2, color_only=1))


def numpy_ray(r):
    return dict(pos=tuple(F(x) for x in r["origin"]), dir=tuple(F(x) for x in r["dir"]), len=F(0.0), energy=F(1.0),
                voxel=0, r=0, t=0)


def numpy_march(vox, r):
    """Tracer.march of one vrt_ray record -> (hit dict, steps, flags)."""
    st = dict(steps=0, flags=0)
    hit = march_tracer(vox, F(r["max_length"])).march(numpy_ray(r), st)
    return hit, st["steps"], st["flags"]


def numpy_shadow(vox, r):
    """Tracer.march_shadow of one vrt_ray record -> (blocked, steps, flags)."""
    st = dict(steps=0, flags=0)
    blocked = march_tracer(vox, F(r["max_length"])).march_shadow(numpy_ray(r), st)
    return bool(blocked), st["steps"], st["flags"]


def assert_nearest_matches(hits, want, vox, rays):
    """RAY_HIT_DTYPE records against march_all's arrays, every field."""
    found = hits["voxel_index"] >= 0
    assert_equal(found, want["found"], "found")
    assert_equal(hits["voxel_index"], np.where(want["found"], want["vidx"], -1), "voxel_index")
    assert_equal(hits["steps"], want["steps"], "steps")
    assert_equal(float_bits(hits["ray_length"]), float_bits(want["len"]), "ray_length bits")
    assert_equal(float_bits(hits["point"]), float_bits(want["point"]), "point bits")
    assert_equal(vrt.hit_normal(hits), want["normal"].astype(np.int8), "normal")
    assert_equal((hits["face"][found] >> 8) & 0xFF, vox[hits["voxel_index"][found]], "face's voxel byte")
    high, miss = hits["face"][found] >> 16, hits["face"][~found]
    assert np.all(high == 0) and np.all(miss == 0), ("face bits", np.flatnonzero(high)[:5].tolist(),
                                                     np.flatnonzero(miss)[:5].tolist())
    other = hits["flags"] & ~np.uint32(abi.VRT_HIT_FLAG_TIE3 | abi.VRT_HIT_FLAG_STEP_CAP)
    assert np.all(other == 0), ("flags", np.flatnonzero(other)[:5].tolist())


# ---- the whole ray tree: numpy_oracle.Tracer -----------------------------------------------------

def make_params(bounces, noise="clean", textured=False, **kw):
    refl, refr = NOISE[noise]
    p = vrt.default_params(*bounces, reflection_noise=refl, refraction_noise=refr, time=3.0, **kw)
    return vrt.textured_params(p, synthetic_atlas()) if textured else p


def tracer(vox, p, max_len):
    d = dict(sun_dir=list(p.sun_dir), time=p.time, ray_noise=p.ray_noise, reflection_noise=p.reflection_noise,
             refraction_noise=p.refraction_noise, max_ray_length=max_len, max_reflections=p.max_reflections,
             max_transparencies=p.max_transparencies, color_only=p.color_only)
    if not p.color_only:
        d.update(atlas=synthetic_atlas(), atlas_size=p.atlas_size, atlas_texture_size=p.atlas_texture_size)
    return numpy_oracle.Tracer(vox, N, d)


def oracle_trace(tr, origin, direction):
    """The loop of Tracer.pixel (numpy_oracle.py:375-396) from stack[0] = Ray(origin, direction, 0, 1, air,
    0, 0): (colour, first pop's (voxel, length), steps and flags, secondary rays popped)."""
    stats = dict(steps=0, flags=0)
    color = (Z, Z, Z)
    stack = [dict(pos=tuple(F(x) for x in origin), dir=tuple(F(x) for x in direction), len=Z, energy=ONE,
                  voxel=0, r=0, t=0)]
    cap = tr.R + tr.T + 1
    first, rec, pops = True, (-1, Z), 0
    while stack:
        ray = stack.pop()
        if not first:
            pops += 1
        hit, color = tr.trace_with_shadow(ray, color, stats)
        if first:
            if hit["found"]:
                rec = (hit["vidx"], hit["len"])
            first = False
        if hit["found"]:
            mat = tr.mats[min(hit["voxel"], 3)]
            if mat[2] and ray["r"] < tr.R:
                if len(stack) < cap:
                    stack.append(tr.reflection_ray(ray, hit))
                else:
                    stats["flags"] |= 4
            if mat[1] and ray["t"] < tr.T and tr.color(hit)[3] != ONE:
                if len(stack) < cap:
                    stack.append(tr.refraction_ray(ray, hit))
                else:
                    stats["flags"] |= 4
    return color, rec, stats, pops


def oracle_records(vox, rays, p):
    """oracle_trace of every ray -> (RAY_COLOR_DTYPE records, secondary rays popped per ray)."""
    out = np.zeros(len(rays), abi.RAY_COLOR_DTYPE)
    pops = np.zeros(len(rays), np.int64)
    tracers = {}
    with np.errstate(all="ignore"):
        for i, r in enumerate(rays):
            ml = F(r["max_length"])
            tr = tracers.setdefault(ml.tobytes(), tracer(vox, p, ml))
            color, rec, st, pops[i] = oracle_trace(tr, r["origin"], r["dir"])
            out[i] = (rec[0], rec[1], st["steps"], st["flags"], (color[0], color[1], color[2], 1.0))
    return out, pops


def store_clamp(c):
    """The framebuffer store's clamp to [0, 1], NaN -> 0 (numpy_oracle.unorm8)."""
    return np.fmin(np.fmax(np.asarray(c, np.float32), F(0.0)), F(1.0))


def assert_matches_oracle(got, want, what=""):
    """RAY_COLOR_DTYPE records against oracle_records': voxel_index, steps, flags and the length's bits
    equal, a NaN channel NaN on both sides, the clamped colour within COLOR_TOL, alpha 1."""
    assert got.dtype == np.dtype(abi.RAY_COLOR_DTYPE) and got.shape == want.shape, (what, got.dtype, got.shape, want.shape)
    assert_equal(got["voxel_index"], want["voxel_index"], (what, "voxel_index"))
    assert_equal(got["steps"], want["steps"], (what, "steps"))
    assert_equal(got["flags"], want["flags"], (what, "flags"))
    assert_equal(float_bits(got["ray_length"]), float_bits(want["ray_length"]), (what, "ray_length bits"))
    g, w = got["rgba"][:, :3], want["rgba"][:, :3]
    assert_equal(np.isnan(g), np.isnan(w), (what, "NaN channels"))
    diff = np.abs(store_clamp(g).astype(np.float64) - store_clamp(w).astype(np.float64)).max()
    print(f"{what}: max |clamped colour difference| {diff:.3e}")
    assert diff <= COLOR_TOL, (what, "max |clamped colour difference|", float(diff), COLOR_TOL)
    assert_equal(got["rgba"][:, 3], np.ones_like(got["rgba"][:, 3]), (what, "alpha"))
