"""GPU: every render path against the CPU oracle on the adversarial volumes (tests/adversarial_volumes.py:
material bytes up to 255, glass clutter, filled faces, the solid, all-glass and empty volumes, the glass /
grass lattice) from six cameras, among them cameras inside a filled voxel, on a lattice point, along the
lattice diagonal and along an axis from outside (TIE3). The other GPU files hold the kernels against the
oracle on the three built scenes only, and hostile volumes only against another GPU instance.

  a. the hit-record instance (Renderer.render) against oracle.render under tests/test_gpu_parity.py's
     contract: voxel index, length bits, steps, flags and every counter equal, clamped colour within
     COLOR_TOL = 1e-4, alpha 1
  b. stats-free float frames in every certified / tree / exact-pass mode and both skip layouts equal (a)'s
     frame bit for bit
  c. the automatic certified mode follows the documented glass-share rule
  d. the RGB8 temporal frame under tests/test_gpu_temporal.py's contract
  e. pick, render_ids, cast_rays and trace_rays against (a)'s hit records and the oracles
  f. the packed skip field against tests/skipfield_reference.py, after uploads and after edits

Frames are 96x64, N is 16 or 32, params are adversarial_volumes.base_params(); one test per (volume, N)
loops over the cameras. The oracle's frames are computed once and shared. adversarial_volumes.check_conditions
asserts on the oracle's output that no case passes empty. Every colour comparison prints its maximum."""
import functools
import os

import numpy as np
import pytest
import torch

import harness
import oracle
import voxelraytracer_amd as vrt
from adversarial_volumes import (CAMERA_IDS, H, NAMES, W, base_params, camera, check_conditions,
                                 sees_a_clamped_byte, volumes)
from harness import (all_modes, all_pixels, assert_ids_equal_pick, assert_same_packed, check_raw, compare,
                     depth_restated, reset_modes, synthetic_atlas)
from harness import float_bits as bits
from ray_oracle import assert_matches_oracle, assert_nearest_matches, march_all, numpy_shadow, oracle_records, ray_list
from ray_oracle import make_params as ray_params
from skipfield_reference import apply_edit, packed_reference
from voxelraytracer_amd import abi

pytestmark = pytest.mark.gpu

THREADS = min(16, os.cpu_count() or 1)
SIZES = (16, 32)
BOUNCES = ((1, 2), (4, 4))
CASES = [(name, n) for name in NAMES for n in SIZES]
VARIANT_CAMERAS = ("c0", "c3")   # also rendered with ray and refraction noise, and textured


def make_params(bounces, variant="base"):
    if variant == "noisy":
        return base_params(*bounces, ray_noise=0.02, refraction_noise=0.01)
    p = base_params(*bounces)
    return vrt.textured_params(p, synthetic_atlas(32, 16), 16) if variant == "textured" else p


def variants(cid):
    return ("base", "noisy", "textured") if cid in VARIANT_CAMERAS else ("base",)


@functools.lru_cache(maxsize=None)
def oracle_frame(name, n, cid, bounces=(4, 4), variant="base"):
    rgba, hits, cnt = oracle.render(camera(n, cid), volumes(n)[name], n, make_params(bounces, variant),
                                    threads=THREADS)
    for a in (rgba, hits):
        a.setflags(write=False)
    if bounces == (4, 4) and variant == "base":   # asserted on the oracle, so no case passes empty
        check_conditions(name, cid, volumes(n)[name], hits, cnt)
        if name == "bytes":
            assert sees_a_clamped_byte(volumes(n)[name], hits), (n, cid)
    return rgba, hits, cnt


def colour_difference(rgba_g, rgba_o, what):
    d = float(np.abs(np.clip(rgba_g[..., :3], 0, 1) - np.clip(rgba_o[..., :3], 0, 1)).max())
    print(f"adversarial colour {what}: max |clamped colour difference| {d:.3e}")
    return d


def float_frame(r, cam, p):
    """The stats-free float frame (no hit records, no counters) through render_rows_async."""
    out = torch.full((cam.height, cam.width, 4), -1.0, dtype=torch.float32, device="cuda")
    r.render_rows_async(cam, p, 0, cam.height, 1, out.data_ptr())
    torch.cuda.synchronize()
    return out.cpu().numpy()


# ---- a. the hit-record instance against the C oracle ---------------------------------------------

@pytest.mark.parametrize("name,n", CASES)
def test_hit_records_match_the_oracle(built, name, n):
    vox = volumes(n)[name]
    with vrt.Renderer(0) as r:
        r.upload_volume(vox, n)
        for cid in CAMERA_IDS:
            cam = camera(n, cid)
            for bounces in BOUNCES:
                for variant in variants(cid):
                    rgba_o, hits_o, cnt_o = oracle_frame(name, n, cid, bounces, variant)
                    rgba_g, hits_g, st = r.render(cam, make_params(bounces, variant))
                    colour_difference(rgba_g, rgba_o, f"{name} {n} {cid} R{bounces[0]}T{bounces[1]} {variant}")
                    compare(rgba_g, hits_g, st, rgba_o, hits_o, cnt_o)
            oracle_frame(name, n, cid)   # the conditions, whatever the order of the loops above


# ---- b. stats-free frames in every mode and both layouts -----------------------------------------

@pytest.mark.parametrize("name,n", CASES)
def test_stats_free_frames_equal_the_exact_frame(built, name, n):
    vox = volumes(n)[name]
    with vrt.Renderer(0) as r:
        want = {}
        for layout in (8, 1):
            reset_modes(r)
            r.set_skip_layout(layout)
            r.upload_volume(vox, n)   # a layout takes effect at the next upload
            assert r._lib.vrt_volume_octants(r._h) == layout
            for cid in CAMERA_IDS:
                cam = camera(n, cid)
                for variant in variants(cid):
                    p = make_params((4, 4), variant)
                    reset_modes(r)
                    exact, hits, _ = r.render(cam, p)
                    if layout == 8:   # (a)'s frame: the exact instance's, whose hit records are the oracle's
                        _, hits_o, _ = oracle_frame(name, n, cid, (4, 4), variant)
                        assert np.array_equal(hits["voxel_index"], hits_o["voxel_index"])
                        assert np.array_equal(bits(hits["ray_length"]), bits(hits_o["ray_length"]))
                        want[cid, variant] = exact
                    assert np.array_equal(bits(exact), bits(want[cid, variant])), (layout, cid, variant)
                    for mode in all_modes(r):
                        got = float_frame(r, cam, p)
                        bad = np.argwhere(np.any(bits(got) != bits(want[cid, variant]), axis=-1))
                        assert bad.size == 0, (layout, cid, variant, mode, len(bad), bad[:5].tolist())


# ---- c. the automatic mode -----------------------------------------------------------------------

@pytest.mark.parametrize("name,n", CASES)
def test_automatic_mode_follows_the_glass_share(built, name, n):
    """vrt_set_certified's automatic mode (0) certifies unless glass (byte 2) makes up more than 1 / 8 of the
    non-empty voxels: derive_glass_flags (csrc/vrt_volume.cpp) keeps it on while glass * 8 <= non_empty.
    `empty` has zero non-empty voxels: 0 * 8 <= 0 holds, so certified() is True; `glass_solid` is all
    glass: False. With certified bounce trees at their default (1) a glass-heavy volume stays certified
    through the trees, so certified() is True for every volume. The frames are equal in either mode."""
    vox = volumes(n)[name]
    glass, non_empty = int(np.count_nonzero(vox == 2)), int(np.count_nonzero(vox))
    expect = glass * 8 <= non_empty
    assert expect is {"empty": True, "glass_solid": False}.get(name, expect)
    cam, p = camera(n, "c3"), make_params((4, 4))
    with vrt.Renderer(0) as r:
        r.upload_volume(vox, n)
        assert r.certified() is True          # cert_trees = 1, the default
        r.set_cert_trees(0)
        assert r.certified() is expect        # the glass-share rule alone
        auto = float_frame(r, cam, p)
        r.set_certified(1)
        assert r.certified() is True
        on = float_frame(r, cam, p)
        r.set_certified(-1)
        assert r.certified() is False
        off = float_frame(r, cam, p)
        exact, _, _ = r.render(cam, p)
    assert np.array_equal(bits(auto), bits(exact))
    assert np.array_equal(bits(on), bits(exact))
    assert np.array_equal(bits(off), bits(exact))


# ---- d. the RGB8 temporal frame ------------------------------------------------------------------

@pytest.mark.parametrize("name,n", CASES)
def test_temporal_frame(built, name, n):
    vox = volumes(n)[name]
    p = make_params((4, 4))
    rng = np.random.default_rng(n + NAMES.index(name))
    near = 0
    with vrt.Renderer(0) as r:
        r.upload_volume(vox, n)
        for cid in CAMERA_IDS:
            cam = camera(n, cid)
            prev = rng.integers(0, 256, (H, W, 4), dtype=np.uint8)
            d_prev = torch.from_numpy(prev).cuda()
            d_cur = torch.zeros((H, W, 4), dtype=torch.uint8, device="cuda")
            d_raw = torch.zeros((H, W, 4), dtype=torch.uint8, device="cuda")
            r.render_temporal_rows_async(cam, p, 0.5, 0, H, 1, d_prev.data_ptr(), d_cur.data_ptr(), d_raw.data_ptr())
            torch.cuda.synchronize()
            raw, cur = d_raw.cpu().numpy(), d_cur.cpu().numpy()
            assert np.array_equal(cur, oracle.temporal_from_raw(raw, prev, 0.5)), cid
            near += check_raw(raw, oracle_frame(name, n, cid)[0])
    print(f"{name} {n}: {near} bytes one LSB from the oracle's, each within COLOR_TOL of a rounding boundary")


# ---- e. queries ----------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def primary_rays(n, cid):
    """pos and dir of every pixel's primary ray as it entered RayMarch (harness.primary_rays). The ray depends
    on the volume through its size alone, so the empty volume serves, whose trees are one ray."""
    return harness.primary_rays(camera(n, cid), volumes(n)["empty"], n, make_params((4, 4)))


@pytest.mark.parametrize("name,n", CASES)
def test_pick_and_ids_equal_the_hit_records(built, name, n):
    vox = volumes(n)[name]
    p = make_params((4, 4))
    pixels = all_pixels(W, H)
    with vrt.Renderer(0) as r:
        r.upload_volume(vox, n)
        for cid in CAMERA_IDS:
            cam = camera(n, cid)
            _, hits_o, _ = oracle_frame(name, n, cid)
            _, hits, _ = r.render(cam, p)
            assert np.array_equal(hits["voxel_index"], hits_o["voxel_index"])
            assert np.array_equal(bits(hits["ray_length"]), bits(hits_o["ray_length"]))
            picks = r.pick(cam, p, pixels).reshape(H, W)
            ids, depth = r.render_ids(cam, p)
            assert np.array_equal(picks["voxel_index"], hits["voxel_index"]), cid
            assert np.array_equal(bits(picks["ray_length"]), bits(hits["ray_length"])), cid
            assert np.array_equal(ids["voxel_index"], hits["voxel_index"]), cid
            assert_ids_equal_pick(ids, picks, (name, n, cid))
            found = picks["voxel_index"] >= 0
            assert np.array_equal((picks["face"][found] >> 8) & 0xFF, vox[picks["voxel_index"][found]]), cid
            assert np.all(np.isposinf(depth[~found]))
            want = depth_restated(picks, *primary_rays(n, cid))
            bad = np.argwhere(depth.view(np.uint32) != want.view(np.uint32))
            assert bad.size == 0, (cid, len(bad), bad[:5].tolist())


RAYS = 300


@functools.lru_cache(maxsize=None)
def rays16():
    return ray_list(1600, RAYS)


@pytest.mark.parametrize("name", NAMES)
def test_cast_rays_match_the_oracles(built, name):
    """nearest: every field against oracle.march_one; occlusion: the blocked bit, the steps and the flags
    against numpy_oracle.Tracer.march_shadow (tests/ray_oracle.py). N = 16."""
    vox, rays = volumes(16)[name], rays16()
    near_want = march_all(vox, rays)
    occ_want = [numpy_shadow(vox, ray) for ray in rays]
    blocked = np.array([w[0] for w in occ_want])
    print(f"{name}: {int(near_want['found'].sum())} nearest hits, {int(blocked.sum())} blocked of {RAYS}")
    if name == "empty":
        assert not near_want["found"].any() and not blocked.any()
    else:
        assert np.count_nonzero(near_want["found"]) >= 100
        assert (np.count_nonzero(blocked) >= 100) == (name != "glass_solid")
    if name == "glass_solid":   # all glass: seen, but never blocking
        assert not blocked.any()
    with vrt.Renderer(0) as r:
        r.upload_volume(vox, 16)
        near = r.cast_rays(rays, "nearest")
        occ = r.cast_rays(rays, "occlusion")
    assert_nearest_matches(near, near_want, vox, rays)
    assert np.array_equal((occ["flags"] & abi.VRT_RAY_FLAG_BLOCKED) != 0, blocked)
    assert np.array_equal(occ["steps"], np.array([w[1] for w in occ_want], np.uint32))
    assert np.array_equal(occ["flags"] & ~np.uint32(abi.VRT_RAY_FLAG_BLOCKED), np.array([w[2] for w in occ_want], np.uint32))
    assert np.all(occ["voxel_index"] == -1) and np.all(occ["ray_length"] == 0)


@pytest.mark.parametrize("name,textured", [("bytes", False), ("glass_clutter", False), ("glass_clutter", True),
                                           ("lattice", False)])
def test_trace_rays_match_the_numpy_oracle(built, name, textured):
    """The same rays through the whole ray tree at (4, 4) against numpy_oracle.Tracer
    (tests/ray_oracle.py::oracle_records), once textured. N = 16."""
    vox, rays = volumes(16)[name], rays16()
    p = ray_params((4, 4), "noisy", textured)
    want, pops = oracle_records(vox, rays, p)
    hits = int(np.count_nonzero(want["voxel_index"] >= 0))
    print(f"{name}: {hits} hits, {np.count_nonzero(pops)} rays with secondary rays, at most {pops.max()} per ray")
    assert hits >= 100 and RAYS - hits >= 25 and np.count_nonzero(pops) >= 10
    if name != "bytes":
        assert np.count_nonzero(pops) >= 100 and pops.max() > 6
    with vrt.Renderer(0) as r:
        r.upload_volume(vox, 16)
        got = r.trace_rays(rays, ray_params((4, 4), "noisy", textured))
    assert_matches_oracle(got, want, f"adversarial colour {name} 16 rays R4T4 {'textured' if textured else 'noisy'}")


# ---- f. the skip field ---------------------------------------------------------------------------

@pytest.mark.parametrize("layout", [8, 1])
@pytest.mark.parametrize("name", NAMES)
def test_skip_field_matches_the_reference(built, name, layout):
    """Every texel of the packed volume(s), the plane-N texels included. `empty` has the skip distances at
    their caps (bounded by the faces), the full volumes have zero everywhere."""
    n, vox = 16, volumes(16)[name]
    want = packed_reference(vox, n, layout)
    if name in ("solid", "glass_solid"):
        assert np.all(want >> 8 == 0)
    if name == "empty":
        assert (want >> 8).max() == (n - 1 if layout == 8 else n // 2)
    with vrt.Renderer(0) as r:
        r.set_skip_layout(layout)
        r.upload_volume(vox, n)
        assert_same_packed(r.debug_packed_volume(), want)


def split_boxes(n):
    """Three boxes (origin (x, y, z), extent (x, y, z)) that tile the volume; between them they touch
    every face."""
    a, b = n // 2 - 1, n // 2 + 1
    return [((0, 0, 0), (a, n, n)), ((a, 0, 0), (n - a, b, n)), ((a, b, 0), (n - a, n - b, n))]


def block_of(vox, n, origin, extent):
    (x, y, z), (ex, ey, ez) = origin, extent
    return vox.reshape(n, n, n)[z:z + ez, y:y + ey, x:x + ex].copy()


@pytest.mark.parametrize("layout", [8, 1])
def test_edits_between_the_extremes(built, layout):
    """update_volume turns `empty` into `bytes` by three boxes that touch every face, and `solid` into
    `empty` by one whole-volume box: the packed volume is byte-identical to a full upload of the target
    (and to the reference), and the automatic mode's counts follow."""
    n = 16
    vols = volumes(n)
    boxes = split_boxes(n)
    covered = np.zeros((n, n, n), bool)
    for (x, y, z), (ex, ey, ez) in boxes:
        assert not covered[z:z + ez, y:y + ey, x:x + ex].any()
        covered[z:z + ez, y:y + ey, x:x + ex] = True
    assert covered.all()
    for a in range(3):   # each face of the volume is touched by a box
        assert any(o[a] == 0 for o, e in boxes) and any(o[a] + e[a] == n for o, e in boxes)
    plans = [("empty", "bytes", boxes), ("solid", "empty", [((0, 0, 0), (n, n, n))])]
    for start, target, edits in plans:
        with vrt.Renderer(0) as r, vrt.Renderer(0) as f:
            for ctx in (r, f):
                ctx.set_skip_layout(layout)
                ctx.set_cert_trees(0)   # certified() then shows the glass-share rule alone
            r.upload_volume(vols[start], n)
            state = vols[start]
            for origin, extent in edits:
                block = block_of(vols[target], n, origin, extent)
                r.update_volume(origin, block)
                state = apply_edit(state, n, origin, block)
            assert np.array_equal(state, vols[target])
            f.upload_volume(vols[target], n)
            got, fresh = r.debug_packed_volume(), f.debug_packed_volume()
            assert got.tobytes() == fresh.tobytes(), (start, target)
            assert_same_packed(got, packed_reference(vols[target], n, layout))
            assert r.certified() == f.certified()
            cam, p = camera(n, "c3"), make_params((4, 4))
            assert np.array_equal(bits(float_frame(r, cam, p)), bits(float_frame(f, cam, p)))
