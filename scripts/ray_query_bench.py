#!/usr/bin/env python3
"""Ray queries against the hit-record frame (DESIGN.md §6 "Ray queries").

Per volume (C3's refraction 128^3, C4's terrain 512^3), GPU time of one launch, from the device
timestamps of vrt_set_launch_timing (recorded when the kernel starts and ends on the device):
  frame      what a caller had to do before: vrt_render_rows_async with d_out_hit over the whole
             1920x1080 benchmark camera (the exact-walk, counted instance: primary ray, shadow rays
             and bounce trees of every pixel);
  pick       vrt_pick_pixels' kernel over every pixel of that camera (the primary ray built in the
             kernel, then one march), pixels listed 8x8 tile by tile as a frame's waves hold them, and
             listed row by row;
  cast       vrt_cast_rays_async (nearest) on the same primary rays read from a buffer (built on the host
             with the vertex stage's float32 operations), in the tile order;
  scattered  2 M rays of the tests' incoherent distribution (origins around the volume, three in four
             aimed at a point of it, every eighth with a short max_length), nearest and occlusion.
Each figure is the median of --reps launches after --warmup, taken in three runs over all arms in one
process; the spread is (max - min) / median of the three medians.

  python scripts/ray_query_bench.py [--reps 21] [--warmup 3] [--out profiles/ray_query_bench.txt]
"""
import argparse
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import voxelraytracer_amd as vrt  # noqa: E402
from voxelraytracer_amd import abi  # noqa: E402

W, H = 1920, 1080
SCATTERED = 2_000_000
F = np.float32


def tile_order_pixels():
    """Every pixel, 8x8 tile by tile (tiles row-major, lane l of a tile at (l % 8, l // 8))."""
    ty, tx, ly, lx = np.meshgrid(np.arange(H // 8), np.arange(W // 8), np.arange(8), np.arange(8), indexing="ij")
    return np.stack([(tx * 8 + lx).reshape(-1), (ty * 8 + ly).reshape(-1)], axis=1).astype(np.int32)


def row_order_pixels():
    y, x = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    return np.stack([x.reshape(-1), y.reshape(-1)], axis=1).astype(np.int32)


def normalize(v):
    return v * (F(1.0) / np.sqrt(v[:, 0] * v[:, 0] + v[:, 1] * v[:, 1] + v[:, 2] * v[:, 2]))[:, None]


def primary_rays(cam, n, pixels, max_length):
    """The frame's primary rays at ray_noise 0 (vertex stage at the pixel centre, voxel.glsl:467-472,
    then main's stack[0], :430), one float32 operation per shader operation."""
    m = np.array(cam.inv_pv, np.float32)
    x = (F(2.0) * (pixels[:, 0].astype(np.float32) + F(0.5))) / F(cam.width) - F(1.0)
    y = (F(2.0) * (pixels[:, 1].astype(np.float32) + F(0.5))) / F(cam.height) - F(1.0)

    def mul(z):
        return [((m[i] * x + m[4 + i] * y) + m[8 + i] * z) + m[12 + i] * F(1.0) for i in range(4)]

    n4, f4 = mul(F(-1.0)), mul(F(1.0))
    near = np.stack([n4[i] / n4[3] for i in range(3)], axis=1)
    far = np.stack([f4[i] / f4[3] for i in range(3)], axis=1)
    dirs = normalize(normalize(far - near))   # RandomizeDirection at noise 0 re-normalises
    return vrt.make_rays(near + F(n) * F(0.5), dirs, max_length)


def scattered_rays(n, count, seed):
    """The distribution of tests/test_gpu_ray_query.py, scaled to the volume: origins uniform in
    [-n/4, n + n/4]^3, three of four aimed at a uniform point of the volume, every fourth an unaimed
    Gaussian direction, max_length 100 n / 16, every eighth uniform in [n/32, 3 n / 4]."""
    rng = np.random.default_rng(seed)
    origins = rng.uniform(-n / 4, n + n / 4, (count, 3)).astype(np.float32)
    dirs = rng.uniform(0.0, n, (count, 3)).astype(np.float32) - origins
    unaimed = np.arange(count) % 4 == 3
    dirs[unaimed] = rng.standard_normal((count, 3)).astype(np.float32)[unaimed]
    max_len = np.full(count, 100.0 * n / 16, np.float32)
    short = np.arange(count) % 8 == 0
    max_len[short] = rng.uniform(n / 32, 0.75 * n, count).astype(np.float32)[short]
    return vrt.make_rays(origins, normalize(dirs), max_len)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=21)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ray_query_bench.txt"))
    args = ap.parse_args()
    import torch

    lines, results = [], []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    def device(a):
        return torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).cuda()

    tiles, rows = tile_order_pixels(), row_order_pixels()
    for name, scene, n, refl, transp in (("C3", "refraction", 128, 4, 4), ("C4", "terrain", 512, 4, 2)):
        vox = vrt.build_scene(scene, n)
        cam = vrt.make_camera(W, H)
        p = vrt.default_params(refl, transp)
        with vrt.Renderer(0) as r:
            r.upload_volume(vox, n)
            d_rgba = torch.empty(W * H * 4, dtype=torch.float32, device="cuda")
            d_fhit = torch.empty(W * H * 16, dtype=torch.uint8, device="cuda")
            prim = primary_rays(cam, n, tiles, p.max_ray_length)
            scat = scattered_rays(n, SCATTERED, seed=n)
            d_prim, d_scat = device(prim), device(scat)
            d_hits = torch.empty(max(SCATTERED, W * H) * 32, dtype=torch.uint8, device="cuda")
            torch.cuda.synchronize()
            arms = {
                "frame": (W * H, lambda: r.render_rows_async(cam, p, 0, H, 1, d_rgba.data_ptr(), d_fhit.data_ptr())),
                "pick_tiles": (W * H, lambda: r.pick(cam, p, tiles)),
                "pick_rows": (W * H, lambda: r.pick(cam, p, rows)),
                "cast_primary": (W * H, lambda: r.cast_rays_async(d_prim.data_ptr(), W * H, d_hits.data_ptr(), "nearest")),
                "scattered_nearest": (SCATTERED, lambda: r.cast_rays_async(d_scat.data_ptr(), SCATTERED,
                                                                           d_hits.data_ptr(), "nearest")),
                "scattered_occlusion": (SCATTERED, lambda: r.cast_rays_async(d_scat.data_ptr(), SCATTERED,
                                                                             d_hits.data_ptr(), "occlusion")),
            }
            # the arms answer the same question: the pick's first 8 bytes are the frame's hit records, and
            # the host-built primary rays are the kernel's
            picks = r.pick(cam, p, tiles)
            arms["frame"][1]()
            torch.cuda.synchronize()
            fhit = d_fhit.cpu().numpy().view(abi.HIT_DTYPE).reshape(H, W)[tiles[:, 1], tiles[:, 0]]
            same_frame = bool(np.array_equal(picks["voxel_index"], fhit["voxel_index"]) and
                              np.array_equal(picks["ray_length"].view(np.uint32), fhit["ray_length"].view(np.uint32)))
            casts = r.cast_rays(prim)
            same_cast = int(np.count_nonzero(casts.view(np.uint8).reshape(-1, 32) != picks.view(np.uint8).reshape(-1, 32)))
            hit_share = float(np.mean(picks["voxel_index"] >= 0))
            scat_hits = r.cast_rays(scat[:200_000])
            say(f"{name} ({scene} {n}^3, {W}x{H}): pick == frame hit records: {same_frame}; cast of host-built primary "
                f"rays vs pick: {same_cast} differing bytes; primary hits {hit_share:.1%}, mean steps "
                f"{picks['steps'].mean():.1f}; scattered hits {np.mean(scat_hits['voxel_index'] >= 0):.1%}, mean steps "
                f"{scat_hits['steps'].mean():.1f}")
            r.set_launch_timing(1)
            medians = {k: [] for k in arms}
            for run in range(args.runs):
                for k, (_, fn) in arms.items():
                    ms = []
                    for i in range(args.warmup + args.reps):
                        fn()
                        t, launches = r.launch_timing()
                        assert launches == 1, launches
                        if i >= args.warmup:
                            ms.append(t)
                    medians[k].append(statistics.median(ms))
            r.set_launch_timing(0)
            frame_ms = statistics.median(medians["frame"])
            for k, (rays, _) in arms.items():
                med = statistics.median(medians[k])
                spread = (max(medians[k]) - min(medians[k])) / med
                res = {"config": name, "scene": scene, "n": n, "arm": k, "rays": rays, "reps": args.reps,
                       "run_medians_ms": [round(v, 5) for v in medians[k]], "ms": round(med, 5),
                       "spread": round(spread, 4), "mrays_per_s": round(rays / med / 1e3, 1),
                       "frame_over_this": round(frame_ms / med, 3)}
                results.append(res)
                say(f"{name} {k}: {med:.4f} ms (runs {', '.join(f'{v:.4f}' for v in medians[k])}; spread "
                    f"{spread:.1%}), {res['mrays_per_s']} Mrays/s, hit-record frame / this = {res['frame_over_this']}")
    say(json.dumps({"ray_query_bench": results}))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
