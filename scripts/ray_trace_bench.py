#!/usr/bin/env python3
"""Shaded ray queries against the hit-record frame (DESIGN.md §6 "Shaded ray queries").

Per volume (C3's refraction 128^3 at (R, T) = (4, 4), C1's glass_cube 128^3 at (1, 2), C4's terrain
512^3 at (4, 2)), GPU time of one launch over the 1920x1080 benchmark camera, from the device timestamps
of vrt_set_launch_timing (recorded when the kernel starts and ends on the device):
  frame          what a caller had to do before for colour and record per pixel: vrt_render_rows_async
                 with d_out_hit (the exact-walk, counted instance). The baseline: frame code is not
                 touched by the trace kernels.
  trace_pixels   vrt_trace_pixels' kernel over every pixel (the primary ray built in the kernel, then the
                 same exact_pixel), pixels listed 8x8 tile by tile as a frame's waves hold them, and
                 listed row by row;
  trace_rays     vrt_trace_rays_async on the same primary rays read from a buffer (built on the host with
                 the vertex stage's float32 operations), in the tile order;
  scattered      2 M rays of the tests' incoherent distribution (origins around the volume, three in four
                 aimed at a point of it, every eighth with a short max_length);
  default_frame  the default stats-free frame (vrt_render_rows_async without records: certified walks,
                 deferred exact pass), for context only.
Each figure is the median of --reps launches after --warmup, taken in three runs over all arms in one
process; the spread is (max - min) / median of the three medians.

  python scripts/ray_trace_bench.py [--reps 21] [--warmup 3] [--out profiles/ray_trace_bench.txt]
"""
import argparse
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import voxelraytracer_amd as vrt  # noqa: E402
from voxelraytracer_amd import abi  # noqa: E402
from ray_query_bench import H, SCATTERED, W, primary_rays, row_order_pixels, scattered_rays, tile_order_pixels  # noqa: E402

CONFIGS = (("C3", "refraction", 128, 4, 4), ("C1", "glass_cube", 128, 1, 2), ("C4", "terrain", 512, 4, 2))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=21)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--configs", default=",".join(c[0] for c in CONFIGS))
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ray_trace_bench.txt"))
    args = ap.parse_args()
    import torch

    lines, results = [], []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    def device(a):
        return torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).cuda()

    tiles, rows = tile_order_pixels(), row_order_pixels()
    for name, scene, n, refl, transp in CONFIGS:
        if name not in args.configs.split(","):
            continue
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
            d_out = torch.empty(max(SCATTERED, W * H) * 32, dtype=torch.uint8, device="cuda")
            torch.cuda.synchronize()
            arms = {
                "frame": (W * H, lambda: r.render_rows_async(cam, p, 0, H, 1, d_rgba.data_ptr(), d_fhit.data_ptr())),
                "trace_pixels_tiles": (W * H, lambda: r.trace_pixels(cam, p, tiles)),
                "trace_pixels_rows": (W * H, lambda: r.trace_pixels(cam, p, rows)),
                "trace_rays_primary": (W * H, lambda: r.trace_rays_async(d_prim.data_ptr(), W * H, p, d_out.data_ptr())),
                "scattered": (SCATTERED, lambda: r.trace_rays_async(d_scat.data_ptr(), SCATTERED, p, d_out.data_ptr())),
                "default_frame": (W * H, lambda: r.render_rows_async(cam, p, 0, H, 1, d_rgba.data_ptr())),
            }
            # the arms answer the same question: a traced pixel is the frame's record and colour, and the
            # host-built primary rays are the kernel's
            traced = r.trace_pixels(cam, p, tiles)
            arms["frame"][1]()
            torch.cuda.synchronize()
            fhit = d_fhit.cpu().numpy().view(abi.HIT_DTYPE).reshape(H, W)[tiles[:, 1], tiles[:, 0]]
            frgba = d_rgba.cpu().numpy().reshape(H, W, 4)[tiles[:, 1], tiles[:, 0]]
            same_hits = bool(np.array_equal(traced.view(np.uint8).reshape(-1, 32)[:, :16],
                                            fhit.view(np.uint8).reshape(-1, 16)))
            same_rgba = bool(np.array_equal(traced["rgba"].view(np.uint32), frgba.view(np.uint32)))
            by_ray = r.trace_rays(prim, p)
            diff_rays = int(np.count_nonzero(np.any(by_ray.view(np.uint8).reshape(-1, 32) !=
                                                    traced.view(np.uint8).reshape(-1, 32), axis=1)))
            scat_out = r.trace_rays(scat[:200_000], p)
            say(f"{name} ({scene} {n}^3, {W}x{H}, (R, T) = ({refl}, {transp})): traced pixels == frame hit records: "
                f"{same_hits}, == frame colours: {same_rgba}; trace of host-built primary rays vs traced pixels: "
                f"{diff_rays} differing records; primary hits {np.mean(traced['voxel_index'] >= 0):.1%}, mean steps "
                f"of a tree {traced['steps'].mean():.1f}; scattered hits {np.mean(scat_out['voxel_index'] >= 0):.1%}, "
                f"mean steps {scat_out['steps'].mean():.1f}")
            r.set_launch_timing(1)
            medians = {k: [] for k in arms}
            for run in range(args.runs):
                for k, (_, fn) in arms.items():
                    ms = []
                    for i in range(args.warmup + args.reps):
                        fn()
                        t, launches = r.launch_timing()
                        # (a default frame's certified pass and exact pass share one pair of timestamps)
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
                       "this_over_frame": round(med / frame_ms, 3)}
                results.append(res)
                say(f"{name} {k}: {med:.4f} ms (runs {', '.join(f'{v:.4f}' for v in medians[k])}; spread "
                    f"{spread:.1%}), {res['mrays_per_s']} Mrays/s, this / hit-record frame = {res['this_over_frame']}")
    say(json.dumps({"ray_trace_bench": results}))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
