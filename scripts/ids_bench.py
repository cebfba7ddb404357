#!/usr/bin/env python3
"""The ID and depth pass against the pick of every pixel and the hit-record frame (DESIGN.md §6 "ID and
depth pass").

Per volume (C3's refraction 128^3, C1's glass_cube 128^3, terrain 512^3) on the 1920x1080 benchmark
camera, GPU time from the device timestamps of vrt_set_launch_timing (recorded when a kernel starts and
ends on the device):
  ids_depth    vrt_render_ids_async with depth (one kernel: every pixel by the exact march, 8x8 tiles);
  ids          the same without depth;
  pick_tiles   vrt_pick_pixels' kernel over every pixel, listed 8x8 tile by tile as a frame's waves hold
               them;
  frame_hits   vrt_render_rows_async with d_out_hit (the exact-walk, counted instance);
  frame        the default stats-free frame, for scale.
The pick and the hit-record frame are code this pass does not touch. Each figure is the median of --reps
launches after --warmup, taken in three runs over all arms in one process; the spread is (max - min) /
median of the three medians. The IDs are asserted equal to the pick's at every pixel.

  python scripts/ids_bench.py [--reps 21] [--warmup 3] [--out profiles/ids_bench.txt]
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

W, H = 1920, 1080


def tile_order_pixels():
    """Every pixel, 8x8 tile by tile (tiles row-major, lane l of a tile at (l % 8, l // 8))."""
    ty, tx, ly, lx = np.meshgrid(np.arange(H // 8), np.arange(W // 8), np.arange(8), np.arange(8), indexing="ij")
    return np.stack([(tx * 8 + lx).reshape(-1), (ty * 8 + ly).reshape(-1)], axis=1).astype(np.int32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=21)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ids_bench.txt"))
    args = ap.parse_args()
    import torch

    lines, results = [], []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    tiles = tile_order_pixels()
    for name, scene, n, refl, transp in (("C3", "refraction", 128, 4, 4), ("C1", "glass_cube", 128, 1, 2),
                                         ("T512", "terrain", 512, 4, 2)):
        vox = vrt.build_scene(scene, n)
        cam = vrt.make_camera(W, H)
        p = vrt.default_params(refl, transp)
        with vrt.Renderer(0) as r:
            r.upload_volume(vox, n)
            d_rgba = torch.empty(W * H * 4, dtype=torch.float32, device="cuda")
            d_fhit = torch.empty(W * H * 16, dtype=torch.uint8, device="cuda")
            d_ids = torch.empty(W * H * 2, dtype=torch.int32, device="cuda")
            d_depth = torch.empty(W * H, dtype=torch.float32, device="cuda")
            torch.cuda.synchronize()
            # the pass answers the pick's question: every pixel's voxel_index and face
            ids, depth = r.render_ids(cam, p)
            pixels, deferred = r.ids_deferred()
            picks = r.pick(cam, p, tiles)
            got = ids[tiles[:, 1], tiles[:, 0]]
            assert np.array_equal(got["voxel_index"], picks["voxel_index"]) and np.array_equal(got["face"], picks["face"])
            found = picks["voxel_index"] >= 0
            gap = np.abs(depth[tiles[:, 1], tiles[:, 0]][found].astype(np.float64) - picks["ray_length"][found])
            say(f"{name} ({scene} {n}^3, {W}x{H}): ids == pick at every pixel: True; primary hits {found.mean():.1%}; "
                f"pixels on the exact kernel {deferred} of {pixels}; "
                f"max |depth - ray_length| {gap.max():.3e}")
            # arm: (timing slots, kernels timed, call)
            arms = {
                "ids_depth": (1, 1, lambda: r.render_ids_async(cam, p, 0, H, W, d_ids.data_ptr(), d_depth.data_ptr())),
                "ids": (1, 1, lambda: r.render_ids_async(cam, p, 0, H, W, d_ids.data_ptr(), 0)),
                "pick_tiles": (1, 1, lambda: r.pick(cam, p, tiles)),
                "frame_hits": (1, 1, lambda: r.render_rows_async(cam, p, 0, H, 1, d_rgba.data_ptr(), d_fhit.data_ptr())),
                "frame": (1, 1, lambda: r.render_rows_async(cam, p, 0, H, 1, d_rgba.data_ptr())),
            }
            medians = {k: [] for k in arms}
            for run in range(args.runs):
                for k, (slots, timed, fn) in arms.items():
                    r.set_launch_timing(slots)
                    ms = []
                    for i in range(args.warmup + args.reps):
                        fn()
                        t, launches = r.launch_timing()
                        assert launches == timed, (k, launches)
                        if i >= args.warmup:
                            ms.append(t)
                    medians[k].append(statistics.median(ms))
            r.set_launch_timing(0)
            med = {k: statistics.median(v) for k, v in medians.items()}
            nan = float("nan")
            for k in arms:
                spread = (max(medians[k]) - min(medians[k])) / med[k]
                res = {"config": name, "scene": scene, "n": n, "arm": k, "reps": args.reps,
                       "run_medians_ms": [round(v, 5) for v in medians[k]], "ms": round(med[k], 5),
                       "spread": round(spread, 4), "pick_over_this": round(med.get("pick_tiles", nan) / med[k], 3),
                       "frame_hits_over_this": round(med.get("frame_hits", nan) / med[k], 3)}
                results.append(res)
                say(f"{name} {k}: {med[k]:.4f} ms (runs {', '.join(f'{v:.4f}' for v in medians[k])}; spread "
                    f"{spread:.1%}), pick / this = {res['pick_over_this']}, hit-record frame / this = "
                    f"{res['frame_hits_over_this']}")
    say(json.dumps({"ids_bench": results}))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
