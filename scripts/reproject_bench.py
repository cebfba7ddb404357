#!/usr/bin/env python3
"""The reprojected temporal filter against the ID pass it reads from and the plain frame loop (DESIGN.md §6
"Reprojected temporal filter").

C3 (refraction 128^3, 4 reflections, 4 transparencies) on the 1920x1080 benchmark camera. GPU time of the
kernel arms from the device timestamps of vrt_set_launch_timing (recorded when a kernel starts and ends on the
device):
  reproject_static   vrt_reproject_temporal_async, previous camera = camera (every pixel fetches its own
                     history);
  reproject_moved    the same with the previous frame from a moved camera (gathered fetches, rejections);
  ids_depth          vrt_render_ids_async with depth, the pass that writes the filter's inputs: code this
                     feature does not touch, the yardstick in the same process.
The synchronous loops, per call, by vrt_stats.kernel_ms (first launch's start to last launch's end) and by the
host's clock around the call:
  frame_sync         vrt_render_frame at alpha 0.3;
  frame_reprojected  vrt_render_frame_reprojected at alpha 0.3 (frame + ID pass + filter + the same copy).
Each figure is the median of --reps launches after --warmup, taken in three runs over all arms in one process;
the spread is (max - min) / median of the three medians. GB/s of the filter: the bytes it moves by its own
outcome counts (every pixel: raw 4 + ids 8 + depth 4 read, 4 written; a pixel that lands inside the previous
image: 8 more for the previous IDs; an accepted one: 4 more for the previous colour) over the kernel time.

  python scripts/reproject_bench.py [--reps 21] [--warmup 3] [--out profiles/reproject_bench.txt]
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import voxelraytracer_amd as vrt  # noqa: E402

W, H = 1920, 1080
ALPHA = 0.3
MOVED = ((-3.05, 2.02, 3.78), (-31.0, -53.0, 0.0))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=21)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "reproject_bench.txt"))
    args = ap.parse_args()
    import torch

    lines, results = [], []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    name, scene, n = "C3", "refraction", 128
    vox = vrt.build_scene(scene, n)
    cam_a = vrt.make_camera(W, H)
    cam_b = vrt.make_camera(W, H, pos=MOVED[0], rot=MOVED[1])
    p = vrt.default_params(4, 4)
    pv_a = vrt.camera_forward(cam_a)
    with vrt.Renderer(0) as r:
        r.upload_volume(vox, n)
        bufs = {}
        for key, cam in (("a", cam_a), ("b", cam_b)):
            ids, depth = r.render_ids(cam, p)
            raw, _ = r.render_frame(cam, p, 1.0)
            bufs[key] = (torch.from_numpy(ids.view(np.int32).reshape(H, 2 * W)).cuda(), torch.from_numpy(depth).cuda(),
                         torch.from_numpy(raw).cuda())
        d_out = torch.empty(W * H, dtype=torch.int32, device="cuda")
        d_src = torch.empty(W * H, dtype=torch.int32, device="cuda")
        d_ids = torch.empty(W * H * 2, dtype=torch.int32, device="cuda")
        d_depth = torch.empty(W * H, dtype=torch.float32, device="cuda")
        torch.cuda.synchronize()

        def reproject(cur, cam, src=0):
            ids, depth, raw = bufs[cur]
            pids, _, prev = bufs["a"]
            r.reproject_temporal_async(cam, p, pv_a, ALPHA, 0, H, W, raw.data_ptr(), ids.data_ptr(), depth.data_ptr(),
                                       prev.data_ptr(), pids.data_ptr(), W, d_out.data_ptr(), src)

        nbytes = {}
        for arm, cur, cam in (("reproject_static", "a", cam_a), ("reproject_moved", "b", cam_b)):
            reproject(cur, cam, d_src.data_ptr())
            torch.cuda.synchronize()
            src = d_src.cpu().numpy()
            acc, outside, behind, mism = (int(np.count_nonzero(m)) for m in (src >= 0, src == -1, src == -2, src == -3))
            nbytes[arm] = 20 * W * H + 8 * (acc + mism) + 4 * acc
            say(f"{name} ({scene} {n}^3, {W}x{H}) {arm}: accepted {acc} ({acc / (W * H):.1%}), outside {outside}, "
                f"behind {behind}, rejected by the IDs {mism}; {nbytes[arm] / (W * H):.1f} bytes per pixel")
        # arm: call (one timed launch each)
        arms = {
            "reproject_static": lambda: reproject("a", cam_a),
            "reproject_moved": lambda: reproject("b", cam_b),
            "ids_depth": lambda: r.render_ids_async(cam_a, p, 0, H, W, d_ids.data_ptr(), d_depth.data_ptr()),
        }
        medians = {k: [] for k in arms}
        sync = {"frame_sync": lambda q: r.render_frame(cam_a, q, ALPHA)[1]["kernel_ms"],
                "frame_reprojected": lambda q: r.render_frame_reprojected(cam_a, q, ALPHA, timing=True)[1]}
        sync_gpu = {k: [] for k in sync}
        sync_host = {k: [] for k in sync}
        for run in range(args.runs):
            for k, fn in arms.items():
                r.set_launch_timing(1)
                ms = []
                for i in range(args.warmup + args.reps):
                    fn()
                    t, launches = r.launch_timing()
                    assert launches == 1, (k, launches)
                    if i >= args.warmup:
                        ms.append(t)
                medians[k].append(statistics.median(ms))
            r.set_launch_timing(0)
            for k, fn in sync.items():
                gpu, host = [], []
                for i in range(args.warmup + args.reps):
                    q = vrt.default_params(4, 4, time=float(i + 1))
                    t0 = time.perf_counter()
                    kms = fn(q)
                    t1 = time.perf_counter()
                    if i >= args.warmup:
                        gpu.append(kms)
                        host.append((t1 - t0) * 1e3)
                sync_gpu[k].append(statistics.median(gpu))
                sync_host[k].append(statistics.median(host))

    def report(k, runs, what):
        med = statistics.median(runs)
        spread = (max(runs) - min(runs)) / med
        res = {"config": name, "arm": k, "what": what, "reps": args.reps, "run_medians_ms": [round(v, 5) for v in runs],
               "ms": round(med, 5), "spread": round(spread, 4)}
        extra = ""
        if k in nbytes:
            res["bytes"] = nbytes[k]
            res["gb_per_s"] = round(nbytes[k] / (med * 1e-3) / 1e9, 1)
            extra = f", {res['gb_per_s']} GB/s"
        results.append(res)
        say(f"{name} {k} ({what}): {med:.4f} ms (runs {', '.join(f'{v:.4f}' for v in runs)}; spread {spread:.1%}){extra}")
        return med

    med = {k: report(k, v, "kernel") for k, v in medians.items()}
    for k in ("reproject_static", "reproject_moved"):
        say(f"{name} {k} / ids_depth = {med[k] / med['ids_depth']:.3f}")
    g = {k: report(k, v, "kernel_ms") for k, v in sync_gpu.items()}
    h = {k: report(k, v, "host ms per call") for k, v in sync_host.items()}
    say(f"{name} frame_reprojected - frame_sync: kernel_ms {g['frame_reprojected'] - g['frame_sync']:+.4f} ms, "
        f"host {h['frame_reprojected'] - h['frame_sync']:+.4f} ms per call "
        f"(ids_depth + reproject_static = {med['ids_depth'] + med['reproject_static']:.4f} ms)")
    say(json.dumps({"reproject_bench": results}))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
