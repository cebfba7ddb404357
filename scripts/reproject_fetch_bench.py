#!/usr/bin/env python3
"""The fetch modes of the reprojected temporal filter against each other (DESIGN.md §6 "Bilinear history
fetch"), by scripts/reproject_bench.py's method.

C3 (refraction 128^3, 4 reflections, 4 transparencies) on the 1920x1080 benchmark camera. GPU time of the
kernel arms from the device timestamps of vrt_set_launch_timing (recorded when a kernel starts and ends on the
device), previous frame from the benchmark camera:
  old_static / old_moved            vrt_reproject_temporal_async, current camera = previous camera / pose B:
                                    the parent's kernel, so timing it in the same process measures the parent;
  nearest_static / nearest_moved    VRT_FETCH_NEAREST through vrt_reproject_temporal_fetch_async without d_taps:
                                    the same kernel, which must lie within the old arm's own spread;
  bilinear_static / bilinear_moved  VRT_FETCH_BILINEAR, the same two cameras.
The synchronous loop, per call, by vrt_stats.kernel_ms (first launch's start to last launch's end):
  loop_nearest / loop_bilinear      vrt_render_frame_reprojected at alpha 0.3 in either mode.
Each figure is the median of --reps launches after --warmup, taken in three runs over all arms in one process;
the spread is (max - min) / median of the three medians. Bytes per pixel, from the outcome counts of an
untimed call with d_src and d_taps: every pixel reads raw 4 + ids 8 + depth 4 and writes 4; nearest: a pixel
that lands inside the previous image reads 8 more (one previous ID), an accepted one 4 more (its colour);
bilinear: a pixel that lands inside reads up to 4 x 8 (the IDs of its taps: four counted, the taps past a
border and those of weight 0 are not loaded), and 4 per valid tap (the popcount of d_taps).
Quality, asserted on nothing: after 16 frames of a slow pan (yaw +0.25 degrees per frame) at alpha 0.1 and
ray_noise 0, the mean absolute byte difference (RGB) between the loop's output and the frame rendered
directly at the final pose, per mode. A history that follows the surface exactly would leave only what the
shading changes with the view.

  python scripts/reproject_fetch_bench.py [--reps 21] [--warmup 3] [--out profiles/reproject_fetch_bench.txt]
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
ALPHA = 0.3
MOVED = ((-3.05, 2.02, 3.78), (-31.0, -53.0, 0.0))
PAN_FRAMES, PAN_STEP, PAN_ALPHA = 16, 0.25, 0.1


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=21)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "reproject_fetch_bench.txt"))
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
        for key, cam in (("static", cam_a), ("moved", cam_b)):
            ids, depth = r.render_ids(cam, p)
            raw, _ = r.render_frame(cam, p, 1.0)
            bufs[key] = (cam, torch.from_numpy(ids.view(np.int32).reshape(H, 2 * W)).cuda(),
                         torch.from_numpy(depth).cuda(), torch.from_numpy(raw).cuda())
        d_out = torch.empty(W * H, dtype=torch.int32, device="cuda")
        d_src = torch.empty(W * H, dtype=torch.int32, device="cuda")
        d_taps = torch.empty(W * H, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()

        def filt(kind, cur, src=0, taps=0):
            cam, ids, depth, raw = bufs[cur]
            _, pids, _, prev = bufs["static"]
            common = (raw.data_ptr(), ids.data_ptr(), depth.data_ptr(), prev.data_ptr(), pids.data_ptr(), W,
                      d_out.data_ptr(), src)
            if kind == "old":
                r.reproject_temporal_async(cam, p, pv_a, ALPHA, 0, H, W, *common)
            else:
                fetch = vrt.FETCH_BILINEAR if kind == "bilinear" else vrt.FETCH_NEAREST
                r.reproject_temporal_fetch_async(cam, p, pv_a, ALPHA, fetch, 0, H, W, *common, taps)

        nbytes = {}
        popcount = np.array([bin(m).count("1") for m in range(16)], np.int64)
        for kind in ("nearest", "bilinear"):
            for cur in ("static", "moved"):
                filt(kind, cur, d_src.data_ptr(), d_taps.data_ptr())
                torch.cuda.synchronize()
                src, taps = d_src.cpu().numpy(), d_taps.cpu().numpy()
                acc, outside, behind, mism = (int(np.count_nonzero(m)) for m in (src >= 0, src == -1, src == -2, src == -3))
                used = int(popcount[taps].sum())
                arm = f"{kind}_{cur}"
                if kind == "nearest":
                    nbytes[arm] = 20 * W * H + 8 * (acc + mism) + 4 * acc
                    nbytes[f"old_{cur}"] = nbytes[arm]
                    detail = ""
                else:
                    nbytes[arm] = 20 * W * H + 32 * (acc + mism) + 4 * used
                    partial = int(np.count_nonzero((src >= 0) & (taps != 15)))
                    detail = f", valid taps {used} ({used / max(acc, 1):.2f} per accepted pixel), partial masks {partial}"
                say(f"{name} ({scene} {n}^3, {W}x{H}) {arm}: accepted {acc} ({acc / (W * H):.1%}), outside {outside}, "
                    f"behind {behind}, rejected by the IDs {mism}{detail}; {nbytes[arm] / (W * H):.1f} bytes per pixel")
        arms = {f"{kind}_{cur}": (lambda kind=kind, cur=cur: filt(kind, cur))
                for kind in ("old", "nearest", "bilinear") for cur in ("static", "moved")}
        medians = {k: [] for k in arms}
        loops = {"loop_nearest": vrt.FETCH_NEAREST, "loop_bilinear": vrt.FETCH_BILINEAR}
        loop_gpu = {k: [] for k in loops}
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
            for k, mode in loops.items():
                r.set_reprojected_fetch(mode)
                gpu = []
                for i in range(args.warmup + args.reps):
                    q = vrt.default_params(4, 4, time=float(i + 1))
                    kms = r.render_frame_reprojected(cam_a, q, ALPHA, timing=True)[1]
                    if i >= args.warmup:
                        gpu.append(kms)
                loop_gpu[k].append(statistics.median(gpu))
        # quality: a slow pan, the loop's last frame against the frame rendered directly at the last pose
        quality = {}
        geom = vrt.default_params(4, 4, ray_noise=0.0)
        for k, mode in loops.items():
            r.set_reprojected_fetch(mode)
            r.reprojected_history_reset()
            for f in range(PAN_FRAMES):
                rot = (vrt.DEFAULT_CAM_ROT[0], vrt.DEFAULT_CAM_ROT[1] + PAN_STEP * f, vrt.DEFAULT_CAM_ROT[2])
                cam = vrt.make_camera(W, H, rot=rot)
                got = r.render_frame_reprojected(cam, geom, PAN_ALPHA)
            direct, _ = r.render_frame(cam, geom, 1.0)
            quality[k] = float(np.abs(got[..., :3].astype(np.int32) - direct[..., :3].astype(np.int32)).mean())
        r.set_reprojected_fetch(vrt.FETCH_NEAREST)

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
    for cur in ("static", "moved"):
        say(f"{name} bilinear_{cur} / old_{cur} = {med[f'bilinear_{cur}'] / med[f'old_{cur}']:.3f}")
    g = {k: report(k, v, "kernel_ms") for k, v in loop_gpu.items()}
    say(f"{name} loop_bilinear - loop_nearest: kernel_ms {g['loop_bilinear'] - g['loop_nearest']:+.4f} ms")
    for k, v in quality.items():
        say(f"{name} {k} quality: mean |loop - direct| = {v:.4f} bytes per channel after {PAN_FRAMES} frames of a "
            f"{PAN_STEP} degree per frame pan at alpha {PAN_ALPHA}, ray_noise 0")
    # the one condition: the same kernel through the new entry point lies within the old arm's own spread
    same = {}
    for cur in ("static", "moved"):
        old = medians[f"old_{cur}"]
        diff, width = abs(med[f"nearest_{cur}"] - med[f"old_{cur}"]), max(old) - min(old)
        same[cur] = diff <= width
        say(f"{name} nearest_{cur} - old_{cur}: {med[f'nearest_{cur}'] - med[f'old_{cur}']:+.5f} ms, old arm's spread "
            f"{width:.5f} ms: {'within' if same[cur] else 'OUTSIDE'}")
    say(json.dumps({"reproject_fetch_bench": results, "quality": quality}))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    assert all(same.values()), same


if __name__ == "__main__":
    main()
