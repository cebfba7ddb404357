#!/usr/bin/env python3
"""The ID-guided spatial filter's kernel time (DESIGN.md §6 "Spatial filter").

On C3 (refraction 128^3, the 1920x1080 benchmark camera), GPU time from the device timestamps of
vrt_set_launch_timing (recorded when a kernel starts and ends on the device):
  pass       one vrt_spatial_filter_async pass per step 1, 2, 4, 8, 16, guide FACE and PLANE, with and without
             d_count, on the context's own noisy frame and noise-free IDs; one arm with d_keep too;
  reproject  vrt_reproject_temporal_async on the same frame, for scale;
  loop       stats->kernel_ms of vrt_render_frame_reprojected with the passes off, SPATIAL_DISPLAY with 3 passes and
             SPATIAL_FILL with 3 passes, three contexts alternating frame by frame along a moving camera.
Each figure is the median of --reps launches after --warmup, taken in three runs over all arms in one process; the
spread is (max - min) / median of the three medians. Beside each pass stands its ratio to the streaming bound: the
bytes a pass must move (8 ID, 4 in, 4 out per pixel, plus the keep and count bytes when present) at the 6.29 TB/s a
float4 copy reaches.
Which kernel form a step launches is the library's (kSpatialLdsSteps, vrt_tuning.h). --variant LIB runs the pass arms
again in a child process on a make variant build, e.g. the direct gather at every step:
  make variant NAME=spatial_direct DEFS=-DVRT_SPATIAL_LDS_STEPS=0
  python scripts/spatial_bench.py --variant build/variants/libvrt_spatial_direct.so --variant-lds-steps 0

  python scripts/spatial_bench.py [--reps 21] [--warmup 3] [--out profiles/spatial_bench.txt]
"""
import argparse
import json
import os
import re
import statistics
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import voxelraytracer_amd as vrt  # noqa: E402

W, H = 1920, 1080
COPY_RATE = 6.29e12   # bytes per second of a float4 copy
STEPS = (1, 2, 4, 8, 16)
CAM_B = ((-3.05, 2.02, 3.78), (-31.0, -53.0, 0.0))


def product_lds_steps():
    text = open(os.path.join(ROOT, "voxelraytracer_amd", "csrc", "vrt_tuning.h")).read()
    return int(re.search(r"#define VRT_SPATIAL_LDS_STEPS (\S+)", text).group(1), 0)


def form(step, lds_steps):
    return "lds" if step in (1, 2, 4) and (lds_steps >> step) & 1 else "direct"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=21)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "spatial_bench.txt"))
    ap.add_argument("--variant", default=None, help="a make variant library for a second pass of the pass arms")
    ap.add_argument("--variant-lds-steps", default="0", help="its VRT_SPATIAL_LDS_STEPS")
    ap.add_argument("--child-lds-steps", default=None, help=argparse.SUPPRESS)
    args = ap.parse_args()
    import torch

    child = args.child_lds_steps is not None
    lds_steps = int(args.child_lds_steps, 0) if child else product_lds_steps()
    lines, results = [], []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    vox = vrt.build_scene("refraction", 128)
    cam, cam_b = vrt.make_camera(W, H), vrt.make_camera(W, H, pos=CAM_B[0], rot=CAM_B[1])
    noisy = vrt.default_params(4, 4, ray_noise=0.05, reflection_noise=0.05, refraction_noise=0.01)
    geom = vrt.default_params(4, 4)
    lib = os.path.relpath(os.environ["VRT_LIB"], ROOT) if os.environ.get("VRT_LIB") else "product"
    say(f"C3 (refraction 128^3, {W}x{H}), library {lib}, "
        f"VRT_SPATIAL_LDS_STEPS = {lds_steps:#x}")
    with vrt.Renderer(0) as r:
        r.upload_volume(vox, 128)
        d_in = torch.zeros((H, W), dtype=torch.int32, device="cuda")
        d_out = torch.zeros((H, W), dtype=torch.int32, device="cuda")
        d_ids = torch.zeros((H, W * 2), dtype=torch.int32, device="cuda")
        d_depth = torch.zeros((H, W), dtype=torch.float32, device="cuda")
        d_prev_ids = torch.zeros((H, W * 2), dtype=torch.int32, device="cuda")
        d_count = torch.zeros((H, W), dtype=torch.uint8, device="cuda")
        r.render_temporal_rows_async(cam, noisy, 1.0, 0, H, 1, d_in.data_ptr(), d_in.data_ptr())
        r.render_ids_async(cam, geom, 0, H, W, d_ids.data_ptr(), d_depth.data_ptr())
        r.render_ids_async(cam_b, geom, 0, H, W, d_prev_ids.data_ptr(), 0)
        torch.cuda.synchronize()
        d_keep = (torch.rand((H, W), device="cuda") < 0.5).to(torch.uint8)
        d_prev = d_in.clone()   # a previous frame for the reproject arm
        pv_b = vrt.camera_forward(cam_b)

        def pass_arm(step, guide, count, keep=False):
            return lambda: r.spatial_filter_async(W, H, W, step, guide, 765, 0, H, d_in.data_ptr(), d_ids.data_ptr(),
                                                  d_keep.data_ptr() if keep else 0, d_out.data_ptr(),
                                                  d_count.data_ptr() if count else 0)

        arms = {}
        for step in STEPS:
            for gname, guide in (("FACE", vrt.GUIDE_FACE), ("PLANE", vrt.GUIDE_PLANE)):
                for count in (False, True):
                    arms[f"pass step {step} {gname} {'count' if count else 'no count'} [{form(step, lds_steps)}]"] = \
                        (pass_arm(step, guide, count), 16 + count)
        arms[f"pass step 1 FACE keep count [{form(1, lds_steps)}]"] = (pass_arm(1, vrt.GUIDE_FACE, True, True), 18)
        arms["reproject (nearest, camera B's IDs as the previous frame)"] = (
            lambda: r.reproject_temporal_async(cam, geom, pv_b, 0.5, 0, H, W, d_in.data_ptr(), d_ids.data_ptr(),
                                               d_depth.data_ptr(), d_prev.data_ptr(), d_prev_ids.data_ptr(), W,
                                               d_out.data_ptr()), None)
        medians = {k: [] for k in arms}
        for run in range(args.runs):
            for k, (fn, _) in arms.items():
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
        torch.cuda.synchronize()
        for k, (_, bpp) in arms.items():
            med = statistics.median(medians[k])
            spread = (max(medians[k]) - min(medians[k])) / med
            res = {"arm": k, "lds_steps": lds_steps, "ms": round(med, 5), "run_medians_ms": [round(v, 5) for v in medians[k]],
                   "spread": round(spread, 4)}
            tail = ""
            if bpp:
                bound = W * H * bpp / COPY_RATE * 1e3
                res.update(bytes_per_pixel=bpp, bound_ms=round(bound, 5), over_bound=round(med / bound, 2))
                tail = f", streaming bound {bound:.4f} ms ({bpp} B/pixel), this / bound = {med / bound:.2f}"
            results.append(res)
            say(f"{k}: {med:.4f} ms (runs {', '.join(f'{v:.4f}' for v in medians[k])}; spread {spread:.1%}){tail}")
    if not child:
        # the loop: three contexts, one per mode, alternating frame by frame along A, B, A, B, ...
        modes = (("off", vrt.SPATIAL_OFF), ("display, 3 passes", vrt.SPATIAL_DISPLAY), ("fill, 3 passes", vrt.SPATIAL_FILL))
        ctxs = []
        for name, mode in modes:
            q = vrt.Renderer(0)
            q.upload_volume(vox, 128)
            q.set_reprojected_spatial(mode, 3, vrt.GUIDE_FACE, 765)
            ctxs.append(q)
        loop = {name: [] for name, _ in modes}
        for run in range(args.runs):
            ms = {name: [] for name, _ in modes}
            for i in range(args.warmup + args.reps):
                c = cam if i % 2 == 0 else cam_b
                noisy.time = float(i + 1)
                for (name, _), q in zip(modes, ctxs):
                    _, t = q.render_frame_reprojected(c, noisy, 0.5, timing=True)
                    if i >= args.warmup:
                        ms[name].append(t)
            for name in ms:
                loop[name].append(statistics.median(ms[name]))
        for q in ctxs:
            q.close()
        for name, _ in modes:
            med = statistics.median(loop[name])
            spread = (max(loop[name]) - min(loop[name])) / med
            results.append({"arm": "loop " + name, "ms": round(med, 5), "run_medians_ms": [round(v, 5) for v in loop[name]],
                            "spread": round(spread, 4)})
            say(f"loop kernel_ms, {name}: {med:.4f} ms (runs {', '.join(f'{v:.4f}' for v in loop[name])}; spread "
                f"{spread:.1%}), over off = {med / statistics.median(loop['off']):.2f}")
    say(json.dumps({"spatial_bench": results}))
    if child:
        return
    if args.variant:
        env = dict(os.environ, VRT_LIB=os.path.abspath(args.variant))
        out = subprocess.run([sys.executable, os.path.abspath(__file__), "--reps", str(args.reps), "--warmup",
                              str(args.warmup), "--runs", str(args.runs), "--child-lds-steps", args.variant_lds_steps],
                             env=env, capture_output=True, text=True, check=True, timeout=600).stdout
        lines.append("---- the pass arms again on the variant library, in a process of its own ----")
        lines.extend(out.strip().splitlines())
        print(out, flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
