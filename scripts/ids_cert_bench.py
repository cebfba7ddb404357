#!/usr/bin/env python3
"""The certified ID kernel against the exact ID kernel (DESIGN.md §6 "ID and depth pass").

Per volume (C3's refraction 128^3, C1's glass_cube 128^3, terrain 512^3) on the 1920x1080 benchmark camera,
GPU time from the device timestamps of vrt_set_launch_timing (recorded when a kernel starts and ends on the
device), scripts/ids_bench.py's method:
  exact_depth / exact   vrt_render_ids_async in mode 0 (ids_exact_kernel: every pixel by the exact march),
                        with depth and without;
  cert_depth / cert     the same calls after vrt_set_ids_certified(1) (ids_cert_kernel: certified walks, the
                        exact march in the lane of a pixel they cannot settle), one launch each;
  reproj_exact / reproj_cert   vrt_render_frame_reprojected's kernel_ms (frame, ID pass and filter) with the
                        mode off and on.
The exact kernel is code the certified mode does not touch, so timing both in one process measures the gain
directly. Each figure is the median of --reps launches after --warmup, taken in three runs over all arms in one
process; the spread is (max - min) / median of the three medians. In every run mode 1's IDs and depth bits are
asserted equal to mode 0's. A gain counts when the exact arm exceeds the certified arm by more than three times
the larger of the two spreads (of the slower arm's time).

  python scripts/ids_cert_bench.py [--reps 21] [--warmup 3] [--out profiles/ids_cert_bench.txt]
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
ALPHA = 0.2


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=21)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ids_cert_bench.txt"))
    args = ap.parse_args()
    import torch

    lines, results = [], []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    for name, scene, n, refl, transp in (("C3", "refraction", 128, 4, 4), ("C1", "glass_cube", 128, 1, 2),
                                         ("T512", "terrain", 512, 4, 2)):
        vox = vrt.build_scene(scene, n)
        cam = vrt.make_camera(W, H)
        p = vrt.default_params(refl, transp)
        with vrt.Renderer(0) as r:
            r.upload_volume(vox, n)
            d_ids = torch.empty(W * H * 2, dtype=torch.int32, device="cuda")
            d_depth = torch.empty(W * H, dtype=torch.float32, device="cuda")
            torch.cuda.synchronize()

            def ids_call(mode, want_depth):
                def fn():
                    r.set_ids_certified(mode)
                    r.render_ids_async(cam, p, 0, H, W, d_ids.data_ptr(), d_depth.data_ptr() if want_depth else 0)
                    return None
                return fn

            def reproj_call(mode):
                def fn():
                    r.set_ids_certified(mode)
                    return r.render_frame_reprojected(cam, p, ALPHA, timing=True)[1]
                return fn

            # arm: (mode, timed launches or None for kernel_ms, call)
            arms = {
                "exact_depth": (0, 1, ids_call(0, True)), "cert_depth": (1, 1, ids_call(1, True)),
                "exact": (0, 1, ids_call(0, False)), "cert": (1, 1, ids_call(1, False)),
                "reproj_exact": (0, None, reproj_call(0)), "reproj_cert": (1, None, reproj_call(1)),
            }
            medians = {k: [] for k in arms}
            deferred = None
            for run in range(args.runs):
                # parity first: mode 1's records and depth bits are mode 0's
                r.set_ids_certified(0)
                ids0, depth0 = r.render_ids(cam, p)
                px0, de0 = r.ids_deferred()
                r.set_ids_certified(1)
                assert r.ids_certified() == 1
                ids1, depth1 = r.render_ids(cam, p)
                deferred = r.ids_deferred()
                assert (px0, de0) == (W * H, W * H) and deferred[0] == W * H
                assert ids1.tobytes() == ids0.tobytes(), (name, run)
                assert np.array_equal(depth1.view(np.uint32), depth0.view(np.uint32)), (name, run)
                for k, (mode, timed, fn) in arms.items():
                    ms = []
                    if timed is None:
                        for i in range(args.warmup + args.reps):
                            t = fn()
                            if i >= args.warmup:
                                ms.append(t)
                    else:
                        r.set_launch_timing(timed)
                        for i in range(args.warmup + args.reps):
                            fn()
                            t, launches = r.launch_timing()
                            assert launches == timed, (k, launches)
                            if i >= args.warmup:
                                ms.append(t)
                        r.set_launch_timing(0)
                    medians[k].append(statistics.median(ms))
            r.set_ids_certified(0)
            found = float(np.mean(ids0["voxel_index"] >= 0))
            say(f"{name} ({scene} {n}^3, {W}x{H}): mode 1 ids and depth bits == mode 0's in every run: True; primary "
                f"hits {found:.1%}; ids_deferred {deferred[1]} of {deferred[0]} ({deferred[1] / deferred[0]:.3%})")
            med = {k: statistics.median(v) for k, v in medians.items()}
            spread = {k: (max(medians[k]) - min(medians[k])) / med[k] for k in arms}
            for k in arms:
                results.append({"config": name, "scene": scene, "n": n, "arm": k, "reps": args.reps,
                                "run_medians_ms": [round(v, 5) for v in medians[k]], "ms": round(med[k], 5),
                                "spread": round(spread[k], 4)})
                say(f"{name} {k}: {med[k]:.4f} ms (runs {', '.join(f'{v:.4f}' for v in medians[k])}; spread "
                    f"{spread[k]:.1%})")
            for slow, fast in (("exact_depth", "cert_depth"), ("exact", "cert"), ("reproj_exact", "reproj_cert")):
                margin = 3.0 * max(spread[slow], spread[fast]) * med[slow]
                gain = med[slow] - med[fast]
                verdict = "clears" if gain > margin else "does NOT clear"
                results.append({"config": name, "pair": [slow, fast], "ratio": round(med[slow] / med[fast], 3),
                                "gain_ms": round(gain, 5), "three_spreads_ms": round(margin, 5),
                                "clears": bool(gain > margin)})
                say(f"{name} {slow} / {fast} = {med[slow] / med[fast]:.2f} ({gain:+.4f} ms; three spreads = "
                    f"{margin:.4f} ms: {verdict} the margin)")
    say(json.dumps({"ids_cert_bench": results, "ids_deferred_per_volume": "see the lines above"}))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
