#!/usr/bin/env python3
"""In-place edit against the full re-upload (DESIGN.md §6 "In-place edits").

Per scene (terrain 512^3, refraction 128^3) and edit size (one voxel, 16^3), two arms alternate, each
bringing the resident volume to the same edited state:
  edit: vrt_update_volume_region_device of the box (the regional rebuild);
  full: vrt_upload_volume_device of the whole edited volume (the same kernels over the box [0, N)^3:
        every pass over N^3, every texel packed).
Both calls end synchronised, so a host clock around them is the cost a caller pays. Successive
iterations toggle the box between its original bytes and their emptiness-inverted bytes, so every
edit changes emptiness and runs the distance passes. Reported: the median of --reps timings after
--warmup, and the voxel visits of each arm's passes and packs computed from the plan.

  python scripts/edit_bench.py [--reps 21] [--warmup 3] [--out profiles/edit_bench.txt]
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

FWD_CAP, DIST_CAP = 128, 64   # kFwdCap (csrc/vrt_tuning.h), kDistCap (csrc/vrt_walk.h)


def span(a, b, n):
    return max(a, 0), min(b, n - 1)


def size(*spans):
    out = 1
    for a, b in spans:
        out *= b - a + 1
    return out


def edit_visits(n, octants, origin, extent):
    """Voxel visits of the regional rebuild's launches: {pass: visits} (octant layout: 2 x, 4 y and
    8 z passes over the anchors and their forward inputs; packs over vrt_volume_edit_plan's boxes)."""
    lo, hi = list(origin), [origin[a] + extent[a] for a in range(3)]
    packs = sum((x1 - x0) * (y1 - y0) * (z1 - z0)
                for x0, y0, z0, x1, y1, z1 in vrt.volume_edit_plan(n, octants, origin, extent))
    if octants == 8:
        r = FWD_CAP - 1
        anchors = lambda a, s: span(lo[a] - r, hi[a] - 1, n) if s > 0 else span(lo[a], hi[a] - 1 + r, n)  # noqa: E731
        inputs = lambda a: span(lo[a] - r, hi[a] - 1 + r, n)  # noqa: E731
        sg = (1, -1)
        return {"x": sum(size(anchors(0, sx), inputs(1), inputs(2)) for sx in sg),
                "y": sum(size(anchors(0, sx), anchors(1, sy), inputs(2)) for sx in sg for sy in sg),
                "z": sum(size(anchors(0, sx), anchors(1, sy), anchors(2, sz)) for sx in sg for sy in sg for sz in sg),
                "pack": packs}
    r = DIST_CAP - 1
    near = lambda a: span(lo[a] - r, hi[a] - 1 + r, n)  # noqa: E731
    far = lambda a: span(lo[a] - 2 * r, hi[a] - 1 + 2 * r, n)  # noqa: E731
    return {"x": size(near(0), far(1), far(2)), "y": size(near(0), near(1), far(2)),
            "z": size(near(0), near(1), near(2)), "pack": packs}


def full_visits(n, octants):
    edge = (n + 1) ** 3 - n ** 3   # plane N of every axis: one visit writes the texel of all packed volumes
    if octants == 8:
        return {"x": 2 * n ** 3, "y": 4 * n ** 3, "z": 8 * n ** 3, "pack": 8 * n ** 3 + edge}
    return {"x": n ** 3, "y": n ** 3, "z": n ** 3, "pack": n ** 3 + edge}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=21)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "edit_bench.txt"))
    args = ap.parse_args()
    import torch

    lines, results = [], []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    for scene, n in (("terrain", 512), ("refraction", 128)):
        vox = vrt.build_scene(scene, n)
        with vrt.Renderer(0) as r:
            r.upload_volume(vox, n)
            octants = r._lib.vrt_volume_octants(r._h)
            for edge in (1, 16):
                origin = (n // 2 + 3, n // 2 - 5, n // 2 + 7)
                extent = (edge, edge, edge)
                v3 = vox.reshape(n, n, n)
                sl = (slice(origin[2], origin[2] + edge), slice(origin[1], origin[1] + edge),
                      slice(origin[0], origin[0] + edge))
                orig = v3[sl].copy()
                blocks = [np.where(orig != 0, 0, 1).astype(np.uint8), orig]   # inverted emptiness, original
                d_blocks, d_fulls = [], []
                for b in blocks:
                    full = v3.copy()
                    full[sl] = b
                    d_blocks.append(torch.from_numpy(np.ascontiguousarray(b).reshape(-1)).cuda())
                    d_fulls.append(torch.from_numpy(full.reshape(-1)).cuda())
                torch.cuda.synchronize()
                t_edit, t_full = [], []
                for i in range(args.warmup + args.reps):
                    k = i & 1
                    t0 = time.perf_counter()
                    r.update_volume_device(origin, extent, d_blocks[k].data_ptr())
                    t1 = time.perf_counter()
                    r.upload_volume_device(d_fulls[k].data_ptr(), n)   # the same edited volume, in full
                    t2 = time.perf_counter()
                    if i >= args.warmup:
                        t_edit.append((t1 - t0) * 1e3)
                        t_full.append((t2 - t1) * 1e3)
                # the fixed part of an edit: rewriting the bytes already there changes no emptiness, so the
                # call is its synchronisations, the staging copy, the box write with the count read-back
                # and the box-sized voxel-byte packs, with no distance pass
                t_same = []
                for i in range(args.warmup + args.reps):
                    t0 = time.perf_counter()
                    r.update_volume_device(origin, extent, d_blocks[k].data_ptr())
                    if i >= args.warmup:
                        t_same.append((time.perf_counter() - t0) * 1e3)
                ms = statistics.median(t_same)
                r.upload_volume(vox, n)   # the original bytes for the next edit size
                ve, vf = edit_visits(n, octants, origin, extent), full_visits(n, octants)
                me, mf = statistics.median(t_edit), statistics.median(t_full)
                res = {"scene": scene, "n": n, "octants": octants, "edit_edge": edge, "reps": args.reps,
                       "edit_ms_median": round(me, 4), "edit_ms_min": round(min(t_edit), 4),
                       "full_ms_median": round(mf, 4), "full_ms_min": round(min(t_full), 4),
                       "same_bytes_edit_ms_median": round(ms, 4), "speedup": round(mf / me, 2),
                       "edit_visits": ve, "full_visits": vf,
                       "visit_ratio": round(sum(vf.values()) / sum(ve.values()), 2)}
                results.append(res)
                say(f"{scene} {n}^3 ({octants} packed), {edge}^3 edit: edit {me:.3f} ms (min {min(t_edit):.3f}), "
                    f"full re-upload {mf:.3f} ms (min {min(t_full):.3f}), median of {args.reps}: "
                    f"{mf / me:.1f}x; same-bytes edit (no distance pass) {ms:.3f} ms; "
                    f"visits edit {ve} = {sum(ve.values())}, full {vf} = {sum(vf.values())}: "
                    f"{res['visit_ratio']}x")
    say(json.dumps({"edit_bench": results}))
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
