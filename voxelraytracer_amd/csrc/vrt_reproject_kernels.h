// vrt_reproject_kernels.h — the reprojected temporal filter (vrt_reproject_temporal_async): per pixel, the
// history is fetched where the pixel's surface point was on screen in the previous frame, and blended in only
// if the previous frame showed the same face of the same voxel there (the ID pass's records, both words
// equal). One streaming kernel, no walk and no volume read. Included by vrt_render.hip after temporal_blend,
// init_ctx, primary_ray and vrt_ids_kernels.h.
#ifndef VRT_REPROJECT_KERNELS_H
#define VRT_REPROJECT_KERNELS_H

#include "vrt_walk.h"

namespace vrt {

// Workgroups of kReprojWg threads: four waves, each an 8x8 pixel tile of a 16x16 tile (wave w at column
// block w & 1, row block w >> 1), so a wave's gathered history reads land in a few lines of the previous
// frame. No LDS (primary_ray reads the context's scalars only), no barrier, no atomics.
// Per pixel, float32 in this order (DESIGN.md §6 "Reprojected temporal filter"): the pixel's primary ray
// as the ID kernel forms it; the surface point pos + depth dir in world coordinates (w = 1), or the
// direction as a point at infinity for a miss (w = 0); its clip coordinates by the previous frame's PV;
// the perspective division, the viewport transform and a nearest fetch. Codes: -4 no history, -2 behind
// the previous camera (or NaN), -1 outside the previous image, -3 another voxel, face or material there.
// Every address is formed from the workgroup and lane ids under the test against a.width and a.rows, from
// (qx, qy), which the float tests have placed inside [0, width) x [0, height), and from the pitches.
__global__ void __launch_bounds__(kReprojWg) reproject_kernel(KArgs a, ReprojArgs r) {
  const uint32_t t = threadIdx.x;
  const int px = int(blockIdx.x) * 16 + int((t >> 6) & 1u) * 8 + int(t & 7u);
  const int li = int(blockIdx.y) * 16 + int(t >> 7) * 8 + int((t >> 3) & 7u);
  if (px >= a.width || li >= a.rows) return;
  const size_t o = size_t(li) * size_t(a.pitch) + size_t(px);
  const uint32_t raw = r.raw[o];
  uint32_t color = raw;
  int32_t code = -4;
  if (r.prev) {
    const uint2 id = r.ids[o];
    const float depth = r.depth[o];
    Ctx c;
    init_ctx(c, a, nullptr);
    c.ax = nullptr;
    const Ray ray = primary_ray(a, a.inv_pv, c, px, a.row0 + li);
    const bool hit = int32_t(id.x) >= 0;
    const float half = c.fn * 0.5f;
    const float vx = hit ? (ray.pos.x + depth * ray.dir.x) - half : ray.dir.x;
    const float vy = hit ? (ray.pos.y + depth * ray.dir.y) - half : ray.dir.y;
    const float vz = hit ? (ray.pos.z + depth * ray.dir.z) - half : ray.dir.z;
    const float w = hit ? 1.0f : 0.0f;
    float clip[4];
#pragma unroll
    for (int q = 0; q < 4; ++q)
      clip[q] = ((r.pv[0 * 4 + q] * vx + r.pv[1 * 4 + q] * vy) + r.pv[2 * 4 + q] * vz) + r.pv[3 * 4 + q] * w;
    if (!(clip[3] > 0.0f)) {
      code = -2;
    } else {
      const float fw = float(a.width), fh = float(a.height);
      const float sx = ((clip[0] / clip[3]) * 0.5f + 0.5f) * fw;
      const float sy = ((clip[1] / clip[3]) * 0.5f + 0.5f) * fh;
      if (!(sx >= 0.0f && sx < fw && sy >= 0.0f && sy < fh)) {
        code = -1;
      } else {
        const int qx = int(__builtin_floorf(sx)), qy = int(__builtin_floorf(sy));
        const size_t po = size_t(qy) * size_t(r.prev_pitch) + size_t(qx);
        const uint2 pid = r.prev_ids[po];
        if (pid.x != id.x || pid.y != id.y) {
          code = -3;
        } else {
          code = qy * a.width + qx;
          color = temporal_blend(raw, r.prev[po], r.alpha);
        }
      }
    }
  }
  r.out[o] = color;
  if (r.src) r.src[o] = code;
}

}  // namespace vrt

#endif  // VRT_REPROJECT_KERNELS_H
