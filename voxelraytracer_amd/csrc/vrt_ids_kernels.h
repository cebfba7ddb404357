// vrt_ids_kernels.h — the ID and depth pass (vrt_render_ids*): per pixel, the voxel and face its primary
// ray hits and the hit's depth, without shading. One kernel: every pixel of the band by the pick's exact
// march, an 8x8 tile per wave. Included by vrt_render.hip after init_ctx, primary_ray and
// vrt_query_kernels.h (ray_hit_face).
#ifndef VRT_IDS_KERNELS_H
#define VRT_IDS_KERNELS_H

#include "vrt_walk.h"

namespace vrt {

// One-wave workgroups, workgroup (x, y) the 8x8 tile at (8 x, 8 y) of the band, each lane with its
// three-float4 LDS axis table: the pixel's primary ray and march<true, false, true>, as
// ray_query_kernel<kQueryPick> runs them for a listed pixel, the record's fields by the same expressions.
// A pixel's record (vrt_pixel_id) is one 8-byte store. depth (if asked for) is the parameter of the hit
// face's plane along the primary ray, (plane - pos[a]) / dir[a] with a the face's axis: one float32
// subtraction and one correctly rounded division. The plane is the hit point's coordinate on that axis,
// an integer up to the walk's rounding (also on coordinate N, whose voxel_index wraps to cell 0).
// Every address is formed from the workgroup and lane ids under the test against a.width and a.rows below.
__global__ void __launch_bounds__(64) ids_exact_kernel(KArgs a, const uint16_t* __restrict__ vox, uint2* __restrict__ ids,
                                                       float* __restrict__ depth) {
  const uint32_t lane = lane_id();
  const int px = int(blockIdx.x) * 8 + int(lane & 7u), li = int(blockIdx.y) * 8 + int(lane >> 3);
  if (px >= a.width || li >= a.rows) return;  // masked for the rest of the kernel (no barrier below)
  Ctx c;
  init_ctx(c, a, vox);
  __shared__ float4 ax_tab[64 * 3];
  c.ax = &ax_tab[lane * kAxLane];
  Ray ray = primary_ray(a, a.inv_pv, c, px, a.row0 + li);
  Counters k;  // the walks' accounting interface; nothing of it leaves the kernel
#pragma unroll
  for (int q = 0; q < VRT_CNT_COUNT; ++q) k.c[q] = 0;
  uint32_t steps = 0, flags = 0;
  const Hit h = march<true, false, true>(c, ray, k, steps, flags);  // a miss leaves h's fields zero
  const size_t o = size_t(li) * size_t(a.pitch) + size_t(px);
  ids[o] = make_uint2(uint32_t(h.found ? h.vidx : -1), ray_hit_face(h));
  if (depth)
    depth[o] = h.found ? (__builtin_rintf(comp(h.point, h.axis)) - comp(ray.pos, h.axis)) / comp(ray.dir, h.axis)
                       : __builtin_inff();
}

}  // namespace vrt

#endif  // VRT_IDS_KERNELS_H
