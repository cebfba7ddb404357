// vrt_query_kernels.h — ray queries on the resident volume (vrt_cast_rays*, vrt_pick_pixels): one
// kernel that runs vrt_walk.h's exact walks for a list of rays, one ray per lane, and writes a
// vrt_ray_hit per ray. Included by vrt_render.hip after init_ctx and primary_ray, which it calls.
#ifndef VRT_QUERY_KERNELS_H
#define VRT_QUERY_KERNELS_H

#include "vrt_walk.h"

namespace vrt {

constexpr int kQueryWg = 64 * kQueryWgWaves;  // kQueryWgWaves: vrt_tuning.h

// vrt_ray_hit::face (and vrt_pixel_id::face) of a march's outcome: 0 for a miss
__device__ __forceinline__ uint32_t ray_hit_face(const Hit& h) {
  // the normal has one non-zero component, -sign(dir[axis])
  const bool neg = h.normal.x + h.normal.y + h.normal.z < 0.0f;
  return h.found ? uint32_t(h.axis) | (neg ? 4u : 0u) | (h.voxel << 8) : 0u;
}

// KIND: VRT_CAST_NEAREST (RayMarch of a ray in air: march<.., PRIMARY>), VRT_CAST_OCCLUSION
// (RayMarchShadow along the ray's own direction: skip_walk<SHADOW>, or the literal dda_walk when a
// component is zero, tiny or huge, as walk_shadow chooses for the sun), kQueryPick (the primary ray of
// pixel {px, py} of the frame `a` describes, then as VRT_CAST_NEAREST). The walks are the frame
// kernels', with the ray's own max_length in the lane's Ctx, so a record is bit-exact against the
// oracle's march of that ray. Query i is lane i % kQueryWg of workgroup i / kQueryWg: rays that are
// neighbours in the list (a pick's pixels, a caller's sorted batch) share a wave; an incoherent list
// pays each wave's longest ray (no sorting here). Nothing validates a ray: the walks bound every ray
// by VRT_MAX_STEPS and clamp every texel address into the volume.
// Launch bounds: the workgroup size only. The instance needs no occupancy promise to stay free of
// spills (registers and scratch: DESIGN.md §6 "Ray queries").
template <int KIND>
__global__ void __launch_bounds__(kQueryWg) ray_query_kernel(KArgs a, const uint16_t* __restrict__ vox,
                                                              const void* __restrict__ in, uint32_t count,
                                                              uint4* __restrict__ hits) {
  const uint32_t first = blockIdx.x * uint32_t(kQueryWg);
  if (first >= count) return;  // a workgroup past the list
  const uint32_t i = first + threadIdx.x;
  if (i >= count) return;  // tail lanes of the last wave: masked for the rest of the kernel (no barrier below)
  Ctx c;
  init_ctx(c, a, vox);
  __shared__ float4 ax_tab[kQueryWg * 3];
  c.ax = &ax_tab[threadIdx.x * kAxLane];
  Ray ray;
  if constexpr (KIND == kQueryPick) {
    const int2 p = static_cast<const int2*>(in)[i];
    ray = primary_ray(a, a.inv_pv, c, p.x, p.y);
  } else {
    // a vrt_ray as two 16-byte loads: {origin, max_length}, {dir, reserved} (the compiler narrows the
    // second to the 12 bytes that are used)
    const float4* r = static_cast<const float4*>(in) + 2u * size_t(i);
    const float4 lo = r[0], hi = r[1];
    ray.pos = mk(lo.x, lo.y, lo.z);
    ray.dir = mk(hi.x, hi.y, hi.z);
    ray.len = 0.0f;
    ray.energy = 1.0f;
    ray.voxel = 0;
    ray.rdepth = 0;
    ray.tdepth = 0;
    c.max_len = lo.w;
  }
  Counters k;  // the walks' accounting interface; only steps and flags leave the kernel
#pragma unroll
  for (int q = 0; q < VRT_CNT_COUNT; ++q) k.c[q] = 0;
  uint32_t steps = 0, flags = 0;
  uint4 r0, r1;
  if constexpr (KIND == VRT_CAST_OCCLUSION) {
    WalkState w;
    walk_init(w, ray);
    int axis;
    int32_t vidx;
    uint32_t v;
    int r;
    if (__builtin_expect(fast_path_ok(ray.dir), 1)) {
      const f3 rcp = mk(opaque(rcp_newton(ray.dir.x)), opaque(rcp_newton(ray.dir.y)), opaque(rcp_newton(ray.dir.z)));
      r = skip_walk<true, true>(c, ray.pos, ray.dir, rcp, ray.len, 0u, w, axis, vidx, v);
    } else {
      r = dda_walk<true, true>(c, ray.pos, ray.dir, ray.dir, ray.len, 0u, w, axis, vidx, v);
    }
    walk_account(w, r, VRT_CNT_SHADOW_STEPS, k, steps, flags);
    if (r == WALK_EVENT) flags |= VRT_RAY_FLAG_BLOCKED;
    r0 = make_uint4(~0u, 0u, steps, flags);
    r1 = make_uint4(0u, 0u, 0u, 0u);
  } else {
    const Hit h = march<true, false, true>(c, ray, k, steps, flags);  // a miss leaves h's fields zero
    const uint32_t face = ray_hit_face(h);
    r0 = make_uint4(uint32_t(h.found ? h.vidx : -1), __float_as_uint(h.len), steps, flags);
    r1 = make_uint4(__float_as_uint(h.point.x), __float_as_uint(h.point.y), __float_as_uint(h.point.z), face);
  }
  // a vrt_ray_hit as two 16-byte stores
  uint4* out = hits + 2u * size_t(i);
  out[0] = r0;
  out[1] = r1;
}

}  // namespace vrt

#endif  // VRT_QUERY_KERNELS_H
