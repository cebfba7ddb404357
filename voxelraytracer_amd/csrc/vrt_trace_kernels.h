// vrt_trace_kernels.h — shaded ray queries on the resident volume (vrt_trace_rays*, vrt_trace_pixels):
// one kernel family that runs fragment main (exact_pixel: trace-with-shadow, the bounce stack, the
// colour folded in the reference's order) for a list of rays or of pixels, one per lane, and writes a
// vrt_ray_color per query. Included by vrt_render.hip after init_ctx, primary_ray and exact_pixel,
// which it calls unchanged.
#ifndef VRT_TRACE_KERNELS_H
#define VRT_TRACE_KERNELS_H

#include "vrt_walk.h"

namespace vrt {

constexpr int kTraceWg = 64 * kTraceWgWaves;  // kTraceWgWaves: vrt_tuning.h

// KIND: kTraceRays (`in` holds vrt_ray records: stack[0] = Ray(origin, dir, 0, 1.0, air, 0, 0) as given,
// no RandomizeDirection, the ray's own max_length in the lane's Ctx for the whole tree) or kTracePixels
// (`in` holds {px, py} pairs: the primary ray of that pixel of the frame `a` describes, a.max_len).
// TEX: textured mode, as render_kernel's. The instance of exact_pixel is the STATS frame instance's
// (render_kernel<true, TEX>): exact walks only, no certified walk, so a record is the shader's for
// every input. Query i is lane i % kTraceWg of workgroup i / kTraceWg, as in ray_query_kernel; here a
// wave lasts as long as its longest bounce tree. Nothing validates a ray: the walks bound every ray by
// VRT_MAX_STEPS and clamp every texel address into the volume.
// Launch bounds: the workgroup size and kTraceMinWaves resident waves per SIMD (vrt_tuning.h; registers,
// scratch and waves per SIMD of the four instances: DESIGN.md §6 "Shaded ray queries"). The lane-local Counters is the walks' accounting interface; only
// steps and flags leave the kernel, with the first march's hit and the colour.
template <int KIND, bool TEX>
__global__ void __launch_bounds__(kTraceWg, kTraceMinWaves) ray_trace_kernel(KArgs a, const uint16_t* __restrict__ vox,
                                                              const void* __restrict__ in, uint32_t count,
                                                              uint4* __restrict__ out) {
  const uint32_t first = blockIdx.x * uint32_t(kTraceWg);
  if (first >= count) return;  // a workgroup past the list
  const uint32_t i = first + threadIdx.x;
  if (i >= count) return;  // tail lanes of the last wave: masked for the rest of the kernel (no barrier below)
  Ctx c;
  init_ctx(c, a, vox);
  // the exact path's axis table and the bounce stack's bottom entry, per lane
  __shared__ float4 ax_tab[kTraceWg * 3];
  __shared__ float lstk[kStackWords * kTraceWg];
  c.ax = &ax_tab[threadIdx.x * kAxLane];
  Ray ray;
  if constexpr (KIND == kTracePixels) {
    const int2 p = static_cast<const int2*>(in)[i];
    ray = primary_ray(a, a.inv_pv, c, p.x, p.y);
  } else {
    // a vrt_ray as two 16-byte loads: {origin, max_length}, {dir, reserved}
    const float4* r = static_cast<const float4*>(in) + 2u * size_t(i);
    const float4 lo = r[0], hi = r[1];
    ray.pos = mk(lo.x, lo.y, lo.z);
    ray.dir = mk(hi.x, hi.y, hi.z);
    ray.len = 0.0f;
    ray.energy = 1.0f;
    ray.voxel = 0;
    ray.rdepth = 0;
    ray.tdepth = 0;
    c.max_len = lo.w;  // u_MaxRayLength of this ray's whole tree
  }
  Counters k;
#pragma unroll
  for (int q = 0; q < VRT_CNT_COUNT; ++q) k.c[q] = 0;
  uint32_t steps = 0, flags = 0;
  int32_t hit_vidx = -1;
  float hit_len = 0.0f;
  f3 color = mk(0.0f, 0.0f, 0.0f);
  (void)exact_pixel<true, TEX, false, false, kTraceWg>(a, c, ray, color, k, steps, flags, hit_vidx, hit_len,
                                                       &lstk[threadIdx.x]);
  // a vrt_ray_color as two 16-byte stores; the record's index re-derived (not kept live across the walks)
  uint4* o = out + 2u * (size_t(blockIdx.x) * size_t(kTraceWg) + size_t(threadIdx.x));
  o[0] = make_uint4(uint32_t(hit_vidx), __float_as_uint(hit_len), steps, flags);
  o[1] = make_uint4(__float_as_uint(color.x), __float_as_uint(color.y), __float_as_uint(color.z),
                    __float_as_uint(1.0f));
}

}  // namespace vrt

#endif  // VRT_TRACE_KERNELS_H
