// vrt_ids_kernels.h — the ID and depth pass (vrt_render_ids*): per pixel, the voxel and face its primary
// ray hits and the hit's depth, without shading. Two kernels, an 8x8 tile per wave either way:
// ids_exact_kernel, every pixel of the band by the pick's exact march, and ids_cert_kernel
// (vrt_set_ids_certified, octant layouts), every pixel by the guarded certified walk and, where that walk
// is unsure, by the exact march in the pixel's own lane. Included by vrt_render.hip after init_ctx,
// primary_ray, vrt_query_kernels.h (ray_hit_face) and vrt_cert_debug_kernels.h (vrt_cert.h).
#ifndef VRT_IDS_KERNELS_H
#define VRT_IDS_KERNELS_H

#include "vrt_cert.h"
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

// The same band in the same shape, for the eight-octant skip layout (the certified walk's skip field): each
// lane forms the primary ray as above and starts the guarded certified walk on it as cert_pixel<.., LEAN =
// false> does (fast_path_ok, exact_start_cell, start_layers_clear<false>, hardware reciprocals, cert_walk<false,
// false, false> from len 0 in air), the form vrt_debug_cert_walks kind 0 holds to the exact walk ray by ray.
// Everything the start and the walk read arrives by value in the launch's arguments, and every load of the
// guarded form tests its address (path_texel, alt_byte): no per-launch host proof, no late-read argument
// block, no state on the device besides the volume.
//  - a certified hit (any byte: glass is an ordinary hit of a primary ray in air) lies in a cell of the
//    volume, entered across the face of its axis: voxel_index is the cell's canonical index, face the axis,
//    the bit of the normal -sign(D_a) and the byte, as ray_hit_face packs them, and the face's plane is the
//    integer c_a + (D_a < 0 ? 1 : 0), which the exact walk's hit coordinate rounds to;
//  - a certified miss is {-1, 0}, depth +inf;
//  - any other lane (the walk unsure, or a start check refused the ray) runs the exact kernel's march in one
//    divergent region after the walk, which a wave enters only if one of its lanes needs it, and stores what
//    ids_exact_kernel stores.
// One store per buffer for all three, the depth by the one expression (plane - pos[a]) / dir[a].
// Every address is formed from the workgroup and lane ids and a.pitch under the band test, as above.
// n_exact (may be null; wave-uniform): one lane of the wave adds the wave's number of exact-path lanes.
// The capturable entry point passes null: no atomics, no state.
__global__ void __launch_bounds__(64) ids_cert_kernel(KArgs a, const uint16_t* __restrict__ vox, uint2* __restrict__ ids,
                                                      float* __restrict__ depth, uint32_t* __restrict__ n_exact) {
  const uint32_t lane = lane_id();
  const int px = int(blockIdx.x) * 8 + int(lane & 7u), li = int(blockIdx.y) * 8 + int(lane >> 3);
  if (px >= a.width || li >= a.rows) return;  // masked for the rest of the kernel (no barrier below)
  Ctx c;
  init_ctx(c, a, vox);
  __shared__ float4 ax_tab[64 * 3];
  c.ax = &ax_tab[lane * kAxLane];
  Ray ray = primary_ray(a, a.inv_pv, c, px, a.row0 + li);
  const f3 P = ray.pos, D = ray.dir;
  int res = CERT_UNSURE;
  bool found = false;
  int axis = 0;
  uint32_t vidx = ~0u, face = 0u;
  float plane = 0.0f;
  int cx, cy, cz;
  if (fast_path_ok(D) && exact_start_cell(c, P, D, cx, cy, cz) && start_layers_clear<false>(c, P, D, cx, cy, cz, 0u)) {
    // hardware reciprocals (<= 1 ulp): the certified walk only needs its own error bounded
    const f3 rcp = mk(__builtin_amdgcn_rcpf(D.x), __builtin_amdgcn_rcpf(D.y), __builtin_amdgcn_rcpf(D.z));
    const CertResult h = cert_walk<false, false, false>(c, P, D, rcp, c.max_len - ray.len, cx, cy, cz, 0.0f,
                                                        mk(0.0f, 0.0f, 0.0f), 0.0f, 0u);
    res = h.res;
    if (res == CERT_HIT) {
      const float da = comp(D, h.axis);
      const int ca = h.axis == 0 ? h.cx : (h.axis == 1 ? h.cy : h.cz);
      found = true;
      axis = h.axis;
      vidx = uint32_t(h.cx + c.n * (h.cy + c.n * h.cz));
      face = uint32_t(h.axis) | (da > 0.0f ? 4u : 0u) | (h.byte << 8);  // the normal is -sign(D_a) e_a
      plane = float(ca + (da < 0.0f ? 1 : 0));
    }
  }
  const bool need = res != CERT_HIT && res != CERT_MISS;
  if (n_exact) {
    const uint64_t m = __ballot(need), act = __ballot(true);
    if (m != 0u && lane == uint32_t(__builtin_ctzll(act))) atomicAdd(n_exact, uint32_t(__builtin_popcountll(m)));
  }
  if (need) {
    Counters k;  // the walks' accounting interface; nothing of it leaves the kernel
#pragma unroll
    for (int q = 0; q < VRT_CNT_COUNT; ++q) k.c[q] = 0;
    uint32_t steps = 0, flags = 0;
    const Hit h = march<true, false, true>(c, ray, k, steps, flags);  // a miss leaves h's fields zero
    found = h.found;
    axis = h.axis;
    vidx = uint32_t(h.found ? h.vidx : -1);
    face = ray_hit_face(h);
    plane = __builtin_rintf(comp(h.point, h.axis));
  }
  const size_t o = size_t(li) * size_t(a.pitch) + size_t(px);
  ids[o] = make_uint2(vidx, face);
  if (depth) depth[o] = found ? (plane - comp(P, axis)) / comp(D, axis) : __builtin_inff();
}

}  // namespace vrt

#endif  // VRT_IDS_KERNELS_H
