// vrt_reproject_kernels.h — the reprojected temporal filter (vrt_reproject_temporal_async): per pixel, the
// history is fetched where the pixel's surface point was on screen in the previous frame, and blended in only
// if the previous frame showed the same face of the same voxel there (the ID pass's records, both words
// equal). One streaming kernel, no walk and no volume read. Included by vrt_render.hip after temporal_blend,
// init_ctx, primary_ray and vrt_ids_kernels.h. Below it, the fetch modes of vrt_reproject_temporal_fetch_async:
// the nearest filter with a tap byte, and the bilinear fetch with its four taps validated by ID.
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

// ---- vrt_reproject_temporal_fetch_async: the fetch modes ------------------------------------------
// reproject_kernel above stays as it is (the old entry point and VRT_FETCH_NEAREST without d_taps launch
// it); the two kernels below restate its steps 1-6 through reproject_screen, which only they call.

// Steps 1-6 of the filter for band pixel (px, li) with record `id` and `depth`, the operations of
// reproject_kernel in its order: 0 with (sx, sy) inside [0, width) x [0, height), else the code -2 or -1.
__device__ __forceinline__ int32_t reproject_screen(const KArgs& a, const ReprojArgs& r, int px, int li, uint2 id,
                                                    float depth, float& sx, float& sy) {
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
  sx = sy = 0.0f;
  if (!(clip[3] > 0.0f)) return -2;
  const float fw = float(a.width), fh = float(a.height);
  sx = ((clip[0] / clip[3]) * 0.5f + 0.5f) * fw;
  sy = ((clip[1] / clip[3]) * 0.5f + 0.5f) * fh;
  if (!(sx >= 0.0f && sx < fw && sy >= 0.0f && sy < fh)) return -1;
  return 0;
}

// VRT_FETCH_NEAREST with a tap buffer: reproject_kernel's pixels, codes and colours (the same operations), and
// taps[o] = 1 for an accepted pixel, 0 otherwise. The same grid, workgroups and address rules.
__global__ void __launch_bounds__(kReprojWg) reproject_nearest_taps_kernel(KArgs a, ReprojArgs r, uint8_t* taps) {
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
    float sx, sy;
    code = reproject_screen(a, r, px, li, id, r.depth[o], sx, sy);
    if (code == 0) {
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
  r.out[o] = color;
  if (r.src) r.src[o] = code;
  taps[o] = code >= 0 ? uint8_t(1) : uint8_t(0);
}

// VRT_FETCH_BILINEAR (DESIGN.md §6 "Bilinear history fetch"): the four texels around (sx - 0.5, sy - 0.5),
// each used only if it lies in the previous image, has a weight > 0 and shows the pixel's own voxel face
// (both ID words); the history is their weighted mean over the valid weights, blended and quantised once.
// reproject_kernel's shape: a wave's four gathers fall into the few lines of the previous frame its 8x8
// tile maps to. No LDS, no barrier, no atomics. A tap's address is formed only after its integer range
// test; a tap that fails it is not loaded, neither its ID nor its colour; an invalid tap's colour is not
// loaded (it enters as an exact zero). taps may be null.
__global__ void __launch_bounds__(kReprojWg) reproject_bilinear_kernel(KArgs a, ReprojArgs r, uint8_t* taps) {
  const uint32_t t = threadIdx.x;
  const int px = int(blockIdx.x) * 16 + int((t >> 6) & 1u) * 8 + int(t & 7u);
  const int li = int(blockIdx.y) * 16 + int(t >> 7) * 8 + int((t >> 3) & 7u);
  if (px >= a.width || li >= a.rows) return;
  const size_t o = size_t(li) * size_t(a.pitch) + size_t(px);
  const uint32_t raw = r.raw[o];
  uint32_t color = raw, mask = 0;
  int32_t code = -4;
  if (r.prev) {
    const uint2 id = r.ids[o];
    float sx, sy;
    code = reproject_screen(a, r, px, li, id, r.depth[o], sx, sy);
    if (code == 0) {
      const float tx = sx - 0.5f, ty = sy - 0.5f;
      const float x0 = __builtin_floorf(tx), y0 = __builtin_floorf(ty);
      const float fx = tx - x0, fy = ty - y0;
      const int ix0 = int(x0), iy0 = int(y0);
      const float gx = 1.0f - fx, gy = 1.0f - fy;
      const float wk[4] = {gx * gy, fx * gy, gx * fy, fx * fy};
      size_t po[4];
      float v[4];
      // the ID loads of the taps in range, all four in flight before the first compare
      uint2 pid[4];
      bool in[4];
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const int qx = ix0 + (k & 1), qy = iy0 + (k >> 1);
        in[k] = qx >= 0 && qx < a.width && qy >= 0 && qy < a.height && wk[k] > 0.0f;
        po[k] = 0;
        pid[k] = make_uint2(0u, 0u);
        if (in[k]) {
          po[k] = size_t(qy) * size_t(r.prev_pitch) + size_t(qx);
          pid[k] = r.prev_ids[po[k]];
        }
      }
      uint32_t hc[4];
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const bool valid = in[k] && pid[k].x == id.x && pid[k].y == id.y;
        v[k] = valid ? wk[k] : 0.0f;
        hc[k] = 0u;
        if (valid) {
          mask |= 1u << k;
          hc[k] = r.prev[po[k]];
        }
      }
      if (mask == 0u) {
        code = -3;
      } else {
        const int qx = int(__builtin_floorf(sx)), qy = int(__builtin_floorf(sy));
        code = qy * a.width + qx;
        const float wsum = ((v[0] + v[1]) + v[2]) + v[3];
        const float om = 1.0f - r.alpha;
        color = 0xFF000000u;
#pragma unroll
        for (int ch = 0; ch < 3; ++ch) {
          const int sh = 8 * ch;
          const float h = (((v[0] * unorm8_read((hc[0] >> sh) & 0xFFu) + v[1] * unorm8_read((hc[1] >> sh) & 0xFFu)) +
                            v[2] * unorm8_read((hc[2] >> sh) & 0xFFu)) +
                           v[3] * unorm8_read((hc[3] >> sh) & 0xFFu)) /
                          wsum;
          color |= unorm8(r.alpha * unorm8_read((raw >> sh) & 0xFFu) + om * h) << sh;
        }
      }
    }
  }
  r.out[o] = color;
  if (r.src) r.src[o] = code;
  if (taps) taps[o] = uint8_t(mask);
}

}  // namespace vrt

#endif  // VRT_REPROJECT_KERNELS_H
