// vrt_spatial_kernels.h — the ID-guided spatial filter (vrt_spatial_filter_async): one edge-stopping à-trous
// pass over an RGBA8 frame whose edge stop is the ID pass's record. A tap counts only if it shows the pixel's
// own surface (the guide's key, words compared for equality) and, optionally, a colour within `range`; there is
// no depth or normal threshold. All integer arithmetic (DESIGN.md §6 "Spatial filter"). Included by
// vrt_render.hip after vrt_reproject_kernels.h; it calls nothing of the render kernels.
//
// Two forms of the same pass, chosen per step by launch_spatial (kSpatialLdsSteps, vrt_tuning.h):
//   spatial_direct_kernel    every tap is a gather from global memory: 25 ID loads and 25 colour loads per pixel;
//   spatial_lds_kernel<STEP> the workgroup stages its 16x16 tile plus a halo of 2 STEP texels, keys and colours,
//                            in LDS once, and every tap is an LDS read (STEP 1, 2, 4: at most 15 KB).
// Both have the reprojection kernels' shape: workgroups of kSpatialWg threads, four waves, each an 8x8 pixel tile
// of a 16x16 tile. Every address is formed from the workgroup and lane ids under the band test, a tap's address
// only after its test against [0, width) x [0, height): a tap outside the image is never loaded, neither its ID
// nor its colour. No atomics; the direct form has no LDS and no barrier.
#ifndef VRT_SPATIAL_KERNELS_H
#define VRT_SPATIAL_KERNELS_H

#include "vrt_internal.h"

namespace vrt {

// The guide's key of a record: VRT_GUIDE_FACE both words as they are; VRT_GUIDE_PLANE, for a hit, the cell
// coordinate along the face's axis in place of the voxel index (voxel_index = x + N y + N^2 z, N = 2^nlog), so
// that coplanar faces of one material and one orientation share a key. A miss (voxel_index < 0) keeps its
// negative word, which no coordinate equals.
__device__ __forceinline__ uint2 spatial_key(uint2 id, bool plane, uint32_t nlog) {
  if (plane && int32_t(id.x) >= 0) id.x = (id.x >> ((id.y & 3u) * nlog)) & ((1u << nlog) - 1u);
  return id;
}

// The running sums of a pixel: R and B side by side (each sum <= 255 * 256 < 2^16), G, the weights, the taps
struct SpatialSums {
  uint32_t rb = 0, g = 0, wsum = 0, cnt = 0;
};

// One tap with key k and colour c against the centre's key kc and colour cc3 (A byte cleared): valid iff it
// lies in the image (in), the keys are equal and |dR| + |dG| + |dB| <= range (one sum of absolute differences
// over the words' bytes, the A bytes cleared on both sides)
__device__ __forceinline__ void spatial_tap(SpatialSums& s, uint32_t w, uint2 k, uint32_t c, uint2 kc, uint32_t cc3,
                                            int32_t range, bool in) {
  const bool ok =
      in && k.x == kc.x && k.y == kc.y && int32_t(__builtin_amdgcn_sad_u8(c & 0x00FFFFFFu, cc3, 0u)) <= range;
  const uint32_t we = ok ? w : 0u;
  s.rb += we * (c & 0x00FF00FFu);
  s.g += we * ((c >> 8) & 0xFFu);
  s.wsum += we;
  s.cnt += ok ? 1u : 0u;
}

// out_c = (2 acc_c + wsum) / (2 wsum), the rounded mean; wsum >= 36 (the centre is always valid). Integer
// division: operands below 2^18
__device__ __forceinline__ uint32_t spatial_resolve(const SpatialSums& s) {
  const uint32_t den = 2u * s.wsum;
  const uint32_t r = (2u * (s.rb & 0xFFFFu) + s.wsum) / den;
  const uint32_t g = (2u * s.g + s.wsum) / den;
  const uint32_t b = (2u * (s.rb >> 16) + s.wsum) / den;
  return r | (g << 8) | (b << 16) | 0xFF000000u;
}

__device__ __forceinline__ uint32_t spatial_weight(int i, int j) {
  constexpr uint32_t k[5] = {1u, 4u, 6u, 4u, 1u};
  return k[i + 2] * k[j + 2];
}

__global__ void __launch_bounds__(kSpatialWg) spatial_direct_kernel(SpatialArgs a) {
  const uint32_t t = threadIdx.x;
  const int px = int(blockIdx.x) * 16 + int((t >> 6) & 1u) * 8 + int(t & 7u);
  const int li = int(blockIdx.y) * 16 + int(t >> 7) * 8 + int((t >> 3) & 7u);
  if (px >= a.width || li >= a.rows) return;
  const int py = a.row0 + li;
  const size_t o = size_t(py) * size_t(a.pitch) + size_t(px);
  const uint32_t cc = a.in[o];
  if (a.keep && a.keep[o] != 0) {
    a.out[o] = cc;
    if (a.count) a.count[o] = 0;
    return;
  }
  const bool plane = a.guide == VRT_GUIDE_PLANE;
  const uint2 kc = spatial_key(a.ids[o], plane, a.nlog);
  const uint32_t cc3 = cc & 0x00FFFFFFu;
  SpatialSums s;
#pragma unroll
  for (int j = -2; j <= 2; ++j) {
    const int ty = py + j * a.step;
    // a row's five taps: the loads of those in range in flight before the first compare
    uint2 id[5];
    uint32_t c[5];
    bool in[5];
#pragma unroll
    for (int i = -2; i <= 2; ++i) {
      const int tx = px + i * a.step;
      in[i + 2] = tx >= 0 && tx < a.width && ty >= 0 && ty < a.height;
      id[i + 2] = make_uint2(0u, 0u);
      c[i + 2] = 0u;
      if (in[i + 2]) {
        const size_t to = size_t(ty) * size_t(a.pitch) + size_t(tx);
        id[i + 2] = a.ids[to];
        c[i + 2] = a.in[to];
      }
    }
#pragma unroll
    for (int i = -2; i <= 2; ++i)
      spatial_tap(s, spatial_weight(i, j), spatial_key(id[i + 2], plane, a.nlog), c[i + 2], kc, cc3, a.range, in[i + 2]);
  }
  a.out[o] = spatial_resolve(s);
  if (a.count) a.count[o] = uint8_t(s.cnt);
}

// The staged tile of spatial_lds_kernel<STEP>: kT x kT texels around the workgroup's 16x16 tile, rows kS texels
// apart. kS = 8 mod 32: the four 8-texel rows that 32 lanes of a wave read for one tap fall into disjoint banks,
// as 4-byte colours (32 banks) and as 8-byte keys (64 banks).
template <int STEP>
struct SpatialTile {
  static constexpr int kHalo = 2 * STEP, kT = 16 + 2 * kHalo, kS = STEP == 4 ? 40 : 24;
  static_assert(STEP == 1 || STEP == 2 || STEP == 4, "LDS-staged steps");
  static_assert(kS >= kT && (kS % 32 == 8 || kS % 32 == 24), "row stride against the banks");
};

template <int STEP>
__global__ void __launch_bounds__(kSpatialWg) spatial_lds_kernel(SpatialArgs a) {
  using Tile = SpatialTile<STEP>;
  __shared__ uint2 s_key[Tile::kT * Tile::kS];
  __shared__ uint32_t s_col[Tile::kT * Tile::kS];
  const uint32_t t = threadIdx.x;
  const bool plane = a.guide == VRT_GUIDE_PLANE;
  // the tile's texels, keys already formed; a texel outside the image is not loaded (and never read as a tap)
  const int x0 = int(blockIdx.x) * 16 - Tile::kHalo, y0 = a.row0 + int(blockIdx.y) * 16 - Tile::kHalo;
  for (int e = int(t); e < Tile::kT * Tile::kT; e += kSpatialWg) {
    const int ly = e / Tile::kT, lx = e - ly * Tile::kT;
    const int gx = x0 + lx, gy = y0 + ly;
    uint2 k = make_uint2(0u, 0u);
    uint32_t c = 0u;
    if (gx >= 0 && gx < a.width && gy >= 0 && gy < a.height) {
      const size_t to = size_t(gy) * size_t(a.pitch) + size_t(gx);
      k = spatial_key(a.ids[to], plane, a.nlog);
      c = a.in[to];
    }
    s_key[ly * Tile::kS + lx] = k;
    s_col[ly * Tile::kS + lx] = c;
  }
  __syncthreads();
  const int tx0 = int((t >> 6) & 1u) * 8 + int(t & 7u), ty0 = int(t >> 7) * 8 + int((t >> 3) & 7u);
  const int px = int(blockIdx.x) * 16 + tx0, li = int(blockIdx.y) * 16 + ty0;
  if (px >= a.width || li >= a.rows) return;
  const int py = a.row0 + li;
  const size_t o = size_t(py) * size_t(a.pitch) + size_t(px);
  const int lc = (ty0 + Tile::kHalo) * Tile::kS + tx0 + Tile::kHalo;
  const uint32_t cc = s_col[lc];
  if (a.keep && a.keep[o] != 0) {
    a.out[o] = cc;
    if (a.count) a.count[o] = 0;
    return;
  }
  const uint2 kc = s_key[lc];
  const uint32_t cc3 = cc & 0x00FFFFFFu;
  SpatialSums s;
  // Every tap's texel lies in the staged tile, so its LDS reads need no test and a row's ten are in flight
  // together; whether the tap lies in the image enters its validity (a texel outside was staged as zeros, not
  // loaded, and counts for nothing)
  bool inx[5];
#pragma unroll
  for (int i = -2; i <= 2; ++i) inx[i + 2] = px + i * STEP >= 0 && px + i * STEP < a.width;
#pragma unroll
  for (int j = -2; j <= 2; ++j) {
    const bool iny = py + j * STEP >= 0 && py + j * STEP < a.height;
    uint2 k[5];
    uint32_t c[5];
#pragma unroll
    for (int i = -2; i <= 2; ++i) {
      const int l = lc + j * STEP * Tile::kS + i * STEP;
      k[i + 2] = s_key[l];
      c[i + 2] = s_col[l];
    }
#pragma unroll
    for (int i = -2; i <= 2; ++i)
      spatial_tap(s, spatial_weight(i, j), k[i + 2], c[i + 2], kc, cc3, a.range, iny && inx[i + 2]);
  }
  a.out[o] = spatial_resolve(s);
  if (a.count) a.count[o] = uint8_t(s.cnt);
}

}  // namespace vrt

#endif  // VRT_SPATIAL_KERNELS_H
