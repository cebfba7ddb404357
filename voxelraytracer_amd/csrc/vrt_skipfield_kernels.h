// vrt_skipfield_kernels.h — the skip field of the packed volume(s): the distance / forward-distance
// passes, the packs and the plane-N pack, plus the box write of an in-place edit with its glass
// counts. One kernel family builds the field for an upload and for vrt_update_volume_region: every
// kernel works on boxes of GLOBAL voxel coordinates (origin + extent) whose values live in
// region-local scratch (x fastest inside the box), and the outside-distance terms use the global
// coordinate, so a pass over a box yields exactly the bytes a pass over the volume has on that box.
// An upload is the edit of the box [0, N)^3: every box is then the whole volume.
// Includes vrt_internal.h, vrt_math.h and vrt_walk.h (kDistCap, the packed texel layout), and
// vrt_skipfield_plan.h (Region, and the host arithmetic that chooses every box the kernels are given).
#ifndef VRT_SKIPFIELD_KERNELS_H
#define VRT_SKIPFIELD_KERNELS_H

#include "vrt_internal.h"
#include "vrt_math.h"
#include "vrt_skipfield_plan.h"
#include "vrt_walk.h"

namespace vrt {

static_assert(kPlanDistCap == kDistCap, "the pass plan's boxes are sized by the kernels' cap");

// Cells are counted in 32 bits. The largest box is the whole volume at N = 1024 (single layout):
// 2^30 cells. A grid-stride counter ends its loop below cells + gridDim * 256 <= 2^30 + 16384 * 256
// = 2^30 + 2^22 < 2^32, so it cannot wrap; a region-local index is < cells. Offsets into the
// canonical or a packed volume ((N+1)^3 texels) are formed in 64 bits.
__host__ __device__ inline uint32_t region_cells(const Region& r) {
  return uint32_t(r.ex) * uint32_t(r.ey) * uint32_t(r.ez);
}

// Write the box-local bytes `src` into the canonical volume's box `b` and count, over the box, the
// glass and non-empty voxels before (out[0], out[1]) and after (out[2], out[3]) and the cells whose
// emptiness changes (out[4]; 0: every skip distance stands): one wave-reduced atomic set per wave.
__global__ void __launch_bounds__(256) edit_apply_kernel(const uint8_t* __restrict__ src,
                                                         uint8_t* __restrict__ vox, Region b, uint32_t n,
                                                         unsigned long long* __restrict__ out) {
  const uint32_t total = region_cells(b);
  uint32_t c[5] = {0u, 0u, 0u, 0u, 0u};
  for (uint32_t q = blockIdx.x * 256u + threadIdx.x; q < total; q += gridDim.x * 256u) {
    const uint32_t lx = q % uint32_t(b.ex), t = q / uint32_t(b.ex);
    const uint32_t ly = t % uint32_t(b.ey), lz = t / uint32_t(b.ey);
    const uint64_t g = uint64_t(b.x0 + lx) + (uint64_t(b.y0 + ly) + uint64_t(b.z0 + lz) * n) * n;
    const uint32_t was = vox[g], now = src[q];
    vox[g] = uint8_t(now);
    c[0] += mat_id(was) == 2u ? 1u : 0u;
    c[1] += was != 0u ? 1u : 0u;
    c[2] += mat_id(now) == 2u ? 1u : 0u;
    c[3] += now != 0u ? 1u : 0u;
    c[4] += (was != 0u) != (now != 0u) ? 1u : 0u;
  }
#pragma unroll
  for (int i = 0; i < 5; ++i) {
    uint32_t v = c[i];
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
    if ((threadIdx.x & 63u) == 0u && v) atomicAdd(out + i, (unsigned long long)v);
  }
}

// One-sided pass of the octant forward distance along `axis` in direction sg = +-1:
// out(v) = min(kFwdCap, distance to the outside pseudo-voxel ahead (N - c or c + 1),
//              min over 0 <= o of max(o, in(v + sg*o*e_axis))),
// where the first (x) pass reads in = 0 for a non-empty voxel and kFwdCap otherwise. x, then y,
// then z: F(v) = min over non-empty / outside u in v's forward octant of max_a |u_a - v_a| (max
// and min commute through the passes), i.e. the edge of the largest empty in-volume cube
// anchored at v and extending along (sx, sy, sz). max(o, .) >= o, so the scan stops at o = d.
// Out box `ob` (region-local), input values in box `ib` (the canonical volume itself for the first
// pass: ib = [0, N)^3). ib holds ob on the other two axes and, along `axis`, ob extended
// kFwdCap - 1 cells ahead (clipped to the volume): the scan reads o < d <= min(kFwdCap, outside
// distance) cells ahead, so every read is inside ib.
__global__ void __launch_bounds__(256) fwd_pass_kernel(const uint8_t* __restrict__ in, Region ib,
                                                       uint8_t* __restrict__ out, Region ob, uint32_t n,
                                                       int axis, int sg, int first) {
  const uint32_t total = region_cells(ob);
  const int64_t stride = axis == 0 ? 1 : (axis == 1 ? int64_t(ib.ex) : int64_t(ib.ex) * ib.ey);
  const int64_t step = sg > 0 ? stride : -stride;
  for (uint32_t q = blockIdx.x * 256u + threadIdx.x; q < total; q += gridDim.x * 256u) {
    const uint32_t lx = q % uint32_t(ob.ex), t = q / uint32_t(ob.ex);
    const uint32_t ly = t % uint32_t(ob.ey), lz = t / uint32_t(ob.ey);
    const int32_t gx = ob.x0 + int32_t(lx), gy = ob.y0 + int32_t(ly), gz = ob.z0 + int32_t(lz);
    const uint32_t coord = uint32_t(axis == 0 ? gx : (axis == 1 ? gy : gz));
    const int64_t base = int64_t(gx - ib.x0) + (int64_t(gy - ib.y0) + int64_t(gz - ib.z0) * ib.ey) * ib.ex;
    uint32_t d = min(sg > 0 ? n - coord : coord + 1u, kFwdCap);
    for (uint32_t o = 0; o < d; ++o) {
      const uint8_t v = in[base + int64_t(o) * step];
      const uint32_t val = first ? (v != 0 ? 0u : kFwdCap) : uint32_t(v);
      d = min(d, max(o, val));
    }
    out[q] = uint8_t(d);
  }
}

// Pack the texel box `pb` of octant (sx, sy, sz)'s padded (N+1)^3 volume `dst`: voxel | G << 8 with
// G(w) = F(w - s) - 1 from the region-local F of box `fb` (0 when w - s is outside the volume or
// F(w - s) = 0). pb lies in [0, N)^3; plane N is edge_pack_kernel's. fwd == nullptr: the edit
// changed no cell's emptiness, the texel keeps its G.
__global__ void __launch_bounds__(256) fwd_pack_kernel(const uint8_t* __restrict__ vox,
                                                       const uint8_t* __restrict__ fwd, Region fb,
                                                       uint16_t* __restrict__ dst, Region pb, uint32_t n,
                                                       int sx, int sy, int sz) {
  const uint32_t total = region_cells(pb);
  const uint64_t p = uint64_t(n) + 1u;
  for (uint32_t q = blockIdx.x * 256u + threadIdx.x; q < total; q += gridDim.x * 256u) {
    const uint32_t lx = q % uint32_t(pb.ex), t = q / uint32_t(pb.ex);
    const uint32_t ly = t % uint32_t(pb.ey), lz = t / uint32_t(pb.ey);
    const int32_t i = pb.x0 + int32_t(lx), j = pb.y0 + int32_t(ly), k = pb.z0 + int32_t(lz);
    const uint64_t sq = uint64_t(i) + (uint64_t(j) + uint64_t(k) * n) * n;
    const uint64_t dq = uint64_t(i) + (uint64_t(j) + uint64_t(k) * p) * p;
    uint32_t g = 0;
    if (fwd) {
      // w - s inside the volume is inside fb (the anchors whose F the edit can change, clipped)
      const int32_t a = i - sx - fb.x0, b = j - sy - fb.y0, c = k - sz - fb.z0;
      if (a >= 0 && b >= 0 && c >= 0 && a < fb.ex && b < fb.ey && c < fb.ez) {
        const uint32_t f = fwd[uint32_t(a) + (uint32_t(b) + uint32_t(c) * uint32_t(fb.ey)) * uint32_t(fb.ex)];
        g = f > 0u ? f - 1u : 0u;
      }
    } else {
      g = uint32_t(dst[dq]) >> 8;
    }
    dst[dq] = uint16_t(vox[sq] | (g << 8));
  }
}

// Chebyshev distance field, one separable pass per axis (x, then y, then z), capped at
// kDistCap: out(v) = min(kDistCap, distance to the boundary pseudo-voxels -1 and N on this axis,
// min over |o| < kDistCap of max(|o|, in(v + o e_axis))), where the x pass reads in = 0 for a
// non-empty voxel and kDistCap otherwise. The composition is the exact L-inf distance transform
// (capped), so D(v) >= 1 guarantees an empty box of half-width D-1 around v inside the volume.
// Boxes as in fwd_pass_kernel: ib holds ob on the other two axes and, along `axis`, ob extended
// kDistCap - 1 cells to both sides (clipped to the volume).
__global__ void __launch_bounds__(256) dist_pass_kernel(const uint8_t* __restrict__ in, Region ib,
                                                        uint8_t* __restrict__ out, Region ob, uint32_t n,
                                                        int axis, int first) {
  const uint32_t total = region_cells(ob);
  const int64_t stride = axis == 0 ? 1 : (axis == 1 ? int64_t(ib.ex) : int64_t(ib.ex) * ib.ey);
  for (uint32_t q = blockIdx.x * 256u + threadIdx.x; q < total; q += gridDim.x * 256u) {
    const uint32_t lx = q % uint32_t(ob.ex), t = q / uint32_t(ob.ex);
    const uint32_t ly = t % uint32_t(ob.ey), lz = t / uint32_t(ob.ey);
    const int32_t gx = ob.x0 + int32_t(lx), gy = ob.y0 + int32_t(ly), gz = ob.z0 + int32_t(lz);
    const uint32_t coord = uint32_t(axis == 0 ? gx : (axis == 1 ? gy : gz));
    const int64_t base = int64_t(gx - ib.x0) + (int64_t(gy - ib.y0) + int64_t(gz - ib.z0) * ib.ey) * ib.ex;
    uint32_t d = min(min(coord + 1u, n - coord), kDistCap);
    // o < d <= the distance to either face keeps v - o and v + o inside the volume
    for (uint32_t o = 0; o < d; ++o) {
      for (int sgn = -1; sgn <= 1; sgn += 2) {
        if (o == 0 && sgn > 0) break;
        const uint8_t v = in[base + int64_t(sgn) * int64_t(o) * stride];
        const uint32_t val = first ? (v != 0 ? 0u : kDistCap) : uint32_t(v);
        d = min(d, max(o, val));
      }
    }
    out[q] = uint8_t(d);
  }
}

// Pack the texel box `pb` of the single-volume layout (N = 1024) into the padded (N+1)^3 format:
// voxel | D << 8 from the region-local D of box `db` (which holds pb). dist == nullptr: the texel
// keeps its D.
__global__ void __launch_bounds__(256) pack_volume_kernel(const uint8_t* __restrict__ vox,
                                                          const uint8_t* __restrict__ dist, Region db,
                                                          uint16_t* __restrict__ dst, Region pb, uint32_t n) {
  const uint32_t total = region_cells(pb);
  const uint64_t p = uint64_t(n) + 1u;
  for (uint32_t q = blockIdx.x * 256u + threadIdx.x; q < total; q += gridDim.x * 256u) {
    const uint32_t lx = q % uint32_t(pb.ex), t = q / uint32_t(pb.ex);
    const uint32_t ly = t % uint32_t(pb.ey), lz = t / uint32_t(pb.ey);
    const int32_t i = pb.x0 + int32_t(lx), j = pb.y0 + int32_t(ly), k = pb.z0 + int32_t(lz);
    const uint64_t sq = uint64_t(i) + (uint64_t(j) + uint64_t(k) * n) * n;
    const uint64_t dq = uint64_t(i) + (uint64_t(j) + uint64_t(k) * p) * p;
    uint32_t g = 0;
    if (dist) {
      const int32_t a = i - db.x0, b = j - db.y0, c = k - db.z0;
      if (a >= 0 && b >= 0 && c >= 0 && a < db.ex && b < db.ey && c < db.ez)
        g = dist[uint32_t(a) + (uint32_t(b) + uint32_t(c) * uint32_t(db.ey)) * uint32_t(db.ex)];
    } else {
      g = uint32_t(dst[dq]) >> 8;
    }
    dst[dq] = uint16_t(vox[sq] | (g << 8));
  }
}

// Plane N of the padded (N+1)^3 format repeats plane 0 (GL_REPEAT folded into the layout) with
// distance 0 there (those texels are only read at c == N exactly). The padded texels behind a box
// `b` that touches coordinate 0 on the axes of `wrap` (bit a: axis a): texel N on such an axis
// repeats voxel 0, edges and corners (two or three axes at N) included. Local index e_a on a
// wrapped axis stands for texel N; every one of the `octants` packed volumes (pvol texels apart)
// gets the same texel. The cells are three disjoint slabs of the box extended by texel N on its
// wrapped axes: z at N (every x, y), then y at N (z below N), then x at N (y, z below N).
struct EdgeSlabs {
  uint32_t wx, cz, cy, cx;  // extended x extent; cells of the z, y and x slabs (0: axis not wrapped)
};
__host__ __device__ inline EdgeSlabs edge_slabs(const Region& b, int wrap) {
  const uint32_t wx = uint32_t(b.ex) + (wrap & 1 ? 1u : 0u), wy = uint32_t(b.ey) + (wrap & 2 ? 1u : 0u);
  // at most 3 * 1025^2 cells in all
  return EdgeSlabs{wx, wrap & 4 ? wx * wy : 0u, wrap & 2 ? wx * uint32_t(b.ez) : 0u,
                   wrap & 1 ? uint32_t(b.ey) * uint32_t(b.ez) : 0u};
}
__global__ void __launch_bounds__(256) edge_pack_kernel(const uint8_t* __restrict__ vox,
                                                        uint16_t* __restrict__ dst, uint64_t pvol,
                                                        int octants, Region b, int wrap, uint32_t n) {
  const EdgeSlabs e = edge_slabs(b, wrap);
  const uint32_t total = e.cz + e.cy + e.cx;
  const uint64_t p = uint64_t(n) + 1u;
  for (uint32_t q = blockIdx.x * 256u + threadIdx.x; q < total; q += gridDim.x * 256u) {
    uint32_t lx, ly, lz;
    if (q < e.cz) {
      lx = q % e.wx, ly = q / e.wx, lz = uint32_t(b.ez);
    } else if (q - e.cz < e.cy) {
      lx = (q - e.cz) % e.wx, ly = uint32_t(b.ey), lz = (q - e.cz) / e.wx;
    } else {
      lx = uint32_t(b.ex), ly = (q - e.cz - e.cy) % uint32_t(b.ey), lz = (q - e.cz - e.cy) / uint32_t(b.ey);
    }
    const bool nx = lx == uint32_t(b.ex), ny = ly == uint32_t(b.ey), nz = lz == uint32_t(b.ez);
    // a wrapped axis starts at 0, so texel N's source voxel 0 is the box's first cell on it
    const uint32_t si = nx ? 0u : uint32_t(b.x0) + lx, sj = ny ? 0u : uint32_t(b.y0) + ly;
    const uint32_t sk = nz ? 0u : uint32_t(b.z0) + lz;
    const uint32_t i = nx ? n : si, j = ny ? n : sj, k = nz ? n : sk;
    const uint16_t v = vox[uint64_t(si) + (uint64_t(sj) + uint64_t(sk) * n) * n];
    const uint64_t dq = uint64_t(i) + (uint64_t(j) + uint64_t(k) * p) * p;
    for (int o = 0; o < octants; ++o) dst[uint64_t(o) * pvol + dq] = v;
  }
}

}  // namespace vrt

#endif  // VRT_SKIPFIELD_KERNELS_H
