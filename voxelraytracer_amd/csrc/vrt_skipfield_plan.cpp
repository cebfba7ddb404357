// vrt_skipfield_plan.cpp — the boxes of a skip-field rebuild (vrt_skipfield_plan.h): the spans of an edit along one
// axis, the texel boxes it may change and the list of passes that rebuild them. Integer arithmetic only: it calls
// nothing of the HIP or RCCL runtime and includes neither's headers, so a plain host compiler builds and links it.
#include <algorithm>
#include <cstdint>

#include "vrt_skipfield_plan.h"

namespace vrt {

namespace {

struct Span {  // cells [a, b] of one axis, clipped to the volume
  int32_t a, b;
};
Span clip_span(int64_t a, int64_t b, int32_t n) {
  return Span{int32_t(std::max<int64_t>(a, 0)), int32_t(std::min<int64_t>(b, int64_t(n) - 1))};
}
// Edit cells [lo, hi) of an axis. An occupied cell kFwdCap or more cells ahead cannot lower a capped
// F, so the anchors whose F can change lie up to kFwdCap - 1 cells behind the edit (against sg) ...
Span fwd_anchors(int32_t lo, int32_t hi, int sg, int32_t n) {
  const int64_t r = int64_t(kFwdCap) - 1;
  return sg > 0 ? clip_span(lo - r, int64_t(hi) - 1, n) : clip_span(lo, int64_t(hi) - 1 + r, n);
}
// ... a pass over them reads its input up to kFwdCap - 1 cells ahead (the same cells for both signs) ...
Span fwd_inputs(int32_t lo, int32_t hi, int32_t n) {
  const int64_t r = int64_t(kFwdCap) - 1;
  return clip_span(lo - r, int64_t(hi) - 1 + r, n);
}
// ... and G(w) = F(w - s) - 1 moves them one cell ahead: the packed texels (with the edit's own
// cells, for the voxel bytes)
Span fwd_texels(int32_t lo, int32_t hi, int sg, int32_t n) {
  const int64_t r = int64_t(kFwdCap) - 1;
  const int64_t a = (sg > 0 ? lo - r : int64_t(lo)) + sg, b = (sg > 0 ? int64_t(hi) - 1 : int64_t(hi) - 1 + r) + sg;
  return clip_span(std::min<int64_t>(a, lo), std::max<int64_t>(b, int64_t(hi) - 1), n);
}
// the centred D (single layout): cells within `reach` of the edit
Span dist_span(int32_t lo, int32_t hi, int64_t reach, int32_t n) {
  return clip_span(lo - reach, int64_t(hi) - 1 + reach, n);
}
Region region_of(Span x, Span y, Span z) {
  return Region{x.a, y.a, z.a, x.b - x.a + 1, y.b - y.a + 1, z.b - z.a + 1};
}

// a distance pass along `axis` (forward: in direction sg) from `in` (src = -1: the canonical volume) into third dst
SkipPass scan_pass(SkipPassKind kind, int axis, int sg, int src, const Region& in, int dst, const Region& out) {
  SkipPass p{};
  p.kind = kind;
  p.first = src < 0;
  p.axis = int8_t(axis);
  p.src = int8_t(src);
  p.dst = int8_t(dst);
  p.octant = -1;
  p.sg[axis] = int8_t(sg);
  p.in = in;
  p.out = out;
  return p;
}
// a pack of the texel box `out` of packed volume `octant` from the distances of `in` in third src (-1: kept)
SkipPass pack_pass(SkipPassKind kind, int octant, int sx, int sy, int sz, int src, const Region& in, const Region& out) {
  SkipPass p{};
  p.kind = kind;
  p.axis = -1;
  p.src = int8_t(src);
  p.dst = -1;
  p.octant = int8_t(octant);
  p.sg[0] = int8_t(sx);
  p.sg[1] = int8_t(sy);
  p.sg[2] = int8_t(sz);
  p.in = in;
  p.out = out;
  return p;
}

}  // namespace

int volume_edit_plan(int32_t n, int octants, const int32_t lo[3], const int32_t ext[3], int32_t* out) {
  for (int o = 0; o < octants; ++o)
    for (int a = 0; a < 3; ++a) {
      const int32_t hi = lo[a] + ext[a];
      const Span t = octants == 8 ? fwd_texels(lo[a], hi, (o >> a & 1) ? -1 : 1, n)
                                  : dist_span(lo[a], hi, int64_t(kPlanDistCap) - 1, n);
      out[o * 6 + a] = t.a;
      out[o * 6 + 3 + a] = t.b + 1;
    }
  return octants;
}

SkipPlan skipfield_passes(int32_t n, int octants, const int32_t lo[3], const int32_t ext[3], bool distances) {
  using K = SkipPassKind;
  SkipPlan plan{};
  auto add = [&plan](const SkipPass& p) { plan.pass[plan.count++] = p; };
  const int32_t hi[3] = {lo[0] + ext[0], lo[1] + ext[1], lo[2] + ext[2]};
  const Region box{lo[0], lo[1], lo[2], ext[0], ext[1], ext[2]};
  const Region whole{0, 0, 0, n, n, n};
  // region-local scratch: every box is clipped to the volume, so each fits N^3 bytes. For an upload
  // (lo = 0, ext = N on every axis) every span clips to [0, N - 1] and every box below is `whole`.
  if (octants == 8) {
    // octant forward distances: 2 x passes, 4 y passes, 8 z passes + packs (x -> y -> z nesting), the x passes'
    // values in third 0, the y passes' in 1, the z passes' in 2
    const Span iy = fwd_inputs(lo[1], hi[1], n), iz = fwd_inputs(lo[2], hi[2], n);
    for (int sx = 1; sx >= -1; sx -= 2) {
      const Span ax = fwd_anchors(lo[0], hi[0], sx, n);
      const Region rx = region_of(ax, iy, iz);  // x pass: the y and z passes' inputs
      if (distances) add(scan_pass(K::kFwdPass, 0, sx, -1, whole, 0, rx));
      for (int sy = 1; sy >= -1; sy -= 2) {
        const Span ay = fwd_anchors(lo[1], hi[1], sy, n);
        const Region ry = region_of(ax, ay, iz);
        if (distances) add(scan_pass(K::kFwdPass, 1, sy, 0, rx, 1, ry));
        for (int sz = 1; sz >= -1; sz -= 2) {
          const Span az = fwd_anchors(lo[2], hi[2], sz, n);
          const Region rz = region_of(ax, ay, az);
          const int o = (sx < 0 ? 1 : 0) | (sy < 0 ? 2 : 0) | (sz < 0 ? 4 : 0);
          if (distances) {
            add(scan_pass(K::kFwdPass, 2, sz, 1, ry, 2, rz));
            const Region pb = region_of(fwd_texels(lo[0], hi[0], sx, n), fwd_texels(lo[1], hi[1], sy, n),
                                        fwd_texels(lo[2], hi[2], sz, n));
            add(pack_pass(K::kFwdPack, o, sx, sy, sz, 2, rz, pb));
          } else {
            add(pack_pass(K::kFwdPack, o, sx, sy, sz, -1, box, box));
          }
        }
      }
    }
  } else if (distances) {
    const int64_t r1 = int64_t(kPlanDistCap) - 1;
    const Span ax = dist_span(lo[0], hi[0], r1, n), ay = dist_span(lo[1], hi[1], r1, n);
    const Span az = dist_span(lo[2], hi[2], r1, n);
    // the z pass reads y-pass values kDistCap - 1 cells to both sides in z, the y pass x-pass values in y
    const Span iy = dist_span(lo[1], hi[1], 2 * r1, n), iz = dist_span(lo[2], hi[2], 2 * r1, n);
    const Region rx = region_of(ax, iy, iz), ry = region_of(ax, ay, iz), rz = region_of(ax, ay, az);
    add(scan_pass(K::kDistPass, 0, 0, -1, whole, 0, rx));
    add(scan_pass(K::kDistPass, 1, 0, 0, rx, 1, ry));
    add(scan_pass(K::kDistPass, 2, 0, 1, ry, 0, rz));
    add(pack_pass(K::kVolumePack, 0, 0, 0, 0, 0, rz, rz));
  } else {
    add(pack_pass(K::kVolumePack, 0, 0, 0, 0, -1, box, box));
  }
  // texel N of an axis repeats voxel 0: rewritten when the box holds coordinate 0 of that axis
  const int wrap = (lo[0] == 0 ? 1 : 0) | (lo[1] == 0 ? 2 : 0) | (lo[2] == 0 ? 4 : 0);
  if (wrap) {
    SkipPass e = pack_pass(K::kEdgePack, -1, 0, 0, 0, -1, box, box);
    e.wrap = int8_t(wrap);
    add(e);
  }
  return plan;
}

}  // namespace vrt
