// vrt_skipfield_plan.h — the boxes of a skip-field rebuild (an upload, vrt_update_volume_region), as host arithmetic:
// which texels an edit may change (volume_edit_plan) and the passes that rebuild them, each with its input and output
// box (skipfield_passes). launch_volume_edit_passes (vrt_render.hip) walks that list; the pass kernels
// (vrt_skipfield_kernels.h) read their input box without a bounds test, so the boxes below are what keeps every read
// of theirs in bounds (tests/test_skipfield_passes.py holds them to it). No HIP: includes <cstdint> and vrt_tuning.h.
#ifndef VRT_SKIPFIELD_PLAN_H
#define VRT_SKIPFIELD_PLAN_H

#include <cstdint>

#include "vrt_tuning.h"

namespace vrt {

// A box of voxels: origin and extent in global coordinates (every extent >= 1, inside [0, N)^3).
struct Region {
  int32_t x0, y0, z0, ex, ey, ez;
};

// kDistCap, the cap of the centred distance D, as the plan sees it: vrt_walk.h defines it among the device code this
// header cannot include, and vrt_skipfield_kernels.h, which includes both, asserts that the two are equal
constexpr uint32_t kPlanDistCap = 64;

// The kinds of pass, one kernel each: fwd_pass_kernel, fwd_pack_kernel (octant layout), dist_pass_kernel,
// pack_volume_kernel (single layout), edge_pack_kernel (plane N of either)
enum class SkipPassKind : uint8_t { kFwdPass, kFwdPack, kDistPass, kVolumePack, kEdgePack };

// One launch of a rebuild. A distance pass scans `axis` (forward: in direction sg[axis]) over the output box `out`,
// reading the values of box `in`: the canonical volume (first; `in` is then the whole volume) or the scratch third
// `src`, and writes third `dst`. A pack writes the texel box `out` of packed volume `octant` (forward pack: the
// octant of steps sg) from the distances of box `in` in third `src`; src = -1: no cell's emptiness changed, the
// texels keep their distances and in = out = the edit's box. The edge pack rewrites texel N behind the edit's box
// (in = out) on the axes of `wrap`, in every packed volume.
struct SkipPass {
  SkipPassKind kind;
  bool first;
  int8_t axis, src, dst, octant, wrap;
  int8_t sg[3];
  Region in, out;
};
// an octant rebuild: 2 x, 4 y and 8 z passes, 8 packs, the edge pack
constexpr int kMaxSkipPasses = 23;
struct SkipPlan {
  int count;
  SkipPass pass[kMaxSkipPasses];
};

// The rebuild after a change inside the box [lo, lo + ext) of an n^3 volume (inside [0, n)^3; an upload is the
// whole volume, and every box of the plan then is), in launch order. octants: 8 (forward distances, 3 scratch
// thirds of n^3 bytes) or 1 (the centred distance, 2 thirds); distances = false: no cell's emptiness changed, only
// the packs run
SkipPlan skipfield_passes(int32_t n, int octants, const int32_t lo[3], const int32_t ext[3], bool distances);

// the packed texels an edit may change, per packed volume o: out[o*6 + 0..5] = {x0,y0,z0,x1,y1,z1}
// (half-open, in [0, N)^3): the packs' boxes of skipfield_passes with distances
int volume_edit_plan(int32_t n, int octants, const int32_t lo[3], const int32_t ext[3], int32_t* out);

}  // namespace vrt

#endif  // VRT_SKIPFIELD_PLAN_H
