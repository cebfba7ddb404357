// vrt_instances.h — the instances of the two frame kernels (render_kernel, and the exact pass's exact_pass_kernel /
// exact_pass_kernel_capped: vrt_render.hip), each listed once with named template arguments, and the choice of a
// launch's instances from what launch_render reads. Host arithmetic: includes <cstdint> and vrt_tuning.h only and
// compiles with a plain host compiler (tests/test_render_instances.py holds the choice to the cascades it replaced).
// vrt_render.hip builds its kernel-pointer tables from these arrays, row I from kRenderInstances[I]'s fields, so a
// row cannot disagree with its kernel: a new instance is a new row and, if it is a new case, a line in the choice.
#ifndef VRT_INSTANCES_H
#define VRT_INSTANCES_H

#include <cstdint>

#include "vrt_tuning.h"

namespace vrt {

// render_kernel<STATS, TEX, CERT, ORD, DEFER, FB, TREE> (the arguments' meaning: at the kernel)
struct RenderInstance {
  bool stats, tex;
  int cert;
  bool ord, defer, fb, tree;
};
constexpr bool operator==(const RenderInstance& a, const RenderInstance& b) {
  return a.stats == b.stats && a.tex == b.tex && a.cert == b.cert && a.ord == b.ord && a.defer == b.defer &&
         a.fb == b.fb && a.tree == b.tree;
}
constexpr RenderInstance kRenderInstances[] = {
    // stats  tex    cert ord    defer  fb     tree
    // launches with hit records or counters: exact walks, one frame
    {true, false, 0, false, false, false, false},
    {true, true, 0, false, false, false, false},
    // in-lane colour frames: exact walks only, certified exact-path rays, certified pixels (these with a tile order
    // and, one frame per launch, with certified trees)
    {false, false, 0, false, false, false, false},
    {false, false, 1, false, false, false, false},
    {false, false, 2, false, false, false, false},
    {false, false, 2, true, false, false, false},
    {false, false, 2, false, false, false, true},
    {false, false, 2, true, false, false, true},
    // the same as frame batches
    {false, false, 0, false, false, true, false},
    {false, false, 1, false, false, true, false},
    {false, false, 2, false, false, true, false},
    {false, false, 2, true, false, true, false},
    // in-lane textured frames: every pixel takes the exact walk, its shadow rays certified walks or not
    {false, true, 0, false, false, false, false},
    {false, true, 1, false, false, false, false},
    {false, true, 0, false, false, true, false},
    {false, true, 1, false, false, true, false},
    // the certified pass of a deferred pair: colour, colour with certified trees, textured; one frame or a batch
    {false, false, 2, false, true, false, false},
    {false, false, 2, false, true, true, false},
    {false, false, 2, false, true, false, true},
    {false, false, 2, false, true, true, true},
    {false, true, 2, false, true, false, false},
    {false, true, 2, false, true, true, false},
};
constexpr int kRenderInstanceCount = int(sizeof(kRenderInstances) / sizeof(kRenderInstances[0]));

// The exact pass of a deferred pair: exact_pass_kernel<TEX, CERT, WAVES, SB, FB>, or where `capped`
// exact_pass_kernel_capped<CERT, SB, FB> (colour only; its waves follow from kExactVgprs, `waves` is not read)
struct ExactInstance {
  bool tex;
  int cert, waves;
  uint32_t sparse_batch;
  bool fb, capped;
};
constexpr bool operator==(const ExactInstance& a, const ExactInstance& b) {
  return a.tex == b.tex && a.cert == b.cert && a.waves == b.waves && a.sparse_batch == b.sparse_batch &&
         a.fb == b.fb && a.capped == b.capped;
}
// the colour whole-frame pair runs under the VGPR cap where one is set
constexpr bool kExactCapped = kExactVgprs != 0;
enum ExactKind { kExactTextured = 0, kExactShortBand = 1, kExactWholeFrame = 2 };
constexpr ExactInstance kExactInstances[] = {
    // tex  cert waves        sparse_batch     fb     capped          (row 2 * ExactKind + fb)
    {true, 1, kExactWaves, kSparseBatchTex, false, false},
    {true, 1, kExactWaves, kSparseBatchTex, true, false},
    {false, 2, kFatWaves, kSparseBatchFat, false, false},
    {false, 2, kFatWaves, kSparseBatchFat, true, false},
    {false, 2, kExactWaves, kSparseBatch, false, kExactCapped},
    {false, 2, kExactWaves, kSparseBatch, true, kExactCapped},
};
constexpr int kExactInstanceCount = int(sizeof(kExactInstances) / sizeof(kExactInstances[0]));

// ---- the choice ---------------------------------------------------------------------------------------------------
// What a launch is, as launch_render reads it: stats (hit records or counters asked for), and of its KArgs textured,
// cert, tree, order != nullptr, defer != nullptr, nframes and exact_fat.

// The deferred pair (certified pass, then the exact pass over the pixels it left) instead of one in-lane launch
constexpr bool deferred_pair(bool stats, int cert, bool defer) { return defer && !stats && cert == 2; }

// The render_kernel instance of a launch, every input it does not read set to its default:
//  - a stats launch reads `textured` alone (exact walks, one frame, dispatch order);
//  - the certified pass of a deferred pair has no tile order (it has no long waves); trees on colour frames only;
//  - in-lane textured frames take CERT 1 for every cert >= 1 (the hit colour needs the exact hit point) and have
//    neither a tile order nor trees;
//  - in-lane colour frames have the tile order and the trees at CERT 2 only, and the trees not in frame batches.
constexpr RenderInstance render_instance_of(bool stats, bool textured, int cert, bool tree, bool order, bool defer,
                                            int nframes) {
  const bool fb = nframes > 1;
  if (deferred_pair(stats, cert, defer)) return {false, textured, 2, false, true, fb, !textured && tree};
  if (stats) return {true, textured, 0, false, false, false, false};
  if (textured) return {false, true, cert >= 1 ? 1 : 0, false, false, fb, false};
  const int c = cert == 2 ? 2 : (cert == 1 ? 1 : 0);
  return {false, false, c, c == 2 && order, false, fb, c == 2 && !fb && tree};
}

// A row's key: its fields packed, the index into kRenderRowOfKey
constexpr unsigned render_key(const RenderInstance& r) {
  return unsigned(r.stats) | unsigned(r.tex) << 1 | unsigned(r.cert) << 2 | unsigned(r.ord) << 4 |
         unsigned(r.defer) << 5 | unsigned(r.fb) << 6 | unsigned(r.tree) << 7;
}
struct RenderRowOfKey {
  int8_t row[256];
};
constexpr RenderRowOfKey render_rows_by_key() {
  RenderRowOfKey t{};
  for (int k = 0; k < 256; ++k) t.row[k] = -1;
  for (int i = 0; i < kRenderInstanceCount; ++i) t.row[render_key(kRenderInstances[i])] = int8_t(i);
  return t;
}
constexpr RenderRowOfKey kRenderRowOfKey = render_rows_by_key();

// The rows of a launch: kRenderInstances[render], and for a deferred pair kExactInstances[exact] (else exact = -1)
struct InstanceChoice {
  int render, exact;
};
constexpr InstanceChoice choose_instances(bool stats, bool textured, int cert, bool tree, bool order, bool defer,
                                          int nframes, bool exact_fat) {
  const int render = kRenderRowOfKey.row[render_key(render_instance_of(stats, textured, cert, tree, order, defer, nframes))];
  if (!deferred_pair(stats, cert, defer)) return {render, -1};
  // textured frames keep their instance in short bands too (they get slower in the short-band one)
  const ExactKind kind = textured ? kExactTextured : (exact_fat ? kExactShortBand : kExactWholeFrame);
  return {render, 2 * int(kind) + (nframes > 1 ? 1 : 0)};
}

// The table holds a row for every launch there is, and no two rows name one kernel
constexpr bool instance_tables_sound() {
  for (int i = 0; i < kRenderInstanceCount; ++i)
    if (kRenderRowOfKey.row[render_key(kRenderInstances[i])] != i) return false;  // a duplicate row
  for (int q = 0; q < 2 * 2 * 4 * 2 * 2 * 2 * 2 * 2; ++q) {
    const bool stats = q & 1, textured = q >> 1 & 1, tree = q >> 4 & 1, order = q >> 5 & 1, defer = q >> 6 & 1;
    const int cert = q >> 2 & 3, nframes = (q >> 7 & 1) ? 8 : 1;
    for (int fat = 0; fat < 2; ++fat) {
      const InstanceChoice c = choose_instances(stats, textured, cert, tree, order, defer, nframes, fat != 0);
      if (c.render < 0) return false;
      if (c.exact < 0) continue;
      const ExactInstance& e = kExactInstances[c.exact];
      if (e.tex != textured || e.fb != (nframes > 1) || e.cert != (textured ? 1 : 2)) return false;
    }
  }
  return true;
}
static_assert(instance_tables_sound(), "every launch has a row of kRenderInstances, each listed once");

}  // namespace vrt

#endif  // VRT_INSTANCES_H
