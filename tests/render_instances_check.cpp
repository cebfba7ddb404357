// render_instances_check.cpp — tests/test_render_instances.py builds and runs this program (host only; it includes
// nothing of the library but csrc/vrt_instances.h). Over every launch launch_render can be given it compares
// choose_instances with the two ternary cascades launch_render held before the instance table, restated below as
// they were written: each `render_kernel<...>` literal became `rk(...)` with the kernel's default template
// arguments, each exact-pass literal `ek(...)` / `ekc(...)`. Exit status 0 and a line "ok ..." when all holds.
#include <cstdint>
#include <cstdio>
#include <set>
#include <tuple>

#include "vrt_instances.h"

using namespace vrt;

// render_kernel<STATS, TEX, CERT = 0, ORD = false, DEFER = false, FB = false, TREE = false>
static RenderInstance rk(bool stats, bool tex, int cert = 0, bool ord = false, bool defer = false, bool fb = false,
                         bool tree = false) {
  return RenderInstance{stats, tex, cert, ord, defer, fb, tree};
}
// exact_pass_kernel<TEX, CERT, WAVES = kExactWaves, SB = kSparseBatch, FB = false>
static ExactInstance ek(bool tex, int cert, int waves = kExactWaves, uint32_t sb = kSparseBatch, bool fb = false) {
  return ExactInstance{tex, cert, waves, sb, fb, false};
}
// exact_pass_kernel_capped<CERT, SB, FB> (a row's `waves` is not read there: the table's rows carry kExactWaves)
static ExactInstance ekc(int cert, uint32_t sb, bool fb) { return ExactInstance{false, cert, kExactWaves, sb, fb, true}; }
// exact_pass_whole_frame<CAP>(fb)
static ExactInstance exact_pass_whole_frame(bool fb) {
  if (kExactVgprs == 0) return fb ? ek(false, 2, kExactWaves, kSparseBatch, true) : ek(false, 2);
  return fb ? ekc(2, kSparseBatch, true) : ekc(2, kSparseBatch, false);
}

struct Launch {  // what launch_render read: stats and the fields of its KArgs
  bool stats;
  int textured, cert, tree;
  bool order, defer;
  int nframes, exact_fat;
};

// the cascades: `pair` is set where launch_render launched the certified pass and then the exact pass k2
static RenderInstance parent_choice(bool stats, const Launch& a, bool& pair, ExactInstance& k2) {
  pair = false;
  if (a.defer && !stats && a.cert == 2) {
    pair = true;
    const bool fb = a.nframes > 1;
    auto k1 = a.textured ? (fb ? rk(false, true, 2, false, true, true) : rk(false, true, 2, false, true))
              : a.tree   ? (fb ? rk(false, false, 2, false, true, true, true)
                               : rk(false, false, 2, false, true, false, true))
                         : (fb ? rk(false, false, 2, false, true, true) : rk(false, false, 2, false, true));
    k2 = a.textured ? (fb ? ek(true, 1, kExactWaves, kSparseBatchTex, true)
                          : ek(true, 1, kExactWaves, kSparseBatchTex))
         : a.exact_fat ? (fb ? ek(false, 2, kFatWaves, kSparseBatchFat, true)
                             : ek(false, 2, kFatWaves, kSparseBatchFat))
                       : exact_pass_whole_frame(fb);
    return k1;
  }
  auto kern = a.textured ? (stats ? rk(true, true)
                            : a.nframes > 1 ? (a.cert >= 1 ? rk(false, true, 1, false, false, true)
                                                           : rk(false, true, 0, false, false, true))
                                            : (a.cert >= 1 ? rk(false, true, 1) : rk(false, true)))
                         : (stats ? rk(true, false)
                            : a.nframes > 1
                                ? (a.cert == 2 ? (a.order ? rk(false, false, 2, true, false, true)
                                                          : rk(false, false, 2, false, false, true))
                                   : a.cert == 1 ? rk(false, false, 1, false, false, true)
                                                 : rk(false, false, 0, false, false, true))
                                : (a.cert == 2 ? (a.tree ? (a.order ? rk(false, false, 2, true, false, false, true)
                                                                    : rk(false, false, 2, false, false, false, true))
                                                 : a.order ? rk(false, false, 2, true)
                                                           : rk(false, false, 2))
                                   : a.cert == 1 ? rk(false, false, 1)
                                                 : rk(false, false, 0)));
  return kern;
}

int main() {
  std::set<int> render_rows, exact_rows;
  int inputs = 0, bad = 0;
  const int frames[3] = {1, 2, 8};
  for (int stats = 0; stats < 2; ++stats)
    for (int textured = 0; textured < 2; ++textured)
      for (int cert = 0; cert < 3; ++cert)
        for (int tree = 0; tree < 2; ++tree)
          for (int order = 0; order < 2; ++order)
            for (int defer = 0; defer < 2; ++defer)
              for (int nf : frames)
                for (int fat = 0; fat < 2; ++fat) {
                  ++inputs;
                  const Launch a{stats != 0, textured, cert, tree, order != 0, defer != 0, nf, fat};
                  bool pair;
                  ExactInstance k2{};
                  const RenderInstance k1 = parent_choice(a.stats, a, pair, k2);
                  const InstanceChoice c = choose_instances(a.stats, a.textured != 0, a.cert, a.tree != 0, a.order,
                                                            a.defer, a.nframes, a.exact_fat != 0);
                  // (c) total: a row of each table, an exact row exactly for the pairs
                  bool ok = c.render >= 0 && c.render < kRenderInstanceCount && (c.exact >= 0) == pair &&
                            c.exact < kExactInstanceCount;
                  // (a) the rows are the cascades' kernels
                  ok = ok && kRenderInstances[c.render] == k1 && (!pair || kExactInstances[c.exact] == k2);
                  if (!ok) {
                    ++bad;
                    std::printf("MISMATCH stats %d textured %d cert %d tree %d order %d defer %d nframes %d fat %d: rows %d %d\n",
                                stats, textured, cert, tree, order, defer, nf, fat, c.render, c.exact);
                    continue;
                  }
                  render_rows.insert(c.render);
                  if (pair) exact_rows.insert(c.exact);
                }
  // (b) 22 + 6 distinct rows, every one of them reached
  std::set<std::tuple<bool, bool, int, bool, bool, bool, bool>> rset;
  for (const RenderInstance& r : kRenderInstances) rset.insert({r.stats, r.tex, r.cert, r.ord, r.defer, r.fb, r.tree});
  std::set<std::tuple<bool, int, int, uint32_t, bool, bool>> eset;
  for (const ExactInstance& e : kExactInstances) eset.insert({e.tex, e.cert, e.waves, e.sparse_batch, e.fb, e.capped});
  int capped = 0;
  for (const ExactInstance& e : kExactInstances) capped += e.capped ? 1 : 0;
  std::printf("inputs %d mismatches %d render rows %d distinct %zu reached %zu exact rows %d distinct %zu reached %zu capped %d\n",
              inputs, bad, kRenderInstanceCount, rset.size(), render_rows.size(), kExactInstanceCount, eset.size(),
              exact_rows.size(), capped);
  const bool ok = inputs == 576 && bad == 0 && kRenderInstanceCount == 22 && rset.size() == 22 &&
                  render_rows.size() == 22 && kExactInstanceCount == 6 && eset.size() == 6 && exact_rows.size() == 6 &&
                  capped == (kExactVgprs != 0 ? 2 : 0);
  std::printf(ok ? "ok\n" : "FAILED\n");
  return ok ? 0 : 1;
}
