// skipfield_passes_check.cpp — tests/test_skipfield_passes.py builds this program from csrc/vrt_skipfield_plan.cpp
// alone (host only) and runs it. fwd_pass_kernel and dist_pass_kernel read their input box with no bounds test, on
// the promise that the box holds every cell they scan; skipfield_passes is what keeps it. For every box of the
// argument's set the program checks each pass of the list (the conditions: at check_plan). Usage: prog N...;
// exit status 0 and a line "ok ..." per N when all holds.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <random>

#include "vrt_skipfield_plan.h"

using namespace vrt;
using K = SkipPassKind;

static long long g_failures = 0;
static int g_n, g_octants, g_dist;
static int32_t g_lo[3], g_ext[3];

static void fail(const char* what, int pass) {
  if (g_failures++ < 20)
    std::printf("FAILED %s: pass %d of n %d octants %d distances %d box (%d %d %d) + (%d %d %d)\n", what, pass, g_n,
                g_octants, g_dist, g_lo[0], g_lo[1], g_lo[2], g_ext[0], g_ext[1], g_ext[2]);
}
#define CHECK(cond, what, pass) \
  do {                          \
    if (!(cond)) fail(what, pass); \
  } while (0)

static bool same(const Region& a, const Region& b) {
  return a.x0 == b.x0 && a.y0 == b.y0 && a.z0 == b.z0 && a.ex == b.ex && a.ey == b.ey && a.ez == b.ez;
}
static void axes(const Region& r, int32_t lo[3], int32_t hi[3]) {  // cells [lo, hi] per axis
  lo[0] = r.x0, lo[1] = r.y0, lo[2] = r.z0;
  hi[0] = r.x0 + r.ex - 1, hi[1] = r.y0 + r.ey - 1, hi[2] = r.z0 + r.ez - 1;
}
// (a) extents >= 1, inside [0, n)^3, at most n^3 cells
static bool sound(const Region& r, int32_t n) {
  int32_t lo[3], hi[3];
  axes(r, lo, hi);
  for (int a = 0; a < 3; ++a)
    if (hi[a] < lo[a] || lo[a] < 0 || hi[a] > n - 1) return false;
  return int64_t(r.ex) * r.ey * r.ez <= int64_t(n) * n * n;
}
// (b), (c): `in` holds `out` on the two other axes and, along `axis`, `out` extended by `behind` cells towards 0
// and `ahead` cells towards n, clipped to the volume
static bool covers(const Region& in, const Region& out, int axis, int64_t behind, int64_t ahead, int32_t n) {
  int32_t il[3], ih[3], ol[3], oh[3];
  axes(in, il, ih);
  axes(out, ol, oh);
  for (int a = 0; a < 3; ++a) {
    int64_t lo = ol[a], hi = oh[a];
    if (a == axis) {
      lo = lo - behind < 0 ? 0 : lo - behind;
      hi = hi + ahead > n - 1 ? n - 1 : hi + ahead;
    }
    if (il[a] > lo || ih[a] < hi) return false;
  }
  return true;
}

// The conditions on the plan of one box:
//  (a) every region is sound (above);
//  (b) a forward pass's input box holds its output box on the two other axes and, along its axis, extended
//      kFwdCap - 1 cells ahead in its direction (clipped): the cells the kernel's scan can read;
//  (c) the same for a distance pass, kDistCap - 1 cells to both sides;
//  (d) a pass's input box is exactly the output box of the pass that last wrote the scratch third it reads, the
//      whole volume for a first pass (which reads the canonical volume); a third is one the layout has;
//  (e) for the whole-volume box every region is the whole volume;
//  (f) the packs' boxes are volume_edit_plan's, every packed volume once (without distances: the edit's box);
//  and the list is the launches of a rebuild, in their order: x -> y -> z nesting with a pack after each z pass,
//  both signs of each, then the edge pack exactly when the box holds coordinate 0 of an axis.
static void check_plan(int32_t n, int octants, const int32_t lo[3], const int32_t ext[3], bool distances) {
  g_n = n, g_octants = octants, g_dist = distances;
  for (int a = 0; a < 3; ++a) g_lo[a] = lo[a], g_ext[a] = ext[a];
  const SkipPlan plan = skipfield_passes(n, octants, lo, ext, distances);
  const Region whole{0, 0, 0, n, n, n}, box{lo[0], lo[1], lo[2], ext[0], ext[1], ext[2]};
  const bool upload = same(box, whole);
  const int wrap = (lo[0] == 0 ? 1 : 0) | (lo[1] == 0 ? 2 : 0) | (lo[2] == 0 ? 4 : 0);
  const int want = (octants == 8 ? (distances ? 22 : 8) : (distances ? 4 : 1)) + (wrap ? 1 : 0);
  CHECK(plan.count == want && plan.count <= kMaxSkipPasses, "pass count", -1);
  if (plan.count != want) return;
  int32_t texels[8 * 6];
  CHECK(volume_edit_plan(n, octants, lo, ext, texels) == octants, "volume_edit_plan", -1);
  const int thirds = octants == 8 ? 3 : 2;
  Region written[3];
  bool has[3] = {false, false, false};
  unsigned packed = 0;
  // the expected order: the nesting's state
  int i = 0;
  auto scan = [&](K kind, int axis, int sg, int src, int dst) {
    const SkipPass& p = plan.pass[i];
    CHECK(p.kind == kind && p.axis == axis && (kind == K::kDistPass || p.sg[axis] == sg), "order of passes", i);
    CHECK(p.first == (src < 0) && p.src == src && p.dst == dst && dst < thirds && src < thirds && src != dst, "thirds", i);
    CHECK(sound(p.in, n) && sound(p.out, n), "(a) region", i);
    if (kind == K::kFwdPass)
      CHECK(covers(p.in, p.out, axis, sg < 0 ? int64_t(kFwdCap) - 1 : 0, sg > 0 ? int64_t(kFwdCap) - 1 : 0, n),
            "(b) forward pass input", i);
    else
      CHECK(covers(p.in, p.out, axis, int64_t(kPlanDistCap) - 1, int64_t(kPlanDistCap) - 1, n), "(c) distance pass input", i);
    CHECK(src < 0 ? same(p.in, whole) : (has[src] && same(p.in, written[src])), "(d) input box", i);
    if (upload) CHECK(same(p.in, whole) && same(p.out, whole), "(e) whole volume", i);
    written[dst] = p.out;
    has[dst] = true;
    ++i;
  };
  auto pack = [&](K kind, int o, int sx, int sy, int sz, int src) {
    const SkipPass& p = plan.pass[i];
    CHECK(p.kind == kind && p.octant == o && p.src == src && p.dst == -1 && !p.first, "order of packs", i);
    if (kind == K::kFwdPack) CHECK(p.sg[0] == sx && p.sg[1] == sy && p.sg[2] == sz, "pack steps", i);
    CHECK(sound(p.in, n) && sound(p.out, n), "(a) region", i);
    if (src >= 0) {
      CHECK(has[src] && same(p.in, written[src]), "(d) pack input box", i);
      const int32_t* t = texels + o * 6;
      CHECK(same(p.out, Region{t[0], t[1], t[2], t[3] - t[0], t[4] - t[1], t[5] - t[2]}), "(f) pack box", i);
    } else {
      CHECK(same(p.in, box) && same(p.out, box), "(f) pack box of an edit that keeps the distances", i);
    }
    if (upload) CHECK(same(p.in, whole) && same(p.out, whole), "(e) whole volume", i);
    CHECK((packed >> o & 1u) == 0u, "(f) a packed volume twice", i);
    packed |= 1u << o;
    ++i;
  };
  if (octants == 8) {
    for (int sx = 1; sx >= -1; sx -= 2) {
      if (distances) scan(K::kFwdPass, 0, sx, -1, 0);
      for (int sy = 1; sy >= -1; sy -= 2) {
        if (distances) scan(K::kFwdPass, 1, sy, 0, 1);
        for (int sz = 1; sz >= -1; sz -= 2) {
          if (distances) scan(K::kFwdPass, 2, sz, 1, 2);
          pack(K::kFwdPack, (sx < 0 ? 1 : 0) | (sy < 0 ? 2 : 0) | (sz < 0 ? 4 : 0), sx, sy, sz, distances ? 2 : -1);
        }
      }
    }
  } else {
    if (distances) {
      scan(K::kDistPass, 0, 0, -1, 0);
      scan(K::kDistPass, 1, 0, 0, 1);
      scan(K::kDistPass, 2, 0, 1, 0);
    }
    pack(K::kVolumePack, 0, 0, 0, 0, distances ? 0 : -1);
  }
  CHECK(packed == (octants == 8 ? 0xFFu : 1u), "(f) every packed volume", -1);
  if (wrap) {
    const SkipPass& p = plan.pass[i];
    CHECK(p.kind == K::kEdgePack && p.wrap == wrap && same(p.in, box) && same(p.out, box), "edge pack", i);
    ++i;
  }
  CHECK(i == plan.count, "passes after the last expected one", i);
}

static long long g_boxes = 0;
static void check_box(int32_t n, int32_t x0, int32_t y0, int32_t z0, int32_t ex, int32_t ey, int32_t ez) {
  const int32_t lo[3] = {x0, y0, z0}, ext[3] = {ex, ey, ez};
  for (int octants : {8, 1})
    for (int distances = 0; distances < 2; ++distances) check_plan(n, octants, lo, ext, distances != 0);
  ++g_boxes;
}

// every box whose extents are all among `exts` (n small)
static void small_volume(int32_t n, const int32_t* exts, int count) {
  for (int a = 0; a < count; ++a)
    for (int b = 0; b < count; ++b)
      for (int c = 0; c < count; ++c)
        for (int32_t z0 = 0; z0 + exts[c] <= n; ++z0)
          for (int32_t y0 = 0; y0 + exts[b] <= n; ++y0)
            for (int32_t x0 = 0; x0 + exts[a] <= n; ++x0) check_box(n, x0, y0, z0, exts[a], exts[b], exts[c]);
}

// where the caps bind and the boxes of a plan are regional
static void large_volume(int32_t n) {
  check_box(n, 0, 0, 0, n, n, n);
  for (int c = 0; c < 8; ++c) check_box(n, c & 1 ? n - 1 : 0, c & 2 ? n - 1 : 0, c & 4 ? n - 1 : 0, 1, 1, 1);
  const int32_t m = n / 2;
  check_box(n, m, m, m, 1, 1, 1);
  for (int f = 0; f < 6; ++f) {  // a 5 x 3 x 7 box flush with face f, mid-volume on the other axes
    int32_t lo[3] = {m - 2, m - 1, m - 3};
    const int32_t ext[3] = {5, 3, 7};
    lo[f >> 1] = f & 1 ? n - ext[f >> 1] : 0;
    check_box(n, lo[0], lo[1], lo[2], ext[0], ext[1], ext[2]);
  }
  std::mt19937_64 rng(20240917u + uint64_t(n));
  for (int q = 0; q < 2000; ++q) {  // extents small, up to a cap's reach, or anything that fits, by turns
    int32_t lo[3], ext[3];
    for (int a = 0; a < 3; ++a) {
      lo[a] = int32_t(rng() % uint64_t(n));
      const int32_t room = n - lo[a], kind = int32_t(rng() % 3u);
      const int32_t most = kind == 0 ? 4 : (kind == 1 ? int32_t(kFwdCap) + 2 : room);
      ext[a] = 1 + int32_t(rng() % uint64_t(most < room ? most : room));
    }
    check_box(n, lo[0], lo[1], lo[2], ext[0], ext[1], ext[2]);
  }
}

int main(int argc, char** argv) {
  for (int q = 1; q < argc; ++q) {
    const int32_t n = std::atoi(argv[q]);
    g_boxes = 0;
    const long long before = g_failures;
    if (n <= 4) {
      int32_t exts[4];
      for (int32_t e = 1; e <= n; ++e) exts[e - 1] = e;
      small_volume(n, exts, n);
    } else if (n <= 16) {
      const int32_t exts[3] = {1, 2, n};
      small_volume(n, exts, 3);
    } else {
      large_volume(n);
    }
    std::printf("%s n %d boxes %lld\n", g_failures == before ? "ok" : "FAILED", n, g_boxes);
  }
  return g_failures == 0 && argc > 1 ? 0 : 1;
}
