// vrt_render.hip — gfx950 HIP kernels for the per-pixel program of res/shaders/voxel.glsl; the
// C-ABI context around them is vrt_context.h and its vrt_*.cpp files (include/vrt.h). One translation unit: this
// file holds the pixel epilogue, the tile order, the primary ray, the bounce-stack exact_pixel, the two
// frame kernels and the host launch wrappers (their instance choice is vrt_instances.h, the boxes of the
// skip-field passes vrt_skipfield_plan.cpp: host arithmetic); the rest is in the headers included below, in
// dependency order (vrt_tuning.h through vrt_internal.h), and in vrt_query_kernels.h,
// vrt_trace_kernels.h, vrt_ids_kernels.h and vrt_reproject_kernels.h (the ray-query, shaded ray-query,
// ID-pass and reprojected-filter kernels, included after the primary ray and exact_pixel they call),
// and in vrt_spatial_kernels.h (the ID-guided spatial filter, which calls none of them).
//
// One work-item per pixel; a 128-thread workgroup covers a 16x8 pixel tile and each wave64 an
// 8x8 sub-tile, so the 64 rays of a wave start coherent. Every float operation of the DDA is
// replayed in the reference's order with -ffp-contract=off and correctly rounded div/sqrt, which
// makes hit records bit-exact against the CPU oracle (DESIGN.md "Numerics").
//
// Device volume layout: (N+1)^3 bytes, x fastest, where plane N repeats plane 0 on each axis.
// GetVoxel's texel for a coordinate c in [0, N] is then simply floor(c) (GL_REPEAT folded into
// the layout), and the hot loop addresses it with two 24-bit multiply-adds.
#include <hip/hip_ext.h>
#include <hip/hip_runtime.h>

#include <algorithm>
#include <array>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>
#include <type_traits>
#include <utility>
#include <vector>

#include "vrt.h"
#include "vrt_internal.h"
#include "vrt_instances.h"
#include "vrt_diag.h"
#include "vrt_math.h"
#include "vrt_walk.h"
#include "vrt_cert.h"
#include "vrt_aux_kernels.h"
#include "vrt_skipfield_kernels.h"

namespace vrt {

// ---- RGB8 framebuffer store + temporal filter (oracle/vrt_oracle.c oracle_temporal) ----------
// GL float -> UNORM8 store into the RGB8 FBO attachments (FrameBuffer.cpp:8): clamp to [0,1]
// (NaN -> 0), scale by 255, round half to even (pinned in DESIGN.md); a texel reads back b / 255.
__device__ __forceinline__ uint32_t unorm8(float f) {
  const float c = __builtin_fminf(__builtin_fmaxf(f, 0.0f), 1.0f);
  return uint32_t(__builtin_rintf(c * 255.0f));
}
// b / 255 rounded correctly, as q0 = b * RN(1/255) plus one fma correction: equal to the IEEE
// division for every byte (exhaustive check, tests/test_div255.py)
__device__ __forceinline__ float unorm8_read(uint32_t b) {
  const float a = float(b), y = 1.0f / 255.0f;
  const float q0 = a * y;
  return __builtin_fmaf(__builtin_fmaf(-255.0f, q0, a), y, q0);
}
__device__ __forceinline__ uint32_t pack_rgb8(float r, float g, float b) {
  return unorm8(r) | (unorm8(g) << 8) | (unorm8(b) << 16) | 0xFF000000u;
}
// temporal.glsl:18  color = u_Alpha * newColor + (1 - u_Alpha) * averageColor, on RGB8 texels
__device__ __forceinline__ uint32_t temporal_blend(uint32_t nw, uint32_t old, float alpha) {
  const float om = 1.0f - alpha;
  uint32_t r = 0xFF000000u;
#pragma unroll
  for (int ch = 0; ch < 3; ++ch) {
    const float v = alpha * unorm8_read((nw >> (8 * ch)) & 0xFFu) + om * unorm8_read((old >> (8 * ch)) & 0xFFu);
    r |= unorm8(v) << (8 * ch);
  }
  return r;
}

// Lane id as a fresh (volatile) value each call, so the compiler cannot keep one copy alive
// across the whole trace.
__device__ __forceinline__ uint32_t lane_id() {
  uint32_t l;
  asm volatile("v_mbcnt_lo_u32_b32 %0, -1, 0\n\tv_mbcnt_hi_u32_b32 %0, -1, %0" : "=v"(l));
  return l;
}
// kWgWaves waves per workgroup (vrt_tuning.h), each rendering an 8x8 pixel tile: a workgroup
// covers kTileW x kTileH pixels (wave = threadIdx.x >> 6, uniform). Tiles are dispatched in row
// order (an XCD-aware order that
// keeps runs of tiles on one XCD's L2 was neutral or worse, profiles/r01_v29_ab_xcd_tile_swizzle_negative.log).

// Heavy tiles first (vrt_set_tile_order). A frame ends with its longest waves, those with exact-path
// pixels (glass bounce stacks, walks the certified walk could not settle); dispatched in row
// order, they start wherever they are in the image. Each stats-free launch therefore records which
// of its tiles had such a pixel (until r02: only bounce stacks; C3 -2 %, profiles/r02_s09), and the
// next launch of the same band (same stream) dispatches those first.
// Workgroups are dealt to the 8 XCDs round-robin (workgroup L on XCD L % 8), and a tile keeps its
// XCD — its L2 — from launch to launch only if it keeps its slot's residue mod 8: every
// permutation that ignored this was 9-60 % slower at C3 (profiles/r02_s12_tileperm, r02_s14).
// So heavy tiles are listed per class r = tile % 8: as a heavy tile finishes, its last wave
// appends it to its class's list (kOrdClasses counters, one 256-byte line each) and stores its
// rank (list position + 1; 0 for the other tiles). The next launch's grid is 8*ord_q + tiles
// workgroups: slot L < 8*ord_q renders entry n - 1 - L / 8 of class L % 8's list (n = its length,
// at most ord_q) if L / 8 < n, else exits — the class's heavy tiles in reverse completion order,
// those that finished last first (C3 -4 % against completion order and against the flag passes,
// profiles/r02_s14); slot 8*ord_q + t renders tile t unless its rank is in [1, ord_q] (rendered by
// the first pass). The list and the ranks of a launch are written together, so every tile is rendered
// exactly once (a fresh zeroed buffer: no heavy tiles). Until r02 s14 the first pass was `tiles`
// workgroups testing per-tile flags (same slot residues), most of them empty.
__device__ __forceinline__ uint32_t* ord_ctr(const KArgs& a, uint32_t set, uint32_t r) {
  return a.order + (set * kOrdClasses + r) * kOrdCtrStride;
}
__device__ __forceinline__ uint32_t* ord_rank(const KArgs& a, uint32_t set) {
  return a.order + kOrdHdr + (1u + set) * a.tiles;
}
__device__ __forceinline__ uint32_t* ord_list(const KArgs& a, uint32_t set) {  // entry j of class r: [j*8 + r]
  return a.order + kOrdHdr + 3u * a.tiles + set * (a.tiles + kOrdClasses);
}
// The tile workgroup L renders, or ~0u (nothing to do)
__device__ __forceinline__ uint32_t ordered_tile(const KArgs& a, uint32_t L) {
  const uint32_t cap = kOrdClasses * a.ord_q;
  if (L < cap) {
    const uint32_t r = L % kOrdClasses, j = L / kOrdClasses;
    if (j == 0u && threadIdx.x == 0u) *ord_ctr(a, a.ctr_z, r) = 0u;  // for the launch after the next
    const uint32_t n = min(*ord_ctr(a, a.ctr_r, r), a.ord_q);
    return j < n ? ord_list(a, a.ord_r)[(n - 1u - j) * kOrdClasses + r] : ~0u;  // last finished first
  }
  const uint32_t t = L - cap;
  return ord_rank(a, a.ord_r)[t] - 1u < a.ord_q ? ~0u : t;  // rank 0 wraps to ~0u: not listed
}
// after the trace: the tile's last wave files it for the next launch
// (counter: bits 0-7 waves done, 8-15 heavy waves)
__device__ __forceinline__ void order_record(const KArgs& a, uint32_t tile, bool heavy_wave) {
  uint32_t* cnt = a.order + kOrdHdr + tile;
  const uint32_t add = 1u | (heavy_wave ? 0x100u : 0u);
  const uint32_t old = atomicAdd(cnt, add);
  if ((old & 0xFFu) != uint32_t(kWgWaves) - 1u) return;
  *cnt = 0u;
  uint32_t rank = 0u;
  if (((old + add) & 0xFF00u) != 0u) {
    const uint32_t r = tile % kOrdClasses;
    const uint32_t k = atomicAdd(ord_ctr(a, a.ctr_w, r), 1u);  // <= tiles / 8: one per tile of class r
    ord_list(a, a.ord_w)[k * kOrdClasses + r] = tile;
    rank = k + 1u;
  }
  ord_rank(a, a.ord_w)[tile] = rank;
}

__device__ __forceinline__ int pixel_x(uint32_t tx, int wave, uint32_t lane) {
  return int(tx) * kTileW + (wave & 1) * 8 + int(lane & 7u);
}
__device__ __forceinline__ int pixel_row(uint32_t ty, int wave, uint32_t lane) {
  return int(ty) * kTileH + (wave >> 1) * 8 + int(lane >> 3);
}
// frame row of band row li: blocks of 2^row_blk_sh adjacent rows, row_step rows apart (ABI v11);
// row_blk_sh = 0 is the cyclic-row band row0 + li * row_step
__device__ __forceinline__ int frame_row(const KArgs& a, int li) {
  return a.row0 + (li >> a.row_blk_sh) * a.row_step + (li & ((1 << a.row_blk_sh) - 1));
}

// Counters (STATS launches): one 64-bit add per wave and counter into replica
// (block % kCntReplicas); a single array would serialise ~300K same-address atomics per 1080p
// frame at the memory side.

// The per-frame fields of frame f of a launch (frame batches, KArgs::nframes): its camera, time
// and outputs (the history is read only at alpha != 1, where launches hold one frame)
struct FrameView {
  const float* pv;
  float time;
  uint32_t* cur;
  uint32_t* raw;
};
__device__ __forceinline__ FrameView frame_view(const KArgs& a, uint32_t f) {
  if (f == 0u) return FrameView{a.inv_pv, a.time, a.cur, a.raw};
  const KArgs::FrameB& b = a.fb[f - 1u];
  return FrameView{b.inv_pv, b.time, b.cur, b.raw};
}

// Per-launch constants of the walk context. LATE (the certified pass): without the sun, the sky
// factor and the atlas, which cert_pixel reads after the primary walk (late_ctx, vrt_cert.h)
template <bool LATE = false>
__device__ __forceinline__ void init_ctx(Ctx& c, const KArgs& a, const uint16_t* __restrict__ vox) {
  c.vox = vox;
  c.ostride = a.ostride;
  c.n = a.n;
  c.p = uint32_t(a.n) + 1u;
  c.fn = a.fn;
  c.max_len = a.max_len;
  c.time = a.time;
  c.refl_noise = a.refl_noise;
  c.refr_noise = a.refr_noise;
  if constexpr (LATE) {
    c.sky_sy = 0.0f;
    c.sun_n = c.sun_rcp = mk(0.0f, 0.0f, 0.0f);
    c.atlas = nullptr;
    c.atlas_mask = 0u;
    c.atlas_fs = c.atlas_fts = 0.0f;
  } else {
    c.sky_sy = a.sky_sy;
    c.sun_n = mk(a.sun_n[0], a.sun_n[1], a.sun_n[2]);
    c.sun_rcp = mk(a.sun_rcp[0], a.sun_rcp[1], a.sun_rcp[2]);
    c.atlas = a.atlas;
    c.atlas_mask = uint32_t(a.atlas_size) - 1u;
    c.atlas_fs = float(a.atlas_size);
    c.atlas_fts = float(a.atlas_tex_size);
  }
  CTRACE_ONLY(c.tr = false;)
}

// The primary ray of pixel (px, frame row py): vertex stage (voxel.glsl:467-472) evaluated at the
// pixel centre, then stack[0] of main (:430)
// a / d correctly rounded for the vertex stage's divisions: Markstein's division (div_rn) from
// y = RN(1/d) when every operand is far from overflow and underflow (|a|, |d| in [2^-60, 2^60]),
// else the IEEE division; bit-identical either way. Zero numerators take the IEEE division: div_rn
// returns +0 for a = -0 (the residual's zeros cancel to +0), IEEE -0 / d keeps the sign, and a
// -0 component of the direction decides RandomizeDirection's hashes.
__device__ __forceinline__ bool markstein_safe(float x) {
  const float m = __builtin_fabsf(x);
  return m >= 0x1p-60f && m <= 0x1p60f;
}
__device__ __forceinline__ f3 div3_rn(float x, float y, float z, float d) {
  if (markstein_safe(x) && markstein_safe(y) && markstein_safe(z) && markstein_safe(d)) {
    const float r = rcp_newton(d);  // |d| in [2^-60, 2^60]: RN(1/d)
    return mk(div_rn(x, d, r), div_rn(y, d, r), div_rn(z, d, r));
  }
  return mk(x / d, y / d, z / d);
}
// The certified pass's form (LEAN) of the same test, in two parts: `rest`, what the host may have proved
// for every pixel of the launch (|x|, |y|, |z| <= 2^60 and |d| in [2^-60, 2^60]: KArgs::vdiv_ok, or the
// lane's own tests behind a wave-uniform branch; they also reject NaN numerators, which the minimum
// drops), and the numerators' lower bound, the smallest |numerator| against 2^-60, which is left to the
// lane. r: RN(1 / d) where d is Markstein-safe (rcp_newton(d), or the host's IEEE division of a
// launch-constant d, KArgs::rcp_wn / rcp_wf: the same float). Each lane takes the same sequence either way.
__device__ __forceinline__ f3 div3_lean(float x, float y, float z, float d, float r, bool rest) {
  const bool safe = rest & (__builtin_fminf(__builtin_fminf(__builtin_fabsf(x), __builtin_fabsf(y)), __builtin_fabsf(z)) >=
                            0x1p-60f);
  if (safe) return mk(div_rn(x, d, r), div_rn(y, d, r), div_rn(z, d, r));
  return mk(x / d, y / d, z / d);
}
__device__ __forceinline__ bool div3_lean_ranges(float x, float y, float z, float d) {
  return int(__builtin_fabsf(x) <= 0x1p60f) & int(__builtin_fabsf(y) <= 0x1p60f) & int(__builtin_fabsf(z) <= 0x1p60f) &
         int(markstein_safe(d));
}

// LEAN (the certified pass's instances): the quantities that are the same for every pixel of the launch come
// from the host (KArgs::fw .. max_len2, and behind the wave-uniform flags of KArgs::setup, each a host proof
// per launch, cert_launch_consts in vrt_launch_consts.cpp):
//  - kSetupW: the w column is not formed: n4.w and f4.w are the launch's wn and wf bit for bit (the x and y
//    terms are absorbed by the z term's rounding), their reciprocals the host's, and the tests of d proved;
//  - kSetupLen: the squared length of vdir is inside normalize3's general range and away from its near-one
//    window for every pixel: rcp_newton(sqrt_fix(s)) without the three range tests.
// The same floats either way.
template <bool LEAN = false>
__device__ __forceinline__ Ray primary_ray(const KArgs& a, const float* __restrict__ inv_pv, const Ctx& c, int px,
                                           int py) {
  // (2 (p + 0.5)) / W with RN(1/W) from the host: the numerator is in (0, 2W), W <= 32768
  const float ndx = div_rn(2.0f * (float(px) + 0.5f), LEAN ? a.fw : float(a.width), a.rcp_w) - 1.0f;
  const float ndy = div_rn(2.0f * (float(py) + 0.5f), LEAN ? a.fh : float(a.height), a.rcp_h) - 1.0f;
  float n4[4], f4[4];
#pragma unroll
  for (int i = 0; i < (LEAN ? 3 : 4); ++i) {
    const float base = inv_pv[0 * 4 + i] * ndx + inv_pv[1 * 4 + i] * ndy;
    n4[i] = (base + inv_pv[2 * 4 + i] * -1.0f) + inv_pv[3 * 4 + i] * 1.0f;
    f4[i] = (base + inv_pv[2 * 4 + i] * 1.0f) + inv_pv[3 * 4 + i] * 1.0f;
  }
  f3 vnear, vdir;
  if constexpr (LEAN) {
    float rn, rf;
    bool rest_n = true, rest_f = true;
    if ((a.setup & kSetupW) != 0u) {  // (implies vdiv_ok)
      n4[3] = a.wn;
      f4[3] = a.wf;
      rn = a.rcp_wn;
      rf = a.rcp_wf;
    } else {
      const float base = inv_pv[0 * 4 + 3] * ndx + inv_pv[1 * 4 + 3] * ndy;
      n4[3] = (base + inv_pv[2 * 4 + 3] * -1.0f) + inv_pv[3 * 4 + 3] * 1.0f;
      f4[3] = (base + inv_pv[2 * 4 + 3] * 1.0f) + inv_pv[3 * 4 + 3] * 1.0f;
      if (a.vdiv_ok == 0u) {
        rest_n = div3_lean_ranges(n4[0], n4[1], n4[2], n4[3]);
        rest_f = div3_lean_ranges(f4[0], f4[1], f4[2], f4[3]);
      }
      rn = rcp_newton(n4[3]);  // RN(1 / d) where d is in range; not used elsewhere
      rf = rcp_newton(f4[3]);
    }
    vnear = div3_lean(n4[0], n4[1], n4[2], n4[3], rn, rest_n);
    vdir = div3_lean(f4[0], f4[1], f4[2], f4[3], rf, rest_f) - vnear;
  } else {
    vnear = div3_rn(n4[0], n4[1], n4[2], n4[3]);
    vdir = div3_rn(f4[0], f4[1], f4[2], f4[3]) - vnear;
  }
  Ray ray;
  const float half_n = LEAN ? a.half_n : c.fn * 0.5f;
  ray.pos = mk(vnear.x + half_n, vnear.y + half_n, vnear.z + half_n);
  f3 dir0;
  if constexpr (LEAN) {
    const float s = vdir.x * vdir.x + vdir.y * vdir.y + vdir.z * vdir.z;
    float inv;
    if ((a.setup & kSetupLen) != 0u)
      inv = rcp_newton(sqrt_fix(s));
    else
      inv = normalize3_scale(s);
    dir0 = vdir * inv;
  } else {
    dir0 = normalize3(vdir);
  }
  ray.dir = randomize<LEAN>(dir0, vnear, a.ray_noise, c.time);
  ray.len = 0.0f;
  ray.energy = 1.0f;
  ray.voxel = 0;
  ray.rdepth = 0;
  ray.tdepth = 0;
  return ray;
}

// Bounce stacks run at raised wave priority (s_setprio): they are a frame's longest waves
// (-2 % at C3, profiles/r01_v45_ab_wave_priority.log).
constexpr int kStackPrio = 3;

// A scratch-stack entry: only reflection rays are stored (exact_pixel), whose medium is air
// (reflection_ray sets voxel 0), with both depths (<= 16) in one word: 9 dwords instead of 11.
struct StackRay {
  f3 pos, dir;
  float len, energy;
  uint32_t depths;
};
__device__ __forceinline__ StackRay pack_stack_ray(const Ray& r) {
  return StackRay{r.pos, r.dir, r.len, r.energy, uint32_t(r.rdepth) | (uint32_t(r.tdepth) << 16)};
}
// The bounce stack's bottom entry of each lane in LDS, component-major (dword j of lane t at
// [j * NL + t]: conflict-free ds_write_b32 / ds_read_b32), the rest in scratch. A pixel whose
// tree holds at most one entry at a time (every C1 pixel: a reflection ray under the first
// refraction ray) then never touches scratch for it.
constexpr int kStackWords = 9;
template <int NL>
__device__ __forceinline__ void lds_stack_put(float* __restrict__ b, const StackRay& e) {
  b[0 * NL] = e.pos.x;
  b[1 * NL] = e.pos.y;
  b[2 * NL] = e.pos.z;
  b[3 * NL] = e.dir.x;
  b[4 * NL] = e.dir.y;
  b[5 * NL] = e.dir.z;
  b[6 * NL] = e.len;
  b[7 * NL] = e.energy;
  b[8 * NL] = __uint_as_float(e.depths);
}
template <int NL>
__device__ __forceinline__ StackRay lds_stack_get(const float* __restrict__ b) {
  return StackRay{mk(b[0 * NL], b[1 * NL], b[2 * NL]), mk(b[3 * NL], b[4 * NL], b[5 * NL]), b[6 * NL],
                  b[7 * NL], __float_as_uint(b[8 * NL])};
}
__device__ __forceinline__ Ray unpack_stack_ray(const StackRay& e) {
  Ray r;
  r.pos = e.pos;
  r.dir = e.dir;
  r.len = e.len;
  r.energy = e.energy;
  r.voxel = 0;
  r.rdepth = int32_t(e.depths & 0xffffu);
  r.tdepth = int32_t(e.depths >> 16);
  return r;
}

// fragment main (voxel.glsl:425-452) with exact walks. The primary ray (stack[0] of the
// reference) stays in registers; the scratch stack only ever holds secondary rays, so pixels that
// spawn none never touch it. CSH: shadow bits by certified walks from the exact hit points where
// they settle (cert_shadow_exact); CSEC: air-medium secondary rays by certified walks first
// (cert_secondary; on glass-heavy frames their glass hits pay both walks, C1 +19 %: off there).
// Returns whether the pixel ran a bounce stack.
// NL: lanes per workgroup of the LDS stack bottom `lstk` (this lane's word 0).
// LATE (the exact pass's colour instances): c comes without the sun, the sky factor and the atlas
// (init_ctx<true>). The primary hit's shading and each iteration of the bounce loop read them, and
// the loop the two depth limits, through the opaque view of the kernel's arguments (late_ctx,
// late_kargs: vrt_cert.h), so that none of them is live across the primary walk or from one
// iteration to the next: as SGPRs they were spilled into VGPR lanes the walks then lacked.
template <bool STATS, bool TEX, bool CSH = false, bool CSEC = false, int NL = kWgThreads, bool LATE = false>
__device__ __forceinline__ bool exact_pixel(const KArgs& a, const Ctx& c, Ray ray, f3& color,
                                            Counters& k, uint32_t& steps, uint32_t& flags,
                                            int32_t& hit_vidx, float& hit_len, float* __restrict__ lstk,
                                            float s_init = -1.0f) {
  static_assert(!LATE || !TEX, "a textured walk reads the atlas");
  StackRay stack[kMaxStack - 2];  // the top entry lives in `ray`, the bottom one in LDS
  const int cap0 = LATE ? 0 : a.max_refl + a.max_transp + 1;
  int sp = 0;
  Hit h0;
  if constexpr (LATE) {
    h0 = march<STATS, TEX, true>(c, ray, k, steps, flags, s_init);
    Ctx lc = c;
    late_ctx(lc);
    shade<STATS, TEX, CSH>(lc, ray, h0, color, k, steps, flags);
  } else {
    h0 = trace_with_shadow<STATS, TEX, true, CSH>(c, ray, color, k, steps, flags, s_init);
  }
  STAMP_PIXEL_BEGIN();
  hit_vidx = h0.found ? h0.vidx : -1;
  hit_len = h0.found ? h0.len : 0.0f;
  if (h0.found && mat_id(h0.voxel) == 2) {  // only glass spawns secondary rays (:440-448)
    __builtin_amdgcn_s_setprio(kStackPrio);  // bounce stacks: the longest waves of a frame
    Hit h = h0;
    for (;;) {
      // The sun vector and its reciprocal are opaque per iteration (an empty asm on SGPR copies, or
      // LATE's reads), so the compiler cannot hoist the per-lane products the loop body forms from
      // them into VGPRs live across the whole loop: those were spilled per lane on loop entry. Scratch
      // 832 -> 720 B per lane, WRITE_SIZE per C3 frame 17.2 -> 14.6 MB (DESIGN.md §6 "HBM writes").
      Ctx lc = c;
      int max_refl, max_transp, cap;
      if constexpr (LATE) {
        late_ctx(lc);
        LateKArgs* ka = late_kargs();
        max_refl = ka->max_refl;
        max_transp = ka->max_transp;
        cap = max_refl + max_transp + 1;
      } else {
        asm volatile("" : "+s"(lc.sun_n.x), "+s"(lc.sun_n.y), "+s"(lc.sun_n.z), "+s"(lc.sun_rcp.x),
                     "+s"(lc.sun_rcp.y), "+s"(lc.sun_rcp.z));
        max_refl = a.max_refl;
        max_transp = a.max_transp;
        cap = cap0;
      }
      // The reference pushes the reflection ray, then the refraction ray, then pops the top
      // (:440-448). The ray pushed last is popped at once, so it goes straight to `ray` and only a
      // reflection ray under a refraction ray is written to the scratch stack: same rays in the
      // same order, same STACK_FULL cases (the cap counts the ray held in `ray` as an entry), and
      // about half the scratch writes of a glass tree.
      bool push_r = false, push_t = false;
      if (h.found) {
        const uint32_t m = mat_id(h.voxel);
        const bool pr = mat_reflective(m) && ray.rdepth < max_refl;
        const bool pt = mat_transparent(m) && ray.tdepth < max_transp && get_color<TEX>(lc, h).w != 1.0f;
        push_r = pr && sp < cap;
        push_t = pt && sp + int(push_r) < cap;
        if ((pr && !push_r) || (pt && !push_t)) flags |= VRT_HIT_FLAG_STACK_FULL;
      }
      if (push_r && push_t) {
        const StackRay e = pack_stack_ray(reflection_ray(lc, ray, h));
        if (sp == 0)
          lds_stack_put<NL>(lstk, e);
        else
          stack[sp - 1] = e;
        ++sp;
        ray = refraction_ray<TEX>(lc, ray, h, k);
      } else if (push_r) {
        ray = reflection_ray(lc, ray, h);
      } else if (push_t) {
        ray = refraction_ray<TEX>(lc, ray, h, k);
      } else {
        if (sp == 0) break;
        --sp;
        ray = unpack_stack_ray(sp == 0 ? lds_stack_get<NL>(lstk) : stack[sp - 1]);
      }
      k.c[VRT_CNT_SECONDARY_RAYS]++;
      if constexpr (CSH && CSEC) {
        bool settled;
        h = march_cert(lc, ray, color, settled, k, steps, flags);
        if (settled) {
          h.found = false;  // a miss or a hit without secondary rays
          continue;
        }
        shade<STATS, TEX, CSH>(lc, ray, h, color, k, steps, flags);
        continue;
      }
      h = trace_with_shadow<STATS, TEX, false, CSH>(lc, ray, color, k, steps, flags);
    }
    STAMP_PIXEL_END();
    return true;
  }
  return false;
}

// output of one pixel: float RGBA, or the fused reference post-pass (RGB8 ray-trace store,
// temporal blend, RGB8 store)
template <class KA>  // KArgs, or the certified pass's late view of them (LateKArgs)
__device__ __forceinline__ void store_pixel(const KA& a, const FrameView& fv, float4* __restrict__ out,
                                            size_t o, const f3 color) {
  if (fv.cur) {
    const uint32_t rw = pack_rgb8(color.x, color.y, color.z);
    if (fv.raw) fv.raw[o] = rw;
    // u_Alpha = 1 (the slider default): 1 * b/255 + 0 * old stores b back for every byte b and any
    // history (exhaustive, tests/test_temporal_oracle.py), so the history is not read
    fv.cur[o] = a.alpha == 1.0f ? rw : temporal_blend(rw, a.prev[o], a.alpha);
  } else {
    out[o] = make_float4(color.x, color.y, color.z, 1.0f);
  }
}

// One work-item per pixel, 8x8 pixels per wave: the exact path (every launch with hit records or
// counters, textured frames, and colour-only frames when the certified pair below cannot run).
// STATS: this instance writes hit records and/or counters. Without it the per-lane counters,
// step/flag/tie tracking are dead code (~20 VGPRs and a VALU per DDA step freed); the rendering
// arithmetic is the same source in both instances. TEX: textured mode (!_COLOR_ONLY).
// CERT (stats-free colour-only instances): 0 exact walks only, 1 certified walks for the exact
// path's shadow and air-medium secondary rays, 2 also whole pixels first.
// DEFER (certified instances): pixels that need the exact path are not rendered here; their lane
// mask per wave goes to a.defer and exact_pass_kernel renders them compacted (see there).
// (resident waves per SIMD of the instances: kMinWaves, kDeferWaves, kTreeWaves in vrt_tuning.h)
// FB: the frame-batch instance (KArgs::nframes > 1: per-frame camera, time and outputs, the frame
// in a deferred entry's top bits); launches of one frame keep the instance without that decode
// (it cost C1 4 %, C3 1 %: profiles/r05_s27)
// TREE (colour-only CERT 2): glass pixels' bounce trees by certified walks (cert_tree), one
// kTreeWords LDS slot per lane.
template <bool STATS, bool TEX, int CERT = 0, bool ORD = false, bool DEFER = false, bool FB = false,
          bool TREE = false>
__global__ void __launch_bounds__(kWgThreads, TREE ? kTreeWaves : (DEFER ? kDeferWaves : kMinWaves)) render_kernel(KArgs a, const uint16_t* __restrict__ vox,
                                                     float4* __restrict__ out,
                                                     vrt_hit* __restrict__ hits,
                                                     unsigned long long* __restrict__ counters) {
  // The pixel is re-derived after the trace from wave-uniform SGPRs and a fresh lane id instead
  // of being kept alive across it: at 80 VGPRs the long-lived copies were spilled to scratch by
  // every wave (~1.8 KB/wave of scratch writes, most of the excess WRITE_SIZE over the frame).
  const int wave = __builtin_amdgcn_readfirstlane(int(threadIdx.x) >> 6);
  STAMP_WAVE_BEGIN(wave);
  uint32_t tile = 0u;  // the linear tile: set and used by the 1-D instances only (ORD's epilogue)
  uint32_t fr = 0u, tx, ty;
  if constexpr (DEFER) {
    // the certified pass is launched as a tiles_x x tiles_y (x frames) grid (launch_render): the
    // tile's column, row and frame are the workgroup id's components, no division. Workgroups are
    // dispatched x fastest, then y, then z: the same order as the linear grid tile = (fr * tiles_y
    // + ty) * tiles_x + tx, so workgroup L still lands on XCD L % 8. (The linear tile itself is
    // not needed here: the deferred list's segment is the tile's column block, whose division by
    // tiles_x below is the one left, in waves that defer a pixel.)
    static_assert(!ORD, "the certified pass has no tile order");
    tx = blockIdx.x;
    ty = blockIdx.y;
    if constexpr (FB) fr = blockIdx.z;
  } else {
    tile = blockIdx.x;
    if constexpr (ORD) {  // heavy-first tile order (a.order): its own instance
      tile = ordered_tile(a, blockIdx.x);
      if (tile == ~0u) return;  // whole workgroup: its tile is rendered by another slot
    }
    tile = __builtin_amdgcn_readfirstlane(tile);
    // frame batches: the tile's frame and its tile within the frame (wave-uniform)
    if constexpr (FB) fr = uint32_t(__builtin_amdgcn_readfirstlane(int(tile / a.frame_tiles)));
    const uint32_t ltile = tile - fr * a.frame_tiles;
    ty = ltile / a.tiles_x;
    tx = ltile - ty * a.tiles_x;
  }
  const int px = pixel_x(tx, wave, lane_id());
  const int li = pixel_row(ty, wave, lane_id());
  const bool valid = px < a.width && li < a.rows;
  bool heavy = false;  // this lane took the exact path (tile order: the tile runs long next frame)
  bool deferred = false;  // DEFER: this lane's pixel is left to the exact pass

  Counters k;
#pragma unroll
  for (int q = 0; q < VRT_CNT_COUNT; ++q) k.c[q] = 0;

  if (valid) {
    Ctx c;
    init_ctx<DEFER>(c, a, vox);
    CTRACE_ONLY(c.tr = px == VRT_TRACE_PX && frame_row(a, li) == VRT_TRACE_PY;)
    if constexpr (FB) c.time = frame_view(a, fr).time;
    // one LDS pool: the exact path's axis table and bounce-stack bottom (in-lane instances), and
    // the certified tree's slots (TREE), which are live only before the exact path starts
    constexpr int kAxFloats = DEFER && !TREE ? 0 : kWgThreads * 3 * 4;
    constexpr int kStkFloats = std::max(DEFER ? 0 : kStackWords * kWgThreads,
                                        TREE ? (kTreeWords - 12) * kWgThreads : 0);
    constexpr int kPool = std::max(kAxFloats + kStkFloats, 4);
    __shared__ float4 lds_pool[kPool / 4];
    c.ax = &lds_pool[threadIdx.x * kAxLane];
    const Ray ray = primary_ray<DEFER>(a, FB ? frame_view(a, fr).pv : a.inv_pv, c, px, frame_row(a, li));
    k.c[VRT_CNT_PIXELS] = 1;
    k.c[VRT_CNT_PRIMARY_RAYS] = 1;
    uint32_t steps = 0, flags = 0;
    int32_t hit_vidx = -1;
    float hit_len = 0.0f;
    // stats-free colour-only frames: certified primary + shadow walks, the exact path for the
    // rest. cert_pixel starts from its own black colour and writes the result only on success,
    // so no colour value is live (and spilled, 1 KB per wave) across its early exits: C3
    // WRITE_SIZE 41 -> 17 MB per frame at equal speed (profiles/r02_s03). Parking the certified
    // colour in LDS, or storing certified pixels before the exact path and re-deriving the
    // primary ray there, was 4-6 % slower.
    // DEFER: the colour has no value until cert_pixel certifies the pixel and writes it; a deferred
    // pixel's colour is never stored here, and a zero was materialised before each of cert_pixel's
    // nested early exits (11 times three moves on the every-pixel path). The in-lane instances keep
    // their zero: exact_pixel starts from it.
    f3 color;
    if constexpr (!DEFER) color = mk(0.0f, 0.0f, 0.0f);
    float* tstk = nullptr;
    if constexpr (TREE) {
      static_assert(CERT == 2 && !TEX && !STATS, "certified trees: stats-free colour-only certified instances");
      tstk = reinterpret_cast<float*>(lds_pool) + kAxFloats + threadIdx.x;   // (and c.ax: tree_put)
    }
    float us = -1.0f;  // the primary walk's certified prefix, for the exact path
    bool need_exact;
    if (DEFER && (PHASE_STOP(0) || PHASE_STOP(1))) {  // phase budget: nothing, or the ray alone, as the colour
      color = PHASE_STOP(1) ? mk(ray.pos.x + ray.dir.x, ray.pos.y + ray.dir.y, ray.pos.z + ray.dir.z)
                            : mk(0.0f, 0.0f, 0.0f);
      need_exact = false;
    } else {
      need_exact = CERT < 2 || !cert_pixel<TEX, TREE, kWgThreads, DEFER>(c, ray, color, a.max_refl, a.max_transp, tstk, &us, &a);
    }
    STAMP_WAVE_CERT(need_exact);
    if constexpr (DEFER) {
      deferred = need_exact;
    } else if (need_exact) {
      color = mk(0.0f, 0.0f, 0.0f);
      heavy = true;
      float* lstk = reinterpret_cast<float*>(lds_pool) + kAxFloats;
      (void)exact_pixel<STATS, TEX, CERT >= 1, CERT == 2>(a, c, ray, color, k, steps, flags, hit_vidx,
                                                         hit_len, &lstk[threadIdx.x], STATS ? -1.0f : us);
    }
    const uint32_t l2 = lane_id();
    const size_t o = size_t(pixel_row(ty, wave, l2)) * size_t(a.pitch) + size_t(pixel_x(tx, wave, l2));
    if (STATS && hits) {
      vrt_hit hr;
      hr.voxel_index = hit_vidx;
      hr.ray_length = hit_len;
      hr.steps = steps;
      hr.flags = flags;
      hits[o] = hr;
    }
    // the frame's outputs read here, where they are used (kept live across the walks they were
    // held in registers, and their spills cost the in-lane exact instance 4 %)
    if constexpr (DEFER) {
      // (the certified pass: through the opaque view of the arguments; the compiler had moved the
      // plain reads above both walks all the same, six SGPRs)
      if (!deferred) {
        LateKArgs* ka = late_kargs();
        uint32_t *cur = ka->cur, *raw = ka->raw;
        if (FB && fr != 0u) {
          cur = ka->fb[fr - 1u].cur;
          raw = ka->fb[fr - 1u].raw;
        }
        store_pixel(*ka, FrameView{nullptr, 0.0f, cur, raw}, out, o, color);
      }
    } else {
      if (!deferred) store_pixel(a, FB ? frame_view(a, fr) : FrameView{a.inv_pv, a.time, a.cur, a.raw}, out, o, color);
    }
  }
  if constexpr (DEFER) {  // the wave's deferred pixels to the exact pass's list: ballot compaction
    const unsigned long long m = __ballot(deferred);
    if (m != 0ull) {
      // segment: the tile's column block of the band (tile column tx * 8 / tiles_x), so that
      // consecutive list entries come from nearby tiles and a sparse batch's rays are alike: C3
      // sparse exact waves 57 -> 49 us median against the 8 XCD classes' every-8th-tile order
      // (profiles/r05_s8 xstamps)
      const uint32_t seg = tx * kOrdClasses / a.tiles_x;
      const uint32_t first = uint32_t(__builtin_ctzll(m));
      const uint32_t cnt = uint32_t(__builtin_popcountll(m));
      // a wave with many deferred pixels (a glass region) keeps them as a chunk of its own, each
      // at its lane (a coherent 8x8 tile of exact work); the others append compactly
      const bool dense = cnt >= kDeferDense;
      uint32_t base = 0;
      if (lane_id() == first)
        base = atomicAdd(a.defer + ((uint32_t(dense) * 2u + a.defer_e) * kOrdClasses + seg) * kOrdCtrStride,
                         dense ? 1u : cnt);
      base = uint32_t(__builtin_amdgcn_readlane(int(base), int(first)));
      uint32_t* list = a.defer + kDeferHdr + seg * a.defer_seg;
      const uint32_t l3 = lane_id();  // the pixel re-derived (not kept live across the walks)
      // frame (3 bits) | band row (13 bits) | column (16 bits): batches need rows < 8192
      const uint32_t id = (fr << 29) | (uint32_t(pixel_row(ty, wave, l3)) << 16) | uint32_t(pixel_x(tx, wave, l3));
      if (dense) {  // chunks fill the segment's region from its end
        list[a.defer_seg - 64u * (base + 1u) + l3] = deferred ? id : ~0u;
      } else if (deferred) {
        const uint32_t rank = __builtin_amdgcn_mbcnt_hi(uint32_t(m >> 32), __builtin_amdgcn_mbcnt_lo(uint32_t(m), 0u));
        list[base + rank] = id;
      }
    }
  }
  if constexpr (ORD) {
    const bool heavy_wave = __ballot(heavy) != 0ull;
    if (lane_id() == 0) order_record(a, tile, heavy_wave);
  }
  STAMP_WAVE_END();  // after the tile-order bookkeeping (its atomic's return): the stamps bracket the whole wave
  if (STATS && counters) {
    unsigned long long* slot = counters + size_t(blockIdx.x % kCntReplicas) * VRT_CNT_COUNT;
#pragma unroll
    for (int q = 0; q < VRT_CNT_COUNT; ++q) {
      unsigned long long v = k.c[q];
#pragma unroll
      for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
      if (lane_id() == 0 && v) atomicAdd(slot + q, v);
    }
  }
}

// The deferred exact pass: the pixels a certified pass (render_kernel<..., DEFER>) left to it,
// rendered with the exact path 64 to a wave — the certified pass's waves end with their certified
// pixels, and the exact walks that would each have held a sparse wave of them run densely here
// (the north_star's __ballot compaction of live rays). Waves that deferred >= kDeferDense pixels
// (glass regions) left them as a chunk in lane order: one batch each, the same coherent 8x8 tile
// of exact work as in place (textured C3 0.0668 -> 0.0633 ms per frame against compact appends only,
// C2-C4 within +-1.5 %, profiles/r03_s21). The rest
// are batches of 64 list entries over the segments in order. Batches b, b + gridDim.x, ... per
// workgroup.
// Every deferred pixel is rendered exactly once, with the same exact path and epilogue as the
// in-lane fallback, so images are identical. Workgroup 0 zeroes the other counter set for the
// next launch on the stream (none of this launch's kernels reads it).
// WAVES: resident waves per SIMD the instance is built for (exact_pass_kernel; the whole-frame instances
// run under a VGPR cap instead, exact_pass_kernel_capped below). Whole frames, whose exact waves share the
// CUs with the next frames' certified passes, ran at 7 (72 VGPRs, ~1 KB of spills per lane) until r13:
// fewer waves cost 10-30 % while the certified waves took 72 VGPRs themselves (profiles/r03_s25; a
// spill-free 3-wave instance there: C3 0.0388 -> 0.049 ms per frame at 8.7 instead of 17.4 MB of HBM writes,
// r06_s11). Against 56-VGPR certified waves, 8 to a SIMD, a 120-VGPR exact wave displaces one of them as
// the 72-VGPR wave did, spills nothing and is the default for colour frames (kExactVgprs, vrt_tuning.h: C3
// 0.0303 -> 0.0287 ms per frame, profiles/r13_exact/); textured frames keep kExactWaves = 7.
// kFatWaves = 3 (no spills: shorter exact walks; 130-134 VGPRs) for colour-only bands of under 4
// dispatch rounds and synchronous frames,
// whose frame time is the certified pass plus this pass's latency (a.exact_fat: C4 k = 8 0.0229 ->
// 0.0222, C3 k = 2 0.0275 -> 0.0267 ms at 4 waves, profiles/r03_s67; 3 waves, which no longer
// spill where 4 now do: C4 synchronous frame 0.2125 -> 0.2059 ms, bands of C3/C4 k = 4, 8
// unchanged, r06_s14; textured bands get slower)
// SB: pixels per sparse batch (kSparseBatch*, vrt_tuning.h). 64 for whole frames; 16 in the short-band instance,
// whose frame time includes this pass's span: a sparse wave's span is its slowest walk, and a lone
// wave's walks cost the same per step with 16 lanes as with 64 (C4 k = 8 band 0.0222 -> 0.0200 ms,
// exact-pass span 58 -> 49 us; whole frames +1-3 %: more waves, profiles/r04_exact/)
//
// The pass's body, shared by the kernels below. Its colour instances (LATE = !TEX) read the launch
// late, as the certified pass does (late_kargs, vrt_cert.h): the Ctx comes without the sun, the sky
// factor and the atlas (exact_pixel reads them after the primary walk and per bounce), and the frame's
// outputs are read at the store. There the segment counters of the deferred list (8 sparse, 8 dense)
// are summed once and read again per batch, through the same opaque view, where the batch's entry is
// looked up: held in SGPRs from the kernel's start they were 16 scalar registers live across every
// walk, spilled into VGPR lanes (v_writelane) that the walks then lacked. The textured instances
// keep them in SGPRs: with the per-batch reads textured C3 and C4 ran 0.4-0.8 % slower than before
// the change, with the counters kept 0.8 % faster (profiles/r13_exact/ab_bench.txt).
template <bool TEX, int CERT, uint32_t SB, bool FB>
__device__ __forceinline__ void exact_pass_body(const KArgs& a, const uint16_t* __restrict__ vox,
                                                float4* __restrict__ out) {
  constexpr bool LATE = !TEX;
  const uint32_t* ctr = a.defer;
  if (blockIdx.x == 0 && threadIdx.x < 2u * kOrdClasses) {  // both kinds of the other set, for the next launch
    const uint32_t l = threadIdx.x;
    a.defer[(((l / kOrdClasses) * 2u + (a.defer_e ^ 1u)) * kOrdClasses + l % kOrdClasses) * kOrdCtrStride] = 0u;
  }
  // (ns, nd: dead in the LATE instances, which read the counters again per batch)
  uint32_t ns[kOrdClasses], nd[kOrdClasses], total_s = 0, total_d = 0;
#pragma unroll
  for (uint32_t q = 0; q < kOrdClasses; ++q) {
    // (readfirstlane: wave-uniform values in SGPRs; as VGPRs the counts were spilled to scratch by every
    // workgroup, idle ones included, before the early exit below)
    ns[q] = uint32_t(__builtin_amdgcn_readfirstlane(int(ctr[(a.defer_e * kOrdClasses + q) * kOrdCtrStride])));
    nd[q] = uint32_t(__builtin_amdgcn_readfirstlane(int(ctr[((2u + a.defer_e) * kOrdClasses + q) * kOrdCtrStride])));
    total_s += ns[q];
    total_d += nd[q];
  }
  static_assert(SB >= 1 && SB <= 64, "lanes SB.. of a sparse batch idle");
  const uint32_t batches = total_d + (total_s + SB - 1u) / SB;
  if (a.batches_out && blockIdx.x == 0 && threadIdx.x == 0)
    *a.batches_out = batches;  // for the grid of a later launch on this slot (host-mapped word)
  if (blockIdx.x >= batches) return;  // idle workgroups leave before touching scratch
  if constexpr (kExactPrio > 0) __builtin_amdgcn_s_setprio(kExactPrio);
  const uint32_t lane = lane_id();
  STAMP_PASS_BEGIN();
  Ctx c;
  init_ctx<LATE>(c, a, vox);
  __shared__ float4 ax_tab[64 * 3];
  c.ax = &ax_tab[lane * kAxLane];
  for (uint32_t b = blockIdx.x; b < batches; b += gridDim.x) {
    // batch b: dense chunk b (in segment order), else sparse entries [SB (b - total_d), + SB)
    // (sparse batches first measured neutral: C3 0.0386 vs 0.0387 ms, the 20-frame command 0.0453
    // vs 0.0459; profiles/r05_s32)
    const bool dense = b < total_d;
    uint32_t idx = dense ? b : (b - total_d) * SB + lane;
    if (!dense && (lane >= SB || idx >= total_s)) continue;
    // the entry's segment. LATE: this kind's counters read again (unchanged since the sums above: only
    // the certified pass before this kernel wrote them), the list's base and segment size with them
    uint32_t seg = 0, e;
    if constexpr (LATE) {
      LateKArgs* kq = late_kargs();
      const uint32_t kind = uint32_t(__builtin_amdgcn_readfirstlane(dense ? 2 : 0));  // (b is wave-uniform)
      const uint32_t* cq = kq->defer + (kind + kq->defer_e) * kOrdClasses * kOrdCtrStride;
#pragma unroll
      for (uint32_t q = 0; q + 1u < kOrdClasses; ++q) {
        const uint32_t nq = uint32_t(__builtin_amdgcn_readfirstlane(int(cq[q * kOrdCtrStride])));
        const bool past = seg == q && idx >= nq;
        idx -= past ? nq : 0u;
        seg += past ? 1u : 0u;
      }
      const uint32_t* list = kq->defer + kDeferHdr + seg * kq->defer_seg;
      e = dense ? list[kq->defer_seg - 64u * (idx + 1u) + lane] : list[idx];
    } else {
#pragma unroll
      for (uint32_t q = 0; q + 1u < kOrdClasses; ++q) {
        const uint32_t nq = dense ? nd[q] : ns[q];
        const bool past = seg == q && idx >= nq;
        idx -= past ? nq : 0u;
        seg += past ? 1u : 0u;
      }
      const uint32_t* list = a.defer + kDeferHdr + seg * a.defer_seg;
      e = dense ? list[a.defer_seg - 64u * (idx + 1u) + lane] : list[idx];
    }
    if (e == ~0u) continue;  // a lane of a dense chunk whose pixel the certified pass settled
    Ray ray;
    if constexpr (FB) {
      const FrameView fv = frame_view(a, e >> 29);
      c.time = fv.time;
      ray = primary_ray(a, fv.pv, c, int(e & 0xFFFFu), frame_row(a, int((e >> 16) & 0x1FFFu)));
    } else {
      ray = primary_ray(a, a.inv_pv, c, int(e & 0xFFFFu), frame_row(a, int(e >> 16)));
    }
    Counters k;
#pragma unroll
    for (int q = 0; q < VRT_CNT_COUNT; ++q) k.c[q] = 0;
    uint32_t steps = 0, flags = 0;
    int32_t hit_vidx = -1;
    float hit_len = 0.0f;
    f3 color = mk(0.0f, 0.0f, 0.0f);
    __shared__ float lstk[kStackWords * 64];
    (void)exact_pixel<false, TEX, CERT >= 1, CERT == 2 && !TEX, 64, LATE>(a, c, ray, color, k, steps, flags,
                                                                          hit_vidx, hit_len, &lstk[lane]);
    // the pixel and its frame re-derived from e (only e stays live across the exact path)
    uint32_t e2 = e;
    if constexpr (FB || LATE) asm volatile("" : "+v"(e2));  // not CSE'd with the decode above (whose results would stay live)
    const uint32_t row = FB ? (e2 >> 16) & 0x1FFFu : e2 >> 16;
    if constexpr (LATE) {
      LateKArgs* ka = late_kargs();
      uint32_t *cur = ka->cur, *raw = ka->raw;
      if constexpr (FB) {
        const uint32_t f = e2 >> 29;
        if (f != 0u) {
          cur = ka->fb[f - 1u].cur;
          raw = ka->fb[f - 1u].raw;
        }
      }
      store_pixel(*ka, FrameView{nullptr, 0.0f, cur, raw}, out, size_t(row) * size_t(ka->pitch) + size_t(e2 & 0xFFFFu),
                  color);
    } else {
      store_pixel(a, FB ? frame_view(a, e2 >> 29) : FrameView{a.inv_pv, a.time, a.cur, a.raw}, out,
                  size_t(row) * size_t(a.pitch) + size_t(e2 & 0xFFFFu), color);
    }
    STAMP_PASS_BATCH(dense);
  }
  STAMP_PASS_END(lane);
}

// The kernel's first argument where it lies, in the kernarg segment (offset 0). The kernels below hand
// their body this view: a reference to the by-value parameter made the frame-batch instances keep a
// copy of all of KArgs in scratch (they index KArgs::fb by a lane's frame), 1.1 KB per lane.
// This view, late_kargs and late_ctx (vrt_cert.h) all read offset 0: KArgs must stay the FIRST parameter
// of every kernel that inlines exact_pass_body or exact_pixel<..., LATE> (the three kernels below), as it
// is of the certified pass. The parameter itself is not read in them: it only lays the segment out.
__device__ __forceinline__ const KArgs& kernel_kargs() {
  return *(const KArgs*)__builtin_amdgcn_kernarg_segment_ptr();
}
template <bool TEX, int CERT, int WAVES = kExactWaves, uint32_t SB = kSparseBatch, bool FB = false>
__global__ void __launch_bounds__(64, WAVES) exact_pass_kernel(KArgs /* first: kernel_kargs() */,
                                                               const uint16_t* __restrict__ vox,
                                                               float4* __restrict__ out) {
  exact_pass_body<TEX, CERT, SB, FB>(kernel_kargs(), vox, out);
}
// The colour whole-frame instances under a VGPR cap (kExactVgprs, vrt_tuning.h) instead of a whole
// number of waves. amdgpu_num_vgpr takes an integer constant, no template argument: hence a kernel of
// its own for the cap.
template <int CERT, uint32_t SB, bool FB>
__global__ void __launch_bounds__(64, exact_cap_waves(kExactVgprs))
    __attribute__((amdgpu_num_vgpr(exact_cap_attr(kExactVgprs))))
    exact_pass_kernel_capped(KArgs /* first: kernel_kargs() */, const uint16_t* __restrict__ vox,
                             float4* __restrict__ out) {
  exact_pass_body<false, CERT, SB, FB>(kernel_kargs(), vox, out);
}

}  // namespace vrt

// the ray-query kernel (vrt_cast_rays*, vrt_pick_pixels): here because it calls init_ctx and primary_ray
#include "vrt_query_kernels.h"
// certified walks for a ray list (vrt_debug_cert_walks): here because it calls init_ctx
#include "vrt_cert_debug_kernels.h"
// the shaded ray-query kernels (vrt_trace_rays*, vrt_trace_pixels): after exact_pixel, which they call
#include "vrt_trace_kernels.h"
// the ID and depth pass (vrt_render_ids*): after primary_ray, the ray-query kernel's ray_hit_face and vrt_cert.h
#include "vrt_ids_kernels.h"
// the reprojected temporal filter (vrt_reproject_temporal_async): after temporal_blend and primary_ray
#include "vrt_reproject_kernels.h"
// the ID-guided spatial filter (vrt_spatial_filter_async): it calls nothing of the kernels above
#include "vrt_spatial_kernels.h"

namespace vrt {

// ------------------------------------------------------------------------------- launches --
// Host wrappers of the kernels above, of vrt_aux_kernels.h, vrt_skipfield_kernels.h,
// vrt_query_kernels.h and vrt_trace_kernels.h (vrt_internal.h); the C-ABI context around them is the
// vrt_*.cpp files of vrt_context.h.

// Every launch of this file: `kern` over grid x block with lds_bytes of dynamic LDS on `s`, its arguments
// converted to the kernel's parameter types. ev_begin / ev_end (either may be null) are recorded when the kernel
// starts / ends on the device, which takes the Ext form of the launch: used exactly when an event is given.
template <class T>
using KernelArg = const std::common_type_t<T>&;
template <class... P>
static void launch_kernel(void (*kern)(P...), dim3 grid, dim3 block, uint32_t lds_bytes, hipStream_t s,
                          hipEvent_t ev_begin, hipEvent_t ev_end, KernelArg<P>... args) {
  if (ev_begin || ev_end)
    hipExtLaunchKernelGGL(kern, grid, block, lds_bytes, s, ev_begin, ev_end, 0, args...);
  else
    hipLaunchKernelGGL(kern, grid, block, lds_bytes, s, args...);
}
// workgroups of 256 for a grid-stride loop over `items`
static unsigned grid_blocks(uint64_t items) { return unsigned(std::min<uint64_t>((items + 255) / 256, 16384)); }
// the untimed launches of such a loop (the kernels of 256 threads that stride over `items` cells)
template <class... P>
static void launch_cells(void (*kern)(P...), uint64_t items, hipStream_t s, KernelArg<P>... args) {
  launch_kernel(kern, dim3(grid_blocks(items)), dim3(256), 0, s, nullptr, nullptr, args...);
}

// The kernel of every row of vrt_instances.h, built from the row's own fields
using RenderFn = void (*)(KArgs, const uint16_t*, float4*, vrt_hit*, unsigned long long*);
using ExactPassFn = void (*)(KArgs, const uint16_t*, float4*);
template <size_t I>
constexpr RenderFn render_instance() {
  constexpr RenderInstance r = kRenderInstances[I];
  return render_kernel<r.stats, r.tex, r.cert, r.ord, r.defer, r.fb, r.tree>;
}
template <size_t I>
constexpr ExactPassFn exact_instance() {
  constexpr ExactInstance r = kExactInstances[I];
  if constexpr (r.capped) {
    static_assert(!r.tex, "the VGPR cap is the colour instances'");
    return exact_pass_kernel_capped<r.cert, r.sparse_batch, r.fb>;
  } else {
    return exact_pass_kernel<r.tex, r.cert, r.waves, r.sparse_batch, r.fb>;
  }
}
template <size_t... I>
static std::array<RenderFn, sizeof...(I)> render_table(std::index_sequence<I...>) {
  return {render_instance<I>()...};
}
template <size_t... I>
static std::array<ExactPassFn, sizeof...(I)> exact_table(std::index_sequence<I...>) {
  return {exact_instance<I>()...};
}
static const auto kRenderKernels = render_table(std::make_index_sequence<kRenderInstanceCount>());
static const auto kExactKernels = exact_table(std::make_index_sequence<kExactInstanceCount>());

void launch_render(const KArgs& a, bool stats, const uint16_t* vox, float4* out, vrt_hit* hit,
                   unsigned long long* cnt_rep, hipStream_t s, hipEvent_t ev_begin, hipEvent_t ev_end) {
  const InstanceChoice c = choose_instances(stats, a.textured != 0, a.cert, a.tree != 0, a.order != nullptr,
                                            a.defer != nullptr, a.nframes, a.exact_fat != 0);
  const RenderFn kern = kRenderKernels[size_t(c.render)];
  if (c.exact < 0) {
    const dim3 grid(a.order ? kOrdClasses * a.ord_q + a.tiles : a.tiles);
    launch_kernel(kern, grid, dim3(kWgThreads), 0, s, ev_begin, ev_end, a, vox, out, hit, cnt_rep);
    return;
  }
  // certified pass, then the exact pass over the pixels it deferred.
  // the certified pass's grid: tile columns x tile rows x frames (render_kernel reads its tile
  // from the workgroup id's components); the same workgroups in the same dispatch order as a.tiles
  const dim3 g1(a.tiles_x, a.frame_tiles / a.tiles_x, uint32_t(a.nframes)),
      g2(a.exact_grid ? a.exact_grid
                      : std::max(64u, a.tiles * uint32_t(kWgWaves) / (a.textured ? kDeferGridDiv : kDeferGridDivColor)));
  const uint32_t pad = a.tree ? 0u : kDeferLdsPad;  // (an occupancy A/B knob, vrt_tuning.h)
  launch_kernel(kern, g1, dim3(kWgThreads), pad, s, ev_begin, nullptr, a, vox, out, hit, cnt_rep);
  launch_kernel(kExactKernels[size_t(c.exact)], g2, dim3(64), 0, s, nullptr, ev_end, a, vox, out);
}

void launch_ray_query(const KArgs& a, int32_t kind, const uint16_t* vox, const void* in, uint32_t count,
                      vrt_ray_hit* hits, hipStream_t s, hipEvent_t ev_begin, hipEvent_t ev_end) {
  auto kern = kind == kQueryPick           ? ray_query_kernel<kQueryPick>
              : kind == VRT_CAST_OCCLUSION ? ray_query_kernel<VRT_CAST_OCCLUSION>
                                           : ray_query_kernel<VRT_CAST_NEAREST>;
  // one lane per query: ceil(count / kQueryWg) workgroups (count <= 2^30)
  const dim3 grid((count + uint32_t(kQueryWg) - 1u) / uint32_t(kQueryWg));
  launch_kernel(kern, grid, dim3(kQueryWg), 0, s, ev_begin, ev_end, a, vox, in, count, reinterpret_cast<uint4*>(hits));
}

void launch_cert_walks_debug(const KArgs& a, int32_t kind, const uint16_t* vox, const void* in, uint32_t count,
                             void* out, hipStream_t s) {
  // one lane per ray: ceil(count / kCertDebugWg) workgroups
  const dim3 grid((count + uint32_t(kCertDebugWg) - 1u) / uint32_t(kCertDebugWg));
  launch_kernel(cert_walks_debug_kernel, grid, dim3(kCertDebugWg), 0, s, nullptr, nullptr, a, vox,
                static_cast<const float4*>(in), count, kind, static_cast<uint4*>(out));
}

void launch_ray_trace(const KArgs& a, int32_t kind, const uint16_t* vox, const void* in, uint32_t count,
                      vrt_ray_color* out, hipStream_t s, hipEvent_t ev_begin, hipEvent_t ev_end) {
  auto kern = kind == kTracePixels
                  ? (a.textured ? ray_trace_kernel<kTracePixels, true> : ray_trace_kernel<kTracePixels, false>)
                  : (a.textured ? ray_trace_kernel<kTraceRays, true> : ray_trace_kernel<kTraceRays, false>);
  // one lane per query: ceil(count / kTraceWg) workgroups (count <= 2^30)
  const dim3 grid((count + uint32_t(kTraceWg) - 1u) / uint32_t(kTraceWg));
  launch_kernel(kern, grid, dim3(kTraceWg), 0, s, ev_begin, ev_end, a, vox, in, count, reinterpret_cast<uint4*>(out));
}

void launch_render_ids(const KArgs& a, const uint16_t* vox, vrt_pixel_id* ids, float* depth, hipStream_t s,
                       hipEvent_t ev_begin, hipEvent_t ev_end, bool certified, uint32_t* n_exact) {
  const dim3 grid(uint32_t(a.width + 7) / 8u, uint32_t(a.rows + 7) / 8u);
  if (certified)
    launch_kernel(ids_cert_kernel, grid, dim3(64), 0, s, ev_begin, ev_end, a, vox, reinterpret_cast<uint2*>(ids), depth,
                  n_exact);
  else
    launch_kernel(ids_exact_kernel, grid, dim3(64), 0, s, ev_begin, ev_end, a, vox, reinterpret_cast<uint2*>(ids), depth);
}

void launch_reproject(const KArgs& a, const ReprojArgs& r, int32_t fetch, uint8_t* taps, hipStream_t s,
                      hipEvent_t ev_begin, hipEvent_t ev_end) {
  const dim3 grid(uint32_t(a.width + 15) / 16u, uint32_t(a.rows + 15) / 16u);
  if (fetch == VRT_FETCH_NEAREST && !taps)
    launch_kernel(reproject_kernel, grid, dim3(kReprojWg), 0, s, ev_begin, ev_end, a, r);
  else
    launch_kernel(fetch == VRT_FETCH_BILINEAR ? reproject_bilinear_kernel : reproject_nearest_taps_kernel, grid,
                  dim3(kReprojWg), 0, s, ev_begin, ev_end, a, r, taps);
}

void launch_spatial(const SpatialArgs& a, hipStream_t s, hipEvent_t ev_begin, hipEvent_t ev_end) {
  auto kern = !spatial_lds_form(a.step) ? spatial_direct_kernel
              : a.step == 1             ? spatial_lds_kernel<1>
              : a.step == 2             ? spatial_lds_kernel<2>
                                        : spatial_lds_kernel<4>;
  const dim3 grid(uint32_t(a.width + 15) / 16u, uint32_t(a.rows + 15) / 16u);
  launch_kernel(kern, grid, dim3(kSpatialWg), 0, s, ev_begin, ev_end, a);
}

void launch_reduce_counters(unsigned long long* rep, unsigned long long* dst, hipStream_t s) {
  launch_kernel(reduce_counters_kernel, dim3(1), dim3(64), 0, s, nullptr, nullptr, rep, dst);
}

// ---- the skip field (upload, vrt_update_volume_region) ---------------------------------------------

void launch_edit_apply(const uint8_t* box, uint8_t* vox, uint32_t n, const int32_t lo[3], const int32_t ext[3],
                       unsigned long long* counts, hipStream_t s) {
  const Region b{lo[0], lo[1], lo[2], ext[0], ext[1], ext[2]};
  launch_cells(edit_apply_kernel, region_cells(b), s, box, vox, b, n, counts);
}

// The passes of skipfield_passes (vrt_skipfield_plan.cpp: every box is chosen there) in its order, one launch
// each. The scratch thirds are N^3 bytes each: every box is clipped to the volume, so each fits one.
void launch_volume_edit_passes(const uint8_t* vox, uint8_t* tmp, uint16_t* packed, uint32_t n, int octants,
                               const int32_t lo[3], const int32_t ext[3], bool distances, hipStream_t s) {
  const uint64_t vol = uint64_t(n) * n * n, pvol = uint64_t(n + 1) * (n + 1) * (n + 1);
  const SkipPlan plan = skipfield_passes(int32_t(n), octants, lo, ext, distances);
  for (int i = 0; i < plan.count; ++i) {
    const SkipPass& p = plan.pass[i];
    // the distances read: the canonical volume (a first pass), a scratch third, or none (a pack that keeps them)
    const uint8_t* src = p.first ? vox : (p.src >= 0 ? tmp + uint64_t(p.src) * vol : nullptr);
    uint8_t* dst = p.dst >= 0 ? tmp + uint64_t(p.dst) * vol : nullptr;
    switch (p.kind) {
      case SkipPassKind::kFwdPass:
        launch_cells(fwd_pass_kernel, region_cells(p.out), s, src, p.in, dst, p.out, n, p.axis, p.sg[p.axis], p.first);
        break;
      case SkipPassKind::kFwdPack:
        launch_cells(fwd_pack_kernel, region_cells(p.out), s, vox, src, p.in, packed + size_t(p.octant) * pvol, p.out,
                     n, p.sg[0], p.sg[1], p.sg[2]);
        break;
      case SkipPassKind::kDistPass:
        launch_cells(dist_pass_kernel, region_cells(p.out), s, src, p.in, dst, p.out, n, p.axis, p.first);
        break;
      case SkipPassKind::kVolumePack:
        launch_cells(pack_volume_kernel, region_cells(p.out), s, vox, src, p.in, packed, p.out, n);
        break;
      case SkipPassKind::kEdgePack: {
        const EdgeSlabs e = edge_slabs(p.out, p.wrap);
        launch_cells(edge_pack_kernel, e.cz + e.cy + e.cx, s, vox, packed, pvol, octants, p.out, p.wrap, n);
        break;
      }
    }
  }
}

void launch_glass_share(const uint8_t* vox, uint64_t total, unsigned long long* out, hipStream_t s) {
  launch_cells(glass_share_kernel, total, s, vox, total, out);
}

void launch_build_scene(uint8_t* vox, int scene, uint32_t n, const float* noise, hipStream_t s) {
  const uint64_t vol = uint64_t(n) * n * n;
  launch_cells(build_scene_kernel, vol, s, vox, scene, n, noise);
}

void launch_assemble_blocks(const uint32_t* bands, uint64_t band_words, int32_t k, int32_t sh, int32_t width,
                            int32_t height, uint32_t* frame, uint64_t frame_pitch, hipStream_t s) {
  if (height <= 0 || width <= 0) return;
  const bool vec = width % 4 == 0 && band_words % 4 == 0 && frame_pitch % 4 == 0 &&
                   (reinterpret_cast<uintptr_t>(bands) & 15u) == 0 && (reinterpret_cast<uintptr_t>(frame) & 15u) == 0;
  launch_kernel(vec ? assemble_blocks_kernel<true> : assemble_blocks_kernel<false>, dim3(uint32_t(height)), dim3(256), 0,
                s, nullptr, nullptr, bands, band_words, k, sh, width, frame, frame_pitch);
}

void launch_pack_rgb8(const uint32_t* rgba, uint64_t pixels, uint8_t* rgb, hipStream_t s) {
  const uint64_t quads = pixels / 4u;
  if (quads == 0) return;
  launch_cells(pack_rgb8_kernel, quads, s, reinterpret_cast<const uint4*>(rgba), quads, reinterpret_cast<uint32_t*>(rgb));
}

void launch_assemble_blocks_rgb8(const uint8_t* bands, uint64_t band_px, int32_t k, int32_t sh, int32_t width,
                                 int32_t height, uint32_t* frame, uint64_t frame_pitch, hipStream_t s) {
  if (height <= 0 || width <= 0) return;
  launch_kernel(assemble_blocks_rgb8_kernel, dim3(uint32_t(height)), dim3(256), 0, s, nullptr, nullptr,
                reinterpret_cast<const uint32_t*>(bands), band_px, k, sh, width, reinterpret_cast<uint4*>(frame),
                frame_pitch);
}

int run_fast_math_check(unsigned long long* host_out) {
  unsigned long long* d = nullptr;
  if (hipMalloc(&d, 7 * sizeof(unsigned long long)) != hipSuccess) return VRT_ERR_OOM;
  const unsigned long long init[7] = {0, 0, 0, 0, ~0ull, 0, 0};
  hipError_t e = hipMemcpy(d, init, sizeof(init), hipMemcpyHostToDevice);
  if (e == hipSuccess) {
    // 2^32 patterns: 2^24 threads of 256 patterns each
    launch_kernel(fast_math_check_kernel, dim3(1u << 16), dim3(256), 0, nullptr, nullptr, nullptr, d);
    e = hipGetLastError();
  }
  if (e == hipSuccess) e = hipMemcpy(host_out, d, sizeof(init), hipMemcpyDeviceToHost);
  (void)hipFree(d);
  return e == hipSuccess ? VRT_OK : VRT_ERR_DEVICE;
}

int run_pow_forms_check(unsigned long long* host_out) {
  unsigned long long* d = nullptr;
  if (hipMalloc(&d, 6 * sizeof(unsigned long long)) != hipSuccess) return VRT_ERR_OOM;
  const unsigned long long init[6] = {0, 0, 0, 0, 0, ~0ull};
  hipError_t e = hipMemcpy(d, init, sizeof(init), hipMemcpyHostToDevice);
  if (e == hipSuccess) {
    // 2^32 patterns: 2^24 threads of 256 patterns each
    launch_kernel(pow_forms_check_kernel, dim3(1u << 16), dim3(256), 0, nullptr, nullptr, nullptr, d);
    e = hipGetLastError();
  }
  if (e == hipSuccess) e = hipMemcpy(host_out, d, sizeof(init), hipMemcpyDeviceToHost);
  (void)hipFree(d);
  return e == hipSuccess ? VRT_OK : VRT_ERR_DEVICE;
}

void launch_randomize(const float* dir, const float* pos, int n, float randomness, float seed,
                      float* out, hipStream_t s) {
  launch_kernel(randomize_kernel, dim3((n + 63) / 64), dim3(64), 0, s, nullptr, nullptr, dir, pos, n, randomness, seed,
                out);
}

}  // namespace vrt
