// vrt_walk.h — the exact walks: Ray / Hit / Counters / Ctx, the packed-volume loads, dda_walk, skip_walk,
// RayMarch / RayMarchShadow, shading and TraceWithShadow. Includes vrt_internal.h, vrt_diag.h and vrt_math.h.
#ifndef VRT_WALK_H
#define VRT_WALK_H

#include "vrt_internal.h"
#include "vrt_diag.h"
#include "vrt_math.h"

namespace vrt {

// ----------------------------------------------------------------------------- ray state --

struct Ray {
  f3 pos, dir;
  float len, energy;
  uint32_t voxel;  // byte value of the medium the ray travels in (0 = air)
  int32_t rdepth, tdepth;
};

struct Hit {
  f3 point, normal;
  float len;
  uint32_t voxel;
  int32_t vidx;  // canonical index x + y*N + z*N*N of the texel read
  int32_t axis;  // intersectionAxis row of the step (tie 3 clamped to 2)
  bool found;
};

struct Counters {
  uint32_t c[VRT_CNT_COUNT];
};

// Crossed-axis operands of a skip step come from a per-lane LDS table (one ds_read_b128 at an
// address selected from the lane's three entry addresses: 2 VALU) instead of three 3-way register
// selects. Lane-major layout: entry a of work-item t at [3t + a] (an axis-major table measured
// neutral, profiles/r01_v37_ab_axis_major_len0_cmpt.log).
constexpr int kAxStride = 1;  // float4s between axes
constexpr int kAxLane = 3;    // float4s between lanes

struct Ctx {
  const uint16_t* __restrict__ vox;  // padded (N+1)^3 layout, voxel | G << 8, one per octant (see pack kernels)
  uint32_t ostride;  // bytes between the octant volumes (0: a single centred-distance volume)
  int32_t n;
  uint32_t p;  // N + 1
  float fn;
  float max_len;
  f3 sun_n, sun_rcp;
  float sky_sy;
  float time, refl_noise, refr_noise;
  float4* ax;  // this lane's 3-entry axis table in LDS: {pos, dir, rcp, sign} per axis
  const uint32_t* atlas;  // textured instances only (TEX)
  uint32_t atlas_mask;   // atlas_size - 1 (power of two)
  float atlas_fs, atlas_fts;  // (float)u_AtlasSize, (float)u_AtlasTextureSize
  CTRACE_ONLY(bool tr;)  // trace builds: this lane's pixel is the traced one
};

// a*b + c on the low 24 bits of a and b: one v_mad_u32_u24 (operands < 2^24 for N <= 1024).
// b is wave-uniform (the padded pitch) and goes in as the instruction's one SGPR operand.
__device__ __forceinline__ uint32_t mad24(uint32_t a, uint32_t b, uint32_t c) {
  uint32_t r;
  asm("v_mad_u32_u24 %0, %1, %2, %3" : "=v"(r) : "v"(a), "s"(b), "v"(c));
  return r;
}

// 16-bit load at a 32-bit byte offset from a wave-uniform base: global_load_ushort with an SGPR
// base (no 64-bit address arithmetic per lane)
__device__ __forceinline__ uint32_t load_u16(const uint16_t* __restrict__ base, uint32_t idx) {
  return *reinterpret_cast<const uint16_t*>(reinterpret_cast<const char*>(base) + (idx << 1));
}
// the same texel in the volume of the ray's direction octant, `obase` bytes after the first one:
// the byte offset (idx << 1) + obase is one v_lshl_add_u32, as the plain shift was
__device__ __forceinline__ uint32_t load_u16_at(const uint16_t* __restrict__ base, uint32_t idx,
                                                uint32_t obase) {
  return *reinterpret_cast<const uint16_t*>(reinterpret_cast<const char*>(base) + ((idx << 1) + obase));
}
// texel fields of the packed word: voxel byte and the skip distance (forward distance G of the
// octant, or the centred Chebyshev D of the single-volume layout; see the skip walk)
constexpr uint32_t kVoxMask = 0xFFu;
constexpr uint32_t kDistShift = 8u;

__device__ __forceinline__ int32_t canonical_index(const Ctx& c, uint32_t i, uint32_t j, uint32_t k) {
  const uint32_t n = uint32_t(c.n);
  i = i == n ? 0u : i;
  j = j == n ? 0u : j;
  k = k == n ? 0u : k;
  return int32_t(i + (j + k * n) * n);
}

// GetVoxel (voxel.glsl:149-154): `>` bounds test, NEAREST + GL_REPEAT, NaN reads 0. Reference
// form, used off the hot loop (refraction probes).
__device__ __forceinline__ uint32_t get_voxel(const Ctx& c, f3 p) {
  if (!(p.x >= 0.0f && p.y >= 0.0f && p.z >= 0.0f && p.x <= c.fn && p.y <= c.fn && p.z <= c.fn))
    return 0u;
  const uint32_t i = uint32_t(__builtin_floorf(p.x));
  const uint32_t j = uint32_t(__builtin_floorf(p.y));
  const uint32_t k = uint32_t(__builtin_floorf(p.z));
  return load_u16(c.vox, mad24(mad24(k, c.p, j), c.p, i)) & kVoxMask;
}

// TestCube (voxel.glsl:248-257) with centre N/2 and size N; bitwise ops, no short-circuit branches.
__device__ __forceinline__ bool test_cube(f3 p, f3 d, float fn) {
  const float hi = fn * 0.5f + fn / 2.0f, lo = fn * 0.5f - fn / 2.0f;
  const bool out = (p.x > hi & d.x > 0.0f) | (p.x < lo & d.x < 0.0f) | (p.y > hi & d.y > 0.0f) |
                   (p.y < lo & d.y < 0.0f) | (p.z > hi & d.z > 0.0f) | (p.z < lo & d.z < 0.0f);
  return !out;
}

__device__ __forceinline__ float next_plane(float d, float p) {
  return d < 0.0f ? __builtin_ceilf(p - 1.0f) : __builtin_floorf(p + 1.0f);
}

__device__ __forceinline__ f3 initial_t(f3 dir, f3 cur, f3 pos) {
  return mk((next_plane(dir.x, cur.x) - pos.x) / dir.x, (next_plane(dir.y, cur.y) - pos.y) / dir.y,
            (next_plane(dir.z, cur.z) - pos.z) / dir.z);
}

__device__ __forceinline__ float sel3(int axis, float x, float y, float z) {
  return axis == 2 ? z : (axis == 1 ? y : x);
}

// a / d correctly rounded, given y = RN(1/d) (Markstein's theorem: q1 is within one ulp of a/d,
// so r1 = a - d*q1 is exact and RN(q1 + r1*y) = RN(a/d); no over/underflow for the fast-path
// operand ranges, see fast_path_ok). Bit-identical to IEEE division, 5 VALU ops instead of the
// ~11 of the scaled div_scale/div_fmas/div_fixup sequence.
__device__ __forceinline__ float div_rn(float a, float d, float y) {
  const float q0 = a * y;
  const float r0 = __builtin_fmaf(-d, q0, a);
  const float q1 = __builtin_fmaf(r0, y, q0);
  const float r1 = __builtin_fmaf(-d, q1, a);
  return __builtin_fmaf(r1, y, q1);
}

// The fast walk needs every direction component normal and not tiny: then every t stays finite
// and never -0 (so v_min3 == GLSL min) and div_rn is exact. Otherwise (a +-0 component: +-inf /
// NaN t values, where the GLSL would spin) the walk replays the reference literally.
__device__ __forceinline__ bool fast_path_ok(f3 d) {
  const float lo = 0x1p-64f;
  return __builtin_fabsf(d.x) >= lo && __builtin_fabsf(d.y) >= lo && __builtin_fabsf(d.z) >= lo &&
         __builtin_fabsf(d.x) <= 1.0e4f && __builtin_fabsf(d.y) <= 1.0e4f &&
         __builtin_fabsf(d.z) <= 1.0e4f;
}

struct WalkState {
  f3 t;            // distance to the next plane per axis, relative to the current step
  f3 cur;          // currentPos
  float len;       // rayLength
  uint32_t it;     // iterations of this RayMarch/RayMarchShadow call (VRT_MAX_STEPS cap)
  uint32_t ties;   // index==3 events
  bool check_cube; // TestCube must be evaluated at the loop top
};

enum : int { WALK_MISS = 0, WALK_EVENT = 1, WALK_CAP = 2 };

// floor(x) -> int in one VALU op; x is already clamped to [0, N] by the caller
__device__ __forceinline__ uint32_t cvt_flr(float x) {
  int32_t r;
  asm("v_cvt_flr_i32_f32 %0, %1" : "=v"(r) : "v"(x));
  return uint32_t(r);
}

// Max of x over the ACTIVE lanes only, as a wave-uniform value. (A __shfl reduction would also
// read inactive lanes' stale registers, e.g. a step count of a lane that already stopped at the
// cap, and stall the others.) Scalar loop: each round takes the value of an active lane holding a
// larger x (ballot covers active lanes only), so it ends after <= 64 rounds, usually one.
__device__ __forceinline__ uint32_t active_max(uint32_t x) {
  uint32_t m = __builtin_amdgcn_readfirstlane(x);
  for (;;) {
    const unsigned long long bigger = __ballot(x > m);
    if (bigger == 0ull) return m;
    m = __builtin_amdgcn_readlane(x, int(__builtin_ctzll(bigger)));
  }
}

// x + (a && b ? 1 : 0) as one v_addc with the lane mask as carry-in (active lanes only). The
// masks of a and b are taken separately (each a plain v_cmp result) and ANDed in SALU; a ballot
// of the combined bool would be materialised in a VGPR first.
__device__ __forceinline__ uint32_t add_if_both(uint32_t x, bool a, bool b) {
  const unsigned long long m = __builtin_amdgcn_ballot_w64(a) & __builtin_amdgcn_ballot_w64(b);
  unsigned long long co;
  asm("v_addc_co_u32_e64 %0, %1, %0, 0, %2" : "+v"(x), "=s"(co) : "s"(m));
  return x;
}

// crossed-axis index from the compare masks: mez ? 2 : (mey ? 1 : 0), two v_cndmask
__device__ __forceinline__ uint32_t axis_index(unsigned long long mey, unsigned long long mez) {
  uint32_t r;
  asm("v_cndmask_b32_e64 %0, 0, 1, %1\n\tv_cndmask_b32_e64 %0, %0, 2, %2" : "=&v"(r) : "s"(mey), "s"(mez));
  return r;
}

// m's lane bit ? if_set : if_clear, as one v_cndmask on an SGPR lane mask
__device__ __forceinline__ float sel_mask(unsigned long long m, float if_set, float if_clear) {
  float r;
  asm("v_cndmask_b32_e64 %0, %1, %2, %3" : "=v"(r) : "v"(if_clear), "v"(if_set), "s"(m));
  return r;
}

// m's lane bit ? if_set : if_clear on 32-bit integers (one v_cndmask)
__device__ __forceinline__ uint32_t sel_mask_u(unsigned long long m, uint32_t if_set, uint32_t if_clear) {
  uint32_t r;
  asm("v_cndmask_b32_e64 %0, %1, %2, %3" : "=v"(r) : "v"(if_clear), "v"(if_set), "s"(m));
  return r;
}

// LDS loads through a 32-bit LDS byte address
typedef __attribute__((address_space(3))) const float4 lds_float4;
__device__ __forceinline__ uint32_t lds_addr(const float4* p) {
  return uint32_t(reinterpret_cast<size_t>((lds_float4*)p));
}
__device__ __forceinline__ float4 lds_load(uint32_t addr) {
  typedef float v4f __attribute__((ext_vector_type(4)));
  typedef __attribute__((address_space(3))) const v4f lds_v4f;
  const v4f r = *(lds_v4f*)(size_t)addr;
  return make_float4(r.x, r.y, r.z, r.w);
}

// keep a per-ray constant in a register (stops the compiler re-deriving it inside the loop: the
// IEEE 1/d per DDA step instead of a register read; v2 of DESIGN.md §6's performance log)
__device__ __forceinline__ float opaque(float x) {
  asm volatile("" : "+v"(x));
  return x;
}

// The DDA loop of RayMarch / RayMarchShadow (voxel.glsl:273-298, :317-382) up to the first event.
// Event: SHADOW -> an opaque voxel (HasVoxel && !transparent); otherwise the sampled byte differs
// from the ray's medium, which covers both the hit (:353) and the leave-transparent case (:357).
// Every float op of a step is the reference's, in its order; only their scheduling differs:
//  - the inner loop exits on a cheap superset of the stop conditions (a sample outside the
//    volume, a byte != medium, the length, the cap); the outer loop then replays the reference's
//    decisions exactly: the event of that iteration, else the next iteration's loop-top tests
//    (length, TestCube — which can only fail after an outside sample — and the cap), and
//    re-enters the inner loop when none fires;
//  - the t update of a step (independent of the voxel) is issued before the voxel-load wait and
//    is simply dead after an event.
template <bool SHADOW, bool EXACT>
__device__ __forceinline__ int dda_walk(const Ctx& c, const f3 pos, const f3 dir, const f3 rcp,
                                        float len0, uint32_t medium, WalkState& w, int& axis_out,
                                        int32_t& vidx_out, uint32_t& v_out) {
  const f3 step = sign3(dir);
  const f3 hs = mk(0.5f * step.x, 0.5f * step.y, 0.5f * step.z);
  f3 t = w.t, cur = w.cur;
  float len = w.len;
  uint32_t it = w.it, ties = w.ties;
  bool check = w.check_cube;
  int result;
  for (;;) {
    // loop-top tests of the reference, in its order: length, TestCube, then our step cap
    if (!(len < c.max_len) || (check && !test_cube(cur, dir, c.fn))) {
      result = WALK_MISS;
      break;
    }
    if (it >= VRT_MAX_STEPS) {
      result = WALK_CAP;
      break;
    }
    // inner loop; live-outs kept in VGPRs (a bool live out of a divergent loop costs SALU mask
    // merges every iteration): the pre-update t (-> crossed axis), the texel coordinates, the raw
    // byte, and pidx_sel = the padded index, or ~0 for an outside sample
    f3 tp;
    uint32_t vi, vj, vk, v_raw, pidx_sel;
    // step counter of this inner loop: wave-uniform (every active lane enters together), so it
    // lives in an SGPR; its bound keeps every lane's total <= VRT_MAX_STEPS, the exact per-lane
    // cap is the outer test above
    const uint32_t k_max = VRT_MAX_STEPS - active_max(it);
    const uint32_t it0 = it;
    uint32_t k = 0;
    for (;;) {
      ++k;
      float tmin;
      if (EXACT) tmin = gmin(t.x, gmin(t.y, t.z));
      else tmin = __builtin_fminf(t.x, __builtin_fminf(t.y, t.z));
      tp = mk(t.x - tmin, t.y - tmin, t.z - tmin);
      len += tmin;
      const float s = len - len0;
      cur = mk(pos.x + s * dir.x, pos.y + s * dir.y, pos.z + s * dir.z);
      const bool ex = tp.x == 0.0f, ey = tp.y == 0.0f, ez = tp.z == 0.0f;
      f3 smp;
      if (EXACT) {
        smp = mk(cur.x + (0.5f * float(ex)) * step.x, cur.y + (0.5f * float(ey)) * step.y,
                 cur.z + (0.5f * float(ez)) * step.z);
      } else {  // same voxel: the +-0 added on an un-crossed axis only flips the sign of a zero
        smp = mk(cur.x + (ex ? hs.x : 0.0f), cur.y + (ey ? hs.y : 0.0f), cur.z + (ez ? hs.z : 0.0f));
      }
      // branch-free fetch: clamp to [0,N] (med3; NaN -> in range), floor; the sample is inside
      // iff clamping left it unchanged (NaN: outside); GL_REPEAT's N -> 0 is in the layout
      const float qx = __builtin_amdgcn_fmed3f(smp.x, 0.0f, c.fn);
      const float qy = __builtin_amdgcn_fmed3f(smp.y, 0.0f, c.fn);
      const float qz = __builtin_amdgcn_fmed3f(smp.z, 0.0f, c.fn);
      const bool inb = (qx == smp.x) & (qy == smp.y) & (qz == smp.z);
      vi = cvt_flr(qx);
      vj = cvt_flr(qy);
      vk = cvt_flr(qz);
      const uint32_t pidx = mad24(mad24(vk, c.p, vj), c.p, vi);
      v_raw = load_u16(c.vox, pidx) & kVoxMask;
      if (ey & ez) ties++;  // intersectionAxis[3]: rare, a skipped branch otherwise
      // t update for the crossed axis (voxel.glsl:296/381), while the load is in flight
      const bool az = ez, ay = ey & !ez, ax = !ey & !ez;  // axis = ez ? 2 : ey ? 1 : 0
      const float pa = az ? pos.z : (ay ? pos.y : pos.x);
      const float da = az ? dir.z : (ay ? dir.y : dir.x);
      const float ca = az ? cur.z : (ay ? cur.y : cur.x);
      // sign(d) on the crossed axis; on the fast path d != 0, so it is copysign(1, d) (one v_bfi)
      const float sa = EXACT ? (az ? step.z : (ay ? step.y : step.x)) : __builtin_copysignf(1.0f, da);
      const float num = (ca + sa) - pa;
      float q;
      if (EXACT) q = num / da;
      else q = div_rn(num, da, az ? rcp.z : (ay ? rcp.y : rcp.x));
      q = q - s;
      t = mk(ax ? q : tp.x, ay ? q : tp.y, az ? q : tp.z);
      pidx_sel = inb ? pidx : ~0u;
      // materialise: no SALU live-out mask for inb (v9, DESIGN.md §6 log: 0.316 -> 0.310 ms with
      // the other live-out masks removed)
      asm volatile("" : "+v"(pidx_sel));
      const bool hit = SHADOW ? (v_raw != 0u && v_raw != 2u) : (v_raw != medium);
      if (!inb | hit | !(len < c.max_len) | (k >= k_max)) break;
    }
    it = it0 + k;
    const bool inb = pidx_sel != ~0u;
    // outside samples read 0 (GetVoxel :151-152)
    const uint32_t v = inb ? v_raw : 0u;
    const bool event = SHADOW ? (v != 0u && v != 2u) : (v != medium);
    if (event) {
      axis_out = tp.z == 0.0f ? 2 : (tp.y == 0.0f ? 1 : 0);
      vidx_out = inb ? canonical_index(c, vi, vj, vk) : -1;
      v_out = v;
      check = !inb;  // on re-entry (new direction after a refraction): re-test iff outside
      result = WALK_EVENT;
      break;
    }
    check = !inb;  // not an event: evaluate the next iteration's loop-top tests
  }
  w.t = t;
  w.cur = cur;
  w.len = len;
  w.it = it;
  w.ties = ties;
  w.check_cube = check;
  return result;
}

// ---------------------------------------------------------------- empty-space step skipping --
//
// The packed volume carries, per voxel v, a skip distance G(v) such that every voxel of a box
// B(v) is empty and inside the volume, where B(v) reaches G voxels ahead of v along the ray's
// direction on every axis (faces (v + c0) + sgn*G, c0 = 0 / 1 for d > 0 / < 0) and at least one
// voxel behind v:
//  - octant layout (N <= 512; 8 volumes, one per direction octant, step s = sign(d)):
//    G(v) = F(v - s) - 1, F(u) = edge of the largest empty in-volume cube anchored at u and
//    extending along s, so B(v) = [v - s, v + (G - 1) s] (capped at kFwdCap - 1, vrt_tuning.h). Looking only
//    ahead, it is far larger than the centred distance behind surfaces: shadow rays leaving the
//    ground and rays moving away from geometry skip up to ~4x fewer sampled steps
//    (scripts/skipsim.py);
//  - single layout (N = 1024, where 8 volumes would overflow 32-bit offsets): G = D, the
//    centred Chebyshev distance to the nearest non-empty voxel or the outside (capped at
//    kDistCap), B(v) = [v - D + 1, v + D - 1]^3.
// Why one voxel behind: on an axis crossed at the sampled step, currentPos = pos + s*dir may round
// to just short of the crossed plane, and a later step that crosses another axis within that
// rounding distance samples floor(currentPos) there, i.e. the voxel behind v on that axis.
// After a sampled step whose texel is empty with G >= 2, an air ray (or a shadow ray) computes
// s_lim, the ray parameter up to which its position provably stays inside B(v) (forward faces
// pulled in by kSkipMargin, far above the float error of cur = pos + s*dir; positions only move
// forward, so the back faces need no test). A step with s < s_lim therefore samples an empty voxel
// inside the volume — no event, no TestCube — and needs only the exact DDA state update; the
// sample, its address and the load are skipped. Every float op that defines the walk's state is
// still executed, in the reference's order, so the walk is bit-identical.
constexpr uint32_t kDistCap = 64;  // (profiles/r01_v32_ab_distance_cap.log: 128/255 add nothing)
static_assert(kDistCap >= 2 && kDistCap <= 255, "D is stored in 8 bits");
constexpr float kSkipMargin = 1.0f / 256.0f;

// LEN0Z: the caller guarantees len0 == +0 (the primary ray, voxel.glsl:430), so
// s = rayLength - ray.rayLength is rayLength itself (x - (+0) == x): one VALU less per step.
// s_init > 0: a first skip window [0, s_init) known from a certified walk of the same ray
// (CertResult::us: every crossing before it settled, each in the volume and not an event), so
// those steps replay only the state update; else the first step samples.
template <bool SHADOW, bool STATS, bool LEN0Z = false>
__device__ __forceinline__ int skip_walk(const Ctx& c, const f3 pos, const f3 dir, const f3 rcp,
                                         float len0, uint32_t medium, WalkState& w, int& axis_out,
                                         int32_t& vidx_out, uint32_t& v_out, float s_init = -1.0f) {
  // fast path: every dir component is non-zero, so sign(d) = copysign(1, d)
  const f3 step = mk(__builtin_copysignf(1.0f, dir.x), __builtin_copysignf(1.0f, dir.y),
                     __builtin_copysignf(1.0f, dir.z));
  const f3 hs = mk(0.5f * step.x, 0.5f * step.y, 0.5f * step.z);
  // skip-box face in travel direction: B = (v + c0) + sgn * (D - margin); c0 = 0 / 1 for d > 0 / < 0
  const f3 c0 = mk(dir.x > 0.0f ? 0.0f : 1.0f, dir.y > 0.0f ? 0.0f : 1.0f, dir.z > 0.0f ? 0.0f : 1.0f);
  const f3 boff = mk((c0.x - pos.x) * rcp.x, (c0.y - pos.y) * rcp.y, (c0.z - pos.z) * rcp.z);
  // the crossed axis' operands per step from this lane's LDS table
  c.ax[0] = make_float4(pos.x, dir.x, rcp.x, step.x);
  c.ax[kAxStride] = make_float4(pos.y, dir.y, rcp.y, step.y);
  c.ax[2 * kAxStride] = make_float4(pos.z, dir.z, rcp.z, step.z);
  uint32_t ax_a0 = lds_addr(c.ax), ax_a1 = ax_a0 + 16u * kAxStride, ax_a2 = ax_a0 + 32u * kAxStride;
  // three VGPRs, not re-derived per step (v34: C4 -2.9 %, C2 -2.7 %,
  // profiles/r01_v34_ab_lds_address_select.log)
  asm volatile("" : "+v"(ax_a0), "+v"(ax_a1), "+v"(ax_a2));
  const bool skip_ok = SHADOW || medium == 0u;
  // this ray's octant volume (its skip distances look along the ray's direction); uniform for
  // shadow rays. Every octant volume holds the same voxel bytes.
  const uint32_t obase =
      ((dir.x < 0.0f ? 1u : 0u) | (dir.y < 0.0f ? 2u : 0u) | (dir.z < 0.0f ? 4u : 0u)) * c.ostride;
  // Skip windows also end where the length test could first fail: s = fl(len - len0) is
  // monotone in len, so s < fl(max_len - len0) implies len < max_len (NaN: no window at all).
  const float s_len = LEN0Z ? c.max_len : c.max_len - len0;
  float s_first = s_init > 0.0f ? __builtin_fminf(s_init, s_len) : -1.0f;
  f3 t = w.t;
  float len = w.len;
  uint32_t it = w.it, ties = w.ties;
  bool check = w.check_cube;
  int result;
  constexpr uint32_t kOutside = 0x100u;
  for (;;) {
    // loop-top tests of the reference, in its order: length, TestCube, then our step cap.
    // check is only set after an outside sample; currentPos is that step's (len unchanged since),
    // recomputed with the same two ops rather than carried through the step loop
    if (!(len < c.max_len)) {
      result = WALK_MISS;
      break;
    }
    if (check) {
      const float sc = LEN0Z ? len : len - len0;
      if (!test_cube(mk(pos.x + sc * dir.x, pos.y + sc * dir.y, pos.z + sc * dir.z), dir, c.fn)) {
        result = WALK_MISS;
        break;
      }
    }
    if (it >= VRT_MAX_STEPS) {
      result = WALK_CAP;
      break;
    }
    const uint32_t k_max = VRT_MAX_STEPS - active_max(it);
    const uint32_t it0 = it;
    uint32_t k = 0;
    // this lane's step count at its exit: set by the stopping (sampled) step; lanes that run
    // into the uniform bound leave with k == k_max. Keeps k from being copied to a VGPR per step.
    uint32_t k_exit = k_max;
    // recorded by the stopping (sampled) step only; lanes that leave on the bound: no event
    uint32_t x_v = SHADOW ? 0u : medium, x_axis = 0u, x_out = 0u;  // x_out: sample was outside
    int32_t x_vidx = -1;
    float s_lim = s_first;  // no skip window yet (-1: the first step samples), or the certified prefix
    s_first = -1.0f;
    for (;;) {
      if (k >= k_max) break;  // wave-uniform step bound (scalar branch)
      ++k;
      const float tmin = __builtin_fminf(t.x, __builtin_fminf(t.y, t.z));
      const f3 tp = mk(t.x - tmin, t.y - tmin, t.z - tmin);
      len += tmin;
      const float s = LEN0Z ? len : len - len0;
      const bool ey = tp.y == 0.0f, ez = tp.z == 0.0f;
      if (STATS) ties = add_if_both(ties, ey, ez);  // intersectionAxis[3] (counter/flag only)
      // t update for the crossed axis (voxel.glsl:296/381)
      // crossed axis: z if ez (index 2, and 3 clamped), else y if ey, else x. Selected with the
      // compare masks kept in SGPRs (the compiler re-derives !ez with another v_cmp otherwise).
      const unsigned long long mey = __builtin_amdgcn_ballot_w64(ey);
      const unsigned long long mez = __builtin_amdgcn_ballot_w64(ez);
      // the crossed axis' entry address straight from the masks: two v_cndmask, no index math
      const float4 ae = lds_load(sel_mask_u(mez, ax_a2, sel_mask_u(mey, ax_a1, ax_a0)));
      const float pa = ae.x, da = ae.y, ra = ae.z, sa = ae.w;
      const float ca = pa + s * da;  // == cur on that axis: the same two ops
      const float num = (ca + sa) - pa;
      const float q = div_rn(num, da, ra) - s;
      t = mk(sel_mask(mey | mez, tp.x, q), sel_mask(mey & ~mez, q, tp.y), sel_mask(mez, q, tp.z));
      // issue the t update before the sample's load wait (v2: its ALU then overlaps the load)
      asm volatile("" :: "v"(t.x), "v"(t.y), "v"(t.z));
      if (!(s < s_lim)) {  // a sampled step (GetVoxel, voxel.glsl:149-154)
        const f3 cur = mk(pos.x + s * dir.x, pos.y + s * dir.y, pos.z + s * dir.z);
        const bool ex = tp.x == 0.0f;
        const f3 smp = mk(cur.x + (ex ? hs.x : 0.0f), cur.y + (ey ? hs.y : 0.0f),
                          cur.z + (ez ? hs.z : 0.0f));
        const float qx = __builtin_amdgcn_fmed3f(smp.x, 0.0f, c.fn);
        const float qy = __builtin_amdgcn_fmed3f(smp.y, 0.0f, c.fn);
        const float qz = __builtin_amdgcn_fmed3f(smp.z, 0.0f, c.fn);
        const bool inb = (qx == smp.x) & (qy == smp.y) & (qz == smp.z);
        const uint32_t vi = cvt_flr(qx), vj = cvt_flr(qy), vk = cvt_flr(qz);
        const uint32_t pidx = mad24(mad24(vk, c.p, vj), c.p, vi);
        const uint32_t packed = load_u16_at(c.vox, pidx, obase);
        const uint32_t v_raw = packed & kVoxMask;
        const uint32_t dist = packed >> kDistShift;
        const uint32_t v_ev = inb ? v_raw : kOutside;
        // exit parameter of the pulled-in box face per axis, ((v + c0) + sgn*fd - pos) * rcp,
        // as v*rcp + (fd*|rcp| + boff): only has to be conservative (error <~ 4e-4 |rcp| for
        // N <= 1024, against the 1/256 * |rcp| face margin), so it may contract
        const float fd = float(dist) - kSkipMargin;
        const float lx = __builtin_fmaf(float(vi), rcp.x, __builtin_fmaf(fd, __builtin_fabsf(rcp.x), boff.x));
        const float ly = __builtin_fmaf(float(vj), rcp.y, __builtin_fmaf(fd, __builtin_fabsf(rcp.y), boff.y));
        const float lz = __builtin_fmaf(float(vk), rcp.z, __builtin_fmaf(fd, __builtin_fabsf(rcp.z), boff.z));
        const bool open = skip_ok & inb & (v_raw == 0u) & (dist >= 2u);
        s_lim = open ? __builtin_fminf(__builtin_fminf(lx, ly), __builtin_fminf(lz, s_len)) : -1.0f;
        // stop the inner loop on: outside sample, a byte that is an event, the length. Only a
        // sampled step can stop it: a skipped one reads an empty in-volume texel and has
        // s < s_len, hence len < max_len (see s_len).
        const bool stop = SHADOW ? ((v_ev & ~2u) != 0u) : (v_ev != medium);
        if (stop | !(len < c.max_len)) {
          k_exit = k;
          x_v = inb ? v_raw : 0u;  // outside samples read 0 (GetVoxel :151-152)
          x_out = inb ? 0u : 1u;
          x_axis = axis_index(mey, mez);
          x_vidx = inb ? int32_t(canonical_index(c, vi, vj, vk)) : -1;
          // integers in VGPRs: a bool carried out of a divergent loop costs SALU mask merges
          // (v28 register-lean walk: 0.2146 -> 0.2038 ms with 8 waves, DESIGN.md §6 log)
          asm volatile("" : "+v"(k_exit), "+v"(x_v), "+v"(x_axis), "+v"(x_vidx), "+v"(x_out));
          break;
        }
      }
    }
    it = it0 + k_exit;
    const bool event = SHADOW ? (x_v != 0u && x_v != 2u) : (x_v != medium);
    asm volatile("" : "+v"(x_out));  // (v28, as above: kept in a VGPR across the exit)
    check = x_out != 0u;
    if (event) {  // events only come from sampled steps
      axis_out = int(x_axis);
      vidx_out = x_vidx;
      v_out = x_v;
      result = WALK_EVENT;
      break;
    }
  }
  const float s_end = LEN0Z ? len : len - len0;  // currentPos of the last step (the hit point on an event)
  w.t = t;
  w.cur = mk(pos.x + s_end * dir.x, pos.y + s_end * dir.y, pos.z + s_end * dir.z);
  w.len = len;
  w.it = it;
  w.ties = ties;
  w.check_cube = check;
  return result;
}

// RayMarch walk: per-ray reciprocals (RN(1/d), kept opaque so they stay loop-invariant).
// (The len0 == 0 specialisation of skip_walk measured neutral: r01_v37_ab_axis_major_len0_cmpt;
// round 4's pipelined, speculative, register-select and prefetching walks all measured slower
// for the exact pass's sparse batches and were removed: DESIGN.md §6, git history before r05.)
template <bool STATS>
__device__ __forceinline__ int walk_ray(const Ctx& c, const f3 pos, const f3 dir, float len0,
                                        uint32_t medium, WalkState& w, int& axis, int32_t& vidx,
                                        uint32_t& v, float s_init = -1.0f) {
  if (__builtin_expect(fast_path_ok(dir), 1)) {
    // (fast_path_ok: every |d| in [2^-64, 1e4], so rcp_newton is RN(1/d))
    const f3 rcp = mk(opaque(rcp_newton(dir.x)), opaque(rcp_newton(dir.y)), opaque(rcp_newton(dir.z)));
    return skip_walk<false, STATS>(c, pos, dir, rcp, len0, medium, w, axis, vidx, v, s_init);
  }
  return dda_walk<false, true>(c, pos, dir, dir, len0, medium, w, axis, vidx, v);
}

// RayMarchShadow walk: the direction is normalize(u_SunDir) for every ray (uniform constants)
template <bool STATS>
__device__ __forceinline__ int walk_shadow(const Ctx& c, const f3 pos, float len0, WalkState& w) {
  int axis;
  int32_t vidx;
  uint32_t v;
  if (__builtin_expect(fast_path_ok(c.sun_n), 1))
    return skip_walk<true, STATS>(c, pos, c.sun_n, c.sun_rcp, len0, 0u, w, axis, vidx, v);
  return dda_walk<true, true>(c, pos, c.sun_n, c.sun_n, len0, 0u, w, axis, vidx, v);
}

// GetReflectionRay (voxel.glsl:203-215)
// GetColor (:174-182). Textured: GetTextureCoordinate (:167-172) on the hit's face plane
// intersectionAxis[axis][1..2] (:93), then texture(u_TextureUnit, uv): NEAREST + REPEAT,
// i = floor(u * S) mod S (GL 4.5 §8.14.2; NaN -> 0 via v_cvt_flr), texels b / 255.
template <bool TEX>
__device__ __forceinline__ float4 get_color(const Ctx& c, const Hit& h) {
  const uint32_t m = mat_id(h.voxel);
  if (!TEX) return mat_color(m);
  const float px = h.axis == 0 ? h.point.z : h.point.x;   // intersectionAxis[a][1]
  const float py = h.axis == 2 ? h.point.y : (h.axis == 1 ? h.point.z : h.point.y);  // [a][2]
  const float fx = px - floorf(px), fy = py - floorf(py);
  const float tx = ((fx + float(mat_tex_x(m))) * c.atlas_fts) / c.atlas_fs;
  const float ty = (((1.0f - fy) + float(mat_tex_y(m))) * c.atlas_fts) / c.atlas_fs;
  const float u = tx, v = 1.0f - ty;
  const uint32_t i = cvt_flr(u * c.atlas_fs) & c.atlas_mask;
  const uint32_t j = cvt_flr(v * c.atlas_fs) & c.atlas_mask;
  const uint32_t t = c.atlas[j * (c.atlas_mask + 1u) + i];
  return make_float4(float(t & 0xFFu) / 255.0f, float((t >> 8) & 0xFFu) / 255.0f,
                     float((t >> 16) & 0xFFu) / 255.0f, float(t >> 24) / 255.0f);
}

__device__ __forceinline__ Ray reflection_ray(const Ctx& c, const Ray& ray, const Hit& h) {
  Ray r;
  r.voxel = 0;
  r.pos = h.point;
  r.dir = randomize(reflect3(ray.dir, h.normal), h.point, c.refl_noise, c.time);
  r.len = h.len;
  r.energy = ray.energy * (1.0f - dot3(mk(-h.normal.x, -h.normal.y, -h.normal.z), ray.dir));
  r.rdepth = ray.rdepth + 1;
  r.tdepth = ray.tdepth;
  return r;
}

// GetRefractionRay (voxel.glsl:217-246)
template <bool TEX>
__device__ __forceinline__ Ray refraction_ray(const Ctx& c, const Ray& ray, const Hit& h, Counters& k) {
  const uint32_t outv = get_voxel(c, h.point + h.normal * 0.5f);
  const uint32_t inv = get_voxel(c, h.point - h.normal * 0.5f);
  k.c[VRT_CNT_REFRACTION_PROBES]++;
  const float eta = mat_refr(outv) / mat_refr(inv);
  Ray r;
  r.voxel = h.voxel;
  r.pos = h.point;
  r.dir = refract3(normalize3(ray.dir), h.normal, eta);
  if (r.dir.x == 0.0f && r.dir.y == 0.0f && r.dir.z == 0.0f) {  // total internal reflection
    r = reflection_ray(c, ray, h);
    r.voxel = ray.voxel;
    r.energy = ray.energy;
  } else {
    r.dir = randomize(r.dir, r.pos, c.refr_noise, c.time);
    r.energy = ray.energy;
    if (ray.voxel == 0) r.energy *= 1.0f - get_color<TEX>(c, h).w;  // :239-240
  }
  r.len = h.len;
  r.rdepth = ray.rdepth;
  r.tdepth = ray.tdepth + 1;
  return r;
}

__device__ __forceinline__ void walk_init(WalkState& w, const Ray& ray) {
  w.len = ray.len;
  w.cur = ray.pos;
  w.t = initial_t(ray.dir, ray.pos, ray.pos);
  w.it = 0;
  w.ties = 0;
  w.check_cube = true;
}

__device__ __forceinline__ void walk_account(const WalkState& w, int r, int steps_slot,
                                             Counters& k, uint32_t& steps, uint32_t& flags) {
  steps += w.it;
  k.c[steps_slot] += w.it;
  k.c[VRT_CNT_TIE3] += w.ties;
  if (w.ties) flags |= VRT_HIT_FLAG_TIE3;
  if (r == WALK_CAP) {
    k.c[VRT_CNT_STEP_CAP]++;
    flags |= VRT_HIT_FLAG_STEP_CAP;
  }
}

// RayMarchShadow (voxel.glsl:259-300): true when an opaque voxel blocks the sun.
template <bool STATS>
__device__ __forceinline__ bool march_shadow(const Ctx& c, const Ray& ray, Counters& k, uint32_t& steps,
                             uint32_t& flags) {
  WalkState w;
  walk_init(w, ray);
  const int r = walk_shadow<STATS>(c, ray.pos, ray.len, w);
  walk_account(w, r, VRT_CNT_SHADOW_STEPS, k, steps, flags);
  return r == WALK_EVENT;
}

// RayMarch (voxel.glsl:302-384); `ray` is inout (in-volume refraction rewrites it, :361)
// PRIMARY: the primary ray (len 0, medium air: every event is a hit, no in-volume refraction)
// s_init (PRIMARY only): the certified prefix of the primary walk (skip_walk)
template <bool STATS, bool TEX, bool PRIMARY = false>
__device__ __forceinline__ Hit march(const Ctx& c, Ray& ray, Counters& k, uint32_t& steps, uint32_t& flags,
                     float s_init = -1.0f) {
  Hit h;
  h.found = false;
  h.vidx = -1;
  h.len = 0.0f;
  h.voxel = 0;
  h.point = mk(0.0f, 0.0f, 0.0f);
  h.normal = h.point;
  h.axis = 0;
  WalkState w;
  walk_init(w, ray);
  uint32_t medium = ray.voxel;
  int internal = 0;
  int r;
  for (;;) {
    int axis;
    int32_t vidx;
    uint32_t v;
    r = walk_ray<STATS>(c, ray.pos, ray.dir, ray.len, PRIMARY ? 0u : medium, w, axis, vidx, v,
                        PRIMARY ? s_init : -1.0f);
    if (r != WALK_EVENT) break;
    f3 normal = mk(0.0f, 0.0f, 0.0f);
    set_comp(normal, axis, -gsign(comp(ray.dir, axis)));
    // HasVoxel(voxel) && voxel != rayVoxel (:353); a primary ray's medium is air, so its
    // every event is a hit
    if (PRIMARY || v != 0u) {
      h.found = true;
      h.voxel = v;
      h.vidx = vidx;
      h.point = w.cur;
      h.len = w.len;
      h.normal = normal;
      h.axis = axis;
      break;
    }
    // rayVoxel != 0 && voxel == 0: leaving a transparent voxel, refract in place (:357-380)
    Hit e;
    e.found = true;
    e.voxel = 0;
    e.vidx = vidx;
    e.point = w.cur;
    e.len = w.len;
    e.normal = normal;
    e.axis = axis;
    const f3 old_dir = ray.dir;
    ray = refraction_ray<TEX>(c, ray, e, k);
    ray.tdepth--;
    if (ray.voxel == medium) {
      internal++;
      if (internal > 10) {
        ray.dir = old_dir;
        ray.voxel = 0;
      }
    }
    medium = ray.voxel;
    w.t = initial_t(ray.dir, w.cur, ray.pos);
    const f3 step = sign3(ray.dir);
    const float q = ((comp(w.cur, axis) + comp(step, axis)) - comp(ray.pos, axis)) /
                        comp(ray.dir, axis) - (w.len - ray.len);
    set_comp(w.t, axis, q);
  }
  walk_account(w, r, VRT_CNT_DDA_STEPS, k, steps, flags);
  return h;
}

// Brightness of a hit that is not in shadow (voxel.glsl:405-409)
template <bool TEX>
__device__ __forceinline__ float lit_brightness(const Hit& h, const f3 sun_dir, const f3 ray_dir) {
  const uint32_t m = mat_id(h.voxel);
  const float diffuse = mat_kd(m) * gmax(dot3(h.normal, sun_dir), 0.0f);
  const float specular =
      mat_ks(m, TEX) * gpow(gmax(dot3(reflect3(sun_dir, h.normal), ray_dir), 0.0f), mat_exp(m, TEX));
  return kAmbient + diffuse + specular;
}

// RayColor (:184-188)
template <bool TEX>
__device__ __forceinline__ void apply_hit_color(const Ctx& c, const Hit& h, float energy,
                                                float brightness, f3& color) {
  const float4 col = get_color<TEX>(c, h);
  color.x = mixf(color.x, col.x * col.w * brightness, energy);
  color.y = mixf(color.y, col.y * col.w * brightness, energy);
  color.z = mixf(color.z, col.z * col.w * brightness, energy);
}

// GetSkyboxColor (:386-393), then the second mix at :420
// FAR (the certified pass's primary misses, cert_pixel<LEAN>): the sun disc without its log and exp where no
// lane of the wave that is here looks within 41 degrees of the sun (a ballot: the branch is wave-uniform).
// With d = dot(sun, u): for d in [-0, 0.75] the power is +0 (400 log2(0.75) = -166 is far below the smallest
// denormal's exponent; log2(+-0) = -inf), and 10 * +0 = +0; for d < 0 or NaN it is NaN, which both gmax below
// drop, whatever its payload (their other operands are no NaN: u is a certified ray's direction). Exhaustive
// over d: vrt_debug_pow_forms, tests/test_gpu_pow_forms.py. The power itself keeps the library's forms: near
// the sun its denormal results reach the float frame.
template <bool FAR = false>
__device__ __forceinline__ void apply_sky_color(const Ctx& c, const Ray& ray, f3& color) {
  const f3 u = normalize3(ray.dir);
  const float d = dot3(c.sun_n, u);
  float sun;
  if (FAR && __ballot(d > 0.75f) == 0ull)
    sun = d >= 0.0f ? 0.0f : __builtin_nanf("");
  else
    sun = 10.0f * gpow(d, 400.0f);
  const float grad = (u.y + 1.0f) * 0.5f;
  const float sy = c.sky_sy;  // gmax(u_SunDir.y, 0), precomputed (a wave-uniform constant)
  const f3 sk = mk(gmax(0.0f, sun) * sy, gmax(grad * 0.75f, sun) * sy, gmax(grad, 0.0f) * sy);
  const float a1 = 1.0f - ray.energy;
  const f3 s1 = mk(mixf(sk.x, color.x, a1), mixf(sk.y, color.y, a1), mixf(sk.z, color.z, a1));
  color = mk(mixf(s1.x, color.x, a1), mixf(s1.y, color.y, a1), mixf(s1.z, color.z, a1));
}

__device__ __forceinline__ int cert_shadow_exact(const Ctx& c, const Hit& h);

// TraceWithShadow's colour update (voxel.glsl:395-423) for the exact march's result h. CSH
// (stats-free colour-only): the shadow bit by a certified walk from the exact hit point when it
// settles it (cert_shadow_exact), and no shadow walk when it cannot change the brightness
// (lit == ambient).
template <bool STATS, bool TEX, bool CSH>
__device__ __forceinline__ void shade(const Ctx& c, const Ray& ray, const Hit& h, f3& color, Counters& k,
                                      uint32_t& steps, uint32_t& flags) {
  static_assert(!CSH || !STATS, "certified shadows in stats-free instances only");
  if (h.found) {
    Ray sr;  // GetShadowRay (:191-201)
    sr.voxel = h.voxel;
    sr.pos = h.point;
    sr.dir = c.sun_n;
    sr.len = h.len;
    sr.energy = ray.energy;
    sr.rdepth = 0;
    sr.tdepth = 0;
    float brightness;
    if (CSH) {
      const float lit = lit_brightness<TEX>(h, c.sun_n, ray.dir);
      int blocked = 0;
      if (lit != kAmbient && !shadow_free_hit(h.voxel, TEX)) {
        blocked = cert_shadow_exact(c, h);
        if (blocked < 0) blocked = march_shadow<STATS>(c, sr, k, steps, flags) ? 1 : 0;
      }
      brightness = blocked ? kAmbient : lit;
    } else {
      k.c[VRT_CNT_SHADOW_RAYS]++;
      const bool in_shadow = march_shadow<STATS>(c, sr, k, steps, flags);
      brightness = in_shadow ? kAmbient : lit_brightness<TEX>(h, sr.dir, ray.dir);
    }
    apply_hit_color<TEX>(c, h, ray.energy, brightness, color);
  } else {
    apply_sky_color(c, ray, color);
  }
}

// TraceWithShadow (voxel.glsl:395-423) and the colour update it performs
template <bool STATS, bool TEX, bool PRIMARY = false, bool CSH = false>
__device__ __forceinline__ Hit trace_with_shadow(const Ctx& c, Ray& ray, f3& color, Counters& k,
                                                 uint32_t& steps, uint32_t& flags, float s_init = -1.0f) {
  const Hit h = march<STATS, TEX, PRIMARY>(c, ray, k, steps, flags, s_init);
  shade<STATS, TEX, CSH>(c, ray, h, color, k, steps, flags);
  return h;
}

}  // namespace vrt

#endif  // VRT_WALK_H
