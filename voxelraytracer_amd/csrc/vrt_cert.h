// vrt_cert.h — the certified walks and nothing else: cert_walk, the certified starts, continuations and
// bounce trees, texel certification and cert_pixel. Includes vrt_walk.h (and through it vrt_diag.h: CTRACE, CERT_DIAG).
#ifndef VRT_CERT_H
#define VRT_CERT_H

#include "vrt_walk.h"

namespace vrt {

// ------------------------------------------------------------ certified walks (stats-free) --
//
// The colour-only image depends on a primary walk only through its outcome — miss, or the first
// event's byte and face axis — and on a shadow walk only through blocked / not blocked
// (voxel.glsl:395-423: no hit point, length or texel index enters the colour of a non-glass hit;
// the sky colour depends on the direction alone). The exact walk (skip_walk) replays every DDA
// step's float state to be bit-identical; the CERTIFIED walk below instead follows the real ray
// with a float DDA that jumps through the empty boxes of the octant distance field, and returns
// the exact walk's outcome only when no rounding of the exact walk can change it:
//  - the exact walk's parameter at any plane crossing differs from the real one by at most
//    gam_b(u) (`cert_gamma`): its len accumulates at most u*|d|_1 + 3 non-zero steps, each adding
//    <= 2^-24 len; each t is re-anchored from currentPos (roundings of magnitude <= N + 2, times
//    1/|d_b|) and then decremented at most K times; zero-length tie steps add no rounding;
//  - crossings of two axes closer than gam_a + gam_b may come in either order or as a tie: the
//    cells the exact walk could sample instead (`alternatives`) must be non-events, else UNSURE;
//  - an event cell is a certified hit only if its entry crossing is isolated (the exact walk
//    then enters it across the same face, index = that axis) and the length test cannot stop
//    the walk first; a walk that leaves the volume or whose previous crossing lies beyond the
//    length budget (by more than the bound) is a certified miss;
//  - cells with an index N are outside on the path (the exact walk reads the GL_REPEAT plane N
//    only at a coordinate exactly N, i.e. at a near-edge crossing, where the alternatives read
//    the padded layout's plane N).
// UNSURE rays (~0.2 % of pixels at the BASELINE configs, scripts/certsim.py) and every pixel
// whose primary hit is glass (its secondary rays start at the exact hit point) take the exact
// path. Only the stats-free colour-only instance uses it: hit records and counters need the
// exact walk, and textured shading reads the hit point.

enum : int { CERT_MISS = 0, CERT_HIT = 1, CERT_UNSURE = 2 };
constexpr int kCertRun = 3;  // inside cert_walk's loop: the walk goes on
constexpr float kCertMargin = 1.0f / 64.0f;  // jump boxes' forward faces pulled in (position)
constexpr int kCertMaxIter = 1024;
constexpr float kCertMaxOrigin = 4e-3f;  // parameter uncertainty of a secondary start beyond which: unsure

struct CertResult {
  int res;
  uint32_t byte;
  int axis;
  int cx, cy, cz;  // hit cell
  float u;         // crossing parameter of the hit
  float eu;        // bound of the exact walk's parameter error there
  // every step of the exact walk with parameter s < us samples an in-volume cell that is not an
  // event (the certified crossings before the last one the walk settled); 0: none known
  float us;
  CERT_DIAG_ONLY(int iters;)
};

__device__ __forceinline__ uint32_t cell_texel(const Ctx& c, int i, int j, int k, uint32_t obase) {
  return load_u16_at(c.vox, mad24(mad24(uint32_t(k), c.p, uint32_t(j)), c.p, uint32_t(i)), obase);
}
// texel of a cell on the certified path: cells outside [0, N)^3 read 0 (empty, G = 0)
__device__ __forceinline__ uint32_t path_texel(const Ctx& c, int i, int j, int k, uint32_t obase) {
  const uint32_t n = uint32_t(c.n);
  if (uint32_t(i) >= n || uint32_t(j) >= n || uint32_t(k) >= n) return 0u;
  return cell_texel(c, i, j, k, obase);
}
// texel of the cell a crossing of the certified path enters from an in-volume cell: only the
// crossed axis' index can be outside [0, N), at -1 or N, so one unsigned maximum is that axis'
// test. No branch around the load: an outside cell reads texel 0 of the ray's octant volume (a -1
// index has no address in the padded layout), so every address formed lies inside the volume, and
// the result is replaced by kTexOutside: byte 0 (empty) as path_texel's, plus a bit above the
// texel's 16 that the walk's MISS test reads (cross_outside) instead of selecting the crossed
// axis' index again. Kept opaque: one VGPR compare there, no lane mask live across the crossing.
constexpr uint32_t kTexOutside = 0x10000u;
__device__ __forceinline__ uint32_t cross_texel(const Ctx& c, int i, int j, int k, uint32_t obase) {
  const bool outside = max(max(uint32_t(i), uint32_t(j)), uint32_t(k)) >= uint32_t(c.n);
  const uint32_t idx = mad24(mad24(uint32_t(k), c.p, uint32_t(j)), c.p, uint32_t(i));
  uint32_t t = load_u16_at(c.vox, outside ? 0u : idx, obase);
  t = outside ? kTexOutside : t;
  asm volatile("" : "+v"(t));
  return t;
}
__device__ __forceinline__ bool cross_outside(uint32_t tex) { return tex >= kTexOutside; }
// path_texel without its branch, for a walk's start (the diagonal neighbour of a cell in the volume:
// any of its indices may be -1 or N): an outside cell loads texel 0 of the octant volume, as in
// cross_texel, and reads 0. The load is issued at once, not behind a lane mask.
__device__ __forceinline__ uint32_t start_texel(const Ctx& c, int i, int j, int k, uint32_t obase) {
  const bool outside = max(max(uint32_t(i), uint32_t(j)), uint32_t(k)) >= uint32_t(c.n);
  const uint32_t idx = mad24(mad24(uint32_t(k), c.p, uint32_t(j)), c.p, uint32_t(i));
  const uint32_t t = load_u16_at(c.vox, outside ? 0u : idx, obase);
  return outside ? 0u : t;
}
// byte of a cell the exact walk might sample at a near-edge crossing (plane N: GL_REPEAT copy)
__device__ __forceinline__ uint32_t alt_byte(const Ctx& c, int i, int j, int k, uint32_t obase) {
  const uint32_t n = uint32_t(c.n);
  if (uint32_t(i) > n || uint32_t(j) > n || uint32_t(k) > n) return 0u;
  return cell_texel(c, i, j, k, obase) & kVoxMask;
}
// an event of the exact walk: shadow rays stop at opaque bytes (not air, not glass), other rays
// at any byte other than their medium's (voxel.glsl:353, :357)
template <bool SHADOW>
__device__ __forceinline__ bool cert_event(uint32_t b, uint32_t medium) {
  return SHADOW ? (b & ~2u) != 0u : b != medium;
}

// What the certified pass (LEAN) hands a walk of its prologue, so that the walk does not form it again.
// CertStartK (the primary walk): the start's sign-folded position Ps_b = s_b P_b, its floor plus one
// fl1_b = fl_b + 1 (exact: an integer far below 2^24) and the sign masks m_b (0 moving up, ~0 moving down),
// as cert_pixel's merged start predicate computed them; the start cell is int(fl_b) ^ m_b. The first planes
// are then (fl_b + 1 - Ps_b) |1/d_b|, the landing form of the loop (proved there: bit for bit (float(c_b +
// u_b) - P_b) rcp_b for a cell in the volume), and fl_b + 1 > Ps_b for every float (fl_b = floor(Ps_b) <=
// Ps_b), so sig_b >= 0: the loop's precondition "no plane behind the start" holds by construction. (With the
// launch's start cell proved on the host, KArgs::setup & kSetupCell, fl1_b is a select of two launch
// constants; fl_b < Ps_b < fl_b + 1 is then part of the proof.)
// b0, U2: the launch's k24 (3 fn + 11) and max_len + 2 (KArgs::walk_b0, max_len2), which the walk would form.
struct CertStartK {
  f3 Ps, fl1;
  int mx, my, mz;
  float b0, U2;
};
// CertShadowK (the shadow walk of a primary hit, cert_shade_hit<.., KAX>): the first planes sig_b = (float(c_b +
// u_b) - X_b) rcp_b as cert_start_sun formed them for its lead test: the walk's own expression on the walk's
// own operands (the shadow origin X, the start cell, sun_rcp, u_b = sun_step[b] > 0), so the walk takes the
// values instead of twelve more instructions: they are the walk's own bit for bit, and nothing it assumes
// about its start changes.
struct CertShadowK {
  f3 sig;
};
// The launch's arguments read again where the certified pass (LEAN) first needs them, after the
// primary walk: KArgs is the kernels' first argument, at offset 0 of the kernarg segment, and the
// pointer is kept opaque so that the scalar loads through it are not hoisted back above the walk. The
// sun, the sky factor and the atlas constants copied into Ctx before the primary ray (init_ctx) were
// 13 SGPRs live across the primary walk, and the frame's outputs six more across both walks: the
// budget the certified pass's SGPR spills came from.
typedef const __attribute__((address_space(4))) KArgs LateKArgs;
__device__ __forceinline__ LateKArgs* late_kargs() {
  LateKArgs* ka = (LateKArgs*)__builtin_amdgcn_kernarg_segment_ptr();
  asm volatile("" : "+s"(ka));
  return ka;
}
// The shadow walk's functions of the sun alone are such arguments (KArgs::sun_*, formed once per launch
// on the host, sun_consts in vrt_launch_consts.cpp: IEEE single operations in the kernel's order, no
// contraction): cert_shade_hit<.., KAX> reads them through a LateKArgs pointer and hands it on to its
// cert_walk<.., KSUN>. sun_ok is fast_path_ok(sun_n); the other fields mean something only then.

// Certified walk from P along D (every |d| in the fast-path range) with rcp ~ 1/D (a few ulp
// suffice: the walk's own rounding is inside the 4e-5 allowance of the bound), starting in cell
// (cx, cy, cz) inside the volume. U = max_len - len0: the exact walk samples the crossing at u iff
// its len before that step is < max_len. e0: parameter uncertainty of the start (a shadow origin
// is the exact primary hit point, known to +-e0 along the primary); ed: per-axis crossing-order
// uncertainty from it; len0b: bound of len0. No crossing lies behind the start, so the start
// cell's box need not cover a cell behind it: it is read from the diagonal neighbour's texel,
// G(v + s) = F(v) - 1, i.e. the box [v, v + G s].
// LEAN: the certified pass's walks (render_kernel's DEFER instances, which run without scratch):
// the same walk with the start's and the landing's texel loaded unguarded, the crossing's texel
// without a branch and the planes after a jump from the floored floats; texels, cells and planes
// are the guarded form's, bit for bit. The other instances keep the guarded forms: they sit at
// their register limit, and the lean forms moved their scratch use up.
// ED false: the caller's ed is zero (a primary ray, a ray from an exact origin) and is not added.
//
// The bound is evaluated factored by what depends on the axis, gam_b(u) = A(u) + |1/d_b| B(u) +
// ed_b, and the jump test as min_b(sig_b + (fg1 - B) |1/d_b| - ed_b) - A without a test of G; the
// landing coordinate is one fma. gam, the jump parameter uj and the landing coordinate are therefore
// not the values of the per-axis form gam_b = (q2 u + q1_b) u + q0_b (a few 2^-24 relative apart:
// tests/test_cert_bound_forms.py), and the walk is sound by the argument, not by equality:
//  - every term of the bound is non-negative (|d|_1, len0b, e0, ed_b, N, |1/d_b| and u = max(s1, 0)
//    are), so A, B and gam_b are sums and products of non-negative floats: no cancellation, each of
//    the at most six roundings on a path changes the value by at most 2^-24 relative, and the float
//    gam_b is within a few 2^-24 relative of the real polynomial. That polynomial carries a factor 2
//    on every 2^-24 term and the 4e-5 constant: a few 2^-24 of the k24 part is nothing against its
//    half, and a few 2^-24 of the rest (<= 4e-5 + e0 + ed_b < 1.3e-2: under 5e-9) nothing against
//    half the k24 part (>= 2^-24 (3N + 11 + 18 / |d|_1) > 3e-6). The float value stays above the
//    bound with 2^-24 for k24;
//  - (fg1 - B) |1/d_b|: fg1 - B rounds by at most 2^-24 max(G, B), which moves the product by
//    2^-24 G |1/d_b| (<= 8e-6 |1/d_b|: G <= 128) or by 2^-24 of B |1/d_b| (inside the factor 2 as
//    above); the fma rounds once at magnitude <= |sig_b| + G |1/d_b|, the subtractions of ed_b and
//    A once each at no more: a few ulps of ~2000 |1/d_b| at most (N = 1024), 4e-4 |1/d_b|, the
//    margin's margin argument made for l_b below, or 2^-24 relative of A where A dominates (the
//    factor 2 again). The jump parameter stays below min_b(l_b - gam_b) evaluated exactly with
//    half of kCertMargin and the bound with 2^-24 for k24 (the CPU test asserts exactly that);
//  - the landing coordinate fma(uj, |d_b|, Ps_b) has one rounding (<= 2^-14 cell at |x| <= 2^10 +
//    2) where the product and sum had two: the landing load's argument holds a fortiori;
//  - G < 2 (G = 0: a cell without a box or outside the volume; G = 1, also the start texel's + 1
//    over such a cell): fg1 = G - 65/64 <= -1/64 exactly, B >= 0, so fg1 - B rounds to a negative
//    float; sig_b plus a negative product rounds to at most sig_b (rounding is monotone, sig_b a
//    float); subtracting ed_b >= 0, taking the minimum (<= s1) and subtracting A >= 0 keep it at most
//    s1: `uj > s1` is false, as the test `G >= 2` decided before. An infinite or NaN A or B (never
//    at fast-path directions) fails the compare too: no jump.
// The two lattice cameras of DESIGN.md §10 (certified trees) are not touched by this.
// KSUN (LEAN): the direction is the sun and sk holds its launch constants (sh0: the caller's first planes too).
// A template flag, not a test of sk: the late pointer is opaque (late_kargs), so `sk != nullptr` was decided
// by every wave, in scalar branches around each constant and nine per-lane selects of wave-uniform values.
template <bool SHADOW, bool LEAN = false, bool ED = true, bool KSUN = false>
__device__ __forceinline__ CertResult cert_walk(const Ctx& c, const f3 P, const f3 D, const f3 rcp, const float U,
                                int cx, int cy, int cz, const float e0, const f3 ed,
                                const float len0b, const uint32_t medium, const uint32_t tex0 = ~0u,
                                const CertStartK* __restrict__ st0 = nullptr,
                                LateKArgs* sk = nullptr, const CertShadowK* __restrict__ sh0 = nullptr) {
  static_assert(!KSUN || (LEAN && SHADOW), "the sun's launch constants: the certified pass's shadow walks");
  CertResult r;
  r.res = CERT_UNSURE;
  r.byte = 0u;
  r.axis = 0;
  r.cx = r.cy = r.cz = 0;
  r.u = 0.0f;
  r.eu = 0.0f;
  r.us = 0.0f;
  // (sk: the shadow walk's direction is the sun: its signs, octant and |S|_1 are launch constants)
  constexpr bool ksun = KSUN;
  const bool kst = LEAN && st0 != nullptr;  // (st0: the primary walk's start and launch constants, CertStartK)
  const bool ksh = KSUN && sh0 != nullptr;  // (sh0: the shadow walk's first planes, CertShadowK)
  const int sx = ksun ? sk->sun_step[0] : (D.x > 0.0f ? 1 : -1), sy = ksun ? sk->sun_step[1] : (D.y > 0.0f ? 1 : -1),
            sz = ksun ? sk->sun_step[2] : (D.z > 0.0f ? 1 : -1);
  const int ux = ksun ? (sk->sun_step[0] > 0 ? 1 : 0) : (D.x > 0.0f ? 1 : 0), uy = ksun ? (sk->sun_step[1] > 0 ? 1 : 0) : (D.y > 0.0f ? 1 : 0),
            uz = ksun ? (sk->sun_step[2] > 0 ? 1 : 0) : (D.z > 0.0f ? 1 : 0);
  const f3 ar = mk(__builtin_fabsf(rcp.x), __builtin_fabsf(rcp.y), __builtin_fabsf(rcp.z));
  const float l1 = ksun ? sk->sun_l1 : __builtin_fabsf(D.x) + __builtin_fabsf(D.y) + __builtin_fabsf(D.z);
  const uint32_t obase =
      ksun ? sk->sun_obase : ((D.x < 0.0f ? 1u : 0u) | (D.y < 0.0f ? 2u : 0u) | (D.z < 0.0f ? 4u : 0u)) * c.ostride;
  // Rounding bounds as polynomials in the crossing parameter u (2x safety factor on 2^-24):
  //   K(u) = u |d|_1 + 3 non-zero exact steps, sum_k len_k <= (K + 3)^2 / (2 |d|_1) + K (len0 + 1),
  //   gam_b(u) = 2^-24 (sum len + 2 (u + len0) + (K + 3N + 8) |1/d_b|) + 4e-5 + e0 + ed_b,
  //   gL(u) = 2^-23 sum len + 1e-4 + e0 (the length test)
  // Factored by what depends on the axis: gam_b(u) = A(u) + |1/d_b| B(u) + ed_b,
  //   A(u) = (q2 u + a1) u + c0, B(u) = b1 u + b0: five scalars per walk, three fma per iteration
  constexpr float k24 = 2.0f * 0x1p-24f;
  const float q2 = ksun ? sk->sun_q2 : 0.5f * k24 * l1;
  // 18 / |d|_1 only bounds a sum: the hardware reciprocal (<= 1 ulp) scaled up by 2^-19 stays above it
  const float lin = 6.0f + l1 * (len0b + 1.0f),
              con = (18.0f * 1.0000020f) * __builtin_amdgcn_rcpf(l1) + 3.0f * (len0b + 1.0f);
  const float a1 = k24 * (lin + 2.0f), b1 = ksun ? sk->sun_b1 : k24 * l1,
              b0 = kst ? st0->b0 : (ksun ? sk->walk_b0 : k24 * (3.0f * c.fn + 11.0f));
  const float c0 = k24 * (con + 2.0f * len0b) + 4e-5f + e0;
  const float g2 = ksun ? sk->sun_g2 : 2.0f * q2, g1 = 2.0f * k24 * lin, g0 = 2.0f * k24 * con + 1e-4f + e0;
  // sign-folded start and direction: Ps_b + u |d_b| = s_b (P_b + u d_b) exactly (negation is exact),
  // so a landing cell is floor(s x) ^ m, m = 0 or ~0 (ceil(x) - 1 = ~floor(-x)), without branches
  // (st0: the caller's start formed them; sk: the negation as the launch's sign bit, one xor)
  const f3 Ps = kst    ? st0->Ps
                : ksun ? mk(__uint_as_float(__float_as_uint(P.x) ^ sk->sun_neg[0]), __uint_as_float(__float_as_uint(P.y) ^ sk->sun_neg[1]),
                            __uint_as_float(__float_as_uint(P.z) ^ sk->sun_neg[2]))
                       : mk(ux ? P.x : -P.x, uy ? P.y : -P.y, uz ? P.z : -P.z);
  const f3 Da = mk(__builtin_fabsf(D.x), __builtin_fabsf(D.y), __builtin_fabsf(D.z));
  const int mx = kst ? st0->mx : ux - 1, my = kst ? st0->my : uy - 1, mz = kst ? st0->mz : uz - 1;
  // (st0: the first planes from the start's floored floats, the landing form below: CertStartK)
  // (sh0: the caller's start formed the expression below already, CertShadowK)
  f3 sig = kst   ? mk((st0->fl1.x - Ps.x) * ar.x, (st0->fl1.y - Ps.y) * ar.y, (st0->fl1.z - Ps.z) * ar.z)
           : ksh ? sh0->sig
                 : mk((float(cx + ux) - P.x) * rcp.x, (float(cy + uy) - P.y) * rcp.y, (float(cz + uz) - P.z) * rcp.z);
  // start: the unguarded box from the diagonal neighbour (G(v + s) + 1 in the guarded formula)
  // (tex0: that texel, loaded by the caller beside an earlier load; ~0u: load it here)
  uint32_t tex = (tex0 != ~0u ? tex0
                              : (LEAN ? start_texel(c, cx + sx, cy + sy, cz + sz, obase)
                                      : path_texel(c, cx + sx, cy + sy, cz + sz, obase))) +
                 (1u << kDistShift);
  CTRACE(c, 100 + int(SHADOW), cx, cy, cz, P.x, P.y, P.z, U);
  CTRACE(c, 101, D.x, D.y, D.z, e0, ed.x, ed.y, ed.z);
  CERT_DIAG_ONLY(r.iters = 0;)
  if (LEAN && PHASE_STOP(SHADOW ? 4 : 2)) {  // phase budget: the prologue's values into the result
    r.u = ((sig.x + sig.y) + (sig.z + q2)) + ((a1 + b1) + (b0 + c0)) + ((g2 + g1) + (g0 + Ps.x)) +
          ((Ps.y + Ps.z) + (Da.x + Da.y)) + ((Da.z + ar.x) + (ar.y + ar.z)) + U;
    r.cx = int(tex + obase) + mx + my + mz;
    return r;
  }
  int st = CERT_UNSURE;
  for (int guard = 0; guard < kCertMaxIter; ++guard) {
    CERT_DIAG_ONLY(r.iters = guard + 1;)
    const float s1 = __builtin_fminf(sig.x, __builtin_fminf(sig.y, sig.z));
    const float uu = gmax(s1, 0.0f);
    const float A = __builtin_fmaf(__builtin_fmaf(q2, uu, a1), uu, c0);
    const float B = __builtin_fmaf(b1, uu, b0);
    // gam_b(uu), formed where a crossing needs it (ED false: the caller's ed is zero, and x + 0.0f
    // would not fold)
    auto gam_of = [&](float arb, float edb) {
      const float g = __builtin_fmaf(B, arb, A);
      return ED ? g + edb : g;
    };
    // empty-space jump: the box [v - s, v + (G - 1) s] of this cell is empty and in the volume
    // (only for rays in air: empty cells are events in a glass medium). No test of G: without a
    // box (G < 2) fg1 - B is negative and the jump parameter below is at most s1 (see above).
    const uint32_t G = tex >> kDistShift;
    bool jumped = false;
    if (SHADOW || medium == 0u) {
      // the box's far face on axis b is G - 1 - margin cells beyond the plane of sig_b: its
      // parameter sig_b + (G - 1 - margin) |1/d_b| up to a few ulps, far inside the margin's
      // margin |1/d_b| (|sig_b| <= ~400 |1/d_b| in a 256^3 volume: 1e-4 |1/d_b| at 3 ulps)
      const float fg1 = float(G) - (1.0f + kCertMargin);
      // per axis: the exact walk crosses the box face of axis b within gam_b of l_b, so its steps
      // up to min_b (l_b - gam_b) sample box cells (a common max(gam) would let one nearly
      // parallel axis, |1/d_b| huge, stop every jump: ~90 us cell-by-cell walks at C3).
      // l_b - gam_b = sig_b + (fg1 - B) |1/d_b| - ed_b - A: the axis' part in one fma, A after the minimum
      const float fb = fg1 - B;
      const float jx = __builtin_fmaf(fb, ar.x, sig.x), jy = __builtin_fmaf(fb, ar.y, sig.y),
                  jz = __builtin_fmaf(fb, ar.z, sig.z);
      const float jm = ED ? __builtin_fminf(jx - ed.x, __builtin_fminf(jy - ed.y, jz - ed.z))
                          : __builtin_fminf(jx, __builtin_fminf(jy, jz));
      const float uj = __builtin_fminf(jm - A, kst ? st0->U2 : U + 2.0f);
      CTRACE(c, 102, G, s1, uj, gam_of(ar.x, ed.x), gam_of(ar.y, ed.y), gam_of(ar.z, ed.z), 0);
      if (uj > s1) {
        // the cell the exact walk is in there: floor(x) moving up, ceil(x) - 1 moving down
        // (one rounding per coordinate: fma)
        const float fx = __builtin_floorf(__builtin_fmaf(uj, Da.x, Ps.x)),
                    fy = __builtin_floorf(__builtin_fmaf(uj, Da.y, Ps.y)),
                    fz = __builtin_floorf(__builtin_fmaf(uj, Da.z, Ps.z));
        cx = int(fx) ^ mx;
        cy = int(fy) ^ my;
        cz = int(fz) ^ mz;
        // the next planes from the floored floats, sign-folded: (fl_b + 1) - Ps_b is s_b (float(c_b +
        // u_b) - P_b) exactly (moving down, c_b = ~fl_b and float(c_b) = -(fl_b + 1); negation is
        // exact, so both forms round the same magnitude) and |1/d_b| = s_b / d_b: the product is
        // (float(c_b + u_b) - P_b) * rcp_b bit for bit, a zero's sign aside: were fl_b + 1 == Ps_b, a
        // down-moving axis would get -0 there and +0 here. Every caller starts the walk with no
        // plane behind the start (sig_b >= 0, see above), and then uj > s1 >= 0 puts the landing at
        // or ahead of P_b and fl_b + 1 > Ps_b; s1 itself is not clamped, so this is the callers'
        // precondition, not the loop's. A zero's sign would not matter either: sig enters minima,
        // compares, differences and fma addends with non-zero products only, where -0 and +0 agree.
        if constexpr (LEAN)
          sig = mk(((fx + 1.0f) - Ps.x) * ar.x, ((fy + 1.0f) - Ps.y) * ar.y, ((fz + 1.0f) - Ps.z) * ar.z);
        else
          sig = mk((float(cx + ux) - P.x) * rcp.x, (float(cy + uy) - P.y) * rcp.y, (float(cz + uz) - P.z) * rcp.z);
        // The landing cell is inside the jump box, and the box inside the volume, so its texel is
        // loaded without path_texel's bounds test: on every axis the sign-folded landing coordinate
        // is at most that of the plane of sig_b plus G - 1 - kCertMargin cells (uj <= l_b - gam_b,
        // gam_b >= 0), the box's far face pulled in by 1/64 cell, against a float error of the
        // coordinate of at most 2^-14 cell (|x| <= N + 2 <= 2^10 + 2, the fma's one rounding); and it is at or
        // ahead of P_b (uj > s1 >= 0, the callers' precondition above), which the box [v - s, v + (G - 1) s] (at the start: [v, v +
        // G s] from the cell of P itself) covers. Every cell of the box is in [0, N)^3 (skip_walk's
        // B(v), vrt_walk.h).
        tex = LEAN ? cell_texel(c, cx, cy, cz, obase) : path_texel(c, cx, cy, cz, obase);
        jumped = true;
      }
    }
    // (the crossing reads sig after the jump's merge, and the axis from it: the planes then live in
    // one set of registers across the iteration; with `continue` in the jump two of them were
    // copied out and back in every iteration)
    // One exit (r09): the crossing below has no `return`. It decides this iteration's outcome st,
    // kCertRun or the walk's result, and the loop's end tests it once; the result's fields are not
    // carried through the loop (eight VGPRs, and a state variable decoded by ~25 scalar instructions
    // in every iteration, jumps included) but read after it from the loop's own variables.
    st = kCertRun;
    if (!jumped) {
      const int a = sig.x == s1 ? 0 : (sig.y == s1 ? 1 : 2);
      // one crossing, s1 on axis a; prev = the crossing before it (the exact walk's len there)
      const f3 gam = mk(gam_of(ar.x, ed.x), gam_of(ar.y, ed.y), gam_of(ar.z, ed.z));
      const f3 back = mk(sig.x - ar.x, sig.y - ar.y, sig.z - ar.z);
      const float mback = gmax(back.x, gmax(back.y, back.z));
      const float prev = gmax(mback, 0.0f);
      const float gL = __builtin_fmaf(__builtin_fmaf(g2, uu, g1), uu, g0);
      // the length test stops the walk before this crossing (decided in the rare block below)
      const bool lenstop = prev > U + gL;
      const int nx = cx + (a == 0 ? sx : 0), ny = cy + (a == 1 ? sy : 0), nz = cz + (a == 2 ? sz : 0);
      const uint32_t ntex = LEAN ? cross_texel(c, nx, ny, nz, obase) : path_texel(c, nx, ny, nz, obase);
      const float ga = a == 0 ? gam.x : (a == 1 ? gam.y : gam.z);
      // near-edge flags per other axis: ahead (crossed within the bound after s1) / behind (before).
      // A plane behind counts down to -gam_b, not 0: a ray that starts ON a plane (a shadow or
      // secondary ray from an exact hit point on the hit face) has that plane at parameter 0 up to
      // rounding, and the exact walk's currentPos stays on it — sampling the voxel beyond it — until
      // the ray has moved half an ulp of the coordinate off it (r02 s18: a shadow ray from
      // (33.000008, 127, 37.02) sampled the panel voxel (32, 127, 37) at its first x crossing, and
      // back.y rounded to just below 0 hid that alternative from the certified walk)
      // nf bits 0-2: ahead x, y, z; 3-5: behind x, y, z. They are rare: a superset test first (the
      // second smallest sig bounds every sig_b, b != a, from below, the latest back every back_b from
      // above, and ga + max gam every ga + gam_b; rounding is monotone), the flags only if it holds.
      const float tg = ga + gmax(gam.x, gmax(gam.y, gam.z));
      // the crossings up to prev are settled (this one, at s1, may not be): an exact step at s <
      // prev - tg has its real crossing before prev (gam_b <= tg), so it samples a settled cell
      if (!lenstop) r.us = prev - tg - 1e-3f;
      const bool near = __builtin_amdgcn_fmed3f(sig.x, sig.y, sig.z) - s1 < tg || s1 - mback < tg;
      const uint32_t nb = ntex & kVoxMask;
      const int na = a == 0 ? nx : (a == 1 ? ny : nz);
      // The crossing's outcome, decided in the order: length test, event, alternatives, outside. The
      // plain cases first, without a branch (no length stop, no near-edge flag): an event is a hit if
      // the length test cannot stop the walk first, else unsure; a cell outside the volume (moving
      // away on axis a) a miss; anything else goes on. The rare block below overrides them. `stop` is
      // the loop's one way out besides its iteration cap, with the result already in res. (Both forms
      // of the decision over every combination of its predicates: tests/test_cert_one_exit_tables.py.)
      // The crossing's texel is loaded before the length test is looked at: its address is in bounds
      // either way (cross_texel / path_texel), and a walk the length test stops reads it for nothing.
      const bool ev = cert_event<SHADOW>(nb, medium);
      const bool lenok = prev + gL < U;  // the length test cannot stop the walk before this crossing
      const bool outside = LEAN ? cross_outside(ntex) : uint32_t(na) >= uint32_t(c.n);
      int res = ev ? (lenok ? CERT_HIT : CERT_UNSURE) : (outside ? CERT_MISS : CERT_UNSURE);
      bool stop = ev || outside;
      CTRACE(c, 104, cx, cy, cz, sig.x, sig.y, sig.z, ga);
      if (lenstop || near) {
        if (lenstop) {
          // the length test stops the walk before this crossing, unless a tie merges it into the
          // step of the one before (that step passed the test): then the exact walk still samples it
          // (a tree ray whose y and z crossings tied at len 101.1 left the glass there, refracting,
          // before its length ended the march; its sky colour took the refracted direction)
          stop = true;
          res = s1 - mback < 2.0f * gmax(gam.x, gmax(gam.y, gam.z)) ? CERT_UNSURE : CERT_MISS;
        } else {
          const bool ahx = a != 0 && sig.x - s1 < ga + gam.x, ahy = a != 1 && sig.y - s1 < ga + gam.y,
                     ahz = a != 2 && sig.z - s1 < ga + gam.z;
          const bool bhx = a != 0 && back.x > -gam.x && s1 - back.x < ga + gam.x;
          const bool bhy = a != 1 && back.y > -gam.y && s1 - back.y < ga + gam.y;
          const bool bhz = a != 2 && back.z > -gam.z && s1 - back.z < ga + gam.z;
          const uint32_t nf = uint32_t(ahx) | uint32_t(ahy) << 1 | uint32_t(ahz) << 2 | uint32_t(bhx) << 3 |
                              uint32_t(bhy) << 4 | uint32_t(bhz) << 5;
          CTRACE(c, 103, nx, ny, nz, s1, a, nf, nb);
          // LEAN: each rare block below decodes a flag where it uses it, from a fresh opaque copy of nf,
          // instead of the six lane masks above (both polarities) being kept across the blocks' loads:
          // they were the walk's SGPR spills, 24 of the hot instance's 61
          auto flag = [&](int bit, bool decoded) {
            if constexpr (LEAN) {
              uint32_t f = nf;
              asm volatile("" : "+v"(f));
              return ((f >> bit) & 1u) != 0u;
            } else {
              return decoded;
            }
          };
          if (nf != 0u && ev) {
            // an event with flags: unsure, but for a shadow walk's one-flag hit
            res = CERT_UNSURE;
            // Blocked whichever way the exact walk goes (nc blocks: the order a, b samples it first):
            //  - near-ahead b: crossed first, the walk samples cell + e_b and then, in a second step, nc +
            //    e_b; tied with a, it samples nc + e_b alone. So nc + e_b must block: a blocking cell + e_b
            //    with a clear nc + e_b is lit in the tie. And it must block as a cell of the volume
            //    (path_texel, not alt_byte's wrapped plane N): with index N on axis b the tie's sample lies
            //    half a cell beyond the volume's face and reads nothing, and the order b, a ends at TestCube
            //    unless the coordinate is N exactly: the plane's copy is what the walk may read, not must;
            //  - near-behind b: the walk samples nc at once, or nc - e_b and then nc in a second step;
            //  - either second step happens only if the walk's len before it is below the limit: the other
            //    crossing's parameter, within gam_a + gam_b <= tg of s1. lenok (prev + gL < U) speaks of the
            //    step at s1 alone, so the block asks s1 + tg + gL < U.
            // (The ray tests found the tie, the plane's copy and the second step's length as shadow rays the
            // walk called blocked and the exact walk ends lit: tests/test_cert_rays.py)
            if (SHADOW && lenok && __builtin_popcount(nf) == 1 && s1 + tg + gL < U) {
              bool ok = true;
              if (nf & 7u) {
                const int bx = (nf & 1u) ? sx : 0, by = (nf & 2u) ? sy : 0, bz = (nf & 4u) ? sz : 0;
                ok = cert_event<true>(path_texel(c, nx + bx, ny + by, nz + bz, obase) & kVoxMask, 0u);
              }
              if (ok) res = CERT_HIT;
            }
          } else if (nf != 0u) {  // cells the exact walk may sample instead of the path's: all must be non-events
            const int nah = int(ahx) + int(ahy) + int(ahz);
            bool bad = false;
            if (__builtin_popcount(nf) >= 2) {  // near a corner: the 2x2x2 block ahead and the cells behind nc
              for (int q = 1; q < 8 && !bad; ++q)
                bad = cert_event<SHADOW>(alt_byte(c, cx + ((q & 1) ? sx : 0), cy + ((q & 2) ? sy : 0),
                                                  cz + ((q & 4) ? sz : 0), obase), medium);
              bad = bad || (flag(3, bhx) && cert_event<SHADOW>(alt_byte(c, nx - sx, ny, nz, obase), medium)) ||
                    (flag(4, bhy) && cert_event<SHADOW>(alt_byte(c, nx, ny - sy, nz, obase), medium)) ||
                    (flag(5, bhz) && cert_event<SHADOW>(alt_byte(c, nx, ny, nz - sz, obase), medium));
            } else if (nah) {  // b may be crossed first, or tie: cell + e_b, nc + e_b
              const int bx = flag(0, ahx) ? sx : 0, by = flag(1, ahy) ? sy : 0, bz = flag(2, ahz) ? sz : 0;
              bad = cert_event<SHADOW>(alt_byte(c, cx + bx, cy + by, cz + bz, obase), medium) ||
                    cert_event<SHADOW>(alt_byte(c, nx + bx, ny + by, nz + bz, obase), medium);
            } else {  // a may have been crossed before b: nc - e_b
              bad = cert_event<SHADOW>(alt_byte(c, nx - (flag(3, bhx) ? sx : 0), ny - (flag(4, bhy) ? sy : 0),
                                                nz - (flag(5, bhz) ? sz : 0), obase), medium);
            }
            if (bad) {  // unsure; else the plain outcome stands: outside a miss, or the walk goes on
              stop = true;
              res = CERT_UNSURE;
            }
          }
        }
      }
      // the cell entered is the walk's cell either way: a walk that stops leaves its last cell and texel
      // (the hit's) in the loop's own variables, and its planes as they are, for the result below
      cx = nx;
      cy = ny;
      cz = nz;
      tex = ntex;
      st = stop ? res : kCertRun;
      if (!stop) {
        if constexpr (LEAN) {
          // the crossed axis' next plane, sign-folded as after a jump: s_a float(na + u_a) is float((na ^
          // m_a) + 1) (moving down ~na + 1 = -na), so (that - Ps_a) |1/d_a| is (np - P_a) rcp_a bit for
          // bit (not a zero either: it is s1 + |1/d_a| up to rounding). P and rcp are then dead in the loop.
          const int ma = a == 0 ? mx : (a == 1 ? my : mz);
          const float fp = float((na ^ ma) + 1);
          if (a == 0) sig.x = (fp - Ps.x) * ar.x;
          else if (a == 1) sig.y = (fp - Ps.y) * ar.y;
          else sig.z = (fp - Ps.z) * ar.z;
        } else {
          const int sa = a == 0 ? sx : (a == 1 ? sy : sz);
          const float np = float(na + (sa > 0 ? 1 : 0));
          if (a == 0) sig.x = (np - P.x) * rcp.x;
          else if (a == 1) sig.y = (np - P.y) * rcp.y;
          else sig.z = (np - P.z) * rcp.z;
        }
      }
    }
    // the loop's one exit besides its iteration cap. The outcome is kept opaque here, after the merge
    // of the jump and the crossing, so that the test is made once, where every lane passes
    asm volatile("" : "+v"(st));
    if (st != kCertRun) break;
    st = CERT_UNSURE;  // (the iteration cap: unsure)
  }
  // The result's fields from what the loop left: the last crossing's cell and texel, and its axis,
  // parameter and bound recomputed from the planes it did not advance: the same operations on the
  // same operands as in the loop (they mean something for a hit only; a shadow walk's caller reads
  // none of them).
  r.res = st;
  {
    const float s1 = __builtin_fminf(sig.x, __builtin_fminf(sig.y, sig.z));
    const float uu = gmax(s1, 0.0f);
    const float A = __builtin_fmaf(__builtin_fmaf(q2, uu, a1), uu, c0);
    const float B = __builtin_fmaf(b1, uu, b0);
    const int a = sig.x == s1 ? 0 : (sig.y == s1 ? 1 : 2);
    const float g = __builtin_fmaf(B, a == 0 ? ar.x : (a == 1 ? ar.y : ar.z), A);
    r.byte = tex & kVoxMask;
    r.axis = a;
    r.cx = cx;
    r.cy = cy;
    r.cz = cz;
    r.u = s1;
    r.eu = ED ? g + (a == 0 ? ed.x : (a == 1 ? ed.y : ed.z)) : g;
  }
  return r;
}

// A ray that starts at a face crossing of a certified walk (a shadow or secondary ray from a hit,
// or a walk restarted by in-volume refraction): the exact origin lies within e (parameter) of
// X = P + u D0 along the parent direction D0, so within e |D0_fa| of the face plane (axis fa),
// possibly on its far side. The exact walk starts in the same cell (cx, cy, cz) on the new
// direction's side of the plane and samples the same cells if, on every other axis, X is farther
// than its uncertainty from a plane and the new ray's first crossing of that axis comes after it
// has left the face plane's neighbourhood (lead). ed: the crossing-order uncertainty the origin
// adds to the new walk.
__device__ __forceinline__ bool cert_start(const f3 X, const f3 D0, const f3 Dn, const f3 rcpn,
                                           int fa, float e, int cx, int cy, int cz, f3& ed) {
  ed = mk(2.0f * e * __builtin_fabsf(D0.x * rcpn.x), 2.0f * e * __builtin_fabsf(D0.y * rcpn.y),
          2.0f * e * __builtin_fabsf(D0.z * rcpn.z));
  const float d0a = fa == 0 ? D0.x : (fa == 1 ? D0.y : D0.z);
  const float rna = fa == 0 ? rcpn.x : (fa == 1 ? rcpn.y : rcpn.z);
  const float lead = (e * __builtin_fabsf(d0a) + 1e-5f) * __builtin_fabsf(rna);
  const float wx = (float(cx + (Dn.x > 0.0f)) - X.x) * rcpn.x;
  const float wy = (float(cy + (Dn.y > 0.0f)) - X.y) * rcpn.y;
  const float wz = (float(cz + (Dn.z > 0.0f)) - X.z) * rcpn.z;
  const f3 fr = mk(X.x - __builtin_floorf(X.x), X.y - __builtin_floorf(X.y), X.z - __builtin_floorf(X.z));
  const f3 dm = mk(e * __builtin_fabsf(D0.x) + 2e-5f, e * __builtin_fabsf(D0.y) + 2e-5f,
                   e * __builtin_fabsf(D0.z) + 2e-5f);
  const bool okx = fa == 0 || (wx >= lead + ed.x + 1e-4f && fr.x >= dm.x && 1.0f - fr.x >= dm.x);
  const bool oky = fa == 1 || (wy >= lead + ed.y + 1e-4f && fr.y >= dm.y && 1.0f - fr.y >= dm.y);
  const bool okz = fa == 2 || (wz >= lead + ed.z + 1e-4f && fr.z >= dm.z && 1.0f - fr.z >= dm.z);
  return okx && oky && okz;
}

// cert_start for the shadow ray of a primary hit (cert_shade_hit<.., KAX>; the new direction is the sun, sk its
// launch constants): the same predicate and the same ed, with
//  - d0a, the parent direction's face component, from the caller (the lit term selected it already);
//  - the first planes kept for the walk (sh.sig: CertShadowK), u_b spelled as the walk spells it, sun_step[b]
//    > 0, which is S_b > 0 (sun_consts): cert_start's w_b, same operations, same operands;
//  - the face axis' exclusion and the conjunctions as integer | and &: the same truth table (each operand a
//    comparison without side effects; tests/test_shadow_start_forms.py), without three branch regions.
__device__ __forceinline__ bool cert_start_sun(const f3 X, const f3 D0, const float d0a, LateKArgs* sk, const f3 rcpn,
                                               int fa, float e, int cx, int cy, int cz, f3& ed, CertShadowK& sh) {
  ed = mk(2.0f * e * __builtin_fabsf(D0.x * rcpn.x), 2.0f * e * __builtin_fabsf(D0.y * rcpn.y),
          2.0f * e * __builtin_fabsf(D0.z * rcpn.z));
  const float rna = fa == 0 ? rcpn.x : (fa == 1 ? rcpn.y : rcpn.z);
  const float lead = (e * __builtin_fabsf(d0a) + 1e-5f) * __builtin_fabsf(rna);
  const int ux = sk->sun_step[0] > 0 ? 1 : 0, uy = sk->sun_step[1] > 0 ? 1 : 0, uz = sk->sun_step[2] > 0 ? 1 : 0;
  sh.sig = mk((float(cx + ux) - X.x) * rcpn.x, (float(cy + uy) - X.y) * rcpn.y, (float(cz + uz) - X.z) * rcpn.z);
  const f3 fr = mk(X.x - __builtin_floorf(X.x), X.y - __builtin_floorf(X.y), X.z - __builtin_floorf(X.z));
  const f3 dm = mk(e * __builtin_fabsf(D0.x) + 2e-5f, e * __builtin_fabsf(D0.y) + 2e-5f,
                   e * __builtin_fabsf(D0.z) + 2e-5f);
  const int okx = int(fa == 0) | (int(sh.sig.x >= lead + ed.x + 1e-4f) & int(fr.x >= dm.x) & int(1.0f - fr.x >= dm.x));
  const int oky = int(fa == 1) | (int(sh.sig.y >= lead + ed.y + 1e-4f) & int(fr.y >= dm.y) & int(1.0f - fr.y >= dm.y));
  const int okz = int(fa == 2) | (int(sh.sig.z >= lead + ed.z + 1e-4f) & int(fr.z >= dm.z) & int(1.0f - fr.z >= dm.z));
  return (okx & oky & okz) != 0;
}

// The cell before a hit cell along D on its crossed axis
__device__ __forceinline__ void cell_before(const CertResult& h, const f3 D, int& x, int& y, int& z) {
  x = h.cx - (h.axis == 0 ? (D.x > 0.0f ? 1 : -1) : 0);
  y = h.cy - (h.axis == 1 ? (D.y > 0.0f ? 1 : -1) : 0);
  z = h.cz - (h.axis == 2 ? (D.z > 0.0f ? 1 : -1) : 0);
}

// A Hit record for a certified hit of `ray`: point and len approximate (within h.eu along the
// ray); only the face, voxel and (in robust positions) the probes derived from it are used
__device__ __forceinline__ Hit cert_hit_record(const Ray& ray, const CertResult& h) {
  Hit hh;
  hh.found = true;
  hh.voxel = h.byte;
  hh.axis = h.axis;
  hh.vidx = -1;
  hh.len = ray.len + h.u;
  hh.point = mk(ray.pos.x + h.u * ray.dir.x, ray.pos.y + h.u * ray.dir.y, ray.pos.z + h.u * ray.dir.z);
  hh.normal = mk(0.0f, 0.0f, 0.0f);
  set_comp(hh.normal, h.axis, -gsign(comp(ray.dir, h.axis)));
  return hh;
}

// The face's normal -sign(D_a) e_a alone, as cert_hit_record forms it
__device__ __forceinline__ f3 cert_hit_normal(const f3 D, int axis) {
  f3 n = mk(0.0f, 0.0f, 0.0f);
  set_comp(n, axis, -gsign(comp(D, axis)));
  return n;
}
// cert_hit_record for a primary hit of the certified pass (LEAN: ray is the launch's primary ray, len 0):
//  - len = h.u: cert_hit_record's 0.0f + h.u is h.u bit for bit unless h.u is -0, and the primary walk's
//    planes are products of a positive difference (fl_b + 1 > Ps_b, CertStartK; a crossing's next plane lies
//    ahead of it) and |1/d_b| > 0: h.u, their minimum, is never negative, -0 included;
//  - the normal stays zero: cert_shade_hit<.., KAX> and cert_texel do not read it, and the generic lit term
//    behind sun_ok == 0 forms it there (cert_hit_normal). It was formed for every hit before that branch.
__device__ __forceinline__ Hit cert_hit_record_primary(const Ray& ray, const CertResult& h) {
  Hit hh;
  hh.found = true;
  hh.voxel = h.byte;
  hh.axis = h.axis;
  hh.vidx = -1;
  hh.len = h.u;
  hh.point = mk(ray.pos.x + h.u * ray.dir.x, ray.pos.y + h.u * ray.dir.y, ray.pos.z + h.u * ray.dir.z);
  hh.normal = mk(0.0f, 0.0f, 0.0f);
  return hh;
}

// TraceWithShadow's colour update (voxel.glsl:395-418) for a certified hit of `ray`: the shadow
// bit by a certified shadow walk from the hit, unless it cannot change the brightness (lit ==
// ambient). false: unsure (colour untouched).
template <bool TEX = false, bool LEAN = false, bool KAX = false>
__device__ __forceinline__ bool cert_shade_hit(const Ctx& c, const Ray& ray, const CertResult& h,
                                               const Hit& hh, f3& color, float4 col = float4(),
                                               LateKArgs* sk = nullptr) {
  const f3 S = c.sun_n;
  // KAX (the certified pass's primary hits; LEAN): sk holds the sun's launch constants. With sk->sun_ok (wave-uniform:
  // every |S_b| in fast_path_ok's range, so no component of S is zero) the lit term takes the face's
  // axis normal n = -sign(D_a) e_a as what it is (ray.dir is in the fast-path range too: D_a != 0):
  //  - dot(n, S) = (n_x S_x + n_y S_y) + n_z S_z has two terms +-0 and the term n_a S_a = -+S_a != 0,
  //    and x + +-0 = x for x != 0: the sum is n_a S_a, the select below, bit for bit;
  //  - reflect(S, n) = S - (2 dot(n, S)) n: component a is S_a - 2 S_a = -S_a exactly, component b is
  //    S_b - (+-0) = S_b (S_b != 0), so dot(reflect(S, n), D) = (p_x + p_y) + p_z with p_b = S_b D_b and
  //    p_a = (-S_a) D_a = -(S_a D_a) (negation commutes with rounding): the same products, the same order.
  // With a zero in S the zeros' signs can differ (-0 - -0 = +0: tests/test_cert_start_lit_forms.py finds
  // such suns), so the generic form stays behind the wave-uniform branch; it defers every lit hit there.
  // (KAX: hh is cert_hit_record_primary's, its normal zero; the generic lit term forms the normal where it runs,
  // from an opaque copy of the axis so that it is not merged back in front of the branch)
  // KAX: the material is stone or grass. h is a certified hit of a primary walk in air, so its byte is an event
  // of the air medium: the loop stops with CERT_HIT only where `ev` holds, cert_event<false>(b, 0), b != 0, and b
  // is the byte it hands back; and cert_pixel has taken the glass hits (mat_id(b) == 2, b == 2) before it shades.
  // The material tables' arms for air and glass (mat_kd, mat_ks, mat_exp, mat_color, shadow_free_hit) are
  // selects on tests whose outcome this decides.
  if constexpr (KAX) __builtin_assume(h.byte != 0u && h.byte != 2u);
  float lit, ns = 0.0f, da = 0.0f;  // da (KAX, sun_ok): D_a, for the shadow's start too (cert_start_sun)
  auto lit_generic = [&]() {
    if constexpr (KAX) {
      int ga = h.axis;
      asm volatile("" : "+v"(ga));
      Hit hg = hh;
      hg.normal = cert_hit_normal(ray.dir, ga);
      return lit_brightness<TEX>(hg, S, ray.dir);
    } else {
      return lit_brightness<TEX>(hh, S, ray.dir);
    }
  };
  if constexpr (KAX) {
    if (sk->sun_ok != 0u) {
      const int a = h.axis;
      // (the direction as opaque values: in the tree instances, where the ray lives in memory, the
      // select of its fields became a load at a selected address and kept the ray in scratch, 48 B)
      f3 D = ray.dir;
      asm volatile("" : "+v"(D.x), "+v"(D.y), "+v"(D.z));
      const float sa = a == 0 ? S.x : (a == 1 ? S.y : S.z);
      da = a == 0 ? D.x : (a == 1 ? D.y : D.z);
      ns = da > 0.0f ? -sa : sa;
      const float px = S.x * D.x, py = S.y * D.y, pz = S.z * D.z;
      const float rd = ((a == 0 ? -px : px) + (a == 1 ? -py : py)) + (a == 2 ? -pz : pz);
      const uint32_t m = mat_id(h.byte);
      const float diffuse = mat_kd(m) * gmax(ns, 0.0f);
      // Colour-only: the power by the bare log and exp (gpow_raw). Where the two forms differ both are below
      // 2^-100, and 0.2 * 2^-100 is far below half an ulp of kAmbient + diffuse >= 0.3 (2^-26): the sum below
      // has the same bits, and nothing else reads the specular term.
      float pw;
      if constexpr (!TEX && kCutSpec)
        pw = gpow_raw(gmax(rd, 0.0f), mat_exp(m, TEX));
      else
        pw = gpow(gmax(rd, 0.0f), mat_exp(m, TEX));
      const float specular = mat_ks(m, TEX) * pw;
      lit = kAmbient + diffuse + specular;
    } else {
      lit = lit_generic();
    }
  } else {
    lit = lit_generic();
  }
  float brightness = kAmbient;
  if (lit != kAmbient && !shadow_free_hit(h.byte, TEX)) {  // otherwise the brightness is the ambient term (or irrelevant)
    if constexpr (KAX) {  // back face, or a sun outside the fast-path range (sk->sun_ok is fast_path_ok(S))
      if (sk->sun_ok == 0u || !(ns > 0.0f)) { CERT_DIAG(5); return false; }
    } else {
      if (!(dot3(hh.normal, S) > 0.0f) || !fast_path_ok(S)) { CERT_DIAG(5); return false; }  // back face
    }
    // shadow origin: the exact hit point; start cell: the air cell in front of the hit face
    int ax, ay, az;
    cell_before(h, ray.dir, ax, ay, az);
    // the shadow walk's start texel (the diagonal neighbour in the sun's octant volume) is loaded
    // first, so its latency overlaps the start checks and the air-cell load (same octant volume:
    // every octant volume holds the same voxel bytes)
    const uint32_t sob =
        KAX ? sk->sun_obase : ((S.x < 0.0f ? 1u : 0u) | (S.y < 0.0f ? 2u : 0u) | (S.z < 0.0f ? 4u : 0u)) * c.ostride;
    // (KAX: by start_texel, path_texel's value without its branch: the merge behind the branch made the wave wait
    // for the load at once, and nothing overlapped it)
    const int tx = ax + (KAX ? sk->sun_step[0] : (S.x > 0.0f ? 1 : -1)), ty = ay + (KAX ? sk->sun_step[1] : (S.y > 0.0f ? 1 : -1)),
              tz = az + (KAX ? sk->sun_step[2] : (S.z > 0.0f ? 1 : -1));
    const uint32_t t0 = KAX ? start_texel(c, tx, ty, tz, sob) : path_texel(c, tx, ty, tz, sob);
    if (KAX && PHASE_STOP(7)) {  // phase budget: the record, the lit term and the start's cell and texel as the colour
      color = mk(lit + hh.len, hh.point.x + hh.point.y + hh.point.z + da, float(int(t0) + ax + ay + az));
      return true;
    }
    f3 ed;
    CertShadowK sh;
    // (KAX: the start's verdict and the air cell's are one flag, and the lanes either of them stops leave
    // together below: each `return` of its own was a region with its saved lane mask, spilled across the walk)
    bool go = true;
    if constexpr (KAX) {
      go = cert_start_sun(hh.point, ray.dir, da, sk, c.sun_rcp, h.axis, h.eu, ax, ay, az, ed, sh);
      if (!go) CERT_DIAG(6);
    } else {
      if (!cert_start(hh.point, ray.dir, S, c.sun_rcp, h.axis, h.eu, ax, ay, az, ed)) {
        CERT_DIAG(6);
        return false;
      }
    }
    if (KAX && PHASE_STOP(8)) {  // phase budget: + the shadow's start
      color = mk(lit + hh.len + ed.x + ed.y + ed.z, sh.sig.x + sh.sig.y + sh.sig.z, float(int(t0) + ax + ay + az));
      return true;
    }
    // The air cell (ax, ay, az) must be inside the volume and hold no shadow event. It is the cell the primary
    // walk was in before its last crossing, and the walk's loop has proved both of every cell it moved into:
    //  - a jump lands inside its box, and a box lies inside the volume and holds empty cells only (byte 0: the
    //    boxes of the skip field, vrt_walk.h; cert_walk's landing argument);
    //  - a crossing that does not end the walk entered a cell that is not outside (`outside` ends the walk)
    //    and whose byte is the medium's, 0 (`ev` ends it: the primary walks in air);
    //  - the walk's cells never repeat (each coordinate moves one way), so a cell that is not the start cell
    //    was moved into, by one of the two.
    // Byte 0 is no shadow event, and every octant volume holds the same bytes. What the loop has not sampled is
    // the start cell itself (a hit at the first crossing, no jump before it: a camera inside a solid voxel, a
    // wall right in front of it): there the test stays. KAX knows the start cell only as the launch's constant
    // (kSetupCell: every pixel's walk starts in start_cell, cert_pixel); without that proof every lane tests.
    bool air_known = false;
    if constexpr (KAX)
      air_known = (sk->setup & kSetupCell) != 0u &&
                  ((ax ^ sk->start_cell[0]) | (ay ^ sk->start_cell[1]) | (az ^ sk->start_cell[2])) != 0;
    if constexpr (KAX) {
      if (go && !air_known) {  // (the load stays behind the bounds test: the cell's address exists only inside the volume)
        const uint32_t n = uint32_t(c.n);
        go = max(max(uint32_t(ax), uint32_t(ay)), uint32_t(az)) < n;
        if (go) go = !cert_event<true>(cell_texel(c, ax, ay, az, sob) & kVoxMask, 0u);
        if (!go) CERT_DIAG(7);
      }
      if (!go) return false;
    } else {
      const uint32_t n = uint32_t(c.n);
      if (uint32_t(ax) >= n || uint32_t(ay) >= n || uint32_t(az) >= n) { CERT_DIAG(7); return false; }
      if (cert_event<true>(cell_texel(c, ax, ay, az, sob) & kVoxMask, 0u)) { CERT_DIAG(7); return false; }
    }
    const CertResult s = cert_walk<true, LEAN, true, KAX>(c, hh.point, S, c.sun_rcp, c.max_len - hh.len, ax, ay, az,
                                                          h.eu, ed, hh.len, 0u, t0, nullptr, KAX ? sk : nullptr,
                                                          KAX ? &sh : nullptr);
    if (LEAN && (PHASE_STOP(4) || PHASE_STOP(5))) {  // phase budget: the shadow walk's result as the colour
      color = mk(s.u + float(s.res), lit + float(s.cx), 0.0f);
      return true;
    }
    if (s.res == CERT_UNSURE) { CERT_DIAG(8); return false; }
    CERT_DIAG(9);
    brightness = s.res == CERT_HIT ? kAmbient : lit;
  } else {
    CERT_DIAG(4);
  }
  if (!TEX) col = get_color<false>(c, hh);  // textured: the certified texel (cert_texel)
  if constexpr (KAX) {
    // The primary hit of a pixel: the colour so far is +0 and the energy 1 (cert_pixel), so mixf forms +0 * (1 -
    // 1) + y * 1 = +0 + y, which is y bit for bit unless y is -0; y = (col_b * col.w) * brightness is a product
    // of factors that are never negative (a material's or an atlas texel's colour, bytes / 255; brightness >=
    // the ambient term: diffuse and specular are a non-negative factor times a maximum with 0 and a power).
    color = mk(col.x * col.w * brightness, col.y * col.w * brightness, col.z * col.w * brightness);
  } else {
    color.x = mixf(color.x, col.x * col.w * brightness, ray.energy);
    color.y = mixf(color.y, col.y * col.w * brightness, ray.energy);
    color.z = mixf(color.z, col.z * col.w * brightness, ray.energy);
  }
  return true;
}

// RayMarch (voxel.glsl:302-384) of a secondary ray by certified walks; `ray` is inout as in
// march(): leaving a glass medium refracts it in place (:357-380), and the walk restarts from
// that crossing. (cx, cy, cz), e0, ed: the start (cert_start). Returns the first non-air event
// (CERT_HIT), CERT_MISS or CERT_UNSURE.
template <bool LEAN = false>
__device__ __forceinline__ CertResult cert_march(const Ctx& c, Ray& ray, int cx, int cy, int cz, float e0, f3 ed) {
  CertResult h;
  h.res = CERT_UNSURE;
  uint32_t medium = ray.voxel;
  int internal = 0;
  for (int seg = 0; seg < 32; ++seg) {
    if (!fast_path_ok(ray.dir) || !(e0 < kCertMaxOrigin)) { CERT_DIAG(24); return h; }
    const f3 rcp = mk(__builtin_amdgcn_rcpf(ray.dir.x), __builtin_amdgcn_rcpf(ray.dir.y),
                      __builtin_amdgcn_rcpf(ray.dir.z));
    h = cert_walk<false, LEAN>(c, ray.pos, ray.dir, rcp, c.max_len - ray.len, cx, cy, cz, e0, ed, ray.len,
                               medium);
    if (h.res == CERT_UNSURE) CERT_DIAG(25);
    if (h.res != CERT_HIT || h.byte != 0u) return h;
    CERT_DIAG(30);
    // in-volume refraction at the crossing into the air cell (h.cx, h.cy, h.cz)
    h.res = CERT_UNSURE;
    const Hit eh = cert_hit_record(ray, h);
    const f3 D0 = ray.dir;
    // the probes at point +- normal/2 (:219-220) read the exact point's cells if the point is
    // robust on the other axes
    const f3 fr = mk(eh.point.x - __builtin_floorf(eh.point.x), eh.point.y - __builtin_floorf(eh.point.y),
                     eh.point.z - __builtin_floorf(eh.point.z));
    const f3 dm = mk(h.eu * __builtin_fabsf(D0.x) + 2e-5f, h.eu * __builtin_fabsf(D0.y) + 2e-5f,
                     h.eu * __builtin_fabsf(D0.z) + 2e-5f);
    if ((h.axis != 0 && !(fr.x >= dm.x && 1.0f - fr.x >= dm.x)) ||
        (h.axis != 1 && !(fr.y >= dm.y && 1.0f - fr.y >= dm.y)) ||
        (h.axis != 2 && !(fr.z >= dm.z && 1.0f - fr.z >= dm.z))) {
      CERT_DIAG(26);
      return h;
    }
    // position-independent directions only (RandomizeDirection's zero-noise identity)
    const float eta = mat_refr(get_voxel(c, eh.point + eh.normal * 0.5f)) /
                      mat_refr(get_voxel(c, eh.point - eh.normal * 0.5f));
    const f3 rd = refract3(normalize3(D0), eh.normal, eta);
    const bool tir = rd.x == 0.0f && rd.y == 0.0f && rd.z == 0.0f;
    if (tir ? !(c.refl_noise == 0.0f && zero_noise_exact(reflect3(D0, eh.normal)))
            : !(c.refr_noise == 0.0f && zero_noise_exact(rd))) {
      CERT_DIAG(27);
      return h;
    }
    Counters kk;
#pragma unroll
    for (int q = 0; q < VRT_CNT_COUNT; ++q) kk.c[q] = 0;
    Ray nr = refraction_ray<false>(c, ray, eh, kk);
    nr.tdepth--;
    if (nr.voxel == medium) {
      internal++;
      if (internal > 10) {
        nr.dir = D0;
        nr.voxel = 0u;
      }
    }
    medium = nr.voxel;
    // restart cell: the crossed cell, or the one before it when the direction turned back
    int nx = h.cx, ny = h.cy, nz = h.cz;
    if ((comp(nr.dir, h.axis) > 0.0f) != (comp(D0, h.axis) > 0.0f)) cell_before(h, D0, nx, ny, nz);
    if (!fast_path_ok(nr.dir)) { CERT_DIAG(28); return h; }
    const f3 rcpn = mk(__builtin_amdgcn_rcpf(nr.dir.x), __builtin_amdgcn_rcpf(nr.dir.y),
                       __builtin_amdgcn_rcpf(nr.dir.z));
    f3 edn;
    if (!cert_start(eh.point, D0, nr.dir, rcpn, h.axis, h.eu, nx, ny, nz, edn)) { CERT_DIAG(28); return h; }
    ray = nr;
    const uint32_t n = uint32_t(c.n);
    if (uint32_t(nx) >= n || uint32_t(ny) >= n || uint32_t(nz) >= n) {
      // out of the volume across the crossed face, moving away: TestCube ends the walk
      h.res = CERT_MISS;
      return h;
    }
    cx = nx;
    cy = ny;
    cz = nz;
    e0 = h.eu;
    ed = edn;
  }
  CERT_DIAG(29);
  h.res = CERT_UNSURE;
  return h;
}

// ------------------------------------------------------------ certified bounce trees --------
//
// The colour of a glass pixel's bounce tree (voxel.glsl:425-452) depends on the exact hit points
// only through the walks' outcomes: reflection and refraction directions, Fresnel energies, the
// sky colour and the brightness are functions of directions and face normals alone
// (:162-165, :203-246, :386-423) once RandomizeDirection is the identity (noise 0, no -0
// component), and the accumulated rayLength enters only through the `< u_MaxRayLength` test. So
// every ray of the tree is walked by a certified walk from its uncertain origin: the parent's
// certified hit, known to its bound eu along the parent (cert_start checks the start cell and
// turns the origin uncertainty into per-axis crossing-order bounds; cert_march carries in-volume
// refraction). Any unsure step sends the whole pixel to the exact path.
//
// A ray in flight is a TreeRay: the Ray the reference would carry (pos and len approximate, dir,
// energy, medium and depths exact) plus its certified start. The DFS keeps the ray the reference
// pops next in registers (the last-pushed child), so only a reflection ray pushed under a
// refraction ray waits, in one per-lane LDS slot; a tree that would hold two such rays at once (never at the BASELINE configs: one glass voxel or
// one-voxel glass walls) goes to the exact path.
struct TreeRay {
  Ray ray;
  int cx, cy, cz;  // start cell (the exact walk's first cell)
  float e0;        // origin uncertainty (parameter along the parent)
  f3 ed;           // per-axis crossing-order uncertainty from it
};
// The slot: 12 words in the lane's own 3 float4s (lane-major; in the in-lane instances the exact
// walk's axis table, c.ax) and 2 words component-major at b[0], b[NL] (there the bounce stack's
// bottom entry): both regions belong to this lane alone, and it is done with the tree before its
// exact path (if any) uses them. (A slot striped over the whole workgroup's pool would overwrite
// the other wave's axis table in the middle of its exact walks.)
constexpr int kTreeWords = 14;
template <int NL>
__device__ __forceinline__ void tree_put(float4* __restrict__ a, float* __restrict__ b, const TreeRay& t) {
  a[0] = make_float4(t.ray.pos.x, t.ray.pos.y, t.ray.pos.z, t.ray.dir.x);
  a[1] = make_float4(t.ray.dir.y, t.ray.dir.z, t.ray.len, t.ray.energy);
  a[2] = make_float4(t.e0, t.ed.x, t.ed.y, t.ed.z);
  // cells in [0, 1024); a stored ray is a reflection ray: medium air
  b[0] = __uint_as_float(uint32_t(t.cx) | uint32_t(t.cy) << 10 | uint32_t(t.cz) << 20);
  b[NL] = __uint_as_float(uint32_t(t.ray.rdepth) | uint32_t(t.ray.tdepth) << 16);
}
template <int NL>
__device__ __forceinline__ TreeRay tree_get(const float4* __restrict__ a, const float* __restrict__ b) {
  TreeRay t;
  const float4 a0 = a[0], a1 = a[1], a2 = a[2];
  t.ray.pos = mk(a0.x, a0.y, a0.z);
  t.ray.dir = mk(a0.w, a1.x, a1.y);
  t.ray.len = a1.z;
  t.ray.energy = a1.w;
  t.e0 = a2.x;
  t.ed = mk(a2.y, a2.z, a2.w);
  const uint32_t w = __float_as_uint(b[0]);
  t.cx = int(w & 1023u);
  t.cy = int((w >> 10) & 1023u);
  t.cz = int((w >> 20) & 1023u);
  const uint32_t dp = __float_as_uint(b[NL]);
  t.ray.rdepth = int(dp & 0xffffu);
  t.ray.tdepth = int(dp >> 16);
  t.ray.voxel = 0u;
  return t;
}

// The certified start of a child ray from the certified hit h of its parent (direction d0 there):
// the start cell, checked inside the volume, and cert_start's bounds. false: unsure.
__device__ __forceinline__ bool tree_start(const Ctx& c, const CertResult& h, const Hit& hh, const f3 d0,
                                           TreeRay& t) {
  if (!fast_path_ok(t.ray.dir)) return false;
  const uint32_t n = uint32_t(c.n);
  if (uint32_t(t.cx) >= n || uint32_t(t.cy) >= n || uint32_t(t.cz) >= n) { CERT_DIAG(31); return false; }
  const f3 rn = mk(__builtin_amdgcn_rcpf(t.ray.dir.x), __builtin_amdgcn_rcpf(t.ray.dir.y),
                   __builtin_amdgcn_rcpf(t.ray.dir.z));
  t.e0 = h.eu;
  return cert_start(hh.point, d0, t.ray.dir, rn, h.axis, h.eu, t.cx, t.cy, t.cz, t.ed);
}

// GetReflectionRay (voxel.glsl:203-215) of a certified hit: the direction must not depend on the
// point (RandomizeDirection's zero-noise identity); it starts back in the cell before the face
template <bool TEX>
__device__ __forceinline__ bool tree_reflection(const Ctx& c, const Ray& ray, const CertResult& h, const Hit& hh,
                                                TreeRay& t) {
  if (!(c.refl_noise == 0.0f && zero_noise_exact(reflect3(ray.dir, hh.normal)))) return false;
  t.ray = reflection_ray(c, ray, hh);
  cell_before(h, ray.dir, t.cx, t.cy, t.cz);
  return tree_start(c, h, hh, ray.dir, t);
}

// GetRefractionRay (voxel.glsl:217-246) of a certified hit: the probes at point +- normal / 2
// (:219-220) read the exact point's cells when the point is robust on the other axes (cert_start
// checks it); total internal reflection turns it into the reflection ray, back before the face
template <bool TEX>
__device__ __forceinline__ bool tree_refraction(const Ctx& c, const Ray& ray, const CertResult& h, const Hit& hh,
                                                TreeRay& t) {
  const float eta = mat_refr(get_voxel(c, hh.point + hh.normal * 0.5f)) /
                    mat_refr(get_voxel(c, hh.point - hh.normal * 0.5f));
  const f3 rd = refract3(normalize3(ray.dir), hh.normal, eta);
  const bool tir = rd.x == 0.0f && rd.y == 0.0f && rd.z == 0.0f;
  if (tir ? !(c.refl_noise == 0.0f && zero_noise_exact(reflect3(ray.dir, hh.normal)))
          : !(c.refr_noise == 0.0f && zero_noise_exact(rd)))
    return false;
  Counters kk;
#pragma unroll
  for (int q = 0; q < VRT_CNT_COUNT; ++q) kk.c[q] = 0;
  t.ray = refraction_ray<TEX>(c, ray, hh, kk);
  t.cx = h.cx;  // into the hit cell, or (total internal reflection) back before it
  t.cy = h.cy;
  t.cz = h.cz;
  if ((comp(t.ray.dir, h.axis) > 0.0f) != (comp(ray.dir, h.axis) > 0.0f)) cell_before(h, ray.dir, t.cx, t.cy, t.cz);
  return tree_start(c, h, hh, ray.dir, t);
}

// One ray of a certified tree: the colour update of `ray`'s walk outcome h, its children, then the
// walk of the ray the reference pops next (ray, h updated). kTreeDone: the tree is complete (colour
// final); kTreeUnsure: it cannot be certified (colour meaningless); kTreeNext: continue with ray, h.
constexpr int kTreeNext = 0, kTreeDone = 1, kTreeUnsure = -1;
template <int NL, bool LEAN = false>
__device__ __forceinline__ int tree_step(const Ctx& c, int max_refl, int max_transp, Ray& ray, CertResult& h,
                                         f3& color, bool& pending, float4* __restrict__ lta,
                                         float* __restrict__ ltb) {
  // the sun vector opaque per ray, as in the exact path's bounce loop (trace_with_shadow): else
  // the shadow walk's per-sun products are hoisted into VGPRs live across the whole tree and
  // spilled on its entry
  Ctx lc = c;
  asm volatile("" : "+s"(lc.sun_n.x), "+s"(lc.sun_n.y), "+s"(lc.sun_n.z), "+s"(lc.sun_rcp.x),
               "+s"(lc.sun_rcp.y), "+s"(lc.sun_rcp.z));
  bool next = false;
  TreeRay t;
  CTRACE(c, 200, h.res, h.byte, h.axis, h.u, h.eu, ray.rdepth, ray.tdepth);
  CTRACE(c, 201, ray.pos.x, ray.pos.y, ray.pos.z, ray.dir.x, ray.dir.y, ray.dir.z, ray.len);
  CTRACE(c, 202, color.x, color.y, color.z, ray.energy, h.cx, h.cy, h.cz);
  if (h.res == CERT_MISS) {
    apply_sky_color(c, ray, color);
  } else {
    const Hit hh = cert_hit_record(ray, h);
    if (!cert_shade_hit<false, LEAN>(lc, ray, h, hh, color)) { CERT_DIAG(22); return kTreeUnsure; }
    // children (:440-448): the reflection ray is pushed first, the refraction ray second and
    // popped first; the stack (R + T + 1 entries) never fills with at most one ray waiting
    const uint32_t m = mat_id(h.byte);
    const bool pr = mat_reflective(m) && ray.rdepth < max_refl;
    const bool pt = mat_transparent(m) && ray.tdepth < max_transp && get_color<false>(c, hh).w != 1.0f;
    if (pr && pt) {
      if (pending) { CERT_DIAG(18); return kTreeUnsure; }
      TreeRay r;
      if (!tree_reflection<false>(c, ray, h, hh, r)) { CERT_DIAG(19); return kTreeUnsure; }
      tree_put<NL>(lta, ltb, r);
      pending = true;
      if (!tree_refraction<false>(c, ray, h, hh, t)) { CERT_DIAG(20); return kTreeUnsure; }
      next = true;
    } else if (pr) {
      if (!tree_reflection<false>(c, ray, h, hh, t)) { CERT_DIAG(19); return kTreeUnsure; }
      next = true;
    } else if (pt) {
      if (!tree_refraction<false>(c, ray, h, hh, t)) { CERT_DIAG(20); return kTreeUnsure; }
      next = true;
    }
  }
  if (!next) {
    if (!pending) { CERT_DIAG(17); return kTreeDone; }
    pending = false;
    t = tree_get<NL>(lta, ltb);
  }
  ray = t.ray;
  h = cert_march<LEAN>(c, ray, t.cx, t.cy, t.cz, t.e0, t.ed);
  if (h.res == CERT_UNSURE) { CERT_DIAG(21); return kTreeUnsure; }
  CERT_DIAG(23);
  return kTreeNext;
}

// The bounce tree of a glass primary hit h0 of ray0 (fragment main, voxel.glsl:425-452) by
// certified walks, colour folded in the reference's DFS order as TraceWithShadow does (:395-423):
// each ray's RayMarch by cert_march, its hit shaded with a certified shadow (none for glass), a
// miss with the sky colour. Colour-only (TEX false) frames. Returns false, colour untouched, when
// any walk, start or direction could differ from the exact path's.
// (Walking the primary ray through this loop too, one walk call site for every ray, made the
// certified pass 3x slower: every pixel then carried the tree's registers; r06_s4.)
// lta / ltb: this lane's LDS slot (tree_put; NL lanes per workgroup).
template <int NL, bool LEAN = false>
__device__ __forceinline__ bool cert_tree(const Ctx& c, int max_refl, int max_transp, const Ray& ray0,
                                          const CertResult& h0, f3& color_out, float4* __restrict__ lta,
                                          float* __restrict__ ltb) {
  f3 color = mk(0.0f, 0.0f, 0.0f);
  Ray ray = ray0;
  CertResult h = h0;
  bool pending = false;  // a reflection ray waits in the LDS slot
  CERT_DIAG(16);
  for (;;) {
    const int r = tree_step<NL, LEAN>(c, max_refl, max_transp, ray, h, color, pending, lta, ltb);
    if (r == kTreeUnsure) return false;
    if (r == kTreeDone) break;
  }
  color_out = color;
  return true;
}

// The exact walk's start cell from P along D (voxel.glsl:306-309: first planes d < 0 ? ceil(p - 1)
// : floor(p + 1)); false when it lies outside the volume or a plane disagrees with the cell's.
__device__ __forceinline__ bool exact_start_cell(const Ctx& c, const f3 P, const f3 D, int& cx, int& cy,
                                                 int& cz) {
  const int sx = D.x > 0.0f ? 1 : -1, sy = D.y > 0.0f ? 1 : -1, sz = D.z > 0.0f ? 1 : -1;
  cx = sx > 0 ? int(__builtin_floorf(P.x)) : int(__builtin_ceilf(P.x)) - 1;
  cy = sy > 0 ? int(__builtin_floorf(P.y)) : int(__builtin_ceilf(P.y)) - 1;
  cz = sz > 0 ? int(__builtin_floorf(P.z)) : int(__builtin_ceilf(P.z)) - 1;
  const float wpx = sx > 0 ? __builtin_floorf(P.x + 1.0f) : __builtin_ceilf(P.x - 1.0f);
  const float wpy = sy > 0 ? __builtin_floorf(P.y + 1.0f) : __builtin_ceilf(P.y - 1.0f);
  const float wpz = sz > 0 ? __builtin_floorf(P.z + 1.0f) : __builtin_ceilf(P.z - 1.0f);
  const uint32_t n = uint32_t(c.n);
  if (uint32_t(cx) >= n || uint32_t(cy) >= n || uint32_t(cz) >= n) return false;
  return wpx == float(cx + (sx > 0)) && wpy == float(cy + (sy > 0)) && wpz == float(cz + (sz > 0));
}

// Cells the exact walk samples behind its start cell. A start coordinate P_a that is an integer k
// with D_a < 0 (a shadow or secondary ray from an exact hit point on its face plane) makes the
// start cell k - 1 on axis a, but until cur_a = P_a + s D_a rounds off k the exact walk samples
// layer k — beyond the plane — at every crossing of another axis (r02 s18: a shadow ray from
// (33.000008, 127, 37.02) going -x, -y sampled the panel voxel (32, 127, 37) at its x crossing
// 8.5e-6 after the start; the certified walk had jumped that crossing). The certified walk cannot
// see those cells, so they are checked here: every cell of layer k the walk may enter across an
// axis crossed within 2 ulp(k) / |D_a| (+1e-5) of the start must be a non-event, else unsure.
template <bool SHADOW>
__device__ __forceinline__ bool start_layers_clear(const Ctx& c, const f3 P, const f3 D, int cx, int cy,
                                                   int cz, uint32_t medium) {
  const float p[3] = {P.x, P.y, P.z}, d[3] = {D.x, D.y, D.z};
  const int cell[3] = {cx, cy, cz};
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    if (!(d[a] < 0.0f) || p[a] != __builtin_floorf(p[a])) continue;
    const float off = (0x1p-22f * __builtin_fmaxf(__builtin_fabsf(p[a]), 1.0f) + 1e-5f) / __builtin_fabsf(d[a]);
    // two crossings of one axis b in layer k (a nearly parallel D_a keeps cur_a on k: a
    // straight-down lattice camera's ray at x = 64 with D_x = -2.2e-8 read plane N's GL_REPEAT
    // copy for 170 units) need off >= 1 / |D_b| >= 1: more cells than checked here, unsure
    if (off >= 1.0f) return false;
    int q[3] = {cell[0], cell[1], cell[2]};
    q[a] += 1;  // layer k
    bool early[3] = {false, false, false};
#pragma unroll
    for (int b = 0; b < 3; ++b) {
      if (b == a) continue;
      const float plane = float(cell[b] + (d[b] > 0.0f ? 1 : 0));
      early[b] = (plane - p[b]) / d[b] < off;  // first crossing of axis b
    }
    const int b1 = a == 0 ? 1 : 0, b2 = a == 2 ? 1 : 2;
    const int s1 = d[b1] > 0.0f ? 1 : -1, s2 = d[b2] > 0.0f ? 1 : -1;
    // shadow walks: the exact walk may cross b in layer k and so never sample the start layer's
    // cell across b, which the certified walk reaches by that crossing and, if it blocks,
    // reports as a hit "whichever way the walk goes" (a straight-down lattice camera's shadow
    // from x = 33.0 going -x sampled (33, 30, 2) at its z crossing and never the solid (32, 30,
    // 2)): unsure whenever a crossing falls in the sliver
    if (SHADOW && (early[b1] || early[b2])) return false;
    int r[3];
    if (early[b1]) {
      r[0] = q[0]; r[1] = q[1]; r[2] = q[2]; r[b1] += s1;
      if (cert_event<SHADOW>(alt_byte(c, r[0], r[1], r[2], 0u), medium)) return false;
    }
    if (early[b2]) {
      r[0] = q[0]; r[1] = q[1]; r[2] = q[2]; r[b2] += s2;
      if (cert_event<SHADOW>(alt_byte(c, r[0], r[1], r[2], 0u), medium)) return false;
    }
    if (early[b1] && early[b2]) {
      r[0] = q[0]; r[1] = q[1]; r[2] = q[2]; r[b1] += s1; r[b2] += s2;
      if (cert_event<SHADOW>(alt_byte(c, r[0], r[1], r[2], 0u), medium)) return false;
    }
  }
  return true;
}

// The shadow bit of an exact hit h by a certified walk: the shadow ray starts at the exact hit
// point h.point with len h.len (GetShadowRay, :191-201), so its start is known exactly, as a
// primary ray's is (e0 = 0, the exact walk's own start cell). 1 blocked, 0 lit, -1 unsure.
__device__ __forceinline__ int cert_shadow_exact(const Ctx& c, const Hit& h) {
  const f3 S = c.sun_n;
  int cx, cy, cz;
  if (!fast_path_ok(S) || !exact_start_cell(c, h.point, S, cx, cy, cz)) return -1;
  if (!start_layers_clear<true>(c, h.point, S, cx, cy, cz, 0u)) return -1;
  const CertResult s = cert_walk<true, false, false>(c, h.point, S, c.sun_rcp, c.max_len - h.len, cx, cy, cz,
                                                     0.0f, mk(0.0f, 0.0f, 0.0f), h.len, 0u);
  return s.res == CERT_UNSURE ? -1 : (s.res == CERT_HIT ? 1 : 0);
}

// An air segment of a bounce-stack ray by a certified walk from the exact point ray.pos (len
// ray.len) in cell (cx, cy, cz); ed: per-axis crossing-order uncertainty of the exact walk's
// planes. In an air medium every event is a hit (:353), and a non-glass hit spawns no rays
// (:440-448). true (colour updated as TraceWithShadow's, :395-423): a miss, or a non-glass hit
// whose shadow certifies. false (colour untouched): the exact march goes on.
__device__ __forceinline__ bool cert_air_segment(const Ctx& c, const Ray& ray, int cx, int cy, int cz,
                                                 const f3 ed, f3& color) {
  const f3 D = ray.dir;
  const f3 rcp = mk(__builtin_amdgcn_rcpf(D.x), __builtin_amdgcn_rcpf(D.y), __builtin_amdgcn_rcpf(D.z));
  const CertResult h = cert_walk<false>(c, ray.pos, D, rcp, c.max_len - ray.len, cx, cy, cz, 0.0f, ed,
                                        ray.len, 0u);
  if (h.res == CERT_UNSURE) return false;
  if (h.res == CERT_MISS) {
    apply_sky_color(c, ray, color);
    return true;
  }
  if (mat_id(h.byte) == 2u) return false;
  return cert_shade_hit(c, ray, h, cert_hit_record(ray, h), color);
}

// A secondary ray from an exact origin (the reflection or refraction ray of an exact hit) in air:
// its walk certifies as a primary's does
__device__ __forceinline__ bool cert_secondary(const Ctx& c, const Ray& ray, f3& color) {
  int cx, cy, cz;
  if (ray.voxel != 0u || !fast_path_ok(ray.dir) || !exact_start_cell(c, ray.pos, ray.dir, cx, cy, cz) ||
      !start_layers_clear<false>(c, ray.pos, ray.dir, cx, cy, cz, 0u))
    return false;
  return cert_air_segment(c, ray, cx, cy, cz, mk(0.0f, 0.0f, 0.0f), color);
}

// The rest of a march after an in-volume refraction into air at the exact crossing w.cur of axis
// fa (march, :357-380): the exact walk goes on from pos = cur, len0 = w.len, with the first
// planes initial_t's on the other axes and cur_fa + sign on axis fa. That plane lies within
// delta = |(cur_fa + sign) - (k + sign)| of the lattice plane (k = rint(cur_fa)), and every later
// axis-fa plane of the walk (cur_fa + sign at each crossing) keeps that offset: the certified walk
// starts in the cell beyond k and takes delta |1/d_fa| (doubled) as that axis's crossing-order
// uncertainty. The step cap (VRT_MAX_STEPS per march) must be out of reach: <= 3N + 4 more steps.
__device__ __forceinline__ bool cert_continuation(const Ctx& c, const Ray& ray, const WalkState& w, int fa,
                                                  f3& color) {
  const f3 D = ray.dir, P = ray.pos;
  if (!fast_path_ok(D) || w.it + 3u * uint32_t(c.n) + 16u > uint32_t(VRT_MAX_STEPS)) return false;
  int cx, cy, cz;
  const float pa = comp(P, fa), da = comp(D, fa);
  const float k = __builtin_rintf(pa);
  const float sa = da > 0.0f ? 1.0f : -1.0f;
  const float delta = __builtin_fabsf((pa + sa) - (k + sa));
  if (!(delta < 1e-3f)) return false;
  // the other axes as a fresh walk's start; axis fa replaced below
  {
    const int sx = D.x > 0.0f ? 1 : -1, sy = D.y > 0.0f ? 1 : -1, sz = D.z > 0.0f ? 1 : -1;
    cx = sx > 0 ? int(__builtin_floorf(P.x)) : int(__builtin_ceilf(P.x)) - 1;
    cy = sy > 0 ? int(__builtin_floorf(P.y)) : int(__builtin_ceilf(P.y)) - 1;
    cz = sz > 0 ? int(__builtin_floorf(P.z)) : int(__builtin_ceilf(P.z)) - 1;
    const float wpx = sx > 0 ? __builtin_floorf(P.x + 1.0f) : __builtin_ceilf(P.x - 1.0f);
    const float wpy = sy > 0 ? __builtin_floorf(P.y + 1.0f) : __builtin_ceilf(P.y - 1.0f);
    const float wpz = sz > 0 ? __builtin_floorf(P.z + 1.0f) : __builtin_ceilf(P.z - 1.0f);
    if ((fa != 0 && wpx != float(cx + (sx > 0))) || (fa != 1 && wpy != float(cy + (sy > 0))) ||
        (fa != 2 && wpz != float(cz + (sz > 0))))
      return false;
    // Another axis b on a plane and moving down (P_b an integer, D_b < 0) puts the cell above at
    // P_b - 1, but the exact walk samples the layer beyond the plane until cur_b rounds off it, as at
    // a fresh start (start_layers_clear). That layer is not checked here: unsure. (A camera straight
    // above glass clutter, z = 16.0 and D_z = -6e-17 after each refraction: the continuations walked
    // layer 15 while the exact walk stayed in layer 16 to the end; one pixel of the frame differed.)
    if ((fa != 0 && D.x < 0.0f && P.x == __builtin_floorf(P.x)) || (fa != 1 && D.y < 0.0f && P.y == __builtin_floorf(P.y)) ||
        (fa != 2 && D.z < 0.0f && P.z == __builtin_floorf(P.z)))
      return false;
    const int ka = int(k) - (da > 0.0f ? 0 : 1);
    if (fa == 0) cx = ka;
    else if (fa == 1) cy = ka;
    else cz = ka;
  }
  const uint32_t n = uint32_t(c.n);
  if (uint32_t(cx) >= n || uint32_t(cy) >= n || uint32_t(cz) >= n) return false;
  // the start cell lies beyond plane k on axis fa, but P_fa may lie before it (by up to delta) or
  // on it: until cur_fa = P_fa + s D_fa is past k, the exact walk samples the layer before k at
  // every crossing of another axis (as start_layers_clear's layer k for a start on a plane), which
  // the certified walk does not see (a glass cube's face voxel beside the refraction point,
  // sampled 3.7e-6 after the start, made a lattice camera's pixel differ before this test):
  // unsure when another axis is crossed that early. By the hardware reciprocal (<= 1 ulp) against
  // a bound widened past its error: never fewer cases than the exact quotients would give.
  {
    const float before = __builtin_fmaxf((k - pa) * sa, 0.0f);
    const float off = (before + 0x1p-22f * __builtin_fmaxf(__builtin_fabsf(pa), 1.0f) + 1e-5f) *
                      __builtin_fabsf(__builtin_amdgcn_rcpf(da)) * 1.00002f;
    const float tx = fa == 0 ? off : (float(cx + (D.x > 0.0f ? 1 : 0)) - P.x) * __builtin_amdgcn_rcpf(D.x);
    const float ty = fa == 1 ? off : (float(cy + (D.y > 0.0f ? 1 : 0)) - P.y) * __builtin_amdgcn_rcpf(D.y);
    const float tz = fa == 2 ? off : (float(cz + (D.z > 0.0f ? 1 : 0)) - P.z) * __builtin_amdgcn_rcpf(D.z);
    if (__builtin_fminf(tx, __builtin_fminf(ty, tz)) < off) return false;
  }
  f3 ed = mk(0.0f, 0.0f, 0.0f);
  set_comp(ed, fa, 2.0f * delta * __builtin_fabsf(__builtin_amdgcn_rcpf(da)) + 1e-6f);
  return cert_air_segment(c, ray, cx, cy, cz, ed, color);
}

// RayMarch + TraceWithShadow of a bounce-stack ray (stats-free, colour-only) with its air
// segments — the whole ray from its exact origin, or the rest after an in-volume refraction into
// air — settled by certified walks where they can be (settled: colour updated, no secondary
// rays); the exact march (as march()) otherwise.
// (Out of line it costs C2-C4 +45 %, profiles/r01_v69_ab_noinline_w6.log.)
__device__ __forceinline__ Hit march_cert(const Ctx& c, Ray& ray, f3& color, bool& settled, Counters& k,
                          uint32_t& steps, uint32_t& flags) {
  Hit h;
  h.found = false;
  h.vidx = -1;
  h.len = 0.0f;
  h.voxel = 0;
  h.point = mk(0.0f, 0.0f, 0.0f);
  h.normal = h.point;
  h.axis = 0;
  settled = cert_secondary(c, ray, color);
  if (settled) return h;
  WalkState w;
  walk_init(w, ray);
  uint32_t medium = ray.voxel;
  int internal = 0;
  for (;;) {
    int axis;
    int32_t vidx;
    uint32_t v;
    const int r = walk_ray<false>(c, ray.pos, ray.dir, ray.len, medium, w, axis, vidx, v);
    if (r != WALK_EVENT) break;
    f3 normal = mk(0.0f, 0.0f, 0.0f);
    set_comp(normal, axis, -gsign(comp(ray.dir, axis)));
    if (v != 0u) {
      h.found = true;
      h.voxel = v;
      h.vidx = vidx;
      h.point = w.cur;
      h.len = w.len;
      h.normal = normal;
      h.axis = axis;
      break;
    }
    Hit e;
    e.found = true;
    e.voxel = 0;
    e.vidx = vidx;
    e.point = w.cur;
    e.len = w.len;
    e.normal = normal;
    e.axis = axis;
    const f3 old_dir = ray.dir;
    ray = refraction_ray<false>(c, ray, e, k);
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
    if (medium == 0u && cert_continuation(c, ray, w, axis, color)) {
      settled = true;
      return h;
    }
  }
  return h;
}

// The whole pixel by certified walks, when it can be certified: a primary miss, or a non-glass
// primary hit with its shadow. The pixel's colour starts black (voxel.glsl:428); color_out is
// written only when the pixel certifies. false when any walk or any derived value could differ
// from the exact path's, or the hit is glass (its secondary rays start at the exact hit point):
// the pixel then takes the exact path.
// Textured mode: the texel GetColor (voxel.glsl:174-182) reads at the exact hit point, from the
// certified hit. The exact hit point is currentPos of the exact walk's hit step; on each face axis
// it lies within delta = eu |D_b| + the roundings of both points' pos + s dir of the certified
// point (eu bounds the exact walk's parameter there, cert_gamma). get_color's texel index is a
// composition of correctly rounded monotone operations of the coordinate (frac by floor, + texX,
// x ts, / S, floor(. x S)), so if both ends of [p - delta, p + delta] lie in the same voxel and give
// the same texel, every point between does: the exact texel is that one. false: unsure.
__device__ __forceinline__ bool texel_pair(const Ctx& c, float p, float d, uint32_t slot, bool flip, uint32_t& t) {
  const float lo = p - d, hi = p + d;
  if (__builtin_floorf(lo) != __builtin_floorf(hi)) return false;
  auto idx = [&](float q) {
    const float f = q - floorf(q);
    if (!flip) {  // tx = ((fx + texX) * ts) / S, u = tx
      const float u = ((f + float(slot)) * c.atlas_fts) / c.atlas_fs;
      return cvt_flr(u * c.atlas_fs) & c.atlas_mask;
    }
    const float ty = (((1.0f - f) + float(slot)) * c.atlas_fts) / c.atlas_fs;  // v = 1 - ty
    return cvt_flr((1.0f - ty) * c.atlas_fs) & c.atlas_mask;
  };
  t = idx(lo);
  return t == idx(hi);
}

__device__ __forceinline__ bool cert_texel(const Ctx& c, const Ray& ray, const CertResult& h, const Hit& hh,
                                           float4& col) {
  const uint32_t m = mat_id(h.byte);
  const float px = hh.axis == 0 ? hh.point.z : hh.point.x;  // intersectionAxis[a][1]
  const float py = hh.axis == 2 ? hh.point.y : (hh.axis == 1 ? hh.point.z : hh.point.y);  // [a][2]
  const float dx = hh.axis == 0 ? ray.dir.z : ray.dir.x;
  const float dy = hh.axis == 2 ? ray.dir.y : (hh.axis == 1 ? ray.dir.z : ray.dir.y);
  const float px0 = hh.axis == 0 ? ray.pos.z : ray.pos.x;
  const float py0 = hh.axis == 2 ? ray.pos.y : (hh.axis == 1 ? ray.pos.z : ray.pos.y);
  // eu along the ray, plus 2 ulp-scale roundings of each point's P + s D (both points), doubled
  const float ex = h.eu * __builtin_fabsf(dx) +
                   0x1p-21f * (__builtin_fabsf(px0) + __builtin_fabsf(h.u * dx) + __builtin_fabsf(px) + 1.0f);
  const float ey = h.eu * __builtin_fabsf(dy) +
                   0x1p-21f * (__builtin_fabsf(py0) + __builtin_fabsf(h.u * dy) + __builtin_fabsf(py) + 1.0f);
  uint32_t i, j;
  if (!texel_pair(c, px, ex, mat_tex_x(m), false, i) || !texel_pair(c, py, ey, mat_tex_y(m), true, j)) return false;
  const uint32_t t = c.atlas[j * (c.atlas_mask + 1u) + i];
  col = make_float4(float(t & 0xFFu) / 255.0f, float((t >> 8) & 0xFFu) / 255.0f,
                    float((t >> 16) & 0xFFu) / 255.0f, float(t >> 24) / 255.0f);
  return true;
}

// the Ctx fields init_ctx<true> leaves out: the same values from the same words
__device__ __forceinline__ void late_ctx(Ctx& c) {
  LateKArgs* ka = late_kargs();
  c.sky_sy = ka->sky_sy;
  c.sun_n = mk(ka->sun_n[0], ka->sun_n[1], ka->sun_n[2]);
  c.sun_rcp = mk(ka->sun_rcp[0], ka->sun_rcp[1], ka->sun_rcp[2]);
  c.atlas = ka->atlas;
  c.atlas_mask = uint32_t(ka->atlas_size) - 1u;
  c.atlas_fs = float(ka->atlas_size);
  c.atlas_fts = float(ka->atlas_tex_size);
}
// TREE (colour-only): a glass primary hit's bounce tree by certified walks too (cert_tree; ltb and c.ax its
// LDS slot), instead of leaving the whole pixel to the exact path.
// us_out: the primary walk's certified prefix (CertResult::us) for the exact path, -1 if none.
// ak (LEAN): the launch's arguments, for the start's launch constants (KArgs::walk_b0 .. start_cell).
template <bool TEX = false, bool TREE = false, int NL = kWgThreads, bool LEAN = false>
__device__ __forceinline__ bool cert_pixel(const Ctx& c0, const Ray& ray0, f3& color_out, int max_refl = 0,
                                           int max_transp = 0, float* __restrict__ ltb = nullptr,
                                           float* us_out = nullptr, const KArgs* ak = nullptr) {
  const f3 P = ray0.pos, D = ray0.dir;
  int cx, cy, cz;
  CertStartK st;
  if constexpr (LEAN) {
    // The start as one predicate, sign-folded as the walk is: q_b = s_b P_b, fl_b = floor(q_b), the cell
    // int(fl_b) ^ m_b. Negation commutes with rounding, so moving down floor(-P) = -ceil(P): the cell
    // ~floor(-P) is ceil(P) - 1 and the plane test floor(-P + 1) == floor(-P) + 1 is ceil(P - 1) ==
    // float(ceil(P) - 1) negated on both sides. Moving up it is exact_start_cell's own test: for a cell
    // in the volume float(c + 1) = fl + 1 exactly, and for any other cell the bounds fail in both forms.
    // fast_path_ok(D), the bounds and the planes are ANDed without a branch; the cells mean something
    // only when the predicate holds. The on-plane trigger, start_layers_clear's per-axis entry test
    // (D_b < 0 and P_b an integer: fast_path_ok excludes D_b = 0, where D_b < 0 and !(D_b > 0) differ),
    // puts that function, unchanged, behind one region.
    // (tests/test_cert_start_lit_forms.py: both forms over the sign octants and the edge positions)
    //
    // kSetupCell (KArgs::setup, wave-uniform; cert_launch_consts in vrt_launch_consts.cpp): the host has proved
    // that every pixel's P_b of the launch lies strictly inside one cell c_b of the volume, at least 2^-9
    // from its planes. Then floor(P_b) = c_b and floor(-P_b) = -c_b - 1 (P_b is no integer), so fl_b + 1
    // is a select of two launch constants and the cell is c_b whatever the sign; the bounds hold; the plane
    // tests hold (q + 1 rounds by at most 2^-14 at q < 1025, inside the margin); the trigger is false
    // (fl_b != q_b). Only fast_path_ok(D) and the sign fold are left to the lane.
    const bool ux = D.x > 0.0f, uy = D.y > 0.0f, uz = D.z > 0.0f;
    st.Ps = mk(ux ? P.x : -P.x, uy ? P.y : -P.y, uz ? P.z : -P.z);
    st.mx = ux ? 0 : -1;
    st.my = uy ? 0 : -1;
    st.mz = uz ? 0 : -1;
    st.b0 = ak->walk_b0;
    st.U2 = ak->max_len2;  // (ray0.len = 0: the walk's U is max_len)
    bool ok;
    if ((ak->setup & kSetupCell) != 0u) {
      st.fl1 = mk(ux ? ak->start_fl1[0] : ak->start_fl1[3], uy ? ak->start_fl1[1] : ak->start_fl1[4],
                  uz ? ak->start_fl1[2] : ak->start_fl1[5]);
      cx = ak->start_cell[0];
      cy = ak->start_cell[1];
      cz = ak->start_cell[2];
      ok = fast_path_ok(D);
    } else {
      const f3 fl = mk(__builtin_floorf(st.Ps.x), __builtin_floorf(st.Ps.y), __builtin_floorf(st.Ps.z));
      st.fl1 = mk(fl.x + 1.0f, fl.y + 1.0f, fl.z + 1.0f);
      cx = int(fl.x) ^ st.mx;
      cy = int(fl.y) ^ st.my;
      cz = int(fl.z) ^ st.mz;
      ok = int(fast_path_ok(D)) & int(max(max(uint32_t(cx), uint32_t(cy)), uint32_t(cz)) < uint32_t(c0.n)) &
           int(__builtin_floorf(st.Ps.x + 1.0f) == st.fl1.x) & int(__builtin_floorf(st.Ps.y + 1.0f) == st.fl1.y) &
           int(__builtin_floorf(st.Ps.z + 1.0f) == st.fl1.z);
      const bool on_plane = (int(!ux) & int(fl.x == st.Ps.x)) | (int(!uy) & int(fl.y == st.Ps.y)) |
                            (int(!uz) & int(fl.z == st.Ps.z));
      if (ok & on_plane) ok = start_layers_clear<false>(c0, P, D, cx, cy, cz, 0u);
    }
    if (!ok) { CERT_DIAG(0); return false; }
  } else {
    if (!fast_path_ok(D)) { CERT_DIAG(0); return false; }
    if (!exact_start_cell(c0, P, D, cx, cy, cz) || !start_layers_clear<false>(c0, P, D, cx, cy, cz, 0u)) {
      CERT_DIAG(0);
      return false;
    }
  }
  // hardware reciprocals (<= 1 ulp): the certified walk only needs its own error bounded
  const f3 rcp = mk(__builtin_amdgcn_rcpf(D.x), __builtin_amdgcn_rcpf(D.y), __builtin_amdgcn_rcpf(D.z));
  CertResult h = cert_walk<false, LEAN, false>(c0, P, D, rcp, c0.max_len - ray0.len, cx, cy, cz, 0.0f,
                                               mk(0.0f, 0.0f, 0.0f), 0.0f, 0u, ~0u, LEAN ? &st : nullptr);
  if (us_out) *us_out = h.us;
  CERT_DIAG_ONLY(cert_diag_iters(10, h.iters);)
  if (LEAN && (PHASE_STOP(2) || PHASE_STOP(3))) {  // phase budget: the primary walk's result as the colour
    color_out = mk(h.u, h.eu, float(h.cx + h.cy + h.cz + h.axis + int(h.byte) + h.res));
    return true;
  }
  if (h.res == CERT_UNSURE) { CERT_DIAG(1); return false; }
  Ctx c = c0;  // LEAN: with the sun, the sky and the atlas read here (late_ctx)
  if constexpr (LEAN) late_ctx(c);
  f3 color = mk(0.0f, 0.0f, 0.0f);
  if (h.res == CERT_MISS) {
    CERT_DIAG(2);
    if (!(LEAN && PHASE_STOP(6))) apply_sky_color<LEAN && kCutSky>(c, ray0, color);
    color_out = color;
    return true;
  }
  if (mat_id(h.byte) == 2u) {  // only glass spawns secondary rays (:440-448)
    CERT_DIAG(3);
    if constexpr (TREE && !TEX) return cert_tree<NL, LEAN>(c, max_refl, max_transp, ray0, h, color_out, c.ax, ltb);
    return false;
  }
  const Hit hh = LEAN ? cert_hit_record_primary(ray0, h) : cert_hit_record(ray0, h);
  float4 col = float4();
  if (TEX && !cert_texel(c, ray0, h, hh, col)) return false;
  if constexpr (LEAN) {  // the sun's constants from the launch's arguments, read here, after the primary walk
    if (!cert_shade_hit<TEX, true, true>(c, ray0, h, hh, color, col, late_kargs())) return false;
  } else {
    if (!cert_shade_hit<TEX, false>(c, ray0, h, hh, color, col)) return false;
  }
  color_out = color;
  return true;
}

}  // namespace vrt

#endif  // VRT_CERT_H
