// vrt_cert_debug_kernels.h — certified walks for a ray list (vrt_debug_cert_walks): one kernel that starts
// vrt_cert.h's certified walk for each listed ray the way the frame kernels start it for a ray from an exact
// origin, one ray per lane, and writes the walk's result. A test hook: it hands a listed ray to cert_walk, which
// no frame or query does, so that the walk can be held to the exact walk ray by ray at the rays that reach its
// rare blocks. Included by vrt_render.hip after init_ctx, which it calls; it changes nothing the frames run.
#ifndef VRT_CERT_DEBUG_KERNELS_H
#define VRT_CERT_DEBUG_KERNELS_H

#include "vrt_cert.h"

namespace vrt {

constexpr int kCertDebugWg = 64;
constexpr int kCertNotStarted = 3;  // the fourth value of a record's res: a start check refused the ray
static_assert(kCertNotStarted != CERT_MISS && kCertNotStarted != CERT_HIT && kCertNotStarted != CERT_UNSURE, "");
// a listed ray's lengths: cert_walk's bound is a polynomial in len0, and an infinite or NaN coefficient would
// pass its jump test (fminf drops a NaN); the frames' lengths are below max_len + a volume's diagonal
constexpr float kCertDebugMaxLen = 1.0e4f;

// kind & 1: 0 the air walk as cert_secondary starts it (cert_walk<false>, medium 0, reciprocals as
// cert_air_segment forms them), 1 the shadow walk as cert_shadow_exact starts it with the ray's own direction
// for the sun (cert_walk<true, .., false>, reciprocals RN(1 / d) as the launch's sun_rcp); kind & 2: the LEAN
// forms of the same two walks. A ray is a vrt_ray with the reserved word read as float len0, its max_length in
// the lane's Ctx as ray_query_kernel does; no uncertain origin (e0 = 0, ed = 0, len0b = len0).
// The start checks are the callers': fast_path_ok, exact_start_cell, start_layers_clear<SHADOW>. They give what
// the LEAN walk's unguarded loads assume: the start cell is inside the volume and holds P (exact_start_cell:
// c_b = floor(P_b) moving up, ceil(P_b) - 1 moving down, in [0, N)), so the first planes are sig_b =
// (float(c_b + u_b) - P_b) rcp_b with c_b + 1 > P_b moving up and c_b < P_b moving down: a difference and a
// reciprocal of one sign, both normal (|d_b| in [2^-64, 1e4], |difference| in [2^-149, N]), sig_b >= 0, no plane
// behind the start. The guarded forms test every address (path_texel, alt_byte); kCertMaxIter bounds the loop.
__global__ void __launch_bounds__(kCertDebugWg) cert_walks_debug_kernel(KArgs a, const uint16_t* __restrict__ vox,
                                                                        const float4* __restrict__ in, uint32_t count,
                                                                        int32_t kind, uint4* __restrict__ out) {
  const uint32_t i = blockIdx.x * uint32_t(kCertDebugWg) + threadIdx.x;
  if (i >= count) return;  // no barrier below
  Ctx c;
  init_ctx(c, a, vox);
  c.ax = nullptr;  // the exact walks' axis table: the certified walks of a ray without a bounce tree do not read it
  const float4 lo = in[2u * size_t(i)], hi = in[2u * size_t(i) + 1u];
  const f3 P = mk(lo.x, lo.y, lo.z), D = mk(hi.x, hi.y, hi.z);
  const float len0 = hi.w;
  c.max_len = lo.w;
  CertResult r;
  r.res = kCertNotStarted;
  r.byte = 0u;
  r.axis = 0;
  r.cx = r.cy = r.cz = 0;
  r.u = r.eu = 0.0f;
  const bool shadow = (kind & 1) != 0;
  const bool lens_ok = len0 >= 0.0f && len0 <= kCertDebugMaxLen && __builtin_fabsf(c.max_len) <= kCertDebugMaxLen;
  int cx, cy, cz;
  if (lens_ok && fast_path_ok(D) && exact_start_cell(c, P, D, cx, cy, cz) &&
      (shadow ? start_layers_clear<true>(c, P, D, cx, cy, cz, 0u) : start_layers_clear<false>(c, P, D, cx, cy, cz, 0u))) {
    const f3 zero = mk(0.0f, 0.0f, 0.0f);
    const float U = c.max_len - len0;
    if (shadow) {
      const f3 rcp = mk(rcp_newton(D.x), rcp_newton(D.y), rcp_newton(D.z));  // fast_path_ok: RN(1 / d)
      r = (kind & 2) ? cert_walk<true, true, false>(c, P, D, rcp, U, cx, cy, cz, 0.0f, zero, len0, 0u)
                     : cert_walk<true, false, false>(c, P, D, rcp, U, cx, cy, cz, 0.0f, zero, len0, 0u);
    } else {
      const f3 rcp = mk(__builtin_amdgcn_rcpf(D.x), __builtin_amdgcn_rcpf(D.y), __builtin_amdgcn_rcpf(D.z));
      r = (kind & 2) ? cert_walk<false, true>(c, P, D, rcp, U, cx, cy, cz, 0.0f, zero, len0, 0u)
                     : cert_walk<false>(c, P, D, rcp, U, cx, cy, cz, 0.0f, zero, len0, 0u);
    }
  }
  out[2u * size_t(i)] = make_uint4(uint32_t(r.res), r.byte, uint32_t(r.axis), uint32_t(r.cx));
  out[2u * size_t(i) + 1u] = make_uint4(uint32_t(r.cy), uint32_t(r.cz), __float_as_uint(r.u), __float_as_uint(r.eu));
}

}  // namespace vrt

#endif  // VRT_CERT_DEBUG_KERNELS_H
