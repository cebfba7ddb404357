// vrt_math.h — GLSL vector semantics on the device: f3, the correctly rounded reciprocal / square root,
// the GLSL built-ins, the hash RNG, RandomizeDirection and the material tables. Includes the HIP runtime only.
#ifndef VRT_MATH_H
#define VRT_MATH_H

#include <hip/hip_runtime.h>

#include <cstdint>

namespace vrt {

// ------------------------------------------------------------------ GLSL vector semantics --

struct f3 {
  float x, y, z;
};

__device__ __forceinline__ f3 mk(float x, float y, float z) { return f3{x, y, z}; }
__device__ __forceinline__ f3 operator+(f3 a, f3 b) { return mk(a.x + b.x, a.y + b.y, a.z + b.z); }
__device__ __forceinline__ f3 operator-(f3 a, f3 b) { return mk(a.x - b.x, a.y - b.y, a.z - b.z); }
__device__ __forceinline__ f3 operator*(f3 a, float s) { return mk(a.x * s, a.y * s, a.z * s); }
__device__ __forceinline__ f3 operator*(float s, f3 a) { return mk(s * a.x, s * a.y, s * a.z); }
__device__ __forceinline__ float dot3(f3 a, f3 b) { return a.x * b.x + a.y * b.y + a.z * b.z; }
__device__ __forceinline__ float comp(f3 a, int i) { return i == 0 ? a.x : (i == 1 ? a.y : a.z); }
__device__ __forceinline__ void set_comp(f3& a, int i, float f) {
  if (i == 0) a.x = f;
  else if (i == 1) a.y = f;
  else a.z = f;
}
// RN(1 / d) from the hardware reciprocal (within 1 ulp) and one Newton step on its exact residual
// (e = 1 - d y by fma): bit-identical to the IEEE division 1.0f / d for every d with a biased
// exponent in [2, 252], i.e. |d| in [2^-125, 2^126) (exhaustive over all 2^32 bit patterns on the
// GPU, 4 211 080 714 of them in that range, 0 mismatches: vrt_debug_fast_math,
// tests/test_gpu_fast_math.py); 3 VALU instead of the division's 11. Operands the caller cannot
// bound take rcp_rn (exponent test, else the division).
__device__ __forceinline__ bool rcp_rn_ok(float d) {
  const uint32_t e = (__float_as_uint(d) >> 23) & 0xFFu;
  return e >= 2u && e <= 252u;
}
__device__ __forceinline__ float rcp_newton(float d) {
  const float y = __builtin_amdgcn_rcpf(d);
  return __builtin_fmaf(__builtin_fmaf(-d, y, 1.0f), y, y);
}
__device__ __forceinline__ float rcp_rn(float d) { return rcp_rn_ok(d) ? rcp_newton(d) : 1.0f / d; }
// RN(sqrt(s)) for s with a biased exponent in [95, 252], i.e. s in [2^-32, 2^126): the hardware
// square root moved to the neighbour its fma residuals pick (the correctly rounded sequence without
// the scaling of s < 2^-32 and the special-value select, which such s never need): bit-identical
// to the IEEE square root on every such s (exhaustive, vrt_debug_fast_math; below 2^-32 the
// unscaled hardware root is off by more than the fix can mend: 2.2 M mismatches when [2^-125,
// 2^-32) was included). Other s take the IEEE square root.
__device__ __forceinline__ bool sqrt_fix_ok(float s) {
  const uint32_t e = (__float_as_uint(s) >> 23) & 0xFFu;
  return e >= 95u && e <= 252u;
}
__device__ __forceinline__ float sqrt_fix(float s) {
  const float y = __builtin_amdgcn_sqrtf(s);
  const float ym = __uint_as_float(__float_as_uint(y) - 1u), yp = __uint_as_float(__float_as_uint(y) + 1u);
  const float rm = __builtin_fmaf(-ym, y, s), rp = __builtin_fmaf(-yp, y, s);
  const float z = rm <= 0.0f ? ym : y;
  return rp > 0.0f ? yp : z;
}
__device__ __forceinline__ float sqrt_rn(float s) { return sqrt_fix_ok(s) ? sqrt_fix(s) : __builtin_sqrtf(s); }

// RN(1 / RN(sqrt(s))) for s within 1024 ulps of 1 (bits b), in closed form: for s = 1 + k 2^-23
// (k >= 0) the correctly rounded square root is 1 + floor(k/2) 2^-23 and its reciprocal
// 1 - floor(k/2) 2^-23; for s = 1 - k 2^-24 they are 1 - ceil(k/2) 2^-24 and 1 + ceil(m/2) 2^-23,
// m = ceil(k/2) (the square root and the reciprocal sit within m^2 2^-48 of those grid points or
// midpoints, on the side that decides the rounding). Exact for |k| < 2898 (exhaustive against
// IEEE sqrt and division: tests/test_normalize_fast.py); a normalised vector's squared length is
// within a few ulps of 1, so RandomizeDirection's, the skybox's and GetRefractionRay's
// normalize of an already normalised direction takes ~6 VALU instead of ~26.
__device__ __forceinline__ float near_one_rsqrt(uint32_t b) {
  const uint32_t one = 0x3F800000u;
  // ((b - one) & ~1u is 0 for b - one < 2: s = 1 and 1 + 2^-23 give 1 without a select)
  const uint32_t r = b >= one ? one - ((b - one) & ~1u) : one + (((((one - b) + 1u) >> 1) + 1u) >> 1);
  return __uint_as_float(r);
}
// normalize's factor RN(1 / RN(sqrt(s))) for any squared length s
__device__ __forceinline__ float normalize3_scale(float s) {
  const uint32_t b = __float_as_uint(s);
  return b - (0x3F800000u - 1024u) <= 2048u ? near_one_rsqrt(b) : rcp_rn(sqrt_rn(s));
}
__device__ __forceinline__ f3 normalize3(f3 v) {
  const float s = v.x * v.x + v.y * v.y + v.z * v.z;
  return v * normalize3_scale(s);
}
__device__ __forceinline__ float gsign(float x) { return x > 0.0f ? 1.0f : (x < 0.0f ? -1.0f : 0.0f); }
__device__ __forceinline__ float gmin(float x, float y) { return y < x ? y : x; }
__device__ __forceinline__ float gmax(float x, float y) { return __builtin_fmaxf(x, y); }
__device__ __forceinline__ float gpow(float x, float y) { return exp2f(y * log2f(x)); }
// The same by the bare v_log_f32 and v_exp_f32, without the library forms' denormal scaling (a compare, a
// select and a multiply or an add around each): the two differ only where x or the result is denormal, and
// there both are below 2^-100 for the specular exponent 10 (exhaustive over x >= 0: vrt_debug_pow_forms,
// tests/test_gpu_pow_forms.py). For a caller that adds the power to a term of ordinary size only.
__device__ __forceinline__ float gpow_raw(float x, float y) {
  return __builtin_amdgcn_exp2f(y * __builtin_amdgcn_logf(x));
}
__device__ __forceinline__ float mixf(float x, float y, float a) { return x * (1.0f - a) + y * a; }
__device__ __forceinline__ f3 reflect3(f3 i, f3 n) {
  const float s = 2.0f * dot3(n, i);
  return i - s * n;
}
__device__ __forceinline__ f3 refract3(f3 i, f3 n, float eta) {
  const float d = dot3(n, i);
  const float k = 1.0f - eta * eta * (1.0f - d * d);
  if (k < 0.0f) return mk(0.0f, 0.0f, 0.0f);
  const float s = eta * d + sqrt_rn(k);
  return eta * i - s * n;
}
__device__ __forceinline__ f3 sign3(f3 d) { return mk(gsign(d.x), gsign(d.y), gsign(d.z)); }

// Jenkins one-at-a-time mix, voxel.glsl:98-125
__device__ __forceinline__ uint32_t hash1(uint32_t x) {
  x += (x << 10u);
  x ^= (x >> 6u);
  x += (x << 3u);
  x ^= (x >> 11u);
  x += (x << 15u);
  return x;
}
__device__ __forceinline__ float random4(float x, float y, float z, float w) {
  const uint32_t h = hash1(__float_as_uint(x) ^ hash1(__float_as_uint(y)) ^
                           hash1(__float_as_uint(z)) ^ hash1(__float_as_uint(w)));
  return __uint_as_float((h & 0x007FFFFFu) | 0x3F800000u) - 1.0f;
}
// RandomizeDirection, voxel.glsl:132-140 (runs even at noise 0: it decides the sign of zeros)
// With randomness == ±0 (every bench config) the added vector is (±0, ±0, ±0), and dir + r equals
// dir bit for bit (x + ±0 = x for x != 0, +0 + ±0 = +0) unless a component is -0.0 (-0 + +0 = +0)
// or NaN: only then do the hashes decide the result, so only then are they computed. Exact.
__device__ __forceinline__ bool zero_noise_exact(f3 d) {
  const uint32_t nz = 0x80000000u;
  return int(__float_as_uint(d.x) != nz) & int(__float_as_uint(d.y) != nz) &
         int(__float_as_uint(d.z) != nz) & int(d.x == d.x) & int(d.y == d.y) & int(d.z == d.z);
}
// The same predicate as one class test per component: -0, signalling NaN or quiet NaN (v_cmp_class
// bits 5, 0, 1). The certified pass's form (LEAN); the truth table is the bit tests' on every pattern.
__device__ __forceinline__ bool zero_noise_exact_class(f3 d) {
  constexpr int kNegZeroOrNan = 0x020 | 0x001 | 0x002;
  return !(__builtin_amdgcn_classf(d.x, kNegZeroOrNan) | __builtin_amdgcn_classf(d.y, kNegZeroOrNan) |
           __builtin_amdgcn_classf(d.z, kNegZeroOrNan));
}
template <bool LEAN = false>
__device__ __forceinline__ f3 randomize(f3 dir, f3 pos, float randomness, float seed) {
  f3 r = mk(0.0f, 0.0f, 0.0f);
  f3 sum = dir;  // LEAN: on the fast path dir + r is dir bit for bit (above), an identity the compiler cannot fold
  if (!(randomness == 0.0f && (LEAN ? zero_noise_exact_class(dir) : zero_noise_exact(dir)))) {
    const f3 p = mk((pos.x + dir.x) + seed, (pos.y + dir.y) + seed, (pos.z + dir.z) + seed);
    const float dx = random4(p.x, p.y, p.z, 0.0f + seed);
    const float dy = random4(p.x, p.y, p.z, 0.5f + seed);
    const float dz = random4(p.x, p.y, p.z, 1.0f + seed);
    r = mk((dx + -0.5f) * randomness, (dy + -0.5f) * randomness, (dz + -0.5f) * randomness);
    sum = dir + r;
  }
  return normalize3(LEAN ? sum : dir + r);
}

// ------------------------------------------------------- materials (_COLOR_ONLY, :71-91) ----

__device__ __forceinline__ uint32_t mat_id(uint32_t b) { return b > 3 ? 3 : b; }
__device__ __forceinline__ float mat_refr(uint32_t b) { return mat_id(b) == 2 ? 1.5f : 1.0f; }
__device__ __forceinline__ bool mat_transparent(uint32_t m) { return m == 0 || m == 2; }
__device__ __forceinline__ bool mat_reflective(uint32_t m) { return m == 2; }
__device__ __forceinline__ float mat_kd(uint32_t m) { return m == 0 ? 0.0f : (m == 2 ? 1.0f : 0.4f); }
// specular factor / exponent: _COLOR_ONLY table (:83-86) or the textured table (:64-67)
__device__ __forceinline__ float mat_ks(uint32_t m, bool tex) {
  return m == 0 ? 0.0f : (m == 2 ? 1.0f : (tex ? (m == 1 ? 0.6f : 0.4f) : 0.2f));
}
__device__ __forceinline__ float mat_exp(uint32_t m, bool tex) {
  return m == 0 ? 0.0f : (m == 2 ? (tex ? 0.3f : 1.0f) : (tex ? (m == 1 ? 60.0f : 20.0f) : 10.0f));
}
// atlas slot (texX, texY) of the textured table (:64-67)
__device__ __forceinline__ uint32_t mat_tex_x(uint32_t m) { return m == 3 ? 1u : 0u; }
__device__ __forceinline__ uint32_t mat_tex_y(uint32_t m) { return m >= 2 ? 1u : 0u; }
__device__ __forceinline__ float4 mat_color(uint32_t m) {
  if (m == 1) return make_float4(0.5f, 0.5f, 0.5f, 1.0f);
  if (m == 3) return make_float4(0.05f, 0.5f, 0.1f, 1.0f);
  return make_float4(0.0f, 0.0f, 0.0f, 0.0f);
}

constexpr float kAmbient = 0.3f;

// Colour-only glass (voxel.glsl:85: colour vec4(0)) adds col.rgb * col.a * brightness = +0 for any
// finite brightness (glass's lit brightness is finite: kd = ks = 1, exponent 1; RayColor, :184-188),
// so a glass hit's colour does not depend on its shadow bit: the stats-free paths skip its shadow
// walk (TraceWithShadow, :400-402). Images unchanged.
__device__ __forceinline__ bool shadow_free_hit(uint32_t byte, bool tex) { return !tex && mat_id(byte) == 2u; }

}  // namespace vrt

#endif  // VRT_MATH_H
